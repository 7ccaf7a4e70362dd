// Parameter identification on the device (include/mi_ilqr.h, "Parameter identification"): from logged transitions
// (x_j, u_j, x_next_j) to the parameter rows MI_F_MODEL_PARAMS takes, Levenberg-Marquardt on the one-step prediction error,
// independently per problem.  One evaluation of the normal equations is one launch of the kernel below; the decisions between two
// evaluations are fit_update_kernel's (no model; defined in k_fit.hip: a plugin unit includes this header for its model's kernel
// and carries none of it).
//
//   fit_normal_kernel<M>, ONE LANE PER (TRANSITION, SLOT), one wave per block, grid B x waves.  G = 1 << log2G slots per transition,
//   G >= P + 1, the slot in the lane's low bits: slot 0 evaluates f at theta, slot i = 1 .. P at theta + h e_k and theta - h e_k,
//   k = free[i - 1], h = fd_rel max(|theta_k|, fd_floor); theta is the problem's TRIAL row of the state record, held in registers,
//   every lane its own copy.  Every lane runs exactly two evaluations of M::step<double> (slot 0's second repeats its first; slots
//   past P and lanes past the problem's count shadow a live item and contribute exact zeros), so the kernel has no divergent call
//   of the step and no wave-level operation under divergent control.  Slot 0 writes r = x_next - f, slot i the column
//   J_i = (f+ - f-) / (2 h) into the wave's LDS - lane l's column at l * S, S = n | 1 odd, so that the lanes of a column read fall
//   into different banks - and after wave_sync slot 0 forms r' W r, slot i forms g_i = J_i' W r and H_ij = J_i' W J_j for j >= i.
//   The wave sums them over its transitions with a butterfly of fixed order over the lane bits >= log2G (DPP inside a 16-lane row,
//   ds_bpermute across rows) and stores ONE row c | g | upper(H) per (problem, wave).  A problem that has finished (its status is
//   not kFitRunning) and a wave wholly past the problem's count leave through a wave-uniform branch at the top, the latter after
//   storing a row of zeros.  Problem-constant inputs (the record, the weights and the count) are read with wave-uniform indices.
//   Nothing depends on the handle's layout, on B or on the other problems.
#pragma once
#include "fastmath.hpp"
#include "host.hpp"           // mi_ilqr, FitArgs, the record's layout, HIPCHK
#include "models.hpp"
#include "wave_ops.hpp"

namespace mi {

struct FitDims {
  double dt, fd_rel, fd_floor;
  int32_t T, P, log2G, waves;
  int32_t free_idx[mi_host::kFitMaxFree];
};

#if defined(__HIPCC__)
// entry (a, b), a <= b, of the upper triangle of a P x P matrix stored row after row
__device__ __forceinline__ int fit_tri(int P, int a, int b) { return a * P - a * (a - 1) / 2 + (b - a); }

// the sum over the lanes that share this lane's low log2G bits, in every one of them; all 64 lanes call it
__device__ __forceinline__ double fit_item_sum(double v, int log2G, int lane) {
  if (log2G <= 1) v += row_xor_f64<2>(v);
  if (log2G <= 2) v += row_xor_f64<4>(v);
  if (log2G <= 3) v += row_xor_f64<8>(v);
  v += lane_read_f64(v, lane ^ 16);
  v += lane_read_f64(v, lane ^ 32);
  return v;
}

template <class M>
__global__ void __launch_bounds__(64) fit_normal_kernel(const double* __restrict__ data, const double* __restrict__ weights,
                                                        const double* __restrict__ state, double* __restrict__ partial, const FitDims d) {
  using namespace mi_host;
  constexpr int n = M::n, m = M::m, np = M::n_params, NP = np > 0 ? np : 1, RW = 2 * n + m, S = n | 1;
  __shared__ double s_col[64 * S];
  const int b = (int)(blockIdx.x / (unsigned)d.waves), w = (int)(blockIdx.x - (unsigned)b * (unsigned)d.waves);
  const int lane = (int)threadIdx.x;
  const double* st = state + (size_t)b * kFitStride;
  if (st[kFitStatus] != kFitRunning) return;                        // (wave-uniform: a finished problem is frozen)
  const int P = d.P, L = fit_row_len(P);
  const double* wrow = weights + (size_t)b * (n + 1);
  const int count = (int)wrow[n], per = 64 >> d.log2G, j0 = w * per;
  double* out = partial + ((size_t)b * d.waves + w) * L;
  if (j0 >= count) {                                                // (wave-uniform: nothing of this wave is in use)
    if (lane < L) out[lane] = 0.0;
    return;
  }
  const int slot = lane & ((1 << d.log2G) - 1), item = lane >> d.log2G, j = j0 + item;
  const bool live_item = j < count, fd = slot >= 1 && slot <= P, live = live_item && slot <= P;
  const int jl = live_item ? j : count - 1;                         // lanes past the count shadow the last row
  int k = -1;
#pragma unroll
  for (int i = 0; i < kFitMaxFree; ++i) k = (fd && slot - 1 == i) ? d.free_idx[i] : k;

  double theta[NP], tk = 0.0;
#pragma unroll
  for (int i = 0; i < NP; ++i) theta[i] = i < np ? st[kFitTrial + i] : 0.0;
#pragma unroll
  for (int i = 0; i < NP; ++i) tk = i == k ? theta[i] : tk;
  const double ak = fabs(tk), hstep = d.fd_rel * (ak > d.fd_floor ? ak : d.fd_floor);

  const double* row = data + ((size_t)b * d.T + jl) * RW;
  double x[n], u[m], fa[n], fb[n];
#pragma unroll
  for (int i = 0; i < n; ++i) x[i] = row[i];
#pragma unroll
  for (int i = 0; i < m; ++i) u[i] = row[n + i];
#pragma unroll
  for (int i = 0; i < n; ++i) fa[i] = 0.0;
  // two evaluations per lane: at theta + h e_k, then at theta - h e_k (k = -1: both at theta); fb ends as the first, fa as the second
#pragma unroll 1
  for (int e = 0; e < 2; ++e) {
    const double dk = e == 0 ? hstep : -hstep;
    double p[NP], xn[n];
#pragma unroll
    for (int i = 0; i < NP; ++i) p[i] = i == k ? theta[i] + dk : theta[i];
    M::template step<double>(x, u, xn, p, d.dt);
#pragma unroll
    for (int i = 0; i < n; ++i) { fb[i] = fa[i]; fa[i] = xn[i]; }
  }
  const double h2 = 2.0 * hstep;
  double* own = s_col + lane * S;
#pragma unroll
  for (int i = 0; i < n; ++i) own[i] = fd ? (fb[i] - fa[i]) / h2 : row[n + m + i] - fb[i];
  wave_sync();

  // slot 0: r' W r; slot i: g_i and H_ij, j = i .. P, from the item's columns (its slot-0 lane is lane - slot)
  const int base = lane - slot;
  const double* rcol = s_col + base * S;
  double val[1 + kFitMaxFree];
  {
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < n; ++i) acc += own[i] * wrow[i] * rcol[i];
    val[0] = live ? acc : 0.0;
  }
#pragma unroll
  for (int dd = 0; dd < kFitMaxFree; ++dd) {
    val[1 + dd] = 0.0;
    if (dd < P) {                                                   // (wave-uniform)
      const bool valid = fd && slot + dd <= P;
      const double* other = s_col + (valid ? base + slot + dd : lane) * S;
      double acc = 0.0;
#pragma unroll
      for (int i = 0; i < n; ++i) acc += own[i] * wrow[i] * other[i];
      val[1 + dd] = (valid && live_item) ? acc : 0.0;
    }
  }
  // the sum over the wave's transitions; every lane takes part in every move
  val[0] = fit_item_sum(val[0], d.log2G, lane);
#pragma unroll
  for (int dd = 0; dd < kFitMaxFree; ++dd)
    if (dd < P) val[1 + dd] = fit_item_sum(val[1 + dd], d.log2G, lane);
  if (item == 0 && slot <= P) {
    out[slot] = val[0];                                             // c (slot 0) | g_slot
#pragma unroll
    for (int dd = 0; dd < kFitMaxFree; ++dd)
      if (fd && slot + dd <= P) out[1 + P + fit_tri(P, slot - 1, slot - 1 + dd)] = val[1 + dd];
  }
}
#endif

}  // namespace mi

namespace mi_host {

template <class M>
int launch_fit_normal(mi_ilqr* h, const FitArgs& a) {
  if (M::n_params == 0) return MI_ILQR_E_UNSUPPORTED;
  if (a.B < 1 || a.T < 1 || a.P < 1 || a.P > kFitMaxFree || a.log2G < 1 || a.log2G > 4 || (1 << a.log2G) < a.P + 1 || !a.data || !a.weights ||
      !a.state || !a.partial)
    return MI_ILQR_E_BAD_ARG;
  const int per = 64 >> a.log2G;
  if (a.waves != (a.T + per - 1) / per) return MI_ILQR_E_BAD_ARG;
  for (int i = 0; i < a.P; ++i)
    if (a.free_idx[i] < 0 || a.free_idx[i] >= M::n_params || (i > 0 && a.free_idx[i] <= a.free_idx[i - 1])) return MI_ILQR_E_BAD_ARG;
  const unsigned long long blocks = (unsigned long long)a.waves * (unsigned long long)a.B;
  if (blocks > 0x7fffffffull) return MI_ILQR_E_UNSUPPORTED;
  FitArgs v = a;
  mi::FitDims d{a.dt, a.fd_rel, a.fd_floor, a.T, a.P, a.log2G, a.waves, {}};
  for (int i = 0; i < kFitMaxFree; ++i) d.free_idx[i] = i < a.P ? a.free_idx[i] : -1;
  void* argv[] = {&v.data, &v.weights, &v.state, &v.partial, &d};
  const void* kern = reinterpret_cast<const void*>(mi::fit_normal_kernel<M>);
  HIPCHK(hipExtLaunchKernel(kern, dim3((unsigned)blocks), dim3(64), argv, 0, h->stream, a.ev0, a.ev1, 0));
  return MI_ILQR_OK;
}

}  // namespace mi_host
