// Sampling-based MPC on the device (include/mi_ilqr.h, "Sampling-based MPC"): MPPI / predictive-sampling updates of every
// problem's nominal plan, the derivative-free counterpart of a solve.  One iteration is two launches, nothing of size S leaves the
// device and nothing of size S (N-1) is ever stored:
//
//   mppi_rollout_kernel<M>, ONE LANE PER SAMPLE, one wave per (problem, 64 samples), grid B x ceil(S / 64).  Sample s of problem b
//   applies v_s[k,t] = clip(u[k,t] + sigma_u[b,k] z) - mppi_applied below: a rounded product and a rounded sum, never an FMA, the
//   clip by comparisons and on a control-limited handle only - and is rolled out open loop with M::step<double>, its state in
//   registers; the cost is policy_rollout_kernel's stage and terminal expressions on the APPLIED control.  z: Philox4x32-10 under the
//   key (seed lo, seed hi) at counter (g, t div hold, b, 1024 + k / 4), g = first_sample + i S + s the global sample number, Box-Muller
//   normal k mod 4 of the block (mppi_block_normals), drawn per lane once per `hold` window.  SAMPLE 0 IS THE ELITE SLOT: it draws
//   nothing and applies clip(u); so does a zero sigma and a padding control (k >= m_user), bit for bit.  The nominal arrives as a
//   time-major staging copy (B, N-1, m) read with wave-uniform indices through `const __restrict__` - one fetch per wave - like the
//   problem's x0, cost matrices, target, parameters, bounds and sigma row.  A sample that meets an infeasible step, a non-finite
//   state or a non-finite cost gets +inf.  Output: cost (B, S) only.  Lanes past a ragged tail shadow the last sample and store
//   nothing; no wave-level operation and no early return.
//
//   mppi_update_kernel (no model; defined in k_mppi.hip, like the two kernels below it: a plugin unit includes this header for its
//   model's rollout and carries none of them), ONE WORKGROUP PER PROBLEM (256 threads), in this order:
//     1. L_min, its sample (ties to the lowest s) and the number of finite samples: a strided scan, the DPP butterfly of wave_ops.hpp
//        inside the wave, LDS across the four waves (a total order: the result does not depend on the order of the combinations).
//     2. e_s = exp(-(L_s - L_min) / temperature) for the finite samples (temperature = 0: 1 for the argmin, 0 else), into LDS, tiles
//        of kMppiTile samples; Z = sum e_s and then Q = sum (e_s / Z)^2, BOTH SUMMED SEQUENTIALLY IN s = 0, 1, .. S - 1 from 0.0,
//        non-finite samples skipped: an order that is a function of S alone.  (Every thread adds the same LDS values up - a broadcast
//        read - so no thread waits for another's sum.)
//     3. the log rows: argmin | L_min | finite, and nominal cost (sample 0's) | ESS = 1 / Q.  No finite sample: -1 | +inf | 0, ESS NaN.
//     4. THE BLEND.  An item is (step t, control block jb = k div 4); thread i of a batch of 256 items REGENERATES v_s[4 jb .. 4 jb + 3, t]
//        for s = 0, 1, .. S - 1 with the functions the rollout uses - so the two agree bit for bit - and accumulates
//        u_new = w_0 v_0 + w_1 v_1 + ..., w_s = e_s / Z, sequentially in s: the first finite sample's rounded product starts the sum,
//        every later one is a rounded product added by a rounded sum (no FMA); non-finite samples are skipped, not multiplied by 0.
//        u_new is clipped again on a limited handle and written time-major (block fastest: consecutive lanes, consecutive
//        addresses).  A problem without a finite sample keeps u.
//   None of this depends on the handle's layout, on B or on the grid.
//
//   mppi_stage_kernel / mppi_handover_kernel (no model): the nominal from the handle's layout into the time-major staging copy before
//   the first iteration; after the closing rollout (S = 1: the final nominal's cost) the final nominal into u_guess in the handle's
//   layout shifted by `shift` steps - walked in the layout's own order, so consecutive lanes store consecutive addresses in all three
//   layouts, which one workgroup per problem could not do for [t][row][b] - into the time-last copy the boundary returns, and the
//   closing row of the cost log.
#pragma once
#include "fastmath.hpp"
#include "host.hpp"           // mi_ilqr, MppiArgs, MppiUpdateArgs, HIPCHK
#include "model_traits.hpp"   // CanFail
#include "models.hpp"
#include "philox.hpp"
#include "wave_ops.hpp"

namespace mi {

constexpr uint32_t kMppiBlock = 1024;      // the samples' first Philox block (0.. states, 256.. controls, 512.. Monte-Carlo draws, 768.. seeds)
constexpr int kMppiThreads = 256;
constexpr int kMppiTile = 2048;            // weights held in LDS at a time (16 KiB)

struct MppiDims {
  size_t param_stride, cost_stride, x_nom_stride;
  double dt;
  int32_t N, S, waves, m_user, hold;
  uint32_t seed_lo, seed_hi, sample0;      // the Philox key and the global number of this launch's sample 0
};

#if defined(__HIPCC__)
__device__ __forceinline__ bool mppi_finite(double v) { return v - v == 0.0; }      // (false for NaN and +-inf)

// The four normals of control block jb for global sample g in window w of problem b; a pair nobody needs is not computed (0).
__device__ __forceinline__ void mppi_block_normals(uint32_t k0, uint32_t k1, uint32_t g, uint32_t w, uint32_t b, uint32_t jb, bool pair0,
                                                   bool pair1, double (&z)[4]) {
  uint32_t c[4] = {g, w, b, kMppiBlock + jb};
  philox4x32_10(k0, k1, c);
  z[0] = z[1] = z[2] = z[3] = 0.0;
  if (pair0) box_muller(c[0], c[1], z[0], z[1]);
  if (pair1) box_muller(c[2], c[3], z[2], z[3]);
}

// v = clip(u + sg z): the product rounded before it is added (no FMA), u itself - bit for bit - where sg = 0; the clip by
// comparisons (a NaN stays one, like np.clip), lim = u_min (m) | u_max (m) or nullptr
__device__ __forceinline__ double mppi_applied(double u, double sg, double z, const double* lim, int m, int k) {
  double v = u;
  if (sg != 0.0) {
    double sz = sg * z;
    asm volatile("" : "+v"(sz));
    v = u + sz;
  }
  if (lim) {
    const double lo = lim[k], hi = lim[m + k];
    v = v < lo ? lo : (v > hi ? hi : v);
  }
  return v;
}

template <class M>
__global__ void __launch_bounds__(64) mppi_rollout_kernel(
    const double* __restrict__ nominal, const double* __restrict__ x0, const double* __restrict__ param_rows,
    const double* __restrict__ cost, const double* __restrict__ x_nom, const double* __restrict__ ulim,
    const double* __restrict__ sigma, double* __restrict__ cost_out, const MppiDims d) {
  constexpr int n = M::n, m = M::m, JB = (m + 3) / 4;
  const int b = (int)(blockIdx.x / (unsigned)d.waves);
  const int s = (int)(blockIdx.x - (unsigned)b * (unsigned)d.waves) * 64 + (int)threadIdx.x;
  const bool live = s < d.S;
  const int sl = live ? s : d.S - 1;                                // lanes past a ragged tail shadow the last sample and store nothing
  const int N = d.N;

  double x[n];
#pragma unroll
  for (int i = 0; i < n; ++i) x[i] = x0[(size_t)b * n + i];
  bool alive = true;
#pragma unroll
  for (int i = 0; i < n; ++i) alive = alive && mppi_finite(x[i]);

  const double* p = param_rows + (size_t)b * d.param_stride;
  const double* Q = cost + (size_t)b * d.cost_stride;
  const double* R = Q + n * n;
  const double* Qf = R + m * m;
  const double* xt = x_nom + (size_t)b * d.x_nom_stride;
  const double* lim = ulim ? ulim + (size_t)b * 2 * m : nullptr;
  const double* row = nominal + (size_t)b * (N - 1) * m;
  // the problem's sigma row (wave-uniform): which Box-Muller pairs of which block anybody needs
  double sg_row[m];
  bool pair0[JB], pair1[JB];
#pragma unroll
  for (int k = 0; k < m; ++k) sg_row[k] = (sigma && k < d.m_user) ? sigma[(size_t)b * m + k] : 0.0;
#pragma unroll
  for (int j = 0; j < JB; ++j) {
    pair0[j] = sg_row[4 * j] != 0.0 || (4 * j + 1 < m && sg_row[4 * j + 1] != 0.0);
    pair1[j] = (4 * j + 2 < m && sg_row[4 * j + 2] != 0.0) || (4 * j + 3 < m && sg_row[4 * j + 3] != 0.0);
  }
  const bool elite = sl == 0;
  const uint32_t g = d.sample0 + (uint32_t)sl;

  double z[4 * JB];
#pragma unroll
  for (int k = 0; k < 4 * JB; ++k) z[k] = 0.0;
  double L = 0.0;
  int left = 0;
  uint32_t w = 0;
  for (int t = 0; t < N - 1; ++t, row += m) {
    if (left == 0) {                                                // a new window: t = w hold
#pragma unroll
      for (int j = 0; j < JB; ++j) {
        if (pair0[j] || pair1[j]) {
          double zz[4];
          mppi_block_normals(d.seed_lo, d.seed_hi, g, w, (uint32_t)b, (uint32_t)j, pair0[j], pair1[j], zz);
#pragma unroll
          for (int c = 0; c < 4; ++c) z[4 * j + c] = zz[c];
        }
      }
      left = d.hold;
      ++w;
    }
    --left;
    double v[m], xn[n], dx[n];
#pragma unroll
    for (int k = 0; k < m; ++k) v[k] = mppi_applied(row[k], elite ? 0.0 : sg_row[k], z[k], lim, m, k);
    M::template step<double>(x, v, xn, p, d.dt);
    bool ok = true;
#pragma unroll
    for (int i = 0; i < n; ++i) ok = ok && mppi_finite(xn[i]);
    if constexpr (CanFail<M>::value) {
#pragma unroll
      for (int i = M::nq; i < n; ++i) ok = ok && !M::infeasible_velocity(xn[i], p);
    }
    // stage cost at (x_t, v_t), no 1/2 factor
    double c = 0.0;
#pragma unroll
    for (int i = 0; i < n; ++i) dx[i] = x[i] - xt[i];
#pragma unroll
    for (int i = 0; i < n; ++i) {
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < n; ++j) acc += Q[i * n + j] * dx[j];
      c += dx[i] * acc;
    }
#pragma unroll
    for (int k = 0; k < m; ++k) {
      double acc = 0.0;
#pragma unroll
      for (int l = 0; l < m; ++l) acc += R[k * m + l] * v[l];
      c += v[k] * acc;
    }
    alive = alive && ok;
    L += alive ? c : 0.0;
#pragma unroll
    for (int i = 0; i < n; ++i) x[i] = alive ? xn[i] : x[i];
  }
  {
    double dx[n], c = 0.0;
#pragma unroll
    for (int i = 0; i < n; ++i) dx[i] = x[i] - xt[i];
#pragma unroll
    for (int i = 0; i < n; ++i) {
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < n; ++j) acc += Qf[i * n + j] * dx[j];
      c += dx[i] * acc;
    }
    L = L + c;
    L = (alive && mppi_finite(L)) ? L : INFINITY;
  }
  if (live) cost_out[(size_t)b * d.S + sl] = L;
}
#endif

}  // namespace mi

namespace mi_host {

template <class M>
int launch_mppi_rollout(mi_ilqr* h, const MppiArgs& a) {
  if (a.r.N < 2 || a.S < 1 || a.S > 0x7fffffff - 63 || a.r.B < 1 || a.hold < 1 || !a.nominal || !a.x0 || !a.cost_out) return MI_ILQR_E_BAD_ARG;
  MppiArgs v = a;
  mi::MppiDims d{a.r.param_stride, a.r.cost_stride, a.r.x_nom_stride, a.r.dt, a.r.N, a.S, (a.S + 63) / 64, a.r.m_user, a.hold,
                 (uint32_t)(a.seed & 0xffffffffull), (uint32_t)(a.seed >> 32), a.sample0};
  void* argv[] = {&v.nominal, &v.x0, &v.r.param_rows, &v.r.cost, &v.r.x_nom, &v.r.ulim, &v.sigma, &v.cost_out, &d};
  const unsigned long long blocks = (unsigned long long)d.waves * (unsigned long long)a.r.B;
  if (blocks > 0x7fffffffull) return MI_ILQR_E_UNSUPPORTED;
  const void* kern = reinterpret_cast<const void*>(mi::mppi_rollout_kernel<M>);
  HIPCHK(hipExtLaunchKernel(kern, dim3((unsigned)blocks), dim3(64), argv, 0, h->stream, a.ev0, a.ev1, 0));
  return MI_ILQR_OK;
}

}  // namespace mi_host
