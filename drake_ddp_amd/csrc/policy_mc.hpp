// Monte-Carlo evaluation of a solved feedback policy ON THE DEVICE (mi_ilqr_set MI_F_POLICY_MC_RUN; include/mi_ilqr.h, "Monte-Carlo
// on the device"): every sample's start state - and, PS, its plant's parameters - is DRAWN where it is used, the lane's rollout is
// policy_rollout_kernel's (policy_mc_lane_rollout below repeats its loop: a sample's cost is the same bits in both), and the results
// are REDUCED here - per problem ten numbers, S | counted | success | mean | M2 | min | max | argmin | argmax
// | steps_total - so that nothing of size S crosses the bus unless the caller asks for the samples.
//
// policy_mc_kernel<M, PS, NZ>: one lane per sample, one wave = one GROUP of 64 consecutive samples of one problem (blockIdx.x =
// problem * groups-of-the-window + group).  For the global sample number g = first_sample + s:
//   x0[i] = mean[i] + spread[i] d_i,   d_i from word (pair) i mod 4 of the Philox block with counter (g, 0, common ? 0 : b, 512 + i / 4)
//   p[j]  = p_mean[j] + p_spread[j] d_j, blocks 768 + j / 4                                     (PS; a distribution of its own)
//   normal: d = the Box-Muller normal of philox.hpp;  uniform: d = (w + 1/2) 2^-31 - 1, exact in fp64, inside (-1, 1)
// under the key of the rollouts' disturbances (blocks 0 .. 9 and 256 .. 259 there: the draws and the noise are independent under one
// seed).  A spread of zero returns the mean's bits.  The problem's sampler row x0_mean | x0_spread | goal | p_mean | p_spread is
// wave-uniform - `const __restrict__`, uniform indices, read through the scalar unit like the policy row - and so is the choice of
// the distribution (a uniform branch); no early return, no divergence beyond per-lane selects.
//
// The reduction order is part of the contract.  A sample is COUNTED iff it ran all N - 1 steps and its cost is finite; lanes past a
// ragged tail and uncounted samples enter with count 0.  The wave's statistic is the butterfly over lane distance 1, 2, 4, 8, 16, 32
// of Chan's merge (mc_merge below; A is always the operand from the lower lane): distances 1 .. 8 are DPP moves inside the 16-lane
// rows (wave_ops.hpp: row_xor_*), 16 and 32 take the four row results through v_readlane - every lane of a row holds its row's
// result, so merge(merge(r0, r16), merge(r32, r48)) IS what the butterfly leaves in every lane.  No LDS.  Lane 0 leaves the group's
// partial, kMcFields doubles, PROBLEM-minor (group, field, B) with ordinary vector stores; with `samples` the kernel also stores
// x0 | params | cost | steps sample-minor.
//
// policy_mc_fold_kernel: one lane per problem folds the window's group partials LEFT TO RIGHT into the running accumulator
// (kMcFields, B), which persists across the host's passes over windows of groups - the result is bitwise independent of the window.
#pragma once
#include "policy_rollout.hpp"   // PolicyDims, policy_finite (and through it host.hpp: PolicyMcArgs, kMcFields; models.hpp; philox.hpp)
#include "wave_ops.hpp"

namespace mi {

constexpr uint32_t kMcX0Block = 512u, kMcParamBlock = 768u;
constexpr int kMcNormal = 0, kMcUniform = 1;

// One operand of the reduction.  Empty: n = 0, mean = m2 = 0, mn = +inf, mx = -inf, amin = amax = -1.
struct McPart { double n, mean, m2, mn, mx, amin, amax, succ, steps; };

__host__ __device__ inline McPart mc_empty() { return McPart{0.0, 0.0, 0.0, INFINITY, -INFINITY, -1.0, -1.0, 0.0, 0.0}; }

// Chan's merge of (count, mean, M2) - A the operand of the LOWER sample numbers - and the exact fields beside it.  A count-0 operand
// returns the other operand's bits; min / max ties keep A: the lower sample number.
__host__ __device__ inline McPart mc_merge(const McPart& A, const McPart& B) {
  const double n = A.n + B.n, delta = B.mean - A.mean;
  const double w = B.n / n, q = (A.n * B.n) / n;
  const double mean = A.mean + delta * w, m2 = (A.m2 + B.m2) + (delta * delta) * q;
  McPart r;
  r.n = n;
  r.mean = B.n == 0.0 ? A.mean : (A.n == 0.0 ? B.mean : mean);
  r.m2 = B.n == 0.0 ? A.m2 : (A.n == 0.0 ? B.m2 : m2);
  const bool lo = B.mn < A.mn, hi = B.mx > A.mx;
  r.mn = lo ? B.mn : A.mn; r.amin = lo ? B.amin : A.amin;
  r.mx = hi ? B.mx : A.mx; r.amax = hi ? B.amax : A.amax;
  r.succ = A.succ + B.succ;
  r.steps = A.steps + B.steps;
  return r;
}

struct PolicyMcDims {
  PolicyDims r;                  // r.waves: the groups of this window; r.S is not used (S below)
  unsigned long long S;          // the call's samples per problem
  size_t win_samples;            // samples of this window (the sample buffer's inner extent)
  uint32_t group0;               // the window's first group
  int32_t B, x0_dist, p_dist;
};

#if defined(__HIPCC__)
// The rollout of ONE LANE's sample, from the state x it holds (alive: x is finite) to the end of the horizon: on return x is the
// last state the sample held, L_out its cost (+inf when it ended early) and steps_out the steps it completed.  p: the plant's
// parameters (a lane's own registers or the problem's wave-uniform row); Q: the problem's Q | R | Qf; xt: its target; lim: its
// u_min | u_max or nullptr; row: its policy rows; sg (NZ): its sigma row, ctr_s / ctr_b the sample and problem words of the Philox
// counter.  This is policy_rollout_kernel's loop REPEATED, statement by statement and in its order - the trajectory stores X / U
// included, behind pointers the host always passes as nullptr today, so that the loop is the same code to the compiler:
// calling one shared function from both kernels changed the instruction mix of policy_rollout_kernel, so that kernel
// stays the text it was and the body lives twice.  Whoever changes one changes the other: tests/test_gpu_policy_mc.py holds the two
// to the same bits per sample.
template <class M, bool NZ>
__device__ __forceinline__ void policy_mc_lane_rollout(double (&x)[M::n], bool& alive, const double* p, const double* Q, const double* xt,
                                                       const double* lim, const double* row, const double* sg, uint32_t ctr_s,
                                                       uint32_t ctr_b, double* X, double* U, bool live, int b, size_t S, size_t sl,
                                                       const PolicyDims& d, double& L_out, int& steps_out) {
  constexpr int n = M::n, m = M::m, W = n + m + m * n;
  const int N = d.N;
  const double* R = Q + n * n;
  const double* Qf = R + m * m;
  const double nan = __builtin_nan("");
  bool noise_x = false, noise_u = false;
  if constexpr (NZ) {
#pragma unroll
    for (int i = 0; i < n; ++i) noise_x = noise_x || sg[i] != 0.0;
#pragma unroll
    for (int k = 0; k < m; ++k) noise_u = noise_u || sg[n + k] != 0.0;
  }
  if (X && live) {
#pragma unroll
    for (int i = 0; i < n; ++i) X[((size_t)b * N * n + i) * S + sl] = x[i];
  }
  double L = 0.0;
  int steps = 0;
  for (int t = 0; t < N - 1; ++t, row += W) {
    double dx[n], u[m], xn[n];
#pragma unroll
    for (int i = 0; i < n; ++i) dx[i] = x[i] - row[i];
#pragma unroll
    for (int k = 0; k < m; ++k) {
      double acc = 0.0;
#pragma unroll
      for (int i = 0; i < n; ++i) acc += row[n + m + k * n + i] * dx[i];
      double uk = row[n + k] - acc;
      if (lim) {                                                    // (comparisons, not fmin / fmax: a NaN stays one, like np.clip)
        const double lo = lim[k], hi = lim[m + k];
        uk = uk < lo ? lo : (uk > hi ? hi : uk);
      }
      u[k] = k < d.m_user ? uk : 0.0;
    }
    if constexpr (NZ) {
      double ua[m];                                                 // the control the plant gets (padding: sigma = 0, the host saw to it)
#pragma unroll
      for (int k = 0; k < m; ++k) ua[k] = u[k];
      if (noise_u) {
#pragma unroll
        for (int j = 0; j < (m + 3) / 4; ++j) {
          double z[4];
          philox_normals(d.seed_lo, d.seed_hi, ctr_s, (uint32_t)t, ctr_b, 256u + j, m - 4 * j > 2, z);
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (4 * j + c < m) ua[4 * j + c] = u[4 * j + c] + sg[n + 4 * j + c] * z[c];
        }
      }
      M::template step<double>(x, ua, xn, p, d.dt);
      if (noise_x) {
#pragma unroll
        for (int j = 0; j < (n + 3) / 4; ++j) {
          double z[4];
          philox_normals(d.seed_lo, d.seed_hi, ctr_s, (uint32_t)t, ctr_b, (uint32_t)j, n - 4 * j > 2, z);
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (4 * j + c < n) xn[4 * j + c] += sg[4 * j + c] * z[c];
        }
      }
    } else {
      M::template step<double>(x, u, xn, p, d.dt);
    }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < n; ++i) ok = ok && policy_finite(xn[i]);
    if constexpr (CanFail<M>::value) {
#pragma unroll
      for (int i = M::nq; i < n; ++i) ok = ok && !M::infeasible_velocity(xn[i], p);
    }
    // stage cost at (x_t, u_t), no 1/2 factor
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
      for (int l = 0; l < m; ++l) acc += R[k * m + l] * u[l];
      c += u[k] * acc;
    }
    alive = alive && ok;
    if (X && live) {
#pragma unroll
      for (int i = 0; i < n; ++i) X[(((size_t)b * N + t + 1) * n + i) * S + sl] = alive ? xn[i] : nan;
    }
    if (U && live) {
#pragma unroll
      for (int k = 0; k < m; ++k) U[(((size_t)b * (N - 1) + t) * m + k) * S + sl] = alive ? u[k] : nan;
    }
    L += alive ? c : 0.0;
    steps += alive ? 1 : 0;
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
    L = alive ? L + c : INFINITY;
  }
  L_out = L;
  steps_out = steps;
}

// COUNT components mean + spread o d of the blocks first_block .. : the words of each block are generated once, in registers
template <int COUNT>
__device__ __forceinline__ void mc_draw(const PolicyDims& d, uint32_t g, uint32_t cb, uint32_t first_block, int dist,
                                        const double* __restrict__ mean, const double* __restrict__ spread, double (&out)[COUNT]) {
#pragma unroll
  for (int j = 0; j < (COUNT + 3) / 4; ++j) {
    double z[4];
    if (dist == kMcNormal) {
      philox_normals(d.seed_lo, d.seed_hi, g, 0u, cb, first_block + (uint32_t)j, COUNT - 4 * j > 2, z);
    } else {
      uint32_t c[4] = {g, 0u, cb, first_block + (uint32_t)j};
      philox4x32_10(d.seed_lo, d.seed_hi, c);
#pragma unroll
      for (int k = 0; k < 4; ++k) z[k] = ((double)c[k] + 0.5) * 0x1p-31 - 1.0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (4 * j + k < COUNT) out[4 * j + k] = spread[4 * j + k] == 0.0 ? mean[4 * j + k] : mean[4 * j + k] + spread[4 * j + k] * z[k];
  }
}

// one butterfly level inside the 16-lane rows: the partner's operand by DPP, the lower lane's as A
template <int D>
__device__ __forceinline__ McPart mc_row_level(const McPart& own) {
  McPart o;
  o.n = row_xor_f64<D>(own.n); o.mean = row_xor_f64<D>(own.mean); o.m2 = row_xor_f64<D>(own.m2);
  o.mn = row_xor_f64<D>(own.mn); o.mx = row_xor_f64<D>(own.mx); o.amin = row_xor_f64<D>(own.amin); o.amax = row_xor_f64<D>(own.amax);
  o.succ = row_xor_f64<D>(own.succ); o.steps = row_xor_f64<D>(own.steps);
  const bool low = ((int)threadIdx.x & D) == 0;
  McPart A, B;
#define MI_MC_PICK(f) A.f = low ? own.f : o.f; B.f = low ? o.f : own.f;
  MI_MC_PICK(n) MI_MC_PICK(mean) MI_MC_PICK(m2) MI_MC_PICK(mn) MI_MC_PICK(mx) MI_MC_PICK(amin) MI_MC_PICK(amax) MI_MC_PICK(succ) MI_MC_PICK(steps)
#undef MI_MC_PICK
  return mc_merge(A, B);
}

__device__ __forceinline__ McPart mc_read_row(const McPart& v, int lane) {
  return McPart{readlane_f64(v.n, lane), readlane_f64(v.mean, lane), readlane_f64(v.m2, lane), readlane_f64(v.mn, lane),
                readlane_f64(v.mx, lane), readlane_f64(v.amin, lane), readlane_f64(v.amax, lane), readlane_f64(v.succ, lane),
                readlane_f64(v.steps, lane)};
}

__device__ __forceinline__ McPart mc_wave_reduce(McPart v) {
  v = mc_row_level<1>(v);
  v = mc_row_level<2>(v);
  v = mc_row_level<4>(v);
  v = mc_row_level<8>(v);
  return mc_merge(mc_merge(mc_read_row(v, 0), mc_read_row(v, 16)), mc_merge(mc_read_row(v, 32), mc_read_row(v, 48)));
}

// PS: the plant's parameters are drawn per sample (else the problem's row, wave-uniform);  NZ: process and actuation noise
template <class M, bool PS, bool NZ>
__global__ void __launch_bounds__(64) policy_mc_kernel(
    const double* __restrict__ policy, const double* __restrict__ dist, const double* __restrict__ param_rows,
    const double* __restrict__ cost, const double* __restrict__ x_nom, const double* __restrict__ ulim,
    const double* __restrict__ noise, double* __restrict__ partials, double* __restrict__ samples, double* __restrict__ X,
    double* __restrict__ U, const PolicyMcDims d) {
  constexpr int n = M::n, m = M::m, np = M::n_params, W = n + m + m * n, DW = 3 * n + 2 * np, SW = n + np + 2;
  const int groups = d.r.waves;
  const int b = (int)(blockIdx.x / (unsigned)groups);
  const unsigned gw = blockIdx.x - (unsigned)b * (unsigned)groups;                      // the group inside the window
  const unsigned long long s = ((unsigned long long)d.group0 + gw) * 64ull + threadIdx.x;
  const bool live = s < d.S;
  const size_t sl = (size_t)(live ? s : d.S - 1);              // lanes past a ragged tail shadow the last sample and count for nothing
  const int N = d.r.N;
  const uint32_t g = d.r.first_sample + (uint32_t)sl, cb = d.r.common ? 0u : (uint32_t)b;

  const double* row_d = dist + (size_t)b * DW;                 // x0_mean | x0_spread | goal | p_mean | p_spread
  // The drawn state enters the rollout the way policy_rollout_kernel's loaded one does: one definition per component, in index
  // order, that the compiler cannot look through (an empty asm on the register).  Without it the components reach the time loop in
  // the order the draw's blocks define them, the optimizer orders the operands of the step's commutative operations by that, and
  // a * b + c * d is contracted around the other product: Quad3D and Synth36 costs then differ from policy_rollout_kernel's in
  // the last bits.
  double x_drawn[n], x[n];
  mc_draw<n>(d.r, g, cb, kMcX0Block, d.x0_dist, row_d, row_d + n, x_drawn);
#pragma unroll
  for (int i = 0; i < n; ++i) {
    x[i] = x_drawn[i];
    asm volatile("" : "+v"(x[i]));
  }
  bool alive = true;
#pragma unroll
  for (int i = 0; i < n; ++i) alive = alive && policy_finite(x[i]);

  double p_lane[np > 0 ? np : 1];
  const double* p = param_rows + (size_t)b * d.r.param_stride;
  if constexpr (PS && np > 0) {
    mc_draw<np>(d.r, g, cb, kMcParamBlock, d.p_dist, row_d + 3 * n, row_d + 3 * n + np, p_lane);
    p = p_lane;
  }
  // the sample as drawn - the very registers the rollout starts from - before the rollout overwrites x
  const size_t ws = d.win_samples, sw = sl - (size_t)d.group0 * 64;
  double* const smp = samples ? samples + (size_t)b * SW * ws + sw : nullptr;
  if (samples && live) {
#pragma unroll
    for (int i = 0; i < n; ++i) smp[(size_t)i * ws] = x[i];
#pragma unroll
    for (int j = 0; j < np; ++j) smp[(size_t)(n + j) * ws] = p[j];
  }
  const double* xt = x_nom + (size_t)b * d.r.x_nom_stride;
  double L = 0.0;
  int steps = 0;
  policy_mc_lane_rollout<M, NZ>(x, alive, p, cost + (size_t)b * d.r.cost_stride, xt, ulim ? ulim + (size_t)b * 2 * m : nullptr,
                                policy + (size_t)b * (N - 1) * W, NZ ? noise + (size_t)b * (n + m) : nullptr, g, cb, X, U, live, b,
                                (size_t)d.win_samples, sl - (size_t)d.group0 * 64, d.r, L, steps);

  const bool counted = live && alive && policy_finite(L);
  bool ok = counted;
#pragma unroll
  for (int i = 0; i < n; ++i) ok = ok && fabs(x[i] - xt[i]) <= row_d[2 * n + i];
  const double gd = (double)g;
  McPart v;
  v.n = counted ? 1.0 : 0.0; v.mean = counted ? L : 0.0; v.m2 = 0.0;
  v.mn = counted ? L : INFINITY; v.mx = counted ? L : -INFINITY; v.amin = counted ? gd : -1.0; v.amax = counted ? gd : -1.0;
  v.succ = ok ? 1.0 : 0.0; v.steps = live ? (double)steps : 0.0;
  v = mc_wave_reduce(v);

  if (threadIdx.x == 0) {
    const unsigned long long left = d.S - ((unsigned long long)d.group0 + gw) * 64ull;   // (> 0: the host launches no empty group)
    double* out = partials + (size_t)gw * mi_host::kMcFields * d.B + b;
    const size_t B = (size_t)d.B;
    out[0 * B] = left < 64ull ? (double)left : 64.0;
    out[1 * B] = v.n; out[2 * B] = v.succ; out[3 * B] = v.mean; out[4 * B] = v.m2; out[5 * B] = v.mn; out[6 * B] = v.mx;
    out[7 * B] = v.amin; out[8 * B] = v.amax; out[9 * B] = v.steps;
  }
  if (samples && live) {
    smp[(size_t)(n + np) * ws] = L;
    smp[(size_t)(n + np + 1) * ws] = (double)steps;
  }
}

// One lane per problem: the window's partials (groups, F, B), left to right, into the accumulator (F, B).  first: the accumulator
// starts empty (the call's first window).
template <int F>
__global__ void __launch_bounds__(256) policy_mc_fold_kernel(const double* __restrict__ partials, double* __restrict__ acc, int B,
                                                               int groups, int first) {
  static_assert(F == mi_host::kMcFields, "the layout of a partial");
  const int b = (int)(blockIdx.x * 256u + threadIdx.x);
  if (b >= B) return;
  const size_t Bz = (size_t)B;
  auto load = [&](const double* q, double& count) {
    count = q[0];
    return McPart{q[1 * Bz], q[3 * Bz], q[4 * Bz], q[5 * Bz], q[6 * Bz], q[7 * Bz], q[8 * Bz], q[2 * Bz], q[9 * Bz]};
  };
  double total = 0.0, c;
  McPart a = mc_empty();
  if (!first) a = load(acc + b, total);
  for (int gi = 0; gi < groups; ++gi) {
    const McPart v = load(partials + (size_t)gi * F * Bz + b, c);
    a = mc_merge(a, v);
    total += c;
  }
  double* o = acc + b;
  o[0] = total; o[1 * Bz] = a.n; o[2 * Bz] = a.succ; o[3 * Bz] = a.mean; o[4 * Bz] = a.m2; o[5 * Bz] = a.mn; o[6 * Bz] = a.mx;
  o[7 * Bz] = a.amin; o[8 * Bz] = a.amax; o[9 * Bz] = a.steps;
}
#endif

}  // namespace mi

#if defined(__HIPCC__)
namespace mi_host {

template <class M, bool PS, bool NZ>
int launch_policy_mc_one(mi_ilqr* h, const PolicyMcArgs& a) {
  PolicyMcArgs v = a;
  const PolicyArgs& r = a.r;
  PolicyMcDims d{};
  d.r = PolicyDims{r.param_stride, r.cost_stride, r.x_nom_stride, r.dt, r.N, 0, a.groups, r.m_user,
                   (uint32_t)(r.seed & 0xffffffffull), (uint32_t)(r.seed >> 32), r.first_sample, r.common};
  d.S = a.S; d.win_samples = a.win_samples; d.group0 = a.group0; d.B = r.B; d.x0_dist = a.x0_dist; d.p_dist = a.p_dist;
  void* argv[] = {&v.r.policy, &v.dist, &v.r.param_rows, &v.r.cost, &v.r.x_nom, &v.r.ulim, &v.r.noise, &v.partials, &v.samples, &v.r.X,
                  &v.r.U, &d};
  const unsigned long long blocks = (unsigned long long)a.groups * (unsigned long long)r.B;
  if (blocks > 0x7fffffffull) return MI_ILQR_E_UNSUPPORTED;
  const void* kern = reinterpret_cast<const void*>(policy_mc_kernel<M, PS, NZ>);
  HIPCHK(hipExtLaunchKernel(kern, dim3((unsigned)blocks), dim3(64), argv, 0, h->stream, a.ev0, a.ev1, 0));
  hipLaunchKernelGGL(policy_mc_fold_kernel<kMcFields>, dim3((unsigned)((r.B + 255) / 256)), dim3(256), 0, h->stream,
                     (const double*)a.partials, a.acc, (int)r.B, (int)a.groups, (int)a.first_pass);
  HIPCHK(hipGetLastError());
  return MI_ILQR_OK;
}

template <class M, bool NZ>
int launch_policy_mc_any(mi_ilqr* h, const PolicyMcArgs& a) {
  if (a.r.N < 2 || a.S < 1 || a.r.B < 1 || a.groups < 1 || (a.r.noise != nullptr) != NZ) return MI_ILQR_E_BAD_ARG;
  if constexpr (M::n_params > 0) if (a.sample_params) return launch_policy_mc_one<M, true, NZ>(h, a);
  if (a.sample_params) return MI_ILQR_E_UNSUPPORTED;
  return launch_policy_mc_one<M, false, NZ>(h, a);
}

// the two launchers of a model (host.hpp: model_entry picks by PolicyArgs::noise), instantiated in units of their own: one window of
// groups - the rollout kernel, carrying the window's events, and the fold behind it
template <class M>
int launch_policy_mc(mi_ilqr* h, const PolicyMcArgs& a) { return launch_policy_mc_any<M, false>(h, a); }
template <class M>
int launch_policy_mc_noise(mi_ilqr* h, const PolicyMcArgs& a) { return launch_policy_mc_any<M, true>(h, a); }

}  // namespace mi_host
#endif
