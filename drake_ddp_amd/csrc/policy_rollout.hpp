// Monte-Carlo rollouts of a solved feedback policy (mi_ilqr_policy_rollout): S samples per problem, ONE LANE PER SAMPLE.
//
//   u_t = u_bar_t - K_t (x_t - x_bar_t)  [clamped to the problem's box on a control-limited handle];  x_{t+1} = f(x_t, u_t; p_s, dt)
//   L  += (x_t - x_nom)' Q (x_t - x_nom) + u_t' R u_t;   L += (x_{N-1} - x_nom)' Qf (x_{N-1} - x_nom)          (ilqr.py:313,325,327)
//
// A lane owns a whole plant: x_t lives in its registers and the step is M::step<double> - none of the cooperative step forms of the
// workgroup-per-problem rollouts (one lane per leg / chain / joint) is used.  Every wave serves ONE problem (workgroup = one wave,
// blockIdx.x = problem * waves-per-problem + wave), so everything that belongs to the problem and the time step is wave-uniform: the
// policy row x_bar_t | u_bar_t | K_t, the cost matrices, the target, the bounds and - without per-sample parameters - the plant's
// parameters.  They are read-only kernel arguments the kernel never writes (`const __restrict__`), indexed by uniform values only:
// the compiler reads them through the scalar unit (s_load into SGPRs, an SGPR operand of the v_fma_f64 that uses the value) - one
// fetch per wave instead of 64 identical vector loads, and no vector register per value.  The policy arrives as the call's own
// time-major copy (h_policy.hip: pack_policy), whatever the layout the handle's solver kernels keep it in.
// What differs between lanes is sample-minor in memory - x0 (B, n, S), the per-sample parameters (B, n_params, S), the outputs - so a
// wave's loads and stores are contiguous.
//
// A sample ENDS at a step the model declares infeasible (M::infeasible_velocity, models that can fail) or whose result is not
// finite, and with a non-finite x0 before its first step: its lane stops advancing (`alive`), keeps the last state it held, reports
// the steps it completed and a cost of +inf, and fills the rest of its trajectories with NaN.  All of this is per-lane selects:
// the kernel has no wave-level operation and no early return, so one failing sample changes nothing for its neighbours.
//
// NZ = true - the handle holds a MI_F_POLICY_NOISE row per problem, sigma_x (n) | sigma_u (m) - adds a disturbance at every step:
//   x_{t+1} = f(x_t, u_t + sigma_u o xi^u_t) + sigma_x o xi^x_t,     xi independent standard normals
// The cost and the U output keep the COMMANDED u_t; the disturbance on u comes after the clamp and is not clamped; the finite and
// infeasible checks see the noisy x_{t+1}.  The normals are generated where they are used, per lane and step, in registers
// (philox.hpp): component i of the state is word i mod 4 of the Philox block with counter (first_sample + s, t, common ? 0 : b, i / 4),
// component k of the control word k mod 4 of block 256 + k / 4, under the key (seed mod 2^32, seed div 2^32) - a normal depends on
// (seed, b, s, t, component) and on nothing else, not on S and not on the launch.  The sigma row is wave-uniform and read through
// the scalar unit like the other rows; a stream whose sigmas are all zero for the problem is skipped (a uniform branch).  NZ = false
// is the kernel without any of it.  The instantiations live in two units: k_policy.hip (NZ = false) and k_policy_noise.hip.
#pragma once
#include "fastmath.hpp"
#include "host.hpp"           // mi_ilqr, PolicyArgs, HIPCHK
#include "model_traits.hpp"   // CanFail
#include "models.hpp"
#include "philox.hpp"

namespace mi {

struct PolicyDims {
  size_t param_stride, cost_stride, x_nom_stride;
  double dt;
  int32_t N, S, waves, m_user;
  uint32_t seed_lo, seed_hi, first_sample;   // NZ kernels: the Philox key and the number of the call's sample 0
  int32_t common;                            // ... and whether every problem gets the same normals
};

__device__ __forceinline__ bool policy_finite(double v) { return v - v == 0.0; }      // (false for NaN and +-inf)

// PS: per-sample model parameters (a row per lane, in registers) instead of the problem's row (wave-uniform)
// NZ: process and actuation noise (`noise`: the problem's sigma row)
template <class M, bool PS, bool NZ>
__global__ void __launch_bounds__(64) policy_rollout_kernel(
    const double* __restrict__ policy, const double* __restrict__ x0, const double* __restrict__ params,
    const double* __restrict__ param_rows, const double* __restrict__ cost, const double* __restrict__ x_nom,
    const double* __restrict__ ulim, const double* __restrict__ noise, double* __restrict__ cost_out, double* __restrict__ x_final, int32_t* __restrict__ steps_out,
    double* __restrict__ X, double* __restrict__ U, const PolicyDims d) {
  constexpr int n = M::n, m = M::m, np = M::n_params, W = n + m + m * n;
  const int b = (int)(blockIdx.x / (unsigned)d.waves);
  const int s = (int)(blockIdx.x - (unsigned)b * (unsigned)d.waves) * 64 + (int)threadIdx.x;
  const bool live = s < d.S;
  const size_t S = (size_t)d.S, sl = live ? (size_t)s : S - 1;     // lanes past a ragged tail shadow the last sample and store nothing
  const int N = d.N;

  double x[n];
#pragma unroll
  for (int i = 0; i < n; ++i) x[i] = x0[((size_t)b * n + i) * S + sl];
  bool alive = true;
#pragma unroll
  for (int i = 0; i < n; ++i) alive = alive && policy_finite(x[i]);

  double p_lane[np > 0 ? np : 1];
  const double* p = param_rows + (size_t)b * d.param_stride;
  if constexpr (PS && np > 0) {
#pragma unroll
    for (int j = 0; j < np; ++j) p_lane[j] = params[((size_t)b * np + j) * S + sl];
    p = p_lane;
  }
  const double* Q = cost + (size_t)b * d.cost_stride;
  const double* R = Q + n * n;
  const double* Qf = R + m * m;
  const double* xt = x_nom + (size_t)b * d.x_nom_stride;
  const double* lim = ulim ? ulim + (size_t)b * 2 * m : nullptr;
  const double* row = policy + (size_t)b * (N - 1) * W;
  const double nan = __builtin_nan("");
  // NZ: the problem's sigma row and which of its two streams has a non-zero entry (wave-uniform)
  const double* sg = nullptr;
  bool noise_x = false, noise_u = false;
  uint32_t ctr_s = 0, ctr_b = 0;
  if constexpr (NZ) {
    sg = noise + (size_t)b * (n + m);
#pragma unroll
    for (int i = 0; i < n; ++i) noise_x = noise_x || sg[i] != 0.0;
#pragma unroll
    for (int k = 0; k < m; ++k) noise_u = noise_u || sg[n + k] != 0.0;
    ctr_s = d.first_sample + (uint32_t)sl;
    ctr_b = d.common ? 0u : (uint32_t)b;
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
  if (live) {
    cost_out[(size_t)b * S + sl] = L;
    if (steps_out) steps_out[(size_t)b * S + sl] = steps;
    if (x_final) {
#pragma unroll
      for (int i = 0; i < n; ++i) x_final[((size_t)b * n + i) * S + sl] = x[i];
    }
  }
}

}  // namespace mi

namespace mi_host {

template <class M, bool PS, bool NZ>
int launch_policy_rollout_one(mi_ilqr* h, const PolicyArgs& a) {
  PolicyArgs v = a;
  PolicyDims d{a.param_stride, a.cost_stride, a.x_nom_stride, a.dt, a.N, a.S, (a.S + 63) / 64, a.m_user,
               (uint32_t)(a.seed & 0xffffffffull), (uint32_t)(a.seed >> 32), a.first_sample, a.common};
  void* argv[] = {&v.policy, &v.x0, &v.params, &v.param_rows, &v.cost, &v.x_nom, &v.ulim, &v.noise, &v.cost_out, &v.x_final, &v.steps, &v.X, &v.U, &d};
  const unsigned long long blocks = (unsigned long long)d.waves * (unsigned long long)a.B;
  if (blocks > 0x7fffffffull) return MI_ILQR_E_UNSUPPORTED;
  const void* kern = reinterpret_cast<const void*>(policy_rollout_kernel<M, PS, NZ>);
  // (the launch carries the handle's policy events itself: launch_timed's form, with the pair that belongs to this entry)
  HIPCHK(hipExtLaunchKernel(kern, dim3((unsigned)blocks), dim3(64), argv, 0, h->stream, h->policy_ev0, h->policy_ev1, 0));
  return MI_ILQR_OK;
}

template <class M, bool NZ>
int launch_policy_rollout_any(mi_ilqr* h, const PolicyArgs& a) {
  if (a.N < 2 || a.S < 1 || a.B < 1 || (a.noise != nullptr) != NZ) return MI_ILQR_E_BAD_ARG;
  if constexpr (M::n_params > 0) if (a.params != nullptr) return launch_policy_rollout_one<M, true, NZ>(h, a);
  if (a.params != nullptr) return MI_ILQR_E_UNSUPPORTED;
  return launch_policy_rollout_one<M, false, NZ>(h, a);
}

// the two launchers of a model (host.hpp: model_entry picks by PolicyArgs::noise), instantiated in units of their own
template <class M>
int launch_policy_rollout(mi_ilqr* h, const PolicyArgs& a) { return launch_policy_rollout_any<M, false>(h, a); }
template <class M>
int launch_policy_rollout_noise(mi_ilqr* h, const PolicyArgs& a) { return launch_policy_rollout_any<M, true>(h, a); }

}  // namespace mi_host
