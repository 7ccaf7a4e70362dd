// The plant of the closed receding-horizon loop (mi_ilqr_mpc_run on a handle that holds MI_F_PLANT_STATE): every problem's own plant
// advanced `steps` = replan_steps steps under the policy the handle holds, ONE LANE PER PROBLEM, between two re-solves.
//
//   u_j = u_bar_j - K_j (x - x_bar_j)   [u_bar_j alone with feedback off; clamped to the problem's box on a control-limited handle]
//   x  <- f(x, u_j + sigma_u o xi^u_k; plant parameters of b, dt) + sigma_x o xi^x_k,      k = clock + j
//   log row k = x_k | u_k (commanded) | l_k,   l_k = (x_k - x_nom_b)' Q_b (x_k - x_nom_b) + u_k' R_b u_k
//
// Contrast with policy_rollout.hpp, where a wave serves one problem and reads the policy through the scalar unit: here a lane IS a
// problem, so the policy row, the cost matrices, the target, the bounds, the sigmas and the parameters all differ between lanes and
// nothing is wave-uniform.  The host stages them PROBLEM-MINOR (h_policy.hip: pack_policy; h_mpc.hip: rows_to_cols_kernel): element e of
// problem b at e * B + b, so that a wave's load of one element is a contiguous run of 64 doubles.  The log is written problem-minor
// too and transposed once when it is read out.  The plant state itself is the (B, n) array the selector exposes: n loads and n
// stores per lane and launch.
//
// The state stays in the lane's registers, the step is M::step<double> - none of the cooperative step forms.  A plant ENDS at a step
// the model declares infeasible (models that can fail) or whose result is not finite - the rule of the policy rollouts, applied to
// the noisy x_{k+1}: the lane stops advancing (`alive`), keeps its last state, logs x_k | NaN | NaN for the step that failed and NaN
// rows after it, and marks its problem in `dead` (kept across launches) and in the MPC log's flags.  All per-lane selects: no LDS,
// no wave-level operation, no early return; lanes past a ragged tail shadow the last problem and store nothing.  `feedback` and the
// bounds are run-time branches every lane takes alike.
//
// NZ = true - the handle holds a MI_F_PLANT_NOISE row per problem - adds the disturbances.  The normals are those of sample 0 of a
// policy rollout at step t = k (philox.hpp; policy_rollout.hpp): counter (0, k, common ? 0 : b, block), state component i in word
// i mod 4 of block i / 4, control component c in word c mod 4 of block 256 + c / 4.  The disturbance on u comes after the clamp and
// is not clamped; the log keeps the COMMANDED control.  A stream whose sigmas are all zero for a problem is skipped by its lane.
// The instantiations live in two units: k_plant.hip (NZ = false) and k_plant_noise.hip.
#pragma once
#include "fastmath.hpp"
#include "host.hpp"           // mi_ilqr, PlantArgs, HIPCHK
#include "model_traits.hpp"   // CanFail
#include "models.hpp"
#include "philox.hpp"

namespace mi {

__device__ __forceinline__ bool plant_finite(double v) { return v - v == 0.0; }      // (false for NaN and +-inf)

template <class M, bool NZ>
__global__ void __launch_bounds__(64) plant_advance_kernel(const mi_host::PlantArgs a) {
  constexpr int n = M::n, m = M::m, np = M::n_params, W = n + m + m * n, C = n + m + 1;
  constexpr int kRowUnrollU = m * n <= 64 ? m : 1, kRowUnrollQ = n <= 8 ? n : 1;
  const int b = (int)(blockIdx.x * 64u + threadIdx.x);
  const bool live = b < a.B;
  const size_t B = (size_t)a.B, bl = live ? (size_t)b : B - 1;     // lanes past a ragged tail shadow the last problem and store nothing

  double x[n];
#pragma unroll
  for (int i = 0; i < n; ++i) x[i] = a.x[bl * n + i];
  bool alive = a.dead[bl] == 0.0;
#pragma unroll
  for (int i = 0; i < n; ++i) alive = alive && plant_finite(x[i]);

  double p[np > 0 ? np : 1];
  p[0] = 0.0;
#pragma unroll
  for (int j = 0; j < np; ++j) p[j] = a.params[(size_t)j * B + bl];

  const double* const Q = a.cost + bl;                   // element e of the lane's Q | R at Q[e * B]
  const double* const R = Q + (size_t)(n * n) * B;
  const double* const xt = a.x_nom + bl;
  const double* const lim = a.ulim ? a.ulim + bl : nullptr;
  const double nan = __builtin_nan("");
  // NZ: which of the lane's two streams has a non-zero sigma
  const double* sg = nullptr;
  bool noise_x = false, noise_u = false;
  uint32_t ctr_b = 0;
  if constexpr (NZ) {
    sg = a.noise + bl;
#pragma unroll
    for (int i = 0; i < n; ++i) noise_x = noise_x || sg[(size_t)i * B] != 0.0;
#pragma unroll
    for (int k = 0; k < m; ++k) noise_u = noise_u || sg[(size_t)(n + k) * B] != 0.0;
    ctr_b = a.common ? 0u : (uint32_t)bl;
  }
  const uint32_t seed_lo = (uint32_t)(a.seed & 0xffffffffull), seed_hi = (uint32_t)(a.seed >> 32);

  const double* row = a.policy + bl;                     // element w of step j's row x_bar_j | u_bar_j | K_j at row[w * B]
  double* lg = a.log + bl;                               // entry c of this launch's log row j at lg[(j * C + c) * B]
  for (int j = 0; j < a.steps; ++j, row += (size_t)W * B, lg += (size_t)C * B) {
    double u[m], xn[n];
    {
      double dx[n];
#pragma unroll
      for (int i = 0; i < n; ++i) dx[i] = x[i] - row[(size_t)i * B];
      // (large models: one control after the other, like the rows of Q below - unrolled, the loads of the whole gain matrix and of
      //  Q, per lane here, would all be hoisted and spilled)
#pragma unroll kRowUnrollU
      for (int k = 0; k < m; ++k) {
        double uk = row[(size_t)(n + k) * B];
        if (a.feedback) {
          double acc = 0.0;
#pragma unroll
          for (int i = 0; i < n; ++i) acc += row[(size_t)(n + m + k * n + i) * B] * dx[i];
          uk -= acc;
        }
        if (lim) {                                                  // (comparisons, not fmin / fmax: a NaN stays one, like np.clip)
          const double lo = lim[(size_t)k * B], hi = lim[(size_t)(m + k) * B];
          uk = uk < lo ? lo : (uk > hi ? hi : uk);
        }
        u[k] = k < a.m_user ? uk : 0.0;
      }
    }
    // stage cost at (x_k, u_k), no 1/2 factor - before the step, while x_{k+1} is not live yet
    double lk = 0.0;
    {
      double dx[n];
#pragma unroll
      for (int i = 0; i < n; ++i) dx[i] = x[i] - xt[(size_t)i * B];
#pragma unroll kRowUnrollQ
      for (int i = 0; i < n; ++i) {
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < n; ++q) acc += Q[(size_t)(i * n + q) * B] * dx[q];
        lk += dx[i] * acc;
      }
#pragma unroll
      for (int k = 0; k < m; ++k) {
        double acc = 0.0;
#pragma unroll
        for (int l = 0; l < m; ++l) acc += R[(size_t)(k * m + l) * B] * u[l];
        lk += u[k] * acc;
      }
    }
    if constexpr (NZ) {
      const uint32_t clk = a.clock + (uint32_t)j;
      double ua[m];                                                 // the control the plant gets (padding: sigma = 0, the host saw to it)
#pragma unroll
      for (int k = 0; k < m; ++k) ua[k] = u[k];
      if (noise_u) {
#pragma unroll
        for (int q = 0; q < (m + 3) / 4; ++q) {
          double z[4];
          philox_normals(seed_lo, seed_hi, 0u, clk, ctr_b, 256u + q, m - 4 * q > 2, z);
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (4 * q + c < m) ua[4 * q + c] = u[4 * q + c] + sg[(size_t)(n + 4 * q + c) * B] * z[c];
        }
      }
      M::template step<double>(x, ua, xn, p, a.dt);
      if (noise_x) {
#pragma unroll
        for (int q = 0; q < (n + 3) / 4; ++q) {
          double z[4];
          philox_normals(seed_lo, seed_hi, 0u, clk, ctr_b, (uint32_t)q, n - 4 * q > 2, z);
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (4 * q + c < n) xn[4 * q + c] += sg[(size_t)(4 * q + c) * B] * z[c];
        }
      }
    } else {
      M::template step<double>(x, u, xn, p, a.dt);
    }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < n; ++i) ok = ok && plant_finite(xn[i]);
    if constexpr (CanFail<M>::value) {
#pragma unroll
      for (int i = M::nq; i < n; ++i) ok = ok && !M::infeasible_velocity(xn[i], p);
    }
    const bool was_alive = alive;
    alive = alive && ok;
    if (live) {
#pragma unroll
      for (int i = 0; i < n; ++i) lg[(size_t)i * B] = was_alive ? x[i] : nan;
#pragma unroll
      for (int k = 0; k < m; ++k) lg[(size_t)(n + k) * B] = alive ? u[k] : nan;
      lg[(size_t)(n + m) * B] = alive ? lk : nan;
    }
#pragma unroll
    for (int i = 0; i < n; ++i) x[i] = alive ? xn[i] : x[i];
  }
  if (live) {
#pragma unroll
    for (int i = 0; i < n; ++i) a.x[bl * n + i] = x[i];
    a.dead[bl] = alive ? 0.0 : 1.0;
    if (!alive) a.mpc_dead[bl] = 1.0;
  }
}

}  // namespace mi

namespace mi_host {

template <class M, bool NZ>
int launch_plant_advance_any(mi_ilqr* h, const PlantArgs& a) {
  if (a.B < 1 || a.steps < 1 || (a.noise != nullptr) != NZ) return MI_ILQR_E_BAD_ARG;
  PlantArgs v = a;
  void* argv[] = {&v};
  const void* kern = reinterpret_cast<const void*>(mi::plant_advance_kernel<M, NZ>);
  // (the launch carries the handle's plant events itself: launch_timed's form, with the pair that belongs to the plant)
  HIPCHK(hipExtLaunchKernel(kern, dim3((unsigned)((a.B + 63) / 64)), dim3(64), argv, 0, h->stream, h->plant_ev0, h->plant_ev1, 0));
  return MI_ILQR_OK;
}

// the two launchers of a model (host.hpp: model_entry picks by PlantArgs::noise), instantiated in units of their own
template <class M>
int launch_plant_advance(mi_ilqr* h, const PlantArgs& a) { return launch_plant_advance_any<M, false>(h, a); }
template <class M>
int launch_plant_advance_noise(mi_ilqr* h, const PlantArgs& a) { return launch_plant_advance_any<M, true>(h, a); }

}  // namespace mi_host
