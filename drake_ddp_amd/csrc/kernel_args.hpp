// What crosses the launch boundary: the argument block every solve kernel takes by value (KArgs), the kernel modes, the per-solve
// statistics record, and the accessors that say where a problem's target, cost matrices and model parameters live.  Shared by the
// host (host.hpp, the host units) and by every kernel family; knows no model and no key-point code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mi_ilqr.h"

namespace mi {

enum KernelMode { MODE_SOLVE = 0, MODE_ROLLOUT = 1, MODE_FORWARD = 2, MODE_LINEARIZE = 3, MODE_BACKWARD = 4, MODE_MPC = 5 };

constexpr int kMaxStateDim = 40;   // largest model state (Synth36: 36), for by-value kernel arguments

// Per-solve aggregate over the batch, written into pinned, device-mapped host memory (one small host
// read after a blocking solve instead of four D2H copies).
struct DevStats {
  long long total_iters, total_ls;
  int n_conv, n_max, n_fail, max_iters_seen, best_index, n_internal, n_not_pd, pad_;
  double best_cost;
};

constexpr int kSyncWords = MI_ILQR_CLUSTER_WORDS;      // (= 40) 64-bit handshake words per problem (KArgs::cluster_sync): 8 + the costs of 4 x 7 line-search candidates
struct KArgs {
  // persistent per-problem solver state, reference layout with a leading batch axis
  double *x_bar, *u_bar, *K, *kappa, *dV, *fx, *fu;
  const double* x0;        // (B,n)
  const double* u_guess;   // (B,m,N-1) pending SetInitialGuess input (used when u_pending)
  double* cost;            // (B,)
  double* hist;            // (B,hist_cap,4)
  double* iter_cyc;        // (B,hist_cap,4) per-iteration stopwatches: line search, linearization, backward pass, whole iteration (cycles)
  double *x_trial, *u_trial, *trial_cost;   // stage outputs
  const double* stage_in;  // (B,) eps (ROLLOUT) or L_last (FORWARD)
  const double* costmat;   // Q[n*n] R[m*m] Qf[n*n] x_nom[n]
  int32_t *iters, *status, *ls_trials, *kp_count, *kp_list;
  long long* prof;         // (B,4) shader-clock cycles: line search, linearization, backward pass, whole solve
  double params[MI_ILQR_MAX_PARAMS];
  double dt, delta, beta, gamma, jerk_thr, err_thr, fd_h;
  int32_t N, B, kp_method, minN, maxN, max_iters, hist_cap;
  int32_t n_store;    // line-search candidates whose trajectories are kept in LDS (>= 1)
  int32_t cold;       // 1: persistent state is all-zero, do not read it
  int32_t u_pending;  // 1: take u_bar from u_guess
  // MODE_MPC: receding-horizon loop kept on the device (acrobot.py:145-155, mini_cheetah.py:190-201)
  int32_t mpc_resolves, mpc_replan;
  double mpc_target_step[kMaxStateDim];   // added to x_nom before every re-solve (mini_cheetah.py:151-156); zeros = fixed target
  double* mpc_log;             // (B, mpc_resolves, n+2): x0 of the re-solve | cost | iterations
  int32_t helpers;             // extra wavefronts per problem that share the linearization (0, 1 or 3), see ilqr_small_kernel
  int32_t seq_backward;        // 0: fastest backward pass; 1: sequential sweep (A/B measurements); 2: the reference's scalar recursion verbatim (asymmetric / indefinite costs)
  int32_t newton_rollout;      // 1: the eps = 1 trial is rolled out parallel in time (Newton on the trajectory) when it converges
  // MODE_SOLVE / MODE_MPC of the wave-per-problem kernels: the last workgroup to finish aggregates the
  // batch statistics itself (no second kernel per solve).  Null: the host launches stats_kernel.
  DevStats* stats_out;
  int32_t* done_counter;       // zero between launches
  // workgroup-per-problem kernels, MODE_SOLVE / MODE_MPC with every step a key-point: `cluster` workgroups per
  // problem - one leader that runs the solve and cluster-1 helpers that share its linearizations
  // (ilqr_large.hpp: cluster handshake).  cluster_sync: kSyncWords 64-bit words per problem, zero at launch.
  // cluster: bits 0-7 workgroups per problem, bits 8-9 their placement (0: consecutive blocks, a cluster spans XCDs; 1, 2: all on
  // one XCD), bit 10: early linearization (the helpers linearize the line search's first trial while it is being rolled out),
  // bit 11: candidate groups (mid-size kernels: the helpers roll out line-search candidates 4 .. beside the leader's four).
  int32_t cluster;
  unsigned long long* cluster_sync;
  // wave-per-problem kernels: optional RESULT SINK (mi_ilqr_set_result_sink) - device-visible, page-locked HOST arrays
  // that receive x_bar (B,n,N), u_bar (B,m,N-1) and the costs (B,) straight from the kernel's write-back, problem by
  // problem as each one finishes: the copy-out of a batch overlaps the launch's stragglers instead of following it.
  double *sink_x, *sink_u, *sink_cost;
  // lane-per-problem kernels with key-points (ilqr_batch.hpp, KP = true): 6 (N-1) x B ints, batch-minor - the lanes' key-point
  // lists, "derivative evaluated" flags and the two bin buffers of the iterative-error bisection
  int32_t* bm_scratch;
  // mid-size workgroup-per-problem kernels (ilqr_large.hpp: mid_rollout4): trial trajectories of the line-search candidates
  // rolled out beside the first, [3][B][N][n] and [3][B][N-1][m]
  double *x_spec, *u_spec;
  int spec_policy;
  // workgroup-per-problem kernels, long horizons: the cost gradients [B][N-1][n+m] in HBM instead of LDS (ilqr_large.hpp)
  double* lxu;
  int pd_continue;                // mi_ilqr_desc.on_indefinite
  int cost_asym;                  // workgroup-per-problem kernels, n <= 32: Q, R or Qf is not symmetric (mi_ilqr_set_cost)
  // control limits (mi_ilqr_set_control_limits; read by the Limited<M> kernels only): (B, 2, m) - u_min | u_max per problem -
  // and S2 = sum_t kappa_t^T Quu_t kappa_t of each problem's last backward pass, (B,), the quadratic term of the expected improvement
  const double* ulim;
  double* s2;
  // per-problem targets (mi_ilqr_set MI_F_X_NOM / MI_F_TARGET_STEP), (B, n) each: x_nom of problem b is row b of x_nom_rows instead
  // of the costmat's shared one, and MODE_MPC adds row b of target_steps (instead of mpc_target_step) before every re-solve.
  // Null: the shared target.
  const double* x_nom_rows;
  const double* target_steps;
  // per-problem model parameters (mi_ilqr_set MI_F_MODEL_PARAMS): the plant of problem b is row b of param_rows instead of `params`.
  // Rows are DENSE: (B, n_params), the row stride is the model's n_params doubles - what mi_ilqr_device_ptr hands out.  The
  // lane-per-problem kernels read param_cols, the same values batch-minor, (n_params, B): a wave's load of parameter k is one
  // coalesced transaction.  Null (both): the shared `params`.  Neither array is written while a kernel runs.
  const double* param_rows;
  const double* param_cols;
  // per-problem cost matrices (mi_ilqr_set MI_F_COST_MATRICES): Q | R | Qf of problem b is row b of cost_rows instead of the head of
  // `costmat` (x_nom stays where the targets put it: x_nom_of).  Rows are DENSE: (B, 2 n^2 + m^2).  The lane-per-problem kernels read
  // cost_cols, the same values batch-minor, (2 n^2 + m^2, B).  Null (both): the shared matrices.  seq_backward / cost_asym carry the
  // class of the most general row.  Neither array is written while a kernel runs.
  const double* cost_rows;
  const double* cost_cols;
  // reference trajectories (mi_ilqr_set MI_F_X_REF / MI_F_REF_CLOCK; workgroup-per-problem kernels only): (B, ref_T, n) rows.  While
  // x_ref is not null, every place a solve uses x_nom at time index t uses row min(ref_clock + t, ref_T - 1) of problem b instead
  // (ilqr_large.hpp: ref_at); MODE_MPC moves the clock by mpc_replan before every re-solve.  ref_qn: (B, N-1, n) scratch the kernel fills with
  // 2 r_t^T Q of the window it solves on - what the backward passes subtract per step where oQn serves a constant target.
  // Null: x_nom.  x_ref is not written while a kernel runs.
  const double* x_ref;
  double* ref_qn;
  int32_t ref_T, ref_clock;
};

// Where problem b's target lives: row b of the per-problem targets, else the shared one in the costmat (Q | R | Qf | x_nom).
template <int n, int m>
__device__ __forceinline__ const double* x_nom_of(const KArgs& a, size_t b) {
  return a.x_nom_rows ? a.x_nom_rows + b * n : a.costmat + 2 * n * n + m * m;
}
// Where problem b's Q | R | Qf live: row b of the per-problem cost matrices, else the head of the shared costmat.  Like x_nom_of: b is
// uniform for the wave, both arms are global pointers out of the kernel arguments, the reads stay scalar loads.
template <int n, int m>
__device__ __forceinline__ const double* cost_of(const KArgs& a, size_t b) {
  return a.cost_rows ? a.cost_rows + b * (2 * n * n + m * m) : a.costmat;
}
// Problem b's per-re-solve step of the MPC target, component i.
template <int n>
__device__ __forceinline__ double target_step_of(const KArgs& a, size_t b, int i) {
  return a.target_steps ? a.target_steps[b * n + i] : a.mpc_target_step[i];
}

// The model parameters of problem b as VALUES: row b of the per-problem rows, else the shared copy in the kernel arguments.  b is
// uniform for the wave (a wave or a workgroup serves one problem): the row is read through the constant address space - scalar
// loads into scalar registers, where the shared copy lives too - once, by whoever constructs this, and handed on as values.  No
// pointer ever selects between the two sources (that would be a generic-address-space or a scratch access).
typedef const double __attribute__((address_space(4))) * const_row_t;
template <class M>
struct ModelParams {
  double v[M::n_params > 0 ? M::n_params : 1];
  // row: this problem's row of KArgs::param_rows, or nullptr
  __device__ __forceinline__ ModelParams(const KArgs& a, const double* row) {
    if (row != nullptr) {
      const const_row_t r = (const_row_t)row;
#pragma unroll
      for (int i = 0; i < M::n_params; ++i) v[i] = r[i];
    } else {
#pragma unroll
      for (int i = 0; i < M::n_params; ++i) v[i] = a.params[i];
    }
    if constexpr (M::n_params == 0) v[0] = 0.0;
  }
};
template <class M>
__device__ __forceinline__ const double* param_row_of(const KArgs& a, size_t b) {
  return a.param_rows ? a.param_rows + b * M::n_params : nullptr;
}

}  // namespace mi
