// Host-side pieces shared by the translation units of libmi_ilqr.so: the handle, the error macro and the
// kernel-launch templates.  mi_ilqr.hip and the h_<concern>.hip units hold the C ABI (what only they share: host_internal.hpp);
// every model's kernels are instantiated in their own k_<model>.hip (built in parallel, drake_ddp_amd/build.py), reached through the model's launch entry (launch_entry below).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/mi_ilqr.h"
#include "kernel_args.hpp"   // KArgs, KernelMode, DevStats, kMaxStateDim

// library-internal: hidden from the dynamic symbol table (the C ABI is mi_ilqr.h)
#define MI_INTERNAL __attribute__((visibility("hidden")))

// One per-problem (B, width) array of a handle (mi_ilqr_set MI_F_X_NOM / MI_F_TARGET_STEP / MI_F_MODEL_PARAMS / MI_F_COST_MATRICES /
// MI_F_POLICY_NOISE / MI_F_PLANT_STATE / MI_F_PLANT_PARAMS / MI_F_PLANT_NOISE;
// h_memory.hip: store_upload / store_drop / store_read).  The host mirror is the truth: what mi_ilqr_get returns without touching the
// stream and what mi_ilqr_mpc_run advances; the device copies follow it on the handle's stream.  `synced` - they equal it - is the
// array's per-problem mode: only then do the kernels get the pointers, a failed copy leaves the mode, and rows the caller repeats
// (Solve() pushes them on every call) are not sent again.  The buffers are allocated on first use and kept when the mode is
// dropped, so a handle that alternates between the modes allocates once.  Problem data: mi_ilqr_reset keeps the rows.
struct RowStore {
  size_t width = 0;                // doubles per problem
  bool batch_minor_copy = false;   // `cols` exists: lane-per-problem handles, the arrays their kernels read per lane
  double *rows = nullptr, *cols = nullptr;   // (B, width) dense; the same values batch-minor, (width, B)
  std::vector<double> mirror;
  bool synced = false;
};

// A solve slot ("Solve slots"): one set of the arrays a MODE_SOLVE launch of the wave-per-problem kernels writes, and
// the stream it runs on.  Slot 0 is what mi_ilqr_create allocates; slot 1 is allocated by the first cold pipelined solve that has a
// solve in flight to overlap with (mi_ilqr.hip: ensure_second_slot).
struct SolveSlot {
  double *x_bar = nullptr, *u_bar = nullptr, *K = nullptr, *kappa = nullptr, *dV = nullptr, *fx = nullptr, *fu = nullptr;
  double *hist = nullptr, *iter_cyc = nullptr, *s2 = nullptr;
  long long* prof = nullptr;
  int32_t *kp_count = nullptr, *kp_list = nullptr, *done_counter = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev = nullptr;         // "everything enqueued on this slot's stream so far" for the other stream to wait on
};

// The two device copies of an input of mi_ilqr_set_initial (x0, u_guess): copy i is what a solve on slot i reads.  `version` says
// which writes a copy holds (-1: nothing to vouch for), `latest` the copy written last - what the handle's x0 / u_guess alias.
struct InputCopies {
  double* copy[2] = {nullptr, nullptr};
  long long version[2] = {0, -1};
  long long writes = 0;
  int latest = 0;
  bool read_across[2] = {false, false};   // copy i was read by a device copy on the OTHER slot's stream since it was written
};

struct mi_ilqr {
  mi_ilqr_desc d;
  int n, m, N, B;
  // the stream of the CURRENT solve slot (slots[solve_slot].stream): what every entry point but a pipelined cold solve works on
  hipStream_t stream = nullptr;
  // Solve slots.  The state fields below (x_bar .. fu, hist, iter_cyc, prof, kp_count, kp_list, done_counter, s2) and `stream`
  // alias the current slot (select_solve_slot), like ev0 .. ls_trials alias the current ring slot.
  SolveSlot slots[2];
  int n_slots = 1;                 // MI_ILQR_SOLVE_SLOTS (1: the single-slot behaviour), 2 for the wave-per-problem family
  int solve_slot = 0;              // the current slot: that of the solve enqueued last
  bool second_slot_ready = false;
  bool other_pending = false;      // the other slot's stream holds work the current stream is not ordered behind
  bool fork_needed = true;         // the current stream may hold work the other stream is not ordered behind
  int hold = 0;                    // > 0: inside an entry point whose launches all stay on the current slot (SlotHold)
  int inflight = 0;                // solves enqueued since the host last waited for the handle
  InputCopies in_x0, in_u;
  double* u_one_copy[2] = {nullptr, nullptr};   // device copies of a shared (m, N-1) initial guess, one per slot's stream
  // Per-launch records (kernel start/stop events + aggregate statistics) live in a ring, so that up to
  // kStatsRing solves can be enqueued back to back (mi_ilqr_solve_async) before anything is collected;
  // ev0/ev1/h_stats/d_stats alias the slot of the most recent launch.
  static constexpr int kStatsRing = 32;
  hipEvent_t ring_ev0[kStatsRing] = {}, ring_ev1[kStatsRing] = {};
  mi::DevStats* h_ring = nullptr;    // pinned host memory, device-mapped
  mi::DevStats* d_ring = nullptr;    // its device alias
  long long seq = 0;             // solves enqueued so far
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  unsigned long long seq_timed = 0;
  int time_every = 1;              // mi_ilqr_set_timing: events on one solve in `time_every` (0 = never)
  bool timed_launch = true;        // this launch carries the events
  bool last_timed = true;          // ... and so did the most recent launch
  int cur_slot = 0;
  bool ring_timed[kStatsRing] = {};
  // double fields
  double *x_bar = nullptr, *u_bar = nullptr, *K = nullptr, *kappa = nullptr, *dV = nullptr, *fx = nullptr, *fu = nullptr;
  double *x0 = nullptr, *u_guess = nullptr, *cost = nullptr, *hist = nullptr, *iter_cyc = nullptr;
  double *x_trial = nullptr, *u_trial = nullptr, *trial_cost = nullptr, *stage_in = nullptr, *costmat = nullptr;
  int32_t *iters = nullptr, *status = nullptr, *ls_trials = nullptr, *kp_count = nullptr, *kp_list = nullptr;
  // cost / iters / status / ls_trials above alias the CURRENT slot of these rings (kStatsRing x B each): every
  // pipelined solve leaves its per-problem results in its own slot, so their reduction to a DevStats record can
  // wait until somebody collects - one stats_kernel launch over all pending slots - instead of one dispatch
  // (6 us + its gap) behind every solve.
  double* cost_ring = nullptr;
  int32_t *iters_ring = nullptr, *status_ring = nullptr, *ls_ring = nullptr;
  long long stats_done = 0;      // solves with sequence number < stats_done have their DevStats record
  bool in_async_solve = false;
  char* pin_in = nullptr;          // page-locked staging ring of small host -> device inputs (stage_h2d)
  size_t pin_off = 0;
  hipEvent_t pin_ev[2] = {nullptr, nullptr};   // the last staged copy on each solve slot's stream
  long long* prof = nullptr;
  int32_t* done_counter = nullptr;   // wave-per-problem kernels: tickets of the in-kernel statistics epilogue
  mi::DevStats* h_stats = nullptr;   // pinned host memory, device-mapped
  mi::DevStats* d_stats = nullptr;   // its device alias
  double* mpc_log = nullptr;     // (B, mpc_log_resolves, n+2)
  int mpc_log_resolves = 0;
  int mpc_resolves = 0, mpc_replan = 0;
  double mpc_target_step[mi::kMaxStateDim] = {};
  bool cold = true;        // persistent state is known to be all zero (fresh object / after reset)
  bool u_pending = false;  // SetInitialGuess input waiting in u_guess
  bool u_zero = false;     // u_bar is to read as all zero (after reset, until a guess is set or re-armed): ilqr.py:71
  int exact_backward = 0;  // cost matrices the fast backward forms do not cover (asymmetric / indefinite): reference recursion
  // tiny batches (B <= 4): the per-solve records - iteration log, stopwatches, iterations, status - live in page-locked host memory the
  // kernels write directly (hist, iter_cyc, prof, iters_ring, status_ring point into it): mi_ilqr_solve_into reads them with a memcpy
  // after the solve's one synchronization instead of five device-to-host copies queued behind the kernel (~5 us each)
  char* host_records = nullptr;       // host address of the block (hipHostMalloc, mapped)
  char* host_records_dev = nullptr;   // the same block as the device sees it
  size_t host_records_bytes = 0;
  bool host_inputs = false;           // x0 and u_guess live in the block too (B <= 4, wave-per-problem kernels)
  int cost_asym = 0;       // workgroup-per-problem kernels, n <= 32: Q, R or Qf is not symmetric (mid_backward then uses no symmetry at all)
  std::vector<double> h_costmat;   // host mirror of costmat (Q | R | Qf | x_nom)
  bool costmat_synced = false;     // the device copy equals the mirror
  unsigned long long* cluster_sync = nullptr;   // workgroup-per-problem kernels: kSyncWords handshake words per problem
  bool last_clustered = false;     // the last MODE_SOLVE / MODE_MPC launch shared its linearizations among clusters (else MI_I64_CLUSTER_WORDS reads as zeros)
  int n_cus = 0;                   // compute units of the device
  double* scratch = nullptr;       // device staging area of the boundary's layout conversions (grow-only)
  size_t scratch_bytes = 0;
  size_t lds = 0;
  bool large = false;      // workgroup-per-problem path: state arrays are TIME-MAJOR in HBM
  int n_store = 1;         // line-search candidate trajectories kept in LDS
  bool batch_minor = false; // lane-per-problem path: state arrays are [t][row][b] in HBM
  double* lxu = nullptr;             // workgroup-per-problem kernels, long horizons: cost gradients in HBM
  int spec_slots = 0;              // trial trajectories x_spec / u_spec hold per problem (3: one workgroup's four candidates; 31: candidate groups)
  double *x_spec = nullptr, *u_spec = nullptr;   // mid-size kernels: trial trajectories of three more line-search candidates
  int32_t* bm_scratch = nullptr;   // lane-per-problem kernels with key-points: integer scratch (ilqr_batch.hpp)
  double *sink_x = nullptr, *sink_u = nullptr, *sink_cost = nullptr;   // result sink (device aliases of host arrays), optional
  // control limits (mi_ilqr_set_control_limits; the m <= 2 kernel families and the mid-size workgroup family, n <= 32): `limited`
  // selects the Limited<M> kernels
  bool limited = false;
  double* ulim = nullptr;          // (B, 2, m): u_min | u_max per problem (allocated on first use, kept when cleared)
  double* s2 = nullptr;            // (B,): S2 of each problem's last limited backward pass (KArgs::s2)
  // the per-problem arrays: targets and target_steps, (B, n) each, enter and leave their mode together; params (B, n_params);
  // costs (B, 2 n^2 + m^2), row b = Q_b | R_b | Qf_b as the kernels get it (after the n >= 33 round-off symmetrisation)
  RowStore targets, target_steps, params, costs;
  bool target_steps_moving = false;   // a row of the steps is non-zero (cluster helpers' candidate groups need a still target)
  // exact_backward / cost_asym above are the class the kernels run with: the shared matrices' (shared_*) in shared mode, that of
  // the most general row of `costs` (rows_*) in per-problem mode
  int shared_exact_backward = 0, shared_cost_asym = 0, rows_exact_backward = 0, rows_cost_asym = 0;
  // lane-per-problem kernels: their per-problem-cost instantiations always read target ROWS; a handle with one target gets the
  // shared x_nom broadcast into these (B, n) rows before a launch (refresh_lane_target_rows)
  RowStore lane_targets;
  // reference trajectories (MI_F_X_REF / MI_F_REF_CLOCK; workgroup-per-problem handles): (B, ref_T * n) rows, `synced` = the handle
  // holds a reference; ref_clock: the row a solve's window starts at (mi_ilqr_mpc_run advances it); ref_qn: (B, N-1, n) kernel
  // scratch (KArgs::ref_qn).  ref_cap: the doubles reference.rows was allocated for (a longer reference gets a new block).
  RowStore reference;
  int ref_T = 0;
  long long ref_clock = 0;
  size_t ref_cap = 0;
  double* ref_qn = nullptr;
  std::vector<void*> owned;       // every device allocation of the handle (dev_alloc): what mi_ilqr_destroy frees
  // mi_ilqr_policy_rollout: start / stop events of its rollout kernel (created on first use; MI_F_POLICY_KERNEL_MS) - its own pair,
  // so that the solves' events and statistics stay what they were
  hipEvent_t policy_ev0 = nullptr, policy_ev1 = nullptr;
  bool policy_ran = false;         // the events hold a launch (a policy rollout has run on this handle)
  // the rollouts' disturbances: MI_F_POLICY_NOISE, (B, n + m) rows sigma_x | sigma_u - `synced` selects the noisy kernels - and
  // MI_F_POLICY_STREAM.  Read by mi_ilqr_policy_rollout only; problem data, mi_ilqr_reset keeps them.
  RowStore policy_noise;
  unsigned long long policy_seed = 0;
  uint32_t policy_first_sample = 0;
  bool policy_common = false;
  // Monte-Carlo on the device (MI_F_POLICY_MC_DIST / _RUN / _STATS / _SAMPLES; policy_mc.hpp).  policy_mc_dist: (B, 3 n + 2 n_params)
  // sampler rows x0_mean | x0_spread | goal | p_mean | p_spread, problem data like the noise rows.  mc_acc: the fold's running
  // accumulator on the device, (10, B) problem-minor; mc_stats: the last run's (B, 10) result (empty: no run yet); mc_samples: its
  // (B, S, n + n_params + 2) rows when it was asked for them (else empty), on the host - what the selectors return.  mc_events: the
  // start / stop pairs of the passes over windows of groups (a fixed few, used in turn); mc_ms: the rollout kernels of the last run, summed - what
  // MI_F_POLICY_KERNEL_MS reports while policy_last_mc says that the last policy launch was such a run.
  RowStore policy_mc_dist;
  double* mc_acc = nullptr;
  std::vector<double> mc_stats, mc_samples;
  std::vector<hipEvent_t> mc_events;
  double mc_ms = 0.0;
  int32_t mc_passes = 0;           // passes of the last run (MI_I_POLICY_MC_PASSES)
  bool policy_last_mc = false;
  // What a run observes beside the cost (MI_F_POLICY_MC_BOX / _OBSERVE / _ENVELOPE / _ENVELOPE_U / _SAFETY; policy_env.hpp).  mc_box:
  // (B, 2 n) rows lo | hi, `synced` = the handle holds a box and runs observe it; mc_observe: bit 0 state envelopes, bit 1 control
  // envelopes.  env_acc_x (B, N n, 8) / env_acc_u (B, (N-1) m, 8) / box_counters (B, 3 + N): the kernels' accumulators on the device,
  // allocated on first use; mc_env_x / mc_env_u / mc_safety: the last run's results on the host (empty: that run did not produce them).
  RowStore mc_box;
  int32_t mc_observe = 0;
  double *env_acc_x = nullptr, *env_acc_u = nullptr;
  unsigned long long* box_counters = nullptr;
  std::vector<double> mc_env_x, mc_env_u, mc_safety;
  // the plant of the closed receding-horizon loop (mi_ilqr_mpc_run; plant_advance.hpp).  plant_state: (B, n), `synced` = the handle
  // holds a plant - its device rows ARE the plant (the kernel advances them in place, mi_ilqr_mpc_run brings the mirror up to date);
  // plant_params: (B, n_params), not synced = every plant runs on its problem's model row; plant_noise: (B, n + m) sigma_x | sigma_u,
  // `synced` selects the noisy kernels.  Problem data like the policy's: mi_ilqr_reset keeps them.
  RowStore plant_state, plant_params, plant_noise;
  unsigned long long plant_seed = 0, plant_clock = 0;   // MI_F_PLANT_STREAM: seed | clock | common | feedback
  bool plant_common = false, plant_feedback = true;
  double* plant_dead = nullptr;    // (B,): 1.0 = the plant has ended (until MI_F_PLANT_STATE is set again)
  double* plant_log = nullptr;     // (rows, n + m + 1, B) problem-minor: x_k | u_k | l_k of the last closed-loop run (grow-only)
  size_t plant_log_cap = 0;        // ... its capacity in doubles
  int plant_log_rows = 0;          // ... and the rows that run wrote (0: no such run yet)
  hipEvent_t plant_ev0 = nullptr, plant_ev1 = nullptr;   // the plant kernel's own event pair (MI_F_PLANT_KERNEL_MS)
  double plant_ms = 0.0;           // summed over the plant kernels of the last closed-loop run
  // multi-start (MI_F_SEEDS_*; seeds.hpp, h_seeds.hip): the handle read as groups of K consecutive problems.  seeds_sigma: (B, m)
  // sigma_u rows of the perturbation, problem data like the noise rows (not synced: zeros).  seeds_best_dev: the (G, 3) rows
  // winner | cost | eligible on the device, room for G = B; seeds_best / seeds_x / seeds_u / seeds_cost: what the last select and
  // the last gather left, on the host - what the read-only selectors return (empty: no such command yet).  seeds_ev0 / seeds_ev1:
  // the command's own event pair (MI_F_SEEDS_KERNEL_MS), seeds_ran: they hold a launch.  seeds_log_dev: the (R + 1, G, 3) selection
  // log of the long form (multi-start in the receding-horizon loop), grow-only, seeds_log_cap doubles.
  RowStore seeds_sigma;
  double* seeds_best_dev = nullptr;
  double* seeds_log_dev = nullptr;
  size_t seeds_log_cap = 0;
  std::vector<double> seeds_best, seeds_x, seeds_u, seeds_cost;
  hipEvent_t seeds_ev0 = nullptr, seeds_ev1 = nullptr;
  bool seeds_ran = false;
  double seeds_ms = 0.0;
  // parameter identification (MI_F_FIT_*; fit.hpp, h_fit.hip).  fit_data: the (B, fit_T, 2 n + m) transitions on the device,
  // grow-only, fit_data_cap doubles.  fit_weights (B, n + 1) w | count, fit_start (B, n_params + 1) theta0 | mu0, fit_bounds
  // (2, n_params): what the setters left, on the host (empty: the defaults); they go to the device with a command.  fit_result
  // (B, n_params + 7) / fit_normal (B, P + P P): the last command's results on the host (empty: none yet).  fit_ev0 / fit_ev1: the
  // command's own event pair.  Nothing of this is read or written by a solve.
  double* fit_data = nullptr;
  size_t fit_data_cap = 0;
  int fit_T = 0;
  std::vector<double> fit_weights, fit_start, fit_bounds, fit_result, fit_normal;
  hipEvent_t fit_ev0 = nullptr, fit_ev1 = nullptr;
  double fit_ms = 0.0;
};

// Run-time switches for A/B runs (README): the environment is read once per process.
struct Switches {
  bool no_helper;        // MI_ILQR_NO_HELPER=1: no helper wavefronts (make_args)
  bool seq_backward;     // MI_ILQR_SEQ_BACKWARD=1: sequential instead of time-parallel backward sweep
  bool seq_rollout;      // MI_ILQR_SEQ_ROLLOUT=1: sequential instead of time-parallel rollout
  int stats_kernel;      // MI_ILQR_STATS_KERNEL: -1 unset, 1 the separate kernel, 0 the in-kernel epilogue (stats_in_kernel)
  int spec;              // MI_ILQR_SPEC: line-search candidate policy of the mid-size kernels (default 1; outside 0..2: 0)
  int cluster;           // MI_ILQR_CLUSTER: workgroups per problem, forced when > 0 (cluster_size)
  int cluster_order;     // MI_ILQR_CLUSTER_ORDER: placement of a cluster's workgroups (default 2)
  int early;             // MI_ILQR_EARLY: early linearization by the helpers (default 1)
  int ls_groups;         // MI_ILQR_LS_GROUPS: candidate groups (default 1)
  int mc_pass_groups;    // MI_ILQR_MC_PASS_GROUPS: groups of 64 samples per pass of the on-device Monte-Carlo, forced when > 0 (tests)
  int solve_slots;       // MI_ILQR_SOLVE_SLOTS: 1 = pipelined cold solves run one at a time on one stream (default 2: DESIGN.md 6)
};
MI_INTERNAL inline const Switches& switches() {
  static const Switches s = [] {
    auto on = [](const char* name) { const char* e = std::getenv(name); return e && e[0] == '1'; };
    auto num = [](const char* name, int dflt) { const char* e = std::getenv(name); return e ? std::atoi(e) : dflt; };
    const char* stats = std::getenv("MI_ILQR_STATS_KERNEL");
    const int spec = num("MI_ILQR_SPEC", 1);
    return Switches{on("MI_ILQR_NO_HELPER"), on("MI_ILQR_SEQ_BACKWARD"), on("MI_ILQR_SEQ_ROLLOUT"),
                    !stats ? -1 : (stats[0] == '1' ? 1 : 0), (spec >= 0 && spec <= 2) ? spec : 0, num("MI_ILQR_CLUSTER", 0),
                    num("MI_ILQR_CLUSTER_ORDER", 2), num("MI_ILQR_EARLY", 1), num("MI_ILQR_LS_GROUPS", 1),
                    num("MI_ILQR_MC_PASS_GROUPS", 0), num("MI_ILQR_SOLVE_SLOTS", 2) == 1 ? 1 : 2};
  }();
  return s;
}

// Small batches of the wave-per-problem kernels aggregate the batch statistics in the solve kernel
// itself (last workgroup to finish): a blocking single-problem solve saves a kernel launch, 5 us of
// 98.  Large batches keep the separate stats_kernel: with pipelined solves the two cost the same per
// step (measured at B = 1024: 0.166 ms either way), and the solve kernel stays 3.6 us shorter.
// MI_ILQR_STATS_KERNEL=1 / =0 forces the separate kernel / the in-kernel epilogue (A/B runs).
static inline bool stats_in_kernel(const mi_ilqr* h) {
  if (h->large || h->batch_minor) return false;
  if (switches().stats_kernel >= 0) return switches().stats_kernel == 0;
  return h->B <= 64;
}
static inline void select_stats_slot(mi_ilqr* h, int slot) {
  h->ev0 = h->ring_ev0[slot]; h->ev1 = h->ring_ev1[slot];
  h->h_stats = h->h_ring + slot; h->d_stats = h->d_ring + slot;
  h->cur_slot = slot;
  const size_t o = (size_t)slot * h->B;
  h->cost = h->cost_ring + o; h->iters = h->iters_ring + o; h->status = h->status_ring + o; h->ls_trials = h->ls_ring + o;
}

// The state fields and the stream alias solve slot `slot` from here on; the inputs alias their latest copies.
static inline void select_solve_slot(mi_ilqr* h, int slot) {
  const SolveSlot& s = h->slots[slot];
  h->x_bar = s.x_bar; h->u_bar = s.u_bar; h->K = s.K; h->kappa = s.kappa; h->dV = s.dV; h->fx = s.fx; h->fu = s.fu;
  h->hist = s.hist; h->iter_cyc = s.iter_cyc; h->s2 = s.s2; h->prof = s.prof; h->kp_count = s.kp_count; h->kp_list = s.kp_list;
  h->done_counter = s.done_counter;
  h->stream = s.stream;
  h->solve_slot = slot;
}

namespace mi_host {
using namespace mi;
#define HIPCHK(expr)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) {                                                               \
      std::fprintf(stderr, "mi_ilqr: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return MI_ILQR_E_HIP;                                                               \
    }                                                                                     \
  } while (0)

constexpr size_t kMaxLds = 160 * 1024;
// A model's launch entry asked with this mode answers MI_ILQR_OK when it carries Limited<M> kernels, launching nothing
// (mi_ilqr_set_control_limits; family-1 plugins carry them when built with them: plugin.py, control_limits=True).
constexpr int kModeProbeLimits = 0x4c494d;
// mi_ilqr_policy_rollout: the launch entry takes a PolicyArgs (below), not a KArgs, and launches policy_rollout_kernel<M>
// (policy_rollout.hpp) whatever kernel family serves the handle's solves.
constexpr int kModePolicyRollout = 0x504f4c;
// mi_ilqr_mpc_run on a handle that holds a plant: the launch entry takes a PlantArgs (below) and launches plant_advance_kernel<M>
// (plant_advance.hpp), again whatever the handle's kernel family.
constexpr int kModePlantAdvance = 0x504c54;
// mi_ilqr_set(MI_F_POLICY_MC_RUN): the launch entry takes a PolicyMcArgs (below) and launches policy_mc_kernel<M> and the fold behind
// it (policy_mc.hpp) for one window of sample groups.
constexpr int kModePolicyMC = 0x504d43;
// mi_ilqr_set(MI_F_SEEDS_RUN) in its sampling form: the launch entry takes a MppiArgs (below) and launches mppi_rollout_kernel<M>
// (mppi.hpp), one lane per sample of the perturbed nominal plan, whatever the handle's kernel family.
constexpr int kModeSampledRollout = 0x4d5050;
// mi_ilqr_set(MI_F_FIT_RUN): the launch entry takes a FitArgs (below) and launches fit_normal_kernel<M> (fit.hpp), one lane per
// (transition, finite-difference slot), whatever the handle's kernel family.
constexpr int kModeFitNormal = 0x464954;
constexpr int kMaxBatchPluginN = 6;      // family-0 models up to this n also get the lane-per-problem kernels

// The dynamic-LDS ceiling of a kernel is raised once per (kernel, device), to the hardware maximum - not
// on every launch.
constexpr int kMaxDevices = 64;
template <class Kern>
int allow_max_lds(Kern kern, bool (&done)[kMaxDevices], int device) {
  if (device >= 0 && device < kMaxDevices && done[device]) return MI_ILQR_OK;
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds));
  if (device >= 0 && device < kMaxDevices) done[device] = true;
  return MI_ILQR_OK;
}

// One dispatch packet per solve: the launch carries the handle's start/stop events itself (the kernel's own
// begin/end timestamps, what rocprofv3 reports for it) instead of two hipEventRecord marker packets around it.
// A profiled dispatch still costs the stream ~5 us of serialization in a pipelined sequence
// (tools/ubench/gap.hip), so mi_ilqr_set_timing can restrict the events to one launch in k.
// `part`: 0 = a launch on its own (start and stop events); 1 / 2 = first / last kernel of a solve made of two launches
// (the start event rides on the first, the stop event on the last: the elapsed time covers both and the gap).
template <class Kern>
int launch_timed(mi_ilqr* h, Kern kern, dim3 grid, dim3 block, size_t lds, const KArgs& a, int part = 0) {
  KArgs args = a;
  void* argv[] = {&args};
  h->ring_timed[h->cur_slot] = h->last_timed = h->timed_launch;
  if (!h->timed_launch) { HIPCHK(hipLaunchKernel(reinterpret_cast<const void*>(kern), grid, block, argv, lds, h->stream)); return MI_ILQR_OK; }
  HIPCHK(hipExtLaunchKernel(reinterpret_cast<const void*>(kern), grid, block, argv, lds, h->stream, part == 2 ? nullptr : h->ev0,
                            part == 1 ? nullptr : h->ev1, 0));
  return MI_ILQR_OK;
}

// Run-time choices turned into template arguments: with_jac calls f(std::integral_constant<int, JAC>{}) for the handle's Jacobian
// mode, with_mode f(std::integral_constant<int, MODE>{}) for `mode` when it is one of MODES (else MI_ILQR_E_BAD_ARG), with_any_mode
// the same over the six kernel modes.  Only what f is called with gets instantiated.
template <class F>
int with_jac(const mi_ilqr* h, F&& f) {
  if (h->d.jacobian_mode == MI_JAC_AUTODIFF) return f(std::integral_constant<int, MI_JAC_AUTODIFF>{});
  return f(std::integral_constant<int, MI_JAC_FD_CENTRAL>{});
}
template <int MODE, int... MODES, class F>
int with_mode(int mode, F&& f) {
  if (mode == MODE) return f(std::integral_constant<int, MODE>{});
  if constexpr (sizeof...(MODES) > 0) return with_mode<MODES...>(mode, f);
  return MI_ILQR_E_BAD_ARG;
}
template <class F>
int with_any_mode(int mode, F&& f) {
  return with_mode<MODE_SOLVE, MODE_ROLLOUT, MODE_FORWARD, MODE_LINEARIZE, MODE_BACKWARD, MODE_MPC>(mode, f);
}

}  // namespace mi_host

// The kernel sets of a model: one launcher per set, (handle, mode, args) -> status.  Instantiated for the built-in models in their
// own translation units (k_<model>.hip, k_<model>_lim.hip, k_batch.hip, k_batch_lim.hip: explicit instantiations), for a plugin model
// in its unit (drake_ddp_amd/plugin.py).
namespace mi_host {
using Launcher = int (*)(mi_ilqr* h, int mode, const KArgs& a);
template <class M> MI_INTERNAL int launch_jac(mi_ilqr* h, int mode, const KArgs& a);                 // launch_small.hpp
template <class M> MI_INTERNAL int launch_limited(mi_ilqr* h, int mode, const KArgs& a);
template <class M> MI_INTERNAL int launch_jac_large(mi_ilqr* h, int mode, const KArgs& a);           // launch_large.hpp
template <class M> MI_INTERNAL int launch_jac_large_limited(mi_ilqr* h, int mode, const KArgs& a);
template <class M> MI_INTERNAL int launch_batch(mi_ilqr* h, int mode, const KArgs& a);               // launch_batch.hpp
template <class M> MI_INTERNAL int launch_batch_limited(mi_ilqr* h, int mode, const KArgs& a);

// Arguments of policy_rollout_kernel<M> (policy_rollout.hpp), all device pointers.  "Sample-minor": the sample index runs fastest.
struct PolicyArgs {
  const double* policy;       // (B, N-1, n + m + m n): row t = x_bar_t | u_bar_t | K_t (m x n, row-major) - the call's time-major copy
  const double* x0;           // (B, n, S) sample-minor
  const double* params;       // (B, n_params, S) sample-minor, or nullptr: every sample runs on param_rows
  const double* param_rows;   // (B or 1, n_params): problem b's row at b * param_stride
  const double* cost;         // Q | R | Qf of problem b at b * cost_stride
  const double* x_nom;        // (n,) of problem b at b * x_nom_stride
  const double* ulim;         // (B, 2, m) u_min | u_max, or nullptr: no clamp
  const double* noise;        // (B, n + m) sigma_x | sigma_u of problem b (MI_F_POLICY_NOISE), or nullptr: the noise-free kernels
  double* cost_out;           // (B, S)
  double* x_final;            // (B, n, S) sample-minor
  int32_t* steps;             // (B, S)
  double* X;                  // (B, N, n, S) sample-minor, or nullptr
  double* U;                  // (B, N-1, m, S) sample-minor, or nullptr
  size_t param_stride, cost_stride, x_nom_stride;
  double dt;
  int32_t N, S, B, m_user;    // m_user: controls m_user .. m-1 are padding and stay exact zeros
  unsigned long long seed;    // MI_F_POLICY_STREAM: the Philox key, the number of the call's sample 0, one stream for all problems
  uint32_t first_sample;
  int32_t common;
};
template <class M> MI_INTERNAL int launch_policy_rollout(mi_ilqr* h, const PolicyArgs& a);          // policy_rollout.hpp; k_policy.hip
template <class M> MI_INTERNAL int launch_policy_rollout_noise(mi_ilqr* h, const PolicyArgs& a);    // ... k_policy_noise.hip

// Arguments of one pass of the on-device Monte-Carlo (policy_mc.hpp: policy_mc_kernel<M> and policy_mc_fold_kernel), device pointers.
// kMcFields: the doubles of a per-problem result and of a group's partial, S | counted | success | mean | M2 | min | max | argmin |
// argmax | steps_total.
constexpr int kMcFields = 10;
struct PolicyMcArgs {
  PolicyArgs r;               // the rollout's: policy, param_rows, cost, x_nom, ulim, noise, the strides, dt, N, B, m_user and the stream
                              // (x0, params, S and the outputs are not used: the samples are drawn, S is below)
  const double* dist;         // (B, 3 n + n_params 2) sampler rows x0_mean | x0_spread | goal | p_mean | p_spread
  double* partials;           // (groups, 10, B) problem-minor: this window's group partials
  double* acc;                // (10, B) problem-minor: the running accumulator
  double* samples;            // (B, n + n_params + 2, win_samples) sample-minor rows x0 | params | cost | steps of this window, or nullptr
  unsigned long long S;       // the call's samples per problem
  size_t win_samples;         // ... and this window's
  uint32_t group0;            // the window: groups group0 .. group0 + groups - 1 of every problem
  int32_t groups;
  int32_t x0_dist, p_dist;    // 0 normal, 1 uniform
  int32_t sample_params;      // the plants' parameters are drawn too (models with parameters)
  int32_t first_pass;         // the accumulator starts empty
  hipEvent_t ev0, ev1;        // the rollout kernel's start / stop events of this pass
};
template <class M> MI_INTERNAL int launch_policy_mc(mi_ilqr* h, const PolicyMcArgs& a);             // policy_mc.hpp; k_policy_mc.hip
template <class M> MI_INTERNAL int launch_policy_mc_noise(mi_ilqr* h, const PolicyMcArgs& a);       // ... k_policy_mc_noise.hip

// The reductions of a window's trajectory buffers behind a pass of the on-device Monte-Carlo (policy_env.hpp; k_policy_env.hip), on the
// handle's stream.  launch_policy_env: buf (B, R, win) sample-minor rows -> acc (B, R, 8), first_global the global number of the
// window's sample 0, first: the accumulators start empty.  launch_policy_box: the X window against box (B, 2 n) -> counters (B, 3 + N).
MI_INTERNAL int launch_policy_env(mi_ilqr* h, const double* buf, double* acc, size_t B, size_t R, size_t win, double first_global, int first);
MI_INTERNAL int launch_policy_box(mi_ilqr* h, const double* X, const double* box, const double* x_nom, size_t x_nom_stride,
                                  const double* goal, size_t goal_stride, unsigned long long* counters, size_t B, int n, int N, size_t win);

// Arguments of seeds_kernel (seeds.hpp; k_seeds.hip), the multi-start command of MI_F_SEEDS_RUN: device pointers, one workgroup per
// group of K consecutive problems.  Trajectory arrays are in the handle's kernel layout, `layout` 0 = [b][row][t], 1 = [b][t][row],
// 2 = [t][row][b] (host_internal.hpp: LAYOUT_TL / TM / BM).
enum { SEEDS_PERTURB = 0, SEEDS_SELECT = 1, SEEDS_RESEED = 2, SEEDS_GATHER = 3 };
struct SeedsArgs {
  const double* u_src;        // (B, m, N-1): the controls as the handle holds them now, or nullptr: zeros.  May BE u_dst (a pending guess)
  double* u_dst;              // (B, m, N-1): the initial guess the next solve starts from (perturb, reseed)
  const double* sigma;        // (B, m) sigma_u rows, or nullptr: zeros
  const double* cost;         // (B,) and
  const int32_t* status;      // (B,) of the last solve (select, reseed, gather)
  double* best;               // (G, 3) rows winner | cost | eligible, written by select, reseed and gather
  const double* x_bar;        // (B, n, N), or nullptr: zeros (gather)
  double *gx, *gu, *gc;       // (G, n, N) and (G, m, N-1), time last, and (G,): the winners' rows (gather)
  unsigned long long seed;    // the Philox key
  uint32_t round;             // counter word 0
  int32_t B, K, n, m, m_user, N, layout, op, hold;   // m_user: controls m_user .. m-1 are padding and get no noise
  hipEvent_t ev0, ev1;        // the kernel's start / stop events
};
MI_INTERNAL int launch_seeds(mi_ilqr* h, const SeedsArgs& a);

// Arguments of seeds_mpc_join_kernel (seeds.hpp; k_seeds.hip), the join between two re-solves of the long form of MI_F_SEEDS_RUN:
// select, then the shifted winner handed to every member of its group.  Source and destination never alias (the host materialises
// a pending guess first).
struct SeedsJoinArgs {
  const double* u_bar;        // (B, m, N-1): the plans of the last solve
  const double* x_bar;        // (B, n, N)
  double* u_guess;            // (B, m, N-1): the initial guess of the next solve
  double* x0;                 // (B, n): its initial states
  const double* sigma;        // (B, m) sigma_u rows, or nullptr: zeros
  const double* cost;         // (B,) and
  const int32_t* status;      // (B,) of the last solve
  double* best;               // (G, 3): this round's row of the selection log
  double* mpc_dead;           // (B,): the MPC log's flags, cleared for the members of a group with a winner
  // the closed loop, one plant per group (all nullptr without a plant): the groups' plants after this round's segment, compact -
  // they become every member's x0 in the place of the prediction, and every member's row of the (B, ..) arrays the selectors read
  const double* plant_x;      // (G, n) states
  const double* plant_ended;  // (G,): 1.0 = the group's plant has ended; its members stop logging, winner or not
  double* plant_rows;         // (B, n): MI_F_PLANT_STATE's rows
  double* plant_dead;         // (B,): the plants' flags per problem
  unsigned long long seed;
  uint32_t round;
  int32_t B, K, n, m, m_user, N, layout, hold, replan;
  hipEvent_t ev0, ev1;
};
MI_INTERNAL int launch_seeds_mpc_join(mi_ilqr* h, const SeedsJoinArgs& a);

// Arguments of mppi_rollout_kernel<M> (mppi.hpp; k_mppi.hip), the sampling form of MI_F_SEEDS_RUN: device pointers.
struct MppiArgs {
  PolicyArgs r;               // the rollout's per-problem data: param_rows, cost, x_nom, ulim, the strides, dt, N, B, m_user (nothing else is read)
  const double* nominal;      // (B, N-1, m) time-major: the plans the samples perturb
  const double* x0;           // (B, n)
  const double* sigma;        // (B, m) sigma_u rows, or nullptr: zeros
  double* cost_out;           // (B, S)
  unsigned long long seed;    // the Philox key
  uint32_t sample0;           // the global number of this launch's sample 0
  int32_t S, hold;
  hipEvent_t ev0, ev1;        // start / stop events riding on the launch, or nullptr
};
template <class M> MI_INTERNAL int launch_mppi_rollout(mi_ilqr* h, const MppiArgs& a);              // mppi.hpp; k_mppi.hip
// ... and of mppi_update_kernel (no model), one workgroup per problem: weights, log rows, the blend into the next nominal
struct MppiUpdateArgs {
  const double* nom_in;       // (B, N-1, m) time-major: the nominal the samples were drawn around
  double* nom_out;            // (B, N-1, m): the next nominal (never nom_in)
  const double* cost;         // (B, S): the samples' costs
  const double* sigma;        // (B, m) or nullptr
  const double* ulim;         // (B, 2, m) or nullptr
  double* best;               // (B, 3): this iteration's row argmin | cost | finite
  double* costlog;            // (B, 2): this iteration's row nominal cost | ESS
  unsigned long long seed;
  double temperature;
  uint32_t sample0;
  int32_t B, S, m, m_user, N, hold;
  hipEvent_t ev0, ev1;
};
MI_INTERNAL int launch_mppi_update(mi_ilqr* h, const MppiUpdateArgs& a);
// the nominal from the handle's layout into the staging copy (src nullptr: zeros); the final nominal into u_guess (shifted), the
// time-last copy and the closing row of the cost log
MI_INTERNAL int launch_mppi_stage(mi_ilqr* h, const double* src, double* nom, int B, int m, int N, int layout, hipEvent_t ev0);
MI_INTERNAL int launch_mppi_handover(mi_ilqr* h, const double* nom, double* u_guess, double* tl, const double* cost1, double* costlog, int B,
                                     int m, int N, int layout, int shift, hipEvent_t ev1);

// Parameter identification (fit.hpp; k_fit.hip; h_fit.hip), the command of MI_F_FIT_RUN.  A problem's state between the launches is
// one record of kFitStride doubles on the device: theta | the trial row | the kept normal equations, laid out like a partial row
// (below) from kFitC on | mu | trials so far | accepted trials | status (kFitRunning until the problem has finished) | the first
// cost | whether the trial row came out of a factorisation that succeeded.
constexpr int kFitMaxFree = MI_FIT_MAX_FREE;
// a partial row, and the kept normal equations: c | g (P) | the upper triangle of H, row after row
constexpr int fit_row_len(int P) { return 1 + P + P * (P + 1) / 2; }
constexpr int kFitTheta = 0, kFitTrial = MI_ILQR_MAX_PARAMS, kFitC = 2 * MI_ILQR_MAX_PARAMS;
constexpr int kFitMu = kFitC + fit_row_len(kFitMaxFree), kFitIters = kFitMu + 1, kFitAccepted = kFitMu + 2, kFitStatus = kFitMu + 3;
constexpr int kFitCost0 = kFitMu + 4, kFitTrialOk = kFitMu + 5, kFitStride = 96;
static_assert(kFitTrialOk < kFitStride, "a problem's record holds every field");
constexpr double kFitRunning = -1.0;
constexpr double kFitMuMin = 1e-12, kFitMuMax = 1e12;
// Arguments of fit_normal_kernel<M>: device pointers.
struct FitArgs {
  const double* data;         // (B, T, 2 n + m): rows x | u | x_next
  const double* weights;      // (B, n + 1): w | count
  const double* state;        // (B, kFitStride): the point to evaluate is the TRIAL row; a problem whose status is not kFitRunning is skipped
  double* partial;            // (B, waves, fit_row_len(P)): one row per (problem, wave)
  double dt, fd_rel, fd_floor;
  int32_t B, T, P, log2G, waves;   // G = 1 << log2G slots per transition, waves = ceil(T / (64 / G)) per problem
  int32_t free_idx[kFitMaxFree];
  hipEvent_t ev0, ev1;        // start / stop events riding on the launch, or nullptr
};
template <class M> MI_INTERNAL int launch_fit_normal(mi_ilqr* h, const FitArgs& a);                  // fit.hpp; k_fit.hip
// ... and of fit_update_kernel (no model), one wave per problem: the fold, the decision, the next trial
struct FitUpdateArgs {
  double* state;              // (B, kFitStride)
  const double* partial;      // (B, waves, fit_row_len(P))
  const double* bounds;       // (2, n_params): lower | upper
  double ftol;
  int32_t B, P, n_params, waves;
  int32_t first, last;        // first: the rows are the normal equations at theta0; last: the closing decision, no further trial
  int32_t free_idx[kFitMaxFree];
  hipEvent_t ev0, ev1;
};
MI_INTERNAL int launch_fit_update(mi_ilqr* h, const FitUpdateArgs& a);

// Arguments of plant_advance_kernel<M> (plant_advance.hpp), all device pointers.  "Problem-minor": element e of problem b at e * B + b.
struct PlantArgs {
  const double* policy;       // (steps, n + m + m n, B) problem-minor: row j = x_bar_j | u_bar_j | K_j (m x n, row-major), the first `steps` columns
  const double* params;       // (n_params, B) problem-minor: the plants' parameters
  const double* cost;         // (n n + m m, B) problem-minor: Q_b | R_b
  const double* x_nom;        // (n, B) problem-minor
  const double* ulim;         // (2 m, B) problem-minor u_min | u_max, or nullptr: no clamp
  const double* noise;        // (n + m, B) problem-minor sigma_x | sigma_u (MI_F_PLANT_NOISE), or nullptr: the noise-free kernels
  double* x;                  // (B, n): the plants' states, advanced in place
  double* dead;               // (B,): 1.0 = the plant has ended; read and written
  double* mpc_dead;           // (B,): the MPC log's flags (mpc_log_fill_kernel), set for a plant that has ended
  double* log;                // (steps, n + m + 1, B) problem-minor: this launch's rows x_k | u_k | l_k
  double dt;
  unsigned long long seed;    // MI_F_PLANT_STREAM: the Philox key
  uint32_t clock;             // ... and the plant clock of this launch's first step
  int32_t B, steps, m_user, feedback, common;   // m_user: controls m_user .. m-1 are padding and stay exact zeros
};
template <class M> MI_INTERNAL int launch_plant_advance(mi_ilqr* h, const PlantArgs& a);            // plant_advance.hpp; k_plant.hip
template <class M> MI_INTERNAL int launch_plant_advance_noise(mi_ilqr* h, const PlantArgs& a);      // ... k_plant_noise.hip

// The launch entry of a model's record (mi_ilqr_model_plugin::launch), built-in or plugin: the handle picks the kernel set - the
// lane-per-problem kernels (h->batch_minor), the Limited<M> ones (h->limited), else the regular ones.  A set the model lacks is
// nullptr; the probe (kModeProbeLimits) answers whether it has Limited<M> kernels, launching nothing.
template <Launcher REGULAR, Launcher LIMITED = nullptr, Launcher BATCH = nullptr, Launcher BATCH_LIMITED = nullptr>
int launch_entry(mi_ilqr* h, int mode, const void* kargs) {
  if (mode == kModeProbeLimits) return LIMITED != nullptr ? MI_ILQR_OK : MI_ILQR_E_UNSUPPORTED;
  const KArgs& a = *static_cast<const KArgs*>(kargs);
  if (h->batch_minor) {
    if constexpr (BATCH != nullptr && BATCH_LIMITED != nullptr) return h->limited ? BATCH_LIMITED(h, mode, a) : BATCH(h, mode, a);
    return MI_ILQR_E_UNSUPPORTED;
  }
  if constexpr (LIMITED != nullptr) if (h->limited) return LIMITED(h, mode, a);
  return REGULAR(h, mode, a);
}
// ... and the same for model M with the policy rollout (kModePolicyRollout) and the plant of the closed MPC loop (kModePlantAdvance),
// each one kernel per model whatever the handle's family
template <class M, Launcher REGULAR, Launcher LIMITED = nullptr, Launcher BATCH = nullptr, Launcher BATCH_LIMITED = nullptr>
int model_entry(mi_ilqr* h, int mode, const void* kargs) {
  if (mode == kModePolicyRollout) {
    const PolicyArgs& a = *static_cast<const PolicyArgs*>(kargs);
    return a.noise ? launch_policy_rollout_noise<M>(h, a) : launch_policy_rollout<M>(h, a);
  }
  if (mode == kModePolicyMC) {
    const PolicyMcArgs& a = *static_cast<const PolicyMcArgs*>(kargs);
    return a.r.noise ? launch_policy_mc_noise<M>(h, a) : launch_policy_mc<M>(h, a);
  }
  if (mode == kModeSampledRollout) return launch_mppi_rollout<M>(h, *static_cast<const MppiArgs*>(kargs));
  if (mode == kModeFitNormal) return launch_fit_normal<M>(h, *static_cast<const FitArgs*>(kargs));
  if (mode == kModePlantAdvance) {
    const PlantArgs& a = *static_cast<const PlantArgs*>(kargs);
    return a.noise ? launch_plant_advance_noise<M>(h, a) : launch_plant_advance<M>(h, a);
  }
  return launch_entry<REGULAR, LIMITED, BATCH, BATCH_LIMITED>(h, mode, kargs);
}
}  // namespace mi_host
