// libmi_ilqr.so - host side of the C ABI declared in include/mi_ilqr.h, the core: the model table, the handle's creation, the
// launch of the solver kernels (make_args, launch) with the solve, collect and stage entry points, the cost, initial-guess and
// control-limit entry points, timing.  The other concerns of the host have units of their own (h_memory.hip, h_fields.hip,
// h_policy.hip, h_mpc.hip, h_seeds.hip, h_mppi.hip, h_comm.hip; host_internal.hpp declares what they share).
//
// The library owns the device-resident solver state of a batch (the persistent attributes of the reference class, ilqr.py:61-91,
// with a leading batch axis), dispatches the gfx950 kernels and moves data across the boundary.  No compute happens on the host:
// without a usable device every compute entry fails with MI_ILQR_E_NO_DEVICE.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <new>
#include <vector>

#include "host.hpp"          // the handle and the launch templates (instantiated in the k_*.hip units)
#include "host_internal.hpp" // what the host units share
#include "kernel_args.hpp"   // KArgs, DevStats
#include "lds_layout.hpp"    // ws_bytes, large_lds_bytes, large_lds_bytes_hbm, kLargeThreads
#include "models.hpp"

using namespace mi;
using namespace mi_host;

namespace {     // the kernel: global, like every kernel of the host units - a name does not change with the unit

// Aggregate per-problem results on the device so a blocking solve costs ONE small host read
// (pinned, device-mapped) instead of four D2H copies.

// One workgroup per ring slot: blockIdx.x-th of `first, first+1, ...` (mod ring); the arrays are the slot-0 bases.
__global__ void __launch_bounds__(256) stats_kernel(const int32_t* iters, const int32_t* status, const int32_t* ls,
                                                    const double* cost, int B, DevStats* out, int first, int ring) {
  {
    const int slot = (first + (int)blockIdx.x) % ring;
    const size_t o = (size_t)slot * B;
    iters += o; status += o; ls += o; cost += o; out += slot;
  }
  __shared__ long long s_it[256], s_ls[256];
  __shared__ int s_c[256], s_m[256], s_f[256], s_mx[256], s_bi[256], s_x[256], s_p[256];
  __shared__ double s_bc[256];
  const int tid = threadIdx.x;
  long long it = 0, l = 0; int c = 0, m = 0, f = 0, mx = 0, bi = -1, xi = 0, npd = 0; double bc = INFINITY;
  for (int b = tid; b < B; b += 256) {
    it += iters[b]; l += ls[b];
    if (iters[b] > mx) mx = iters[b];
    const int st = status[b] & ~MI_STATUS_FLAG_INDEFINITE;      // (the flag rides on the solve's own outcome; counted in n_not_pd as well)
    if (status[b] & MI_STATUS_FLAG_INDEFINITE) npd++;
    if (st == MI_STATUS_CONVERGED) { c++; if (cost[b] < bc) { bc = cost[b]; bi = b; } }
    else if (st == MI_STATUS_MAX_ITERS) m++;
    else if (st == MI_STATUS_INTERNAL) xi++;
    else if (st == MI_STATUS_NOT_PD) npd++;
    else f++;
  }
  s_x[tid] = xi; s_p[tid] = npd;
  s_it[tid] = it; s_ls[tid] = l; s_c[tid] = c; s_m[tid] = m; s_f[tid] = f; s_mx[tid] = mx; s_bi[tid] = bi; s_bc[tid] = bc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      s_it[tid] += s_it[tid + o]; s_ls[tid] += s_ls[tid + o]; s_c[tid] += s_c[tid + o]; s_m[tid] += s_m[tid + o]; s_f[tid] += s_f[tid + o];
      s_x[tid] += s_x[tid + o]; s_p[tid] += s_p[tid + o];
      if (s_mx[tid + o] > s_mx[tid]) s_mx[tid] = s_mx[tid + o];
      // ties resolve to the lower problem index, like a sequential scan
      if (s_bc[tid + o] < s_bc[tid] || (s_bc[tid + o] == s_bc[tid] && s_bi[tid + o] >= 0 && (s_bi[tid] < 0 || s_bi[tid + o] < s_bi[tid]))) { s_bc[tid] = s_bc[tid + o]; s_bi[tid] = s_bi[tid + o]; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    out->total_iters = s_it[0]; out->total_ls = s_ls[0]; out->n_conv = s_c[0]; out->n_max = s_m[0]; out->n_fail = s_f[0];
    out->max_iters_seen = s_mx[0]; out->best_index = s_bi[0]; out->best_cost = s_bc[0]; out->n_internal = s_x[0]; out->n_not_pd = s_p[0];
  }
}

}  // namespace

namespace mi_host {

namespace {

constexpr int kAnyB = 1 << 30;

template <int n, int m>
size_t wave_lds(int32_t N, int32_t n_store) { return ws_bytes<n, m>(N, n_store); }
template <int n, int m>   // (n_store < 0: the cost gradients in HBM, long horizons)
size_t workgroup_lds(int32_t N, int32_t n_store) { return n_store < 0 ? large_lds_bytes_hbm<n, m>(N) : large_lds_bytes<n, m>(N); }

template <class M>
Model builtin(int family, size_t (*lds)(int32_t, int32_t), int (*launch)(mi_ilqr*, int, const void*), int cluster_max_B,
              std::initializer_list<double> defaults) {
  Model r{};
  r.p.n = M::n; r.p.m = M::m; r.p.n_params = M::n_params; r.p.family = family;
  std::copy(defaults.begin(), defaults.end(), r.p.default_params);
  r.p.lds_bytes = lds; r.p.launch = launch;
  r.cluster_max_B = cluster_max_B;
  return r;
}
// wave-per-problem kernels (k_<model>.hip, k_<model>_lim.hip) and the lane-per-problem ones (k_batch.hip, k_batch_lim.hip); every
// model's policy-rollout kernels are in k_policy.hip and, with noise, k_policy_noise.hip, its sampled rollout in k_mppi.hip
template <class M>
Model wave_model(std::initializer_list<double> defaults) {
  return builtin<M>(0, wave_lds<M::n, M::m>,
                    model_entry<M, launch_jac<M>, launch_limited<M>, launch_batch<M>, launch_batch_limited<M>>, 0, defaults);
}
// workgroup-per-problem kernels (k_<model>.hip; with control limits, k_<model>_lim.hip)
template <class M, Launcher LIMITED = nullptr>
Model workgroup_model(int cluster_max_B, std::initializer_list<double> defaults) {
  return builtin<M>(1, workgroup_lds<M::n, M::m>, model_entry<M, launch_jac_large<M>, LIMITED>, cluster_max_B, defaults);
}

const Model kBuiltins[] = {
    wave_model<Pendulum>({0.25, 0.1, 4.905}),                                                        // MI_MODEL_PENDULUM
    wave_model<Acrobot>({1.0, 1.0, 1.0, 0.5, 1.0, 0.083, 0.33, 0.1, 0.1, 9.81}),                     // MI_MODEL_ACROBOT
    wave_model<CartPole>({10.0, 1.0, 0.5, 9.81}),                                                    // MI_MODEL_CARTPOLE
    wave_model<CartPoleWall>({10.0, 1.0, 0.5, 9.81, -0.45, 0.05, 2000.0, 0.01}),                     // MI_MODEL_CARTPOLE_WALL
    workgroup_model<Synth36>(64, {4.0, 0.5, 6.0, 0.1}),                                              // MI_MODEL_SYNTH36
    workgroup_model<PlanarQuad>(kAnyB, {9.81, 4000.0, 0.004, 0.3, 0.15, 0.05, 0.02, 2.0, 60.0}),     // MI_MODEL_PLANAR_QUAD
    workgroup_model<Quad3D>(kAnyB, {9.81, 4000.0, 0.004, 0.3, 0.15, 0.3, 60.0, 9.0, 0.07, 0.26, 0.28, 0.06, 0.06, 0.04}),  // MI_MODEL_QUAD3D
    workgroup_model<Arm27, launch_jac_large_limited<Arm27>>(
        64, {9.81, 1500.0, 0.005, 0.5, 1.0, 0.5, 0.2, 0.1, 0.05, 1.0, 0.8, 0.6, 0.3, 0.1, 0.04}),    // MI_MODEL_ARM27
    workgroup_model<Arm27C, launch_jac_large_limited<Arm27C>>(
        64, {9.81, 1500.0, 0.005, 0.5, 1.0, 0.5, 0.2, 0.1, 0.05, 1.0, 0.8, 0.3, 0.15, 0.05, 0.04, 0.6}),  // MI_MODEL_ARM27C
};
constexpr int kNumBuiltins = sizeof(kBuiltins) / sizeof(kBuiltins[0]);
static_assert(kNumBuiltins == MI_MODEL_ARM27C + 1, "one row per built-in model id, in id order");

// models registered at run time (mi_ilqr_register_model): id = MI_MODEL_PLUGIN_BASE + slot
// Registrations take the mutex; a slot is filled once and read lock-free afterwards: `used` is published LAST with release
// ordering and read with acquire ordering, so a thread that sees it set also sees the slot's contents (a create or a launch on
// one thread may race a registration on another).
struct PluginSlot { Model model; std::atomic<bool> used{false}; };
PluginSlot g_plugins[MI_ILQR_MAX_PLUGINS];
std::mutex g_plugins_mutex;

// every step is a key-point (ilqr.py:417-432): the linearization covers the whole horizon
bool every_step_keypoint(const mi_ilqr_desc& d) { return d.keypoint_method == MI_KP_SET_INTERVAL && d.minN == 1; }

// Workgroups per problem of a workgroup-per-problem launch: with few problems per GPU most CUs idle - up to 8 workgroups per
// problem share the linearization (ilqr_large.hpp: cluster handshake), as many as keep every workgroup of the launch on its own
// CU.  MI_ILQR_CLUSTER=k forces k (1 = off) for A/B runs.  make_args launches with it; mi_ilqr_create sizes the trial buffers
// (spec_slots) for it.
int cluster_size(const mi_ilqr* h) {
  if (!every_step_keypoint(h->d)) return 1;
  const int forced = switches().cluster;
  if (forced > 0) return std::min(forced, 8);
  if (h->B > model_of(h->d.model_id)->cluster_max_B) return 1;
  // Forward-mode duals (a parity / testing mode - the benchmarked path is central differences) are not clustered unless forced.
  // Round 5: the helper path of ilqr_large_kernel<PlanarQuad, JAC = 1, MODE_SOLVE> faulted (HSA memory aperture violation in a
  // flat load of the item loop of large_jac_at_tree) after two unrelated edits inside large_backward, each alone enough, and
  // stopped faulting with a bounds check added next to it.  Under rocgdb the faulting helper wavefront sits at the top of the item
  // loop with an EXEC mask that is no prefix of the lanes (0x316eaa6bf7995fc5) and garbage in the lanes' time index - a state no
  // path of the source produces (the loop's lanes leave in order); the spilled scalars it restores there (361 - 932 SGPRs of these
  // kernels live in VGPR lanes) were written correctly at kernel start.  Root cause not established beyond that - it points at
  // the compiler's handling of this kernel's spills, not at the handshake - so the instantiation is kept off the default path
  // and the full GPU suite stays the safety net for the clustered central-difference kernels, which every bench config runs.
  if (h->d.jacobian_mode == MI_JAC_AUTODIFF) return 1;
  return std::clamp(h->n_cus > 0 ? h->n_cus / h->B : 1, 1, 8);
}

// a per-problem array's device rows / batch-minor copy (host.hpp: RowStore) - in its per-problem mode only, else nullptr
const double* device_rows(const RowStore& s) { return s.synced ? s.rows : nullptr; }
const double* device_cols(const RowStore& s) { return s.synced ? s.cols : nullptr; }

KArgs make_args(const mi_ilqr* h) {
  KArgs a;
  std::memset(&a, 0, sizeof(a));
  a.x_bar = h->x_bar; a.u_bar = h->u_bar; a.K = h->K; a.kappa = h->kappa; a.dV = h->dV; a.fx = h->fx; a.fu = h->fu;
  a.x0 = h->x0; a.u_guess = h->u_guess; a.cost = h->cost; a.hist = h->hist; a.iter_cyc = h->iter_cyc;
  a.x_trial = h->x_trial; a.u_trial = h->u_trial; a.trial_cost = h->trial_cost; a.stage_in = h->stage_in;
  a.costmat = h->costmat;
  a.iters = h->iters; a.status = h->status; a.ls_trials = h->ls_trials; a.kp_count = h->kp_count; a.kp_list = h->kp_list;
  a.prof = h->prof;
  for (int i = 0; i < MI_ILQR_MAX_PARAMS; ++i) a.params[i] = h->d.model_params[i];
  a.dt = h->d.dt; a.delta = h->d.delta; a.beta = h->d.beta; a.gamma = h->d.gamma;
  a.jerk_thr = h->d.jerk_threshold; a.err_thr = h->d.iterative_error_threshold; a.fd_h = h->d.fd_step;
  a.N = h->N; a.B = h->B; a.kp_method = h->d.keypoint_method; a.minN = h->d.minN; a.maxN = h->d.maxN;
  a.max_iters = h->d.max_iters; a.hist_cap = h->d.hist_cap;
  a.n_store = h->n_store;
  a.cold = h->cold ? 1 : 0;
  a.u_pending = h->u_pending ? 1 : 0;
  a.mpc_resolves = h->mpc_resolves; a.mpc_replan = h->mpc_replan; a.mpc_log = h->mpc_log;
  for (int i = 0; i < kMaxStateDim; ++i) a.mpc_target_step[i] = h->mpc_target_step[i];
  // wave-per-problem kernels: helper wavefronts share the linearization when every step is a key-point
  // (the default) - as many as keep the whole batch resident at ONE wave per SIMD (1024 slots): every
  // wave of the kernel carries the main wave's register allocation (> 256 VGPRs with the time-parallel
  // rollout and sweep), so a second resident wave per SIMD does not fit and extra waves would queue.
  // MI_ILQR_NO_HELPER=1 turns them off (A/B measurements).
  const Switches& sw = switches();
  a.seq_backward = h->exact_backward ? 2 : (sw.seq_backward ? 1 : 0);
  a.newton_rollout = sw.seq_rollout ? 0 : 1;
  // (not for n = 2 with the time-parallel rollout: its final pass differentiates the steps it holds in registers,
  //  which beats sharing them - C2's batch at B = 512: 0.141 ms without helpers, 0.149 ms with one; tools/helper_ab.py)
  const bool fused_linearization = h->n == 2 && h->m == 1 && h->N - 1 <= 256 && a.newton_rollout != 0;
  a.helpers = 0;
  if (!sw.no_helper && !h->large && !h->batch_minor && every_step_keypoint(h->d) &&
      (h->N - 1) * (h->n + h->m) > 128 && !fused_linearization)
    a.helpers = h->B <= 256 ? 3 : (h->B <= 512 ? 1 : 0);
  // wave-per-problem kernels aggregate the batch statistics themselves (MODE_SOLVE / MODE_MPC)
  const bool own_stats = stats_in_kernel(h);
  a.stats_out = own_stats ? h->d_stats : nullptr;
  a.done_counter = own_stats ? h->done_counter : nullptr;
  a.sink_x = h->sink_x; a.sink_u = h->sink_u; a.sink_cost = h->sink_cost;
  a.bm_scratch = h->bm_scratch;
  a.x_spec = h->x_spec; a.u_spec = h->u_spec;
  a.lxu = h->lxu;
  a.pd_continue = h->d.on_indefinite == 1 ? 1 : 0;
  a.cost_asym = h->cost_asym ? 1 : 0;
  a.ulim = h->limited ? h->ulim : nullptr;
  a.s2 = h->s2;
  a.x_nom_rows = device_rows(h->targets);
  a.target_steps = device_rows(h->target_steps);
  a.cost_rows = device_rows(h->costs);
  a.cost_cols = device_cols(h->costs);
  // (the lane kernels' per-problem-cost instantiations read target rows in any case: the shared target, broadcast by launch())
  if (a.cost_cols && !a.x_nom_rows) a.x_nom_rows = device_rows(h->lane_targets);
  a.param_rows = device_rows(h->params);
  a.param_cols = device_cols(h->params);
  a.x_ref = device_rows(h->reference);
  a.ref_qn = h->ref_qn; a.ref_T = h->ref_T; a.ref_clock = (int32_t)h->ref_clock;
  a.spec_policy = h->x_spec ? sw.spec : 0;
  a.cluster = 1;
  a.cluster_sync = h->cluster_sync;
  // workgroup-per-problem kernels: clusters (cluster_size)
  // (limited handles: one workgroup per problem - no clusters, hence no early linearization or candidate groups either)
  if (h->large && h->cluster_sync && !h->limited && every_step_keypoint(h->d)) {
    const int g = cluster_size(h);
    // placement (MI_ILQR_CLUSTER_ORDER, A/B runs): 2 = a cluster on ONE XCD, the XCD's leaders in its first slots (default: measured
    // best or level for every model once early linearization is on); 1 = one XCD, members in consecutive slots (the quadrupeds'
    // helpers run 40 - 70 % slower next to leaders: neighbouring CUs share an instruction cache, and their linearization loops are
    // 50 - 90 KB of code); 0 = consecutive blocks, a cluster spans XCDs (what rounds 2 - 4 did; no early linearization there)
    // Early linearization (MI_ILQR_EARLY=0|1): every model, built-in or plugin (round 6).  Round 5 opened it for the built-in models
    // only: forced onto plugin chains with steps of a few hundred cycles the helpers linearized rows of the previous trial.  The cause
    // was not the progress word's lag but the helpers' side of the hand-shake - `buffer_inv sc0` does not drop another CU's lines
    // from the vector L1 (tools/ubench/l1_probe.hip), and a small trajectory survives there from one iteration to the next; the
    // helpers now read the trial with agent-scope loads and the progress word follows a full drain (ilqr_large.hpp).
    // candidate groups (MI_ILQR_LS_GROUPS=0|1): the helpers need trial buffers of their own, and - they keep their own LDS copy of
    // the cost constants - a target that does not move inside the launch
    bool still = true;
    for (int i = 0; i < h->n; ++i) still = still && h->mpc_target_step[i] == 0.0;
    if (h->target_steps_moving) still = false;
    if (h->reference.synced) still = false;     // (a reference trajectory: the window moves with the clock, and only the leader follows it)
    const bool lsg = sw.ls_groups && still && h->spec_slots >= 4 * g - 1 && g > 1;
    a.cluster = g | ((sw.cluster_order & 3) << 8) | ((sw.early ? 1 : 0) << 10) | ((lsg ? 1 : 0) << 11);
  }
  return a;
}

// Launch `mode` for the handle's model; afterwards the persistent state is no
// longer known-zero for the fields the mode writes, and u_bar is materialized.
// DevStats records of every enqueued solve that has none yet: ONE launch, a workgroup per pending ring slot.
int reduce_pending_stats(mi_ilqr* h) {
  { const int rc = join_slots(h); if (rc != MI_ILQR_OK) return rc; }      // (the pending slots' solves ran on both streams)
  long long first = h->stats_done;
  if (h->seq - first > mi_ilqr::kStatsRing) first = h->seq - mi_ilqr::kStatsRing;    // older slots were overwritten
  const int count = (int)(h->seq - first);
  if (count > 0) { const int rc = reduce_stats(h, (int)(first % mi_ilqr::kStatsRing), count); if (rc != MI_ILQR_OK) return rc; }
  h->stats_done = h->seq;
  return MI_ILQR_OK;
}

// ---- solve slots (host.hpp: SolveSlot, InputCopies; host_internal.hpp: join_slots)
// Stream `to` waits, on the device, for everything enqueued on stream `from` so far.
int order_behind(mi_ilqr* h, int from, int to) {
  HIPCHK(hipEventRecord(h->slots[from].ev, h->slots[from].stream));
  HIPCHK(hipStreamWaitEvent(h->slots[to].stream, h->slots[from].ev, 0));
  return MI_ILQR_OK;
}

// Before anything is enqueued on the OTHER slot's stream: it follows whatever the current stream got from the entry points that
// joined (uploads of costs or targets, a warm solve, an MPC loop ...) - one event after such work, none between two pipelined solves.
int fork_to_other(mi_ilqr* h) {
  if (h->fork_needed) {
    const int rc = order_behind(h, h->solve_slot, 1 - h->solve_slot);
    if (rc != MI_ILQR_OK) return rc;
    h->fork_needed = false;
  }
  h->other_pending = true;
  return MI_ILQR_OK;
}

// The second slot, allocated by the first launch that can use it: its arrays zeroed like slot 0's at create, the second copies of
// the inputs (nothing to vouch for yet), its stream.
int ensure_second_slot(mi_ilqr* h) {
  if (h->second_slot_ready) return MI_ILQR_OK;
  const size_t n = h->n, m = h->m, N = h->N, B = h->B, cap = (size_t)h->d.hist_cap;
  SolveSlot& s = h->slots[1];
  int rc = MI_ILQR_OK;
  auto zeroed = [&](auto*& p, size_t count) { if (rc == MI_ILQR_OK && !p) rc = dev_alloc(h, p, count, true); };
  zeroed(s.x_bar, B * n * N);
  zeroed(s.u_bar, B * m * (N - 1));
  zeroed(s.K, B * m * n * (N - 1));
  zeroed(s.kappa, B * m * (N - 1));
  zeroed(s.dV, B * (N - 1));
  zeroed(s.fx, B * n * n * (N - 1));
  zeroed(s.fu, B * n * m * (N - 1));
  zeroed(s.hist, B * cap * 4);
  zeroed(s.iter_cyc, B * cap * 4);
  zeroed(s.prof, B * 4);
  zeroed(s.kp_count, B);
  zeroed(s.kp_list, B * (N - 1));
  zeroed(s.done_counter, 1);
  if (h->slots[0].s2) zeroed(s.s2, B);
  zeroed(h->in_x0.copy[1], B * n);
  zeroed(h->in_u.copy[1], B * m * (N - 1));
  if (rc != MI_ILQR_OK) return rc;
  HIPCHK(hipStreamSynchronize(nullptr));      // (the zeros went through the null stream, which the slots' streams do not follow)
  if (!s.stream) HIPCHK(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
  for (SolveSlot& q : h->slots) if (!q.ev) HIPCHK(hipEventCreateWithFlags(&q.ev, hipEventDisableTiming));
  h->second_slot_ready = true;
  return MI_ILQR_OK;
}

// A launch on slot t reads copy t of the inputs: brought up to date, on t's stream, when the latest write went to the other copy (the
// first launch on the slot, or a mi_ilqr_set_initial that could not tell where the next solve would go).
int sync_input(mi_ilqr* h, InputCopies& in, int t, size_t bytes) {
  if (in.version[t] != in.version[in.latest]) {
    const int src = in.latest;
    const int rc = order_behind(h, src, t);
    if (rc != MI_ILQR_OK) return rc;
    HIPCHK(hipMemcpyAsync(in.copy[t], in.copy[src], bytes, hipMemcpyDeviceToDevice, h->slots[t].stream));
    in.version[t] = in.version[src];
    in.read_across[src] = true;
  }
  in.latest = t;
  return MI_ILQR_OK;
}
int sync_inputs(mi_ilqr* h, int t) {
  int rc = sync_input(h, h->in_x0, t, (size_t)h->B * h->n * 8);
  if (rc == MI_ILQR_OK) rc = sync_input(h, h->in_u, t, (size_t)h->B * h->m * (h->N - 1) * 8);
  h->x0 = h->in_x0.copy[h->in_x0.latest]; h->u_guess = h->in_u.copy[h->in_u.latest];
  return rc;
}

// mi_ilqr_set_initial(_shared) write "the inputs of the NEXT solve" and return at once.  The slot whose copy and stream the write
// goes to is the one that solve will take as far as the handle can tell now: the other one while solves are in flight on a handle
// that overlaps them, else the current one.  A wrong guess costs overlap, not correctness (sync_inputs).
int input_slot(const mi_ilqr* h) {
  const bool other = h->second_slot_ready && h->n_slots == 2 && !h->sink_x && h->hold == 0 && h->inflight > 0;
  return other ? 1 - h->solve_slot : h->solve_slot;
}
// ... and the write itself, between begin and end: on slot w's stream (h->stream names it meanwhile), behind every solve that reads
// copy w - those run on the same stream - and behind a device copy that read it from the other one.
struct InputWrite {
  mi_ilqr* h;
  int w;
  hipStream_t keep;
  int rc = MI_ILQR_OK;
  explicit InputWrite(mi_ilqr* h_) : h(h_), w(input_slot(h_)), keep(h_->stream) {
    if (w != h->solve_slot) rc = fork_to_other(h);
    for (InputCopies* in : {&h->in_x0, &h->in_u})
      if (rc == MI_ILQR_OK && in->read_across[w]) { rc = order_behind(h, 1 - w, w); in->read_across[w] = false; }
    h->stream = h->slots[w].stream;
  }
  ~InputWrite() { h->stream = keep; }
  double* begin(InputCopies& in) const { return in.copy[w]; }
  void end(InputCopies& in, double*& alias) const { in.version[w] = ++in.writes; in.latest = w; alias = in.copy[w]; }
};

double bytes_per_iteration(int n, int m, int N, int ls) {
  const double roll = 2.0 * n * N + (3.0 * m + (double)m * n) * (N - 1) + n + 1;
  const double deriv = (N - 1.0) * ((n + m) + ((double)n * n + (double)n * m));
  const double back = (N - 1.0) * ((n + m) + ((double)n * n + (double)n * m) + ((double)m * n + m + 1)) + n;
  return 8.0 * (ls * roll + deriv + back);
}

// The device and host resources of a new handle, zeroed.  mi_ilqr_create destroys the handle when this fails, which frees whatever
// was allocated up to there.
int create_resources(mi_ilqr* h, bool lxu_hbm) {
  const size_t n = h->n, m = h->m, N = h->N, B = h->B;
  const bool large = h->large, batch_minor = h->batch_minor, every_step = every_step_keypoint(h->d);
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->d.device_id) == hipSuccess) h->n_cus = cus;
  }
  int rc = MI_ILQR_OK;      // (sticky: after a failed allocation the ones behind it are not tried)
  auto zeroed = [&](auto*& p, size_t count) { if (rc == MI_ILQR_OK) rc = dev_alloc(h, p, count, true); };
  zeroed(h->x_bar, B * n * N);
  zeroed(h->u_bar, B * m * (N - 1));
  zeroed(h->K, B * m * n * (N - 1));
  zeroed(h->kappa, B * m * (N - 1));
  zeroed(h->dV, B * (N - 1));
  zeroed(h->fx, B * n * n * (N - 1));
  zeroed(h->fu, B * n * m * (N - 1));
  const bool host_rec = B <= 4;              // (host.hpp: host_records)
  const bool host_in = host_rec && !large && !batch_minor;   // ... and the inputs x0, u_guess (wave-per-problem kernels: the boundary's layout)
  if (!host_in) {
    zeroed(h->x0, B * n);
    zeroed(h->u_guess, B * m * (N - 1));
  }
  zeroed(h->cost_ring, B * mi_ilqr::kStatsRing);
  if (host_rec) {
    auto up = [](size_t v) { return (v + 63) & ~(size_t)63; };
    const size_t s_hist = up(B * (size_t)h->d.hist_cap * 4 * 8), s_prof = up(B * 4 * 8), s_ring = up(B * mi_ilqr::kStatsRing * 4);
    const size_t s_x0 = host_in ? up(B * n * 8) : 0, s_ug = host_in ? up(B * m * (N - 1) * 8) : 0;
    h->host_records_bytes = 2 * s_hist + s_prof + 2 * s_ring + s_x0 + s_ug;
    void* dv = nullptr;
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h->host_records), h->host_records_bytes, hipHostMallocMapped));
    HIPCHK(hipHostGetDevicePointer(&dv, h->host_records, 0));
    std::memset(h->host_records, 0, h->host_records_bytes);
    h->host_records_dev = static_cast<char*>(dv);
    char* q = h->host_records_dev;
    h->hist = reinterpret_cast<double*>(q); q += s_hist;
    h->iter_cyc = reinterpret_cast<double*>(q); q += s_hist;
    h->prof = reinterpret_cast<long long*>(q); q += s_prof;
    h->iters_ring = reinterpret_cast<int32_t*>(q); q += s_ring;
    h->status_ring = reinterpret_cast<int32_t*>(q); q += s_ring;
    if (host_in) { h->x0 = reinterpret_cast<double*>(q); q += s_x0; h->u_guess = reinterpret_cast<double*>(q); h->host_inputs = true; }
  } else {
    zeroed(h->hist, B * (size_t)h->d.hist_cap * 4);
    zeroed(h->iter_cyc, B * (size_t)h->d.hist_cap * 4);
  }
  zeroed(h->x_trial, B * n * N);
  zeroed(h->u_trial, B * m * (N - 1));
  zeroed(h->trial_cost, B * 2);
  zeroed(h->stage_in, B);
  zeroed(h->costmat, cost_len(h) + n);
  if (!host_rec) {
    zeroed(h->iters_ring, B * mi_ilqr::kStatsRing);
    zeroed(h->status_ring, B * mi_ilqr::kStatsRing);
    zeroed(h->prof, B * 4);
  }
  zeroed(h->ls_ring, B * mi_ilqr::kStatsRing);
  zeroed(h->kp_count, B);
  zeroed(h->kp_list, B * (N - 1));
  zeroed(h->done_counter, 1);
  if (large) zeroed(h->cluster_sync, B * kSyncWords);
  if (lxu_hbm) zeroed(h->lxu, B * (N - 1) * (n + m));
  if (batch_minor && !every_step) zeroed(h->bm_scratch, B * 6 * (N - 1));
  if (rc != MI_ILQR_OK) return rc;
  if (large && n <= 32) {
    // mid-size kernels: four line-search candidates per pass - an optimization, so a batch too large for three more
    // trial buffers simply searches one candidate at a time (make_args: spec_policy = 0 without them)
    // (batches small enough for clusters: 31 slots - the candidates 1 .. 31 of a first pass that the leader and up to seven helper
    //  workgroups roll out together, ilqr_large.hpp: candidate groups)
    // ... as many as the cluster size make_args will pick asks for (cluster_size): 4 g - 1 (15 at B = 64 on 256 CUs), 3 when the
    // launch will not be clustered - plugin models unless MI_ILQR_CLUSTER forces it, batches beyond 64, fewer than two CUs per
    // problem.  (Round 5 allocated 31 for every batch up to 64: 1 GB of HBM for nothing on an n = 32, N = 2000 plugin.)
    // (a failure here is an answer, not an error: plain hipMalloc, and the pair joins the handle's allocations once it stands)
    const int g = cluster_size(h);
    h->spec_slots = g > 1 ? 4 * g - 1 : 3;
    for (;;) {
      const size_t xb = (size_t)h->spec_slots * B * n * N * sizeof(double), ub = (size_t)h->spec_slots * B * m * (N - 1) * sizeof(double);
      if (hipMalloc(reinterpret_cast<void**>(&h->x_spec), xb) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&h->u_spec), ub) == hipSuccess) break;
      (void)hipGetLastError();
      if (h->x_spec) (void)hipFree(h->x_spec);
      h->x_spec = nullptr; h->u_spec = nullptr;
      if (h->spec_slots == 3) { h->spec_slots = 0; break; }
      h->spec_slots = 3;
    }
    if (h->x_spec) { h->owned.push_back(h->x_spec); h->owned.push_back(h->u_spec); }
  }
  if (batch_minor && every_step) {
    // the KP = false lane-per-problem kernels never write the key-point list: every step is a key-point (ilqr.py:417-432), the
    // same list for every problem and every linearization - stored once here
    std::vector<int32_t> kl(B * (N - 1));
    for (size_t i = 0; i < kl.size(); ++i) kl[i] = (int32_t)(i % (N - 1));
    HIPCHK(hipMemcpy(h->kp_list, kl.data(), kl.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  // defaults Q=I, R=I, Qf=I, x_nom=0 (ilqr.py:61-67)
  {
    std::vector<double> cm(cost_len(h) + n, 0.0);
    for (size_t i = 0; i < n; ++i) { cm[i * n + i] = 1.0; cm[n * n + m * m + i * n + i] = 1.0; }
    for (size_t i = 0; i < m; ++i) cm[n * n + i * m + i] = 1.0;
    HIPCHK(hipMemcpy(h->costmat, cm.data(), cm.size() * 8, hipMemcpyHostToDevice));
    h->h_costmat = cm;
    h->costmat_synced = true;
  }
  HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  {
    // slot 0 is what was allocated above.  Which handles get a second one, lazily: the wave-per-problem family - its SOLVE kernel has
    // no synchronisation between workgroups but the statistics ticket (a slot's own) -, more than four problems (tiny batches read
    // their inputs from mapped host memory and serialize by design), and at most four launches' worth of one wave per SIMD:
    // beyond that a batch's own later workgroups fill the SIMDs its finished problems leave.
    SolveSlot& s = h->slots[0];
    s.x_bar = h->x_bar; s.u_bar = h->u_bar; s.K = h->K; s.kappa = h->kappa; s.dV = h->dV; s.fx = h->fx; s.fu = h->fu;
    s.hist = h->hist; s.iter_cyc = h->iter_cyc; s.prof = h->prof; s.kp_count = h->kp_count; s.kp_list = h->kp_list;
    s.done_counter = h->done_counter; s.stream = h->stream;
    h->in_x0.copy[0] = h->x0; h->in_u.copy[0] = h->u_guess;
    const bool family = !large && !batch_minor && B > 4;
    h->n_slots = (switches().solve_slots == 2 && family && h->n_cus > 0 && B <= 16 * (size_t)h->n_cus) ? 2 : 1;
  }
  for (int i = 0; i < mi_ilqr::kStatsRing; ++i) {
    HIPCHK(hipEventCreate(&h->ring_ev0[i]));
    HIPCHK(hipEventCreate(&h->ring_ev1[i]));
  }
  HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h->h_ring), sizeof(DevStats) * mi_ilqr::kStatsRing, hipHostMallocMapped));
  HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->d_ring), h->h_ring, 0));
  std::memset(h->h_ring, 0, sizeof(DevStats) * mi_ilqr::kStatsRing);
  select_stats_slot(h, 0);
  return MI_ILQR_OK;
}

// Symmetric positive semi-definite (definite with `strict`)?  Cholesky of A + eps*I; the matrices are tiny.
bool is_sym_psd(const double* A, int k, bool strict) {
  double scale = 0.0;
  for (int i = 0; i < k * k; ++i) { if (!(std::fabs(A[i]) < INFINITY)) return false; scale = std::fmax(scale, std::fabs(A[i])); }
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < i; ++j) if (A[i * k + j] != A[j * k + i]) return false;
  std::vector<double> L((size_t)k * k, 0.0);
  const double eps = strict ? 0.0 : 1e-12 * scale * k;
  for (int j = 0; j < k; ++j) {
    double d = A[j * k + j] + eps;
    for (int q = 0; q < j; ++q) d -= L[j * k + q] * L[j * k + q];
    if (strict ? !(d > 0.0) : !(d >= 0.0)) return false;
    const double ld = std::sqrt(d);
    L[j * k + j] = ld;
    for (int i = j + 1; i < k; ++i) {
      double v = A[i * k + j];
      for (int q = 0; q < j; ++q) v -= L[i * k + q] * L[j * k + q];
      if (ld > 0.0) L[i * k + j] = v / ld;
      else if (std::fabs(v) > 1e-12 * scale) return false;      // zero pivot with a non-zero column: indefinite
    }
  }
  return true;
}

// The cost class of one set of matrices, cm = Q | R | Qf (mi_ilqr_set_cost and every row of MI_F_COST_MATRICES decide it here):
// `regular` - symmetric, Q and Qf positive semi-definite, R positive definite: the fast backward forms; otherwise the reference's
// recursion (exact_backward), and on the workgroup-per-problem kernels `asym` when a matrix is not symmetric.  May write cm: the
// n >= 33 kernels' round-off symmetrisation.  MI_ILQR_E_UNSUPPORTED: a non-finite entry the workgroup-per-problem kernels cannot take
// (mi_ilqr_set_cost only: the rows of MI_F_COST_MATRICES are finite when they get here - set_cost_rows refuses others up front,
// for every kernel family, with the MI_ILQR_E_BAD_ARG the header documents).
int classify_cost(const mi_ilqr* h, double* cm, bool* regular_out, bool* asym_out) {
  const size_t n = h->n, m = h->m;
  // The time-parallel / matrix-core backward passes use Vxx = Vxx^T and (scan) PSD second-order terms; the
  // reference accepts ANY Q, R, Qf and never symmetrizes (ilqr.py:182,653-667).  Matrices outside that
  // class are served by the reference's recursion verbatim (wave- and lane-per-problem kernels), by the mid-size
  // matrix-core pass with every use of symmetry switched off (n <= 32), or refused (n >= 33).
  if (h->large && n > 32) {
    // The n >= 33 workgroup-per-problem kernels' matrix-core pass has no form without symmetry (the plain-arithmetic pass that
    // takes over - large_backward_asym - is ~4 x slower per step), and matrices built as A^T A or by float arithmetic are often
    // symmetric only to round-off: asymmetries up to a few ulps of the largest entry are averaged away here
    // (|A - A^T| <= 8 eps max|A|) so that they keep the fast pass; anything larger is followed as given.
    // (n <= 32: matrices are taken as given, like the reference does.)
    auto symmetrize = [](double* A, size_t k) {
      double scale = 0.0;
      for (size_t i = 0; i < k * k; ++i) scale = std::fmax(scale, std::fabs(A[i]));
      for (size_t i = 0; i < k; ++i)
        for (size_t j = 0; j < i; ++j) if (std::fabs(A[i * k + j] - A[j * k + i]) > 8 * 2.220446049250313e-16 * scale) return;
      for (size_t i = 0; i < k; ++i)
        for (size_t j = 0; j < i; ++j) A[i * k + j] = A[j * k + i] = 0.5 * (A[i * k + j] + A[j * k + i]);
    };
    symmetrize(cm, n); symmetrize(cm + n * n, m); symmetrize(cm + n * n + m * m, n);
  }
  const bool regular = is_sym_psd(cm, (int)n, false) && is_sym_psd(cm + n * n + m * m, (int)n, false) &&
                       is_sym_psd(cm + n * n, (int)m, true);
  bool asym = false;
  if (!regular && h->large) {
    // Definiteness is not required of the workgroup-per-problem kernels - they check it where it matters: every
    // Quu = 2R + fu^T Vxx fu of every backward pass (MI_STATUS_NOT_PD, or mi_ilqr_desc.on_indefinite = 1: inverted with partial
    // pivoting like the reference's np.linalg.inv, ilqr.py:655).  SYMMETRY: the mid-size kernels (n <= 32, mid_backward) follow
    // the reference on any matrices - lxx = 2Q and luu = 2R as given, lx = 2Qx - 2 x_nom^T Q, Vx' = Qx - Qu^T Quu^{-1} Qux with
    // the inverse of a Quu that is not symmetric, Vxx stored in full (ilqr.py:180-184,651-667); the n >= 33 kernels, whose
    // matrix-core pass mirrors tiles of the symmetric products, take a plain-arithmetic pass for such matrices (round 6:
    // large_backward_asym; they refused them before).
    auto finite = [](const double* A, size_t k) {
      for (size_t i = 0; i < k * k; ++i) if (!(std::fabs(A[i]) < INFINITY)) return false;
      return true;
    };
    auto symmetric = [](const double* A, size_t k) {
      for (size_t i = 0; i < k; ++i)
        for (size_t j = 0; j < i; ++j) if (A[i * k + j] != A[j * k + i]) return false;
      return true;
    };
    if (!(finite(cm, n) && finite(cm + n * n, m) && finite(cm + n * n + m * m, n))) return MI_ILQR_E_UNSUPPORTED;
    asym = !(symmetric(cm, n) && symmetric(cm + n * n, m) && symmetric(cm + n * n + m * m, n));
  }
  *regular_out = regular; *asym_out = asym;
  return MI_ILQR_OK;
}

// the class the kernels run with: the rows' in per-problem mode, the shared matrices' otherwise
void apply_cost_class(mi_ilqr* h) {
  h->exact_backward = h->costs.synced ? h->rows_exact_backward : h->shared_exact_backward;
  h->cost_asym = h->costs.synced ? h->rows_cost_asym : h->shared_cost_asym;
}

void drop_per_problem_costs(mi_ilqr* h) {
  store_drop(h->costs);
  apply_cost_class(h);
}

// tiny batches of the wave-per-problem kernels keep x0 / u_guess in page-locked host memory the kernels read directly (host.hpp:
// host_inputs): setting them is a memcpy once nothing on the stream can still be reading the old values - no copy engine, no
// broadcast kernel in front of the solve (C1: two ~5 us copies + one launch off the critical path of every Solve())
int host_inputs_write(mi_ilqr* h, const double* x0, const double* u_guess, bool shared) {
  const hipError_t q = hipStreamQuery(h->stream);
  if (q == hipErrorNotReady) HIPCHK(hipStreamSynchronize(h->stream));
  else if (q != hipSuccess) return MI_ILQR_E_HIP;
  char* const base = h->host_records;
  if (x0) std::memcpy(base + (reinterpret_cast<char*>(h->x0) - h->host_records_dev), x0, (size_t)h->B * h->n * 8);
  if (u_guess) {
    const size_t one = (size_t)h->m * (h->N - 1) * 8;
    char* dst = base + (reinterpret_cast<char*>(h->u_guess) - h->host_records_dev);
    for (int b = 0; b < h->B; ++b) std::memcpy(dst + b * one, reinterpret_cast<const char*>(u_guess) + (shared ? 0 : b * one), one);
    h->u_pending = true;
    h->u_zero = false;
  }
  return MI_ILQR_OK;
}

// Whether a workgroup-per-problem handle has Limited<M> kernels: the mid-size layout (n <= 32), and kernels the model was built
// with (asked through its launch entry, which launches nothing for the probe).
bool large_accepts_limits(mi_ilqr* h) {
  if (h->n > 32) return false;
  const KArgs a = make_args(h);
  return model_of(h->d.model_id)->p.launch(h, kModeProbeLimits, &a) == MI_ILQR_OK;
}

void fill_stats(mi_ilqr* h, int slot, mi_ilqr_stats* st) {
  std::memset(st, 0, sizeof(*st));
  const DevStats ds = h->h_ring[slot];   // written by stats_kernel, visible after a stream sync
  st->total_iters = ds.total_iters; st->total_ls_trials = ds.total_ls;
  st->n_converged = ds.n_conv; st->n_max_iters = ds.n_max; st->n_ls_failed = ds.n_fail;
  st->max_iters_seen = ds.max_iters_seen; st->best_cost = ds.best_cost; st->best_index = ds.best_index;
  st->n_internal = ds.n_internal; st->n_not_pd = ds.n_not_pd;
  float ms = 0.f;
  if (h->ring_timed[slot] && hipEventElapsedTime(&ms, h->ring_ev0[slot], h->ring_ev1[slot]) == hipSuccess) st->kernel_ms = ms;
  // bytes_iter is affine in ls: sum over iterations = ls_total*roll + iters*(deriv+back)
  const double per_ls = bytes_per_iteration(h->n, h->m, h->N, 1) - bytes_per_iteration(h->n, h->m, h->N, 0);
  const double fixed = bytes_per_iteration(h->n, h->m, h->N, 0);
  st->algorithmic_bytes = per_ls * (double)st->total_ls_trials + fixed * (double)st->total_iters;
}

int upload_stage_in(mi_ilqr* h, const double* v) {
  if (!v) return MI_ILQR_E_BAD_ARG;
  HIPCHK(hipSetDevice(h->d.device_id));
  { const int rc = join_slots(h); if (rc != MI_ILQR_OK) return rc; }
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(h->stage_in, v, (size_t)h->B * 8, hipMemcpyHostToDevice));
  return MI_ILQR_OK;
}

}  // namespace

int reduce_stats(mi_ilqr* h, int first_slot, int count) {
  hipLaunchKernelGGL(stats_kernel, dim3(count), dim3(256), 0, h->stream, h->iters_ring, h->status_ring, h->ls_ring, h->cost_ring,
                     h->B, h->d_ring, first_slot, (int)mi_ilqr::kStatsRing);
  HIPCHK(hipGetLastError());
  return MI_ILQR_OK;
}

int join_slots_now(mi_ilqr* h) {
  if (h->other_pending) {
    HIPCHK(hipSetDevice(h->d.device_id));
    const int rc = order_behind(h, 1 - h->solve_slot, h->solve_slot);
    if (rc != MI_ILQR_OK) return rc;
    h->other_pending = false;
  }
  h->fork_needed = true;
  return MI_ILQR_OK;
}

const Model* model_of(int id) {
  if (id >= 0 && id < kNumBuiltins) return &kBuiltins[id];
  const int s_ = id - MI_MODEL_PLUGIN_BASE;
  return (s_ >= 0 && s_ < MI_ILQR_MAX_PLUGINS && g_plugins[s_].used.load(std::memory_order_acquire)) ? &g_plugins[s_].model : nullptr;
}

int launch(mi_ilqr* h, int mode) {
  HIPCHK(hipSetDevice(h->d.device_id));
  if (!h->in_async_solve) { const int rc = join_slots(h); if (rc != MI_ILQR_OK) return rc; }   // (mi_ilqr_solve_async has chosen the slot)
  if (h->costs.synced && h->batch_minor && !h->targets.synced) { const int rc = refresh_lane_target_rows(h); if (rc != MI_ILQR_OK) return rc; }
  // any launch other than a pipelined solve reuses the current ring slot: settle the statistics still owed first
  if (!h->in_async_solve) { const int rc = reduce_pending_stats(h); if (rc != MI_ILQR_OK) return rc; }
  if (h->u_zero && !h->u_pending) HIPCHK(hipMemsetAsync(h->u_bar, 0, (size_t)h->B * h->m * (h->N - 1) * 8, h->stream));
  h->u_zero = false;
  const KArgs a = make_args(h);
  return model_of(h->d.model_id)->p.launch(h, mode, &a);
}

// When the state is lazily-zero (cold) but a kernel is about to write only part
// of it, materialize the zeros first.
int materialize_zero_state(mi_ilqr* h) {
  if (!h->cold) return MI_ILQR_OK;
  { const int rc = join_slots(h); if (rc != MI_ILQR_OK) return rc; }
  const size_t n = h->n, m = h->m, N = h->N, B = h->B;
  HIPCHK(hipMemsetAsync(h->x_bar, 0, B * n * N * 8, h->stream));
  HIPCHK(hipMemsetAsync(h->K, 0, B * m * n * (N - 1) * 8, h->stream));
  HIPCHK(hipMemsetAsync(h->kappa, 0, B * m * (N - 1) * 8, h->stream));
  HIPCHK(hipMemsetAsync(h->dV, 0, B * (N - 1) * 8, h->stream));
  HIPCHK(hipMemsetAsync(h->fx, 0, B * n * n * (N - 1) * 8, h->stream));
  HIPCHK(hipMemsetAsync(h->fu, 0, B * n * m * (N - 1) * 8, h->stream));
  if (h->s2) HIPCHK(hipMemsetAsync(h->s2, 0, B * 8, h->stream));
  h->cold = false;
  return MI_ILQR_OK;
}

int materialize_u(mi_ilqr* h) {
  { const int rc = join_slots(h); if (rc != MI_ILQR_OK) return rc; }
  if (h->u_zero && !h->u_pending) HIPCHK(hipMemsetAsync(h->u_bar, 0, (size_t)h->B * h->m * (h->N - 1) * 8, h->stream));
  h->u_zero = false;
  if (!h->u_pending) return MI_ILQR_OK;
  HIPCHK(hipMemcpyAsync(h->u_bar, h->u_guess, (size_t)h->B * h->m * (h->N - 1) * 8, h->host_inputs ? hipMemcpyDefault : hipMemcpyDeviceToDevice, h->stream));
  h->u_pending = false;
  return MI_ILQR_OK;
}

// Per-problem cost matrices (MI_F_COST_MATRICES): (B, 2 n^2 + m^2) rows, row b = Q_b | R_b | Qf_b.  Every row is classified like
// mi_ilqr_set_cost classifies the shared matrices, and the handle runs the most general form a row needs.  What is stored (and
// mi_ilqr_get returns) is the rows as the kernels get them, i.e. after the n >= 33 round-off symmetrisation.  src == NULL with
// bytes == 0: back to the shared matrices.
int set_cost_rows(mi_ilqr* h, const double* src, size_t bytes) {
  const size_t B = h->B, len = cost_len(h);
  if (const int rc = rows_given(h->costs, src, bytes, B * len); rc != kRowsGiven) {
    if (rc == MI_ILQR_OK) apply_cost_class(h);       // (dropped: the shared matrices' class again)
    return rc;
  }
  for (size_t i = 0; i < B * len; ++i) if (!std::isfinite(src[i])) return MI_ILQR_E_BAD_ARG;
  std::vector<double> rows(src, src + B * len);
  bool regular_all = true, asym_any = false;
  for (size_t b = 0; b < B; ++b) {
    bool regular = true, asym = false;
    const int rc = classify_cost(h, rows.data() + b * len, &regular, &asym);
    if (rc != MI_ILQR_OK) return rc;
    regular_all = regular_all && regular;
    asym_any = asym_any || asym;
  }
  // the rows' class is committed with the rows: a call refused above changes nothing, a failed copy leaves the shared matrices' class
  const int rc = store_upload(h, h->costs, rows.data());
  if (rc == MI_ILQR_OK) { h->rows_exact_backward = regular_all ? 0 : 1; h->rows_cost_asym = asym_any ? 1 : 0; }
  apply_cost_class(h);
  return rc;
}

}  // namespace mi_host

extern "C" {

int mi_ilqr_abi_version(void) { return MI_ILQR_ABI_VERSION; }
void mi_ilqr_struct_sizes(int32_t* desc_bytes, int32_t* stats_bytes, int32_t* plugin_bytes) {
  if (desc_bytes) *desc_bytes = (int32_t)sizeof(mi_ilqr_desc);
  if (stats_bytes) *stats_bytes = (int32_t)sizeof(mi_ilqr_stats);
  if (plugin_bytes) *plugin_bytes = (int32_t)sizeof(mi_ilqr_model_plugin);
}

const char* mi_ilqr_strerror(int code) {
  switch (code) {
    case MI_ILQR_OK: return "ok";
    case MI_ILQR_E_BAD_SHAPE: return "bad shape";
    case MI_ILQR_E_BAD_METHOD: return "unknown interpolation method";
    case MI_ILQR_E_LINESEARCH: return "linesearch failed";
    case MI_ILQR_E_HIP: return "HIP runtime error";
    case MI_ILQR_E_NO_DEVICE: return "no usable gfx950 device (there is no CPU fallback)";
    case MI_ILQR_E_BAD_ARG: return "bad argument";
    case MI_ILQR_E_UNSUPPORTED: return "model/size/cost combination not supported by any kernel";
    case MI_ILQR_E_RCCL: return "RCCL error (librccl missing, or a communicator / collective call failed)";
  }
  return "unknown error";
}

int mi_ilqr_register_model(const mi_ilqr_model_plugin* p, int32_t* model_id_out) {
  if (!p || !model_id_out || !p->launch || !p->lds_bytes) return MI_ILQR_E_BAD_ARG;
  if (p->abi_version != MI_ILQR_ABI_VERSION || p->kernel_args_bytes != (int32_t)sizeof(KArgs) || p->handle_bytes != (int32_t)sizeof(mi_ilqr)) {
    std::fprintf(stderr, "mi_ilqr_register_model: plugin built against other headers (ABI %d, %d-byte kernel arguments, %d-byte handle; the library: %d, %d, %d)\n",
                 p->abi_version, p->kernel_args_bytes, p->handle_bytes, MI_ILQR_ABI_VERSION, (int)sizeof(KArgs), (int)sizeof(mi_ilqr));
    return MI_ILQR_E_BAD_ARG;
  }
  if (p->n < 1 || p->m < 1 || p->n > kMaxStateDim || p->n_params < 0 || p->n_params > MI_ILQR_MAX_PARAMS) return MI_ILQR_E_BAD_SHAPE;
  if (p->m_user < 0 || p->m_user > p->m) return MI_ILQR_E_BAD_SHAPE;     // (0: no padding controls)
  // family 0: wave-per-problem kernels (m <= 2); family 1: workgroup-per-problem kernels - n <= 32 with any m <= 16
  // (mid_backward), 32 < n <= 40 with m % 4 == 0 and 2 m <= n (large_backward's wave roles)
  if (p->family == 0 ? p->m > 2
                     : (p->family != 1 || p->m > 16 || (p->n > 32 && (2 * p->m > p->n || p->m % 4 != 0)))) return MI_ILQR_E_UNSUPPORTED;
  std::lock_guard<std::mutex> lock(g_plugins_mutex);                     // (readers: model_of, lock-free)
  for (int s_ = 0; s_ < MI_ILQR_MAX_PLUGINS; ++s_) {
    if (g_plugins[s_].used.load(std::memory_order_relaxed)) continue;
    PluginSlot& ps = g_plugins[s_];
    ps.model = Model{*p, 0};
    ps.used.store(true, std::memory_order_release);
    *model_id_out = MI_MODEL_PLUGIN_BASE + s_;
    return MI_ILQR_OK;
  }
  return MI_ILQR_E_UNSUPPORTED;                                       // registry full
}

int mi_ilqr_model_info(int model_id, int32_t* n, int32_t* m, int32_t* n_params, double* default_params) {
  const Model* mod = model_of(model_id);
  if (!mod) return MI_ILQR_E_BAD_ARG;
  const mi_ilqr_model_plugin& p = mod->p;
  if (n) *n = p.n;
  if (m) *m = p.m;
  if (n_params) *n_params = p.n_params;
  if (default_params) for (int i = 0; i < MI_ILQR_MAX_PARAMS; ++i) default_params[i] = i < p.n_params ? p.default_params[i] : 0.0;
  return MI_ILQR_OK;
}

double mi_ilqr_bytes_per_iteration(int32_t n, int32_t m, int32_t N, int32_t ls) { return bytes_per_iteration(n, m, N, ls); }

size_t mi_ilqr_lds_bytes(const mi_ilqr_desc* d) {
  const Model* mod = d ? model_of(d->model_id) : nullptr;
  return mod ? mod->p.lds_bytes(d->N, 1) : 0;
}

int mi_ilqr_create(const mi_ilqr_desc* desc, mi_ilqr_t** out) {
  if (!desc || !out) return MI_ILQR_E_BAD_ARG;
  *out = nullptr;
  const Model* mod = model_of(desc->model_id);
  if (!mod) return MI_ILQR_E_BAD_ARG;
  const mi_ilqr_model_plugin& model = mod->p;
  if (desc->n != model.n || desc->m != model.m) return MI_ILQR_E_BAD_SHAPE;
  if (desc->N < 2 || desc->B < 1) return MI_ILQR_E_BAD_SHAPE;
  if (desc->keypoint_method < MI_KP_SET_INTERVAL || desc->keypoint_method > MI_KP_ITERATIVE_ERROR) return MI_ILQR_E_BAD_METHOD;
  if (desc->minN < 1) return MI_ILQR_E_BAD_ARG;
  // adaptiveJerk with maxN < 1 can append two key-points per step (ilqr.py:452-463): its list would outgrow the N - 1 slots
  // of every key-point buffer.  The other methods never read maxN (callers pass 0 with setInterval).
  if (desc->keypoint_method == MI_KP_ADAPTIVE_JERK && desc->maxN < 1) return MI_ILQR_E_BAD_ARG;
  if (desc->jacobian_mode != MI_JAC_FD_CENTRAL && desc->jacobian_mode != MI_JAC_AUTODIFF) return MI_ILQR_E_BAD_ARG;
  if (desc->jacobian_mode == MI_JAC_FD_CENTRAL && !(desc->fd_step > 0.0)) return MI_ILQR_E_BAD_ARG;

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MI_ILQR_E_NO_DEVICE;
  if (desc->device_id < 0 || desc->device_id >= ndev) return MI_ILQR_E_NO_DEVICE;
  HIPCHK(hipSetDevice(desc->device_id));

  const bool large = model.family == 1;
  size_t lds = model.lds_bytes(desc->N, 1);
  int n_store = 1;
  if (lds == 0) return MI_ILQR_E_UNSUPPORTED;
  bool batch_minor = false;
  if (desc->kernel_mode < MI_KERNEL_AUTO || desc->kernel_mode > MI_KERNEL_THROUGHPUT) return MI_ILQR_E_BAD_ARG;
  if (desc->on_indefinite != 0 && desc->on_indefinite != 1) return MI_ILQR_E_BAD_ARG;
  {
    // (every key-point configuration since round 4: the KP instantiation of the lane-per-problem kernels)
    // family 0 with n <= 6: the models whose units instantiate the lane-per-problem kernels as well (every built-in one; per-lane
    // register arrays of n x n doubles set the limit)
    const bool can = model.family == 0 && model.n <= kMaxBatchPluginN;
    if (desc->kernel_mode == MI_KERNEL_THROUGHPUT && !can) return MI_ILQR_E_UNSUPPORTED;
    // n = 2 within the time-parallel passes' horizon: the wave-per-problem kernel is the faster one at
    // every batch size (B = 65536: 68 M vs 42 M it/s, profiles/r01n_c2_modes_batch_sweep.txt)
    const bool time_parallel = model.n == 2 && model.m == 1 && desc->N - 1 <= 256;
    batch_minor = can && (desc->kernel_mode == MI_KERNEL_THROUGHPUT ||
                          (desc->kernel_mode == MI_KERNEL_AUTO && desc->B >= 8192 && !time_parallel));
    // horizons whose per-problem state exceeds the 160 KB of LDS (e.g. acrobot.py's literal N = 750) are
    // served by the HBM-streaming kernel, which has no such limit
    if (!batch_minor && lds > kMaxLds && can && desc->kernel_mode == MI_KERNEL_AUTO) batch_minor = true;
  }
  bool lxu_hbm = false;
  if (!batch_minor && lds > kMaxLds && large) {
    // the horizon's cost gradients do not fit beside the fixed block: keep them in HBM (lds_layout.hpp: large_lds_bytes_hbm)
    const size_t l = model.lds_bytes(desc->N, -1);
    if (l != 0 && l <= kMaxLds) { lds = l; lxu_hbm = true; }
  }
  if (!batch_minor && lds > kMaxLds) return MI_ILQR_E_UNSUPPORTED;
  if (batch_minor) lds = 0;
  if (!large && !batch_minor && desc->beta <= 0.75) {
    // Coarse backtracking (beta <= 0.75) accepts one of the first few eps values: keep up to 6
    // candidate trajectories in LDS as long as that does not lower the problems-per-CU this
    // batch needs (256 CUs) — it removes the second rollout of a backtracking iteration.
    const size_t per_cu_needed = ((size_t)desc->B + 255) / 256;
    for (int ns = 6; ns > 1; --ns) {
      const size_t l = model.lds_bytes(desc->N, ns);
      if (l <= kMaxLds && kMaxLds / l >= per_cu_needed) { n_store = ns; lds = l; break; }
    }
  }

  mi_ilqr* h = new (std::nothrow) mi_ilqr();
  if (!h) return MI_ILQR_E_BAD_ARG;
  h->d = *desc;
  if (h->d.max_iters <= 0) h->d.max_iters = 1000;
  if (h->d.hist_cap <= 0) h->d.hist_cap = 64;
  h->n = desc->n; h->m = desc->m; h->N = desc->N; h->B = desc->B;
  h->lds = lds;
  h->large = large;
  h->n_store = n_store;
  h->batch_minor = batch_minor;
  h->targets.width = h->target_steps.width = h->lane_targets.width = h->n;
  h->params.width = model.n_params;
  h->costs.width = cost_len(h);
  h->policy_noise.width = h->plant_noise.width = h->n + h->m;
  h->policy_mc_dist.width = 3 * (size_t)h->n + 2 * (size_t)model.n_params;
  h->mc_box.width = 2 * (size_t)h->n;
  h->seeds_sigma.width = h->m;
  h->plant_state.width = h->n;
  h->plant_params.width = model.n_params;
  h->params.batch_minor_copy = h->costs.batch_minor_copy = batch_minor;   // (what the lane kernels read batch-minor: KArgs::param_cols, cost_cols)
  const int rc = create_resources(h, lxu_hbm);
  if (rc != MI_ILQR_OK) { mi_ilqr_destroy(h); return rc; }
  *out = h;
  return MI_ILQR_OK;
}

void mi_ilqr_destroy(mi_ilqr_t* h) {
  if (!h) return;
  (void)hipSetDevice(h->d.device_id);
  for (const SolveSlot& s : h->slots) if (s.stream) (void)hipStreamSynchronize(s.stream);
  for (void* p : h->owned) (void)hipFree(p);
  if (h->host_records) (void)hipHostFree(h->host_records);
  if (h->h_ring) (void)hipHostFree(h->h_ring);
  if (h->pin_in) (void)hipHostFree(h->pin_in);
  for (int i = 0; i < mi_ilqr::kStatsRing; ++i) {
    if (h->ring_ev0[i]) (void)hipEventDestroy(h->ring_ev0[i]);
    if (h->ring_ev1[i]) (void)hipEventDestroy(h->ring_ev1[i]);
  }
  for (hipEvent_t e : h->pin_ev) if (e) (void)hipEventDestroy(e);
  for (const SolveSlot& s : h->slots) if (s.ev) (void)hipEventDestroy(s.ev);
  if (h->policy_ev0) (void)hipEventDestroy(h->policy_ev0);
  if (h->policy_ev1) (void)hipEventDestroy(h->policy_ev1);
  for (hipEvent_t e : h->mc_events) (void)hipEventDestroy(e);
  if (h->seeds_ev0) (void)hipEventDestroy(h->seeds_ev0);
  if (h->seeds_ev1) (void)hipEventDestroy(h->seeds_ev1);
  if (h->plant_ev0) (void)hipEventDestroy(h->plant_ev0);
  if (h->plant_ev1) (void)hipEventDestroy(h->plant_ev1);
  if (h->fit_ev0) (void)hipEventDestroy(h->fit_ev0);
  if (h->fit_ev1) (void)hipEventDestroy(h->fit_ev1);
  if (!h->slots[0].stream && h->stream) (void)hipStreamDestroy(h->stream);      // (a create that failed before the slots were set up)
  for (const SolveSlot& s : h->slots) if (s.stream) (void)hipStreamDestroy(s.stream);
  delete h;
}

int mi_ilqr_set_cost(mi_ilqr_t* h, const double* Q, const double* R, const double* Qf, const double* x_nom) {
  if (!h) return MI_ILQR_E_BAD_ARG;
  HIPCHK(hipSetDevice(h->d.device_id));
  const size_t n = h->n, m = h->m;
  if (x_nom) drop_per_problem_targets(h);   // one target for the batch again: the per-problem targets and steps are dropped
  {
    std::vector<double> cm = h->h_costmat;
    if (Q) std::memcpy(cm.data(), Q, n * n * 8);
    if (R) std::memcpy(cm.data() + n * n, R, m * m * 8);
    if (Qf) std::memcpy(cm.data() + n * n + m * m, Qf, n * n * 8);
    if (x_nom) std::memcpy(cm.data() + cost_len(h), x_nom, n * 8);
    bool regular = true, asym = false;
    if (classify_cost(h, cm.data(), &regular, &asym) != MI_ILQR_OK) {
      std::fprintf(stderr, "mi_ilqr_set_cost: Q, R, Qf must be finite\n");
      return MI_ILQR_E_UNSUPPORTED;
    }
    h->shared_cost_asym = asym ? 1 : 0;
    h->shared_exact_backward = regular ? 0 : 1;
    // one set of matrices for the batch again: the per-problem cost matrices are dropped (x_nom alone leaves them alone)
    if (Q || R || Qf) drop_per_problem_costs(h);
    else apply_cost_class(h);
    // the device copy mirrors h_costmat: nothing to send when the caller repeats the matrices it set before
    // (Solve() pushes them on every call, like the reference reads its attributes on every call)
    if (h->costmat_synced && std::memcmp(cm.data(), h->h_costmat.data(), cm.size() * 8) == 0) return MI_ILQR_OK;
    h->h_costmat.swap(cm);
  }
  h->costmat_synced = false;                                  // (a failed copy must not leave the mirror believed)
  // (joined only here: matrices the caller repeats between pipelined solves leave their overlap alone)
  { const int rc = join_slots(h); if (rc != MI_ILQR_OK) return rc; }
  const int rc = stage_h2d(h, h->costmat, h->h_costmat.data(), h->h_costmat.size() * 8);    // Q | R | Qf | x_nom: one copy
  h->costmat_synced = rc == MI_ILQR_OK;
  return rc;
}

int mi_ilqr_set_initial(mi_ilqr_t* h, const double* x0, const double* u_guess) {
  if (!h) return MI_ILQR_E_BAD_ARG;
  HIPCHK(hipSetDevice(h->d.device_id));
  if (h->host_inputs) return host_inputs_write(h, x0, u_guess, false);
  const InputWrite wr(h);
  if (wr.rc != MI_ILQR_OK) return wr.rc;
  if (x0) {
    const int rc = stage_h2d(h, wr.begin(h->in_x0), x0, (size_t)h->B * h->n * 8);
    if (rc != MI_ILQR_OK) return rc;
    wr.end(h->in_x0, h->x0);
  }
  if (u_guess) {
    const size_t cnt = (size_t)h->B * h->m * (h->N - 1);
    double* const dst = wr.begin(h->in_u);
    int rows = 0, len = 0;
    if (needs_relayout(h, MI_F_U_BAR, &rows, &len)) {
      int rc = ensure_scratch(h, cnt * 8);
      if (rc != MI_ILQR_OK) return rc;
      HIPCHK(hipStreamSynchronize(h->stream));
      HIPCHK(hipMemcpy(h->scratch, u_guess, cnt * 8, hipMemcpyHostToDevice));
      if ((rc = relayout(h, h->scratch, dst, rows, len, true)) != MI_ILQR_OK) return rc;
      HIPCHK(hipStreamSynchronize(h->stream));
    } else {
      const int rc = stage_h2d(h, dst, u_guess, cnt * 8);
      if (rc != MI_ILQR_OK) return rc;
    }
    wr.end(h->in_u, h->u_guess);
    h->u_pending = true;
    h->u_zero = false;
  }
  return MI_ILQR_OK;
}

int mi_ilqr_set_initial_shared(mi_ilqr_t* h, const double* x0, const double* u_guess_one) {
  if (!h) return MI_ILQR_E_BAD_ARG;
  HIPCHK(hipSetDevice(h->d.device_id));
  if (h->host_inputs) return host_inputs_write(h, x0, u_guess_one, true);
  const InputWrite wr(h);
  if (wr.rc != MI_ILQR_OK) return wr.rc;
  if (x0) {
    const int rc = stage_h2d(h, wr.begin(h->in_x0), x0, (size_t)h->B * h->n * 8);
    if (rc != MI_ILQR_OK) return rc;
    wr.end(h->in_x0, h->x0);
  }
  if (u_guess_one) {
    const size_t one = (size_t)h->m * (h->N - 1);
    double*& u_one = h->u_one_copy[wr.w];        // (the staged sequence: one per stream, the broadcast behind an earlier write may not have run yet)
    int rc = u_one ? MI_ILQR_OK : dev_alloc(h, u_one, one);
    if (rc == MI_ILQR_OK) rc = stage_h2d(h, u_one, u_guess_one, one * 8);
    if (rc == MI_ILQR_OK) rc = broadcast_u(h, u_one, wr.begin(h->in_u));
    if (rc != MI_ILQR_OK) return rc;
    wr.end(h->in_u, h->u_guess);
    h->u_pending = true;
    h->u_zero = false;
  }
  return MI_ILQR_OK;
}

int mi_ilqr_host_alloc(size_t bytes, void** out) {
  if (!out || bytes == 0) return MI_ILQR_E_BAD_ARG;
  *out = nullptr;
  HIPCHK(hipHostMalloc(out, bytes, hipHostMallocMapped));            // page-locked AND device-visible (result sinks)
  return MI_ILQR_OK;
}

int mi_ilqr_set_result_sink(mi_ilqr_t* h, double* x_bar_host, double* u_bar_host, double* cost_host) {
  if (!h) return MI_ILQR_E_BAD_ARG;
  if (h->large || h->batch_minor) return MI_ILQR_E_UNSUPPORTED;     // (their kernel layouts are not the boundary's)
  HIPCHK(hipSetDevice(h->d.device_id));
  { const int rc = join_slots(h); if (rc != MI_ILQR_OK) return rc; }
  HIPCHK(hipStreamSynchronize(h->stream));
  h->sink_x = h->sink_u = h->sink_cost = nullptr;
  if (!x_bar_host && !u_bar_host && !cost_host) return MI_ILQR_OK;
  if (!x_bar_host || !u_bar_host || !cost_host) return MI_ILQR_E_BAD_ARG;
  void *dx = nullptr, *du = nullptr, *dc = nullptr;
  if (hipHostGetDevicePointer(&dx, x_bar_host, 0) != hipSuccess || hipHostGetDevicePointer(&du, u_bar_host, 0) != hipSuccess ||
      hipHostGetDevicePointer(&dc, cost_host, 0) != hipSuccess) {
    (void)hipGetLastError();
    return MI_ILQR_E_BAD_ARG;                                        // not page-locked, device-visible host memory
  }
  h->sink_x = static_cast<double*>(dx); h->sink_u = static_cast<double*>(du); h->sink_cost = static_cast<double*>(dc);
  return MI_ILQR_OK;
}

int mi_ilqr_solve_into(mi_ilqr_t* h, double* x_bar, double* u_bar, double* cost, int32_t page_locked, int32_t n_extra,
                       const int32_t* which, void* const* dst, const size_t* bytes, mi_ilqr_stats* stats, int32_t* sink_used) {
  if (!h || !x_bar || !u_bar || !cost || n_extra < 0 || (n_extra > 0 && (!which || !dst || !bytes))) return MI_ILQR_E_BAD_ARG;
  if (sink_used) *sink_used = 0;
  int rc;
  bool sink = false;
  if (page_locked && !h->large && !h->batch_minor) {
    rc = mi_ilqr_set_result_sink(h, x_bar, u_bar, cost);
    if (rc == MI_ILQR_OK) sink = true;
    else if (rc != MI_ILQR_E_BAD_ARG) return rc;                      // (BAD_ARG: not page-locked after all - copy out instead)
  }
  auto clear = [&]() { h->sink_x = h->sink_u = h->sink_cost = nullptr; };
  if ((rc = mi_ilqr_solve_async(h)) != MI_ILQR_OK) { clear(); return rc; }
  if (!sink) {
    const int f3[3] = {MI_F_X_BAR, MI_F_U_BAR, MI_F_COST};
    void* const d3[3] = {x_bar, u_bar, cost};
    for (int i = 0; i < 3; ++i)
      if ((rc = mi_ilqr_get_async(h, f3[i], d3[i], field_of(h, f3[i]).bytes)) != MI_ILQR_OK) return rc;
  }
  // records the kernel writes straight into host memory (tiny batches, host.hpp: host_records): a memcpy after the synchronization
  auto host_side = [&](int w) -> const char* {
    if (!h->host_records || !(w == MI_F_HIST || w == MI_F_ITER_CYCLES || w == MI_I64_STAGE_CYCLES || w == MI_I_ITERS || w == MI_I_STATUS)) return nullptr;
    return h->host_records + (static_cast<const char*>(field_of(h, w).ptr) - h->host_records_dev);
  };
  for (int i = 0; i < n_extra; ++i) {
    if (host_side(which[i])) {
      const size_t fb = field_of(h, which[i]).bytes;
      if (bytes[i] != fb && !prefix_ok(which[i], bytes[i], fb)) { clear(); return MI_ILQR_E_BAD_SHAPE; }
      continue;
    }
    if ((rc = mi_ilqr_get_async(h, which[i], dst[i], bytes[i])) != MI_ILQR_OK) { clear(); return rc; }
  }
  rc = stats ? mi_ilqr_collect_stats_n(h, 1, stats) : mi_ilqr_synchronize(h);
  clear();                                                             // (the stream is idle: no later kernel of the handle writes the caller's arrays)
  if (rc == MI_ILQR_OK)
    for (int i = 0; i < n_extra; ++i)
      if (const char* src = host_side(which[i])) std::memcpy(dst[i], src, bytes[i]);
  if (sink_used) *sink_used = sink ? 1 : 0;
  return rc;
}

int mi_ilqr_host_free(void* p) {
  if (p) HIPCHK(hipHostFree(p));
  return MI_ILQR_OK;
}

int mi_ilqr_reset(mi_ilqr_t* h) {
  if (!h) return MI_ILQR_E_BAD_ARG;
  h->cold = true;          // zeros are materialized lazily (the kernels skip the HBM read)
  h->u_zero = true;        // a fresh reference object has u_bar = 0 until SetInitialGuess (ilqr.py:71,148-156)
  h->u_pending = false;
  return MI_ILQR_OK;
}

int mi_ilqr_set_control_limits(mi_ilqr_t* h, const double* u_min, const double* u_max, int32_t per_problem) {
  if (!h) return MI_ILQR_E_BAD_ARG;
  // workgroup-per-problem kernels: the mid-size family (n <= 32) only - the built-in arms, family-1 plugins built with limits
  if (h->large && !large_accepts_limits(h)) return MI_ILQR_E_UNSUPPORTED;
  if (!u_min && !u_max) { h->limited = false; return MI_ILQR_OK; }   // the regular kernels again, state untouched
  if (!u_min || !u_max) return MI_ILQR_E_BAD_ARG;
  const int m = h->m, B = h->B;
  const size_t rows = per_problem ? (size_t)B : 1;
  for (size_t i = 0; i < rows * m; ++i) {
    const double lo = u_min[i], hi = u_max[i];
    if (lo != lo || hi != hi || lo > hi) return MI_ILQR_E_BAD_ARG;   // NaN, or an empty box
  }
  HIPCHK(hipSetDevice(h->d.device_id));
  { const int rc = join_slots(h); if (rc != MI_ILQR_OK) return rc; }
  if (!h->s2) {
    int rc = h->ulim ? MI_ILQR_OK : dev_alloc(h, h->ulim, (size_t)B * 2 * m);
    for (int i = 0; i < (h->second_slot_ready ? 2 : 1); ++i) {          // S2 is solver state: one array per solve slot
      if (rc == MI_ILQR_OK && !h->slots[i].s2) rc = dev_alloc(h, h->slots[i].s2, (size_t)B);
      if (rc == MI_ILQR_OK) HIPCHK(hipMemsetAsync(h->slots[i].s2, 0, (size_t)B * 8, h->stream));
    }
    if (rc != MI_ILQR_OK) return rc;
    h->s2 = h->slots[h->solve_slot].s2;
  }
  std::vector<double> box((size_t)B * 2 * m);     // (B, 2, m): u_min | u_max, shared bounds broadcast here
  for (int b = 0; b < B; ++b) {
    const size_t src = per_problem ? (size_t)b * m : 0;
    for (int k = 0; k < m; ++k) { box[((size_t)b * 2) * m + k] = u_min[src + k]; box[((size_t)b * 2 + 1) * m + k] = u_max[src + k]; }
  }
  const int rc = stage_h2d(h, h->ulim, box.data(), box.size() * 8);
  if (rc != MI_ILQR_OK) return rc;
  h->limited = true;
  return MI_ILQR_OK;
}

int mi_ilqr_rearm_initial_guess(mi_ilqr_t* h) {
  if (!h) return MI_ILQR_E_BAD_ARG;
  h->u_pending = true;     // next kernel takes u_bar from the resident u_guess again
  h->u_zero = false;
  return MI_ILQR_OK;
}

int mi_ilqr_synchronize(mi_ilqr_t* h) {
  if (!h) return MI_ILQR_E_BAD_ARG;
  HIPCHK(hipSetDevice(h->d.device_id));
  { const int rc = join_slots(h); if (rc != MI_ILQR_OK) return rc; }
  HIPCHK(hipStreamSynchronize(h->stream));
  slots_idle(h);
  return MI_ILQR_OK;
}

int mi_ilqr_solve_async(mi_ilqr_t* h) {
  if (!h) return MI_ILQR_E_BAD_ARG;
  HIPCHK(hipSetDevice(h->d.device_id));
  // A cold solve reads no solver state, so between two of them only their outputs collide: it takes the OTHER solve slot - arrays and
  // stream - and shares the device with the solve before it.  With nothing in flight there is nothing to share it with.
  bool overlap = h->n_slots == 2 && h->cold && !h->sink_x && h->hold == 0 && h->inflight > 0;
  if (overlap && ensure_second_slot(h) != MI_ILQR_OK) {
    (void)hipGetLastError();
    h->n_slots = 1;                      // (no room for a second slot: one at a time, as before)
    overlap = false;
  }
  if (overlap) {
    int rc = fork_to_other(h);
    if (rc != MI_ILQR_OK) return rc;
    select_solve_slot(h, 1 - h->solve_slot);
    if ((rc = sync_inputs(h, h->solve_slot)) != MI_ILQR_OK) return rc;
  } else {
    const int rc = join_slots(h);
    if (rc != MI_ILQR_OK) return rc;
  }
  const int slot = (int)(h->seq++ % mi_ilqr::kStatsRing);
  select_stats_slot(h, slot);
  // pipelined solves: the events ride on one launch in `time_every` (every other entry point times its launches)
  h->timed_launch = h->time_every > 0 && (h->seq_timed++ % h->time_every) == 0;
  h->in_async_solve = true;
  int rc = launch(h, MODE_SOLVE);
  h->in_async_solve = false;
  h->timed_launch = true;
  if (rc != MI_ILQR_OK) return rc;
  // (the batch statistics of this solve: by the kernel itself, or by reduce_pending_stats when somebody collects)
  if (stats_in_kernel(h) && h->stats_done == h->seq - 1) h->stats_done = h->seq;
  h->cold = false;
  h->u_pending = false;
  ++h->inflight;
  return MI_ILQR_OK;
}

int mi_ilqr_collect_stats(mi_ilqr_t* h, mi_ilqr_stats* st) {
  if (!h || !st) return MI_ILQR_E_BAD_ARG;
  HIPCHK(hipSetDevice(h->d.device_id));
  { const int rc = reduce_pending_stats(h); if (rc != MI_ILQR_OK) return rc; }
  HIPCHK(hipStreamSynchronize(h->stream));
  slots_idle(h);
  fill_stats(h, (int)(h->h_stats - h->h_ring), st);
  return MI_ILQR_OK;
}

int mi_ilqr_collect_stats_n(mi_ilqr_t* h, int32_t count, mi_ilqr_stats* st) {
  if (!h || !st || count < 1 || count > mi_ilqr::kStatsRing || count > h->seq) return MI_ILQR_E_BAD_ARG;
  HIPCHK(hipSetDevice(h->d.device_id));
  { const int rc = reduce_pending_stats(h); if (rc != MI_ILQR_OK) return rc; }
  HIPCHK(hipStreamSynchronize(h->stream));
  slots_idle(h);
  for (int i = 0; i < count; ++i) fill_stats(h, (int)((h->seq - count + i) % mi_ilqr::kStatsRing), st + i);
  return MI_ILQR_OK;
}

int mi_ilqr_solve(mi_ilqr_t* h, mi_ilqr_stats* stats) {
  int rc = mi_ilqr_solve_async(h);
  if (rc != MI_ILQR_OK) return rc;
  if (stats) return mi_ilqr_collect_stats(h, stats);
  return mi_ilqr_synchronize(h);
}

int mi_ilqr_rollout(mi_ilqr_t* h, const double* eps) {
  if (!h) return MI_ILQR_E_BAD_ARG;
  int rc = upload_stage_in(h, eps);
  if (rc != MI_ILQR_OK) return rc;
  rc = launch(h, MODE_ROLLOUT);          // reads only; cold/u_pending stay as they are
  if (rc != MI_ILQR_OK) return rc;
  return mi_ilqr_synchronize(h);
}

int mi_ilqr_forward(mi_ilqr_t* h, const double* L_last) {
  if (!h) return MI_ILQR_E_BAD_ARG;
  int rc = upload_stage_in(h, L_last);
  if (rc != MI_ILQR_OK) return rc;
  if ((rc = materialize_zero_state(h)) != MI_ILQR_OK) return rc;   // forward leaves K/kappa/dV untouched
  rc = launch(h, MODE_FORWARD);
  if (rc != MI_ILQR_OK) return rc;
  h->u_pending = false;
  return mi_ilqr_synchronize(h);
}

int mi_ilqr_linearize(mi_ilqr_t* h) {
  if (!h) return MI_ILQR_E_BAD_ARG;
  int rc;
  if ((rc = materialize_zero_state(h)) != MI_ILQR_OK) return rc;
  if ((rc = materialize_u(h)) != MI_ILQR_OK) return rc;
  rc = launch(h, MODE_LINEARIZE);
  if (rc != MI_ILQR_OK) return rc;
  return mi_ilqr_synchronize(h);
}

int mi_ilqr_backward(mi_ilqr_t* h) {
  if (!h) return MI_ILQR_E_BAD_ARG;
  int rc;
  if ((rc = materialize_zero_state(h)) != MI_ILQR_OK) return rc;
  if ((rc = materialize_u(h)) != MI_ILQR_OK) return rc;
  rc = launch(h, MODE_BACKWARD);
  if (rc != MI_ILQR_OK) return rc;
  return mi_ilqr_synchronize(h);
}

int mi_ilqr_set_timing(mi_ilqr_t* h, int32_t every) {
  if (!h || every < 0) return MI_ILQR_E_BAD_ARG;
  h->time_every = every;
  h->seq_timed = 0;
  return MI_ILQR_OK;
}

int mi_ilqr_last_kernel_ms(mi_ilqr_t* h, float* ms) {
  if (!h || !ms) return MI_ILQR_E_BAD_ARG;
  if (!h->last_timed) { *ms = 0.0f; return MI_ILQR_OK; }
  HIPCHK(hipSetDevice(h->d.device_id));
  { const int rc = join_slots(h); if (rc != MI_ILQR_OK) return rc; }
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipEventElapsedTime(ms, h->ev0, h->ev1));
  return MI_ILQR_OK;
}

int mi_ilqr_get_cycles(mi_ilqr_t* h, int64_t* dst, size_t bytes) {
  if (!h || !dst) return MI_ILQR_E_BAD_ARG;
  if (bytes != (size_t)h->B * 4 * 8) return MI_ILQR_E_BAD_SHAPE;
  HIPCHK(hipSetDevice(h->d.device_id));
  { const int rc = join_slots(h); if (rc != MI_ILQR_OK) return rc; }
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(dst, h->prof, bytes, hipMemcpyDefault));
  return MI_ILQR_OK;
}

int mi_ilqr_get_stream(mi_ilqr_t* h, void** hip_stream) {
  if (!h || !hip_stream) return MI_ILQR_E_BAD_ARG;
  // the current slot's stream, ordered behind the other one's: work a caller enqueues on it follows every solve enqueued so far
  { const int rc = join_slots(h); if (rc != MI_ILQR_OK) return rc; }
  *hip_stream = reinterpret_cast<void*>(h->stream);
  return MI_ILQR_OK;
}

}  // extern "C"
