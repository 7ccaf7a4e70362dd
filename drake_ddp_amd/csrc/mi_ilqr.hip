// libmi_ilqr.so — host side of the C ABI declared in include/mi_ilqr.h.
//
// Owns the device-resident solver state of a batch (the persistent attributes of
// the reference class, /root/reference/ilqr.py:61-91, with a leading batch axis),
// dispatches the gfx950 kernels and moves data across the boundary.  No compute
// happens on the host: without a usable device every compute entry fails with
// MI_ILQR_E_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <dlfcn.h>
#include <rccl/rccl.h>     // types and enum VALUES only (ncclFloat64, ncclMin): the symbols are bound at run time (dlopen below)

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <initializer_list>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/mi_ilqr.h"
#include "host.hpp"          // the handle and the launch templates (instantiated in the k_*.hip units)
#include "kernel_args.hpp"   // KArgs, DevStats
#include "lds_layout.hpp"    // ws_bytes, large_lds_bytes, large_lds_bytes_hbm, kLargeThreads
#include "models.hpp"

using namespace mi;
using namespace mi_host;

namespace {


// One record per model id: the plugin record (n, m, parameters and their defaults, family, LDS bytes, launch entry) - filled in
// below for the built-in models, by mi_ilqr_register_model for those registered at run time - and the clustering policy.
struct Model {
  mi_ilqr_model_plugin p;
  // Workgroup-per-problem launches of batches up to this size share their linearizations in clusters (cluster_size): the models
  // whose linearization is worth a handshake (round 5: ~20 k cycles - six memory round trips - since the cache-wide write-backs are
  // gone; with the helpers linearizing the line search's first trial WHILE it is rolled out - early linearization, ilqr_large.hpp -
  // the stage shrinks to the wait for the last block: 36-state chain 74 k -> 12 k cycles at B = 64, 3-D quadruped 92 k -> 30 k,
  // planar quadruped 164 k -> 132 k (its helpers cannot keep up with the rollout)).  The arm + ball's dense linearization (100 k
  // single) up to B = 64; plugin models: the library cannot know what their step costs - a cheap one loses to the handshake, so
  // they are not clustered unless forced (0).
  int cluster_max_B;
};
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
// model's policy-rollout kernels are in k_policy.hip and, with noise, k_policy_noise.hip
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

const Model* model_of(int id) {
  if (id >= 0 && id < kNumBuiltins) return &kBuiltins[id];
  const int s_ = id - MI_MODEL_PLUGIN_BASE;
  return (s_ >= 0 && s_ < MI_ILQR_MAX_PLUGINS && g_plugins[s_].used.load(std::memory_order_acquire)) ? &g_plugins[s_].model : nullptr;
}

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

// costmat and its host mirror are Q | R | Qf | x_nom: the length of the matrices, and the shared x_nom (host mirror) behind them
size_t cost_len(const mi_ilqr* h) { return 2 * (size_t)h->n * h->n + (size_t)h->m * h->m; }
const double* shared_x_nom(const mi_ilqr* h) { return h->h_costmat.data() + cost_len(h); }

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
int reduce_pending_stats(mi_ilqr* h);

int refresh_lane_target_rows(mi_ilqr* h);

int launch(mi_ilqr* h, int mode) {
  HIPCHK(hipSetDevice(h->d.device_id));
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
  if (h->u_zero && !h->u_pending) HIPCHK(hipMemsetAsync(h->u_bar, 0, (size_t)h->B * h->m * (h->N - 1) * 8, h->stream));
  h->u_zero = false;
  if (!h->u_pending) return MI_ILQR_OK;
  HIPCHK(hipMemcpyAsync(h->u_bar, h->u_guess, (size_t)h->B * h->m * (h->N - 1) * 8, h->host_inputs ? hipMemcpyDefault : hipMemcpyDeviceToDevice, h->stream));
  h->u_pending = false;
  return MI_ILQR_OK;
}

__global__ void mpc_shift_kernel(const double* x_bar, const double* u_bar, double* x0, double* u_guess,
                                 int B, int n, int m, int N, int r) {
  const int b = blockIdx.x;
  if (b >= B) return;
  for (int i = threadIdx.x; i < n; i += blockDim.x) x0[(size_t)b * n + i] = x_bar[((size_t)b * n + i) * N + r];
  const int M1 = N - 1;
  for (int idx = threadIdx.x; idx < m * M1; idx += blockDim.x) {
    const int k = idx / M1, t = idx - k * M1;
    const int src = (t + r < M1) ? t + r : M1 - 1;
    u_guess[((size_t)b * m + k) * M1 + t] = u_bar[((size_t)b * m + k) * M1 + src];
  }
}

__global__ void mpc_shift_kernel_tm(const double* x_bar, const double* u_bar, double* x0, double* u_guess,
                                    int B, int n, int m, int N, int r) {
  const int b = blockIdx.x;
  if (b >= B) return;
  for (int i = threadIdx.x; i < n; i += blockDim.x) x0[(size_t)b * n + i] = x_bar[((size_t)b * N + r) * n + i];
  const int M1 = N - 1;
  for (int idx = threadIdx.x; idx < m * M1; idx += blockDim.x) {
    const int t = idx / m, k = idx - t * m;
    const int src = (t + r < M1) ? t + r : M1 - 1;
    u_guess[((size_t)b * M1 + t) * m + k] = u_bar[((size_t)b * M1 + src) * m + k];
  }
}

__global__ void mpc_shift_kernel_bm(const double* x_bar, const double* u_bar, double* x0, double* u_guess,
                                    int B, int n, int m, int N, int r) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  for (int i = 0; i < n; ++i) x0[(size_t)b * n + i] = x_bar[((size_t)r * n + i) * B + b];
  const int M1 = N - 1;
  for (int t = 0; t < M1; ++t) {
    const int src = (t + r < M1) ? t + r : M1 - 1;
    for (int k = 0; k < m; ++k) u_guess[((size_t)t * m + k) * B + b] = u_bar[((size_t)src * m + k) * B + b];
  }
}

// Layouts of a (B, rows, len) trajectory array: TL time-last [b][row][t] (the reference's, SURVEY F5 - what
// crosses the C ABI); TM time-major [b][t][row] (workgroup-per-problem kernels); BM batch-minor
// [t][row][b] (lane-per-problem kernels).  The conversions run on the DEVICE, between the field and a
// staging buffer; the host copy is then one linear transfer.
enum { LAYOUT_TL = 0, LAYOUT_TM = 1, LAYOUT_BM = 2 };
int layout_of(const mi_ilqr* h) { return h->batch_minor ? LAYOUT_BM : (h->large ? LAYOUT_TM : LAYOUT_TL); }

// TL <-> TM: a per-problem (rows x len) transpose; both sides of a problem fit the caches, a gather is enough.
__global__ void __launch_bounds__(256) relayout_tm_kernel(const double* __restrict__ src, double* __restrict__ dst,
                                                            int rows, int len, int to_tm) {
  const size_t base = (size_t)blockIdx.x * rows * len;
  for (int e = threadIdx.x; e < rows * len; e += 256) {
    int r, t;
    if (to_tm) { t = e / rows; r = e - t * rows; dst[base + e] = src[base + (size_t)r * len + t]; }
    else { r = e / len; t = e - r * len; dst[base + e] = src[base + (size_t)t * rows + r]; }
  }
}

// TL <-> BM: for every row r a (B x len) <-> (len x B) transpose with pitches; 32 x 32 tiles through LDS
// so that both the reads and the writes are coalesced.  grid = (ceil(len/32), ceil(B/32), rows).
__global__ void __launch_bounds__(256) relayout_bm_kernel(const double* __restrict__ src, double* __restrict__ dst,
                                                            int B, int rows, int len, int to_bm) {
  __shared__ double tile[32][33];
  const int r = blockIdx.z, t0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;          // 32 x 8 threads
  if (to_bm) {
    for (int j = ty; j < 32; j += 8) {                             // read TL: t fastest
      const int b = b0 + j, t = t0 + tx;
      if (b < B && t < len) tile[j][tx] = src[((size_t)b * rows + r) * len + t];
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {                             // write BM: b fastest
      const int t = t0 + j, b = b0 + tx;
      if (b < B && t < len) dst[((size_t)t * rows + r) * B + b] = tile[tx][j];
    }
  } else {
    for (int j = ty; j < 32; j += 8) {                             // read BM: b fastest
      const int t = t0 + j, b = b0 + tx;
      if (b < B && t < len) tile[j][tx] = src[((size_t)t * rows + r) * B + b];
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {                             // write TL: t fastest
      const int b = b0 + j, t = t0 + tx;
      if (b < B && t < len) dst[((size_t)b * rows + r) * len + t] = tile[tx][j];
    }
  }
}

// The handle's device memory: every allocation is recorded in h->owned, which is what mi_ilqr_destroy frees - a buffer allocated on
// first use, or by a create that fails half-way, needs no line of its own there.  dev_free releases one early (buffers that are re-grown).
template <class T>
int dev_alloc(mi_ilqr* h, T*& p, size_t count, bool zero = false) {
  void* q = nullptr;
  HIPCHK(hipMalloc(&q, count * sizeof(T)));
  h->owned.push_back(q);
  if (zero) HIPCHK(hipMemset(q, 0, count * sizeof(T)));
  p = static_cast<T*>(q);
  return MI_ILQR_OK;
}
template <class T>
int dev_free(mi_ilqr* h, T*& p) {
  if (!p) return MI_ILQR_OK;
  void* q = p;
  const auto it = std::find(h->owned.begin(), h->owned.end(), q);
  if (it != h->owned.end()) h->owned.erase(it);
  p = nullptr;
  HIPCHK(hipFree(q));
  return MI_ILQR_OK;
}

int ensure_scratch(mi_ilqr* h, size_t bytes) {
  if (h->scratch_bytes >= bytes) return MI_ILQR_OK;
  HIPCHK(hipStreamSynchronize(h->stream));
  h->scratch_bytes = 0;
  int rc = dev_free(h, h->scratch);
  if (rc == MI_ILQR_OK) rc = dev_alloc(h, h->scratch, (bytes + 7) / 8);
  if (rc == MI_ILQR_OK) h->scratch_bytes = bytes;
  return rc;
}

// Convert between the handle's kernel layout and time-last, on the handle's stream.
int relayout(mi_ilqr* h, const double* src, double* dst, int rows, int len, bool to_kernel_layout) {
  if (layout_of(h) == LAYOUT_BM) {
    const dim3 grid((len + 31) / 32, (h->B + 31) / 32, rows);
    hipLaunchKernelGGL(relayout_bm_kernel, grid, dim3(256), 0, h->stream, src, dst, h->B, rows, len, to_kernel_layout ? 1 : 0);
  } else {
    hipLaunchKernelGGL(relayout_tm_kernel, dim3(h->B), dim3(256), 0, h->stream, src, dst, rows, len, to_kernel_layout ? 1 : 0);
  }
  HIPCHK(hipGetLastError());
  return MI_ILQR_OK;
}

// One control sequence (m, len), time last, written for every problem in the handle's layout:
// layout 0 = [b][k][t] (wave-per-problem), 1 = [b][t][k] (workgroup-per-problem), 2 = [t][k][b] (lane-per-problem).
__global__ void __launch_bounds__(256) broadcast_u_kernel(const double* __restrict__ src, double* __restrict__ dst,
                                                            int B, int m, int len, int layout) {
  const size_t total = (size_t)B * m * len;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    int k, t;
    if (layout == 0) { const size_t r = e % ((size_t)m * len); k = (int)(r / len); t = (int)(r - (size_t)k * len); }
    else if (layout == 1) { const size_t r = e % ((size_t)m * len); t = (int)(r / m); k = (int)(r - (size_t)t * m); }
    else { const size_t r = e / B; t = (int)(r / m); k = (int)(r - (size_t)t * m); }
    dst[e] = src[(size_t)k * len + t];
  }
}

// mi_ilqr_policy_rollout: the call's time-major copy of the policy, (B, N-1, W) with W = n + m + m n and row t = x_bar_t | u_bar_t |
// K_t (m x n, row-major), gathered from the handle's kernel layout (LAYOUT_TL / TM / BM).  A source that is nullptr reads as zeros:
// the state of a cold handle, the controls of a reset one.
__global__ void __launch_bounds__(256) policy_pack_kernel(const double* __restrict__ x_bar, const double* __restrict__ u_bar,
                                                            const double* __restrict__ K, double* __restrict__ dst,
                                                            int B, int n, int m, int N, int layout) {
  const int W = n + m + m * n, M1 = N - 1;
  const size_t total = (size_t)B * M1 * W;
  auto at = [&](const double* f, int rows, int len, int b, int r, int t) -> double {
    if (!f) return 0.0;
    if (layout == LAYOUT_TL) return f[((size_t)b * rows + r) * len + t];
    if (layout == LAYOUT_TM) return f[((size_t)b * len + t) * rows + r];
    return f[((size_t)t * rows + r) * B + b];
  };
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int w = (int)(e % W);
    const size_t bt = e / W;
    const int t = (int)(bt % M1), b = (int)(bt / M1);
    dst[e] = w < n ? at(x_bar, n, N, b, w, t) : (w < n + m ? at(u_bar, m, M1, b, w - n, t) : at(K, m * n, M1, b, w - n - m, t));
  }
}

// The closed MPC loop's plant (plant_advance.hpp: a lane is a problem) reads everything PROBLEM-MINOR, element e of problem b at
// e * B + b.  plant_pack_kernel: the first `steps` columns of the policy, (steps, W, B) with row j = x_bar_j | u_bar_j | K_j, gathered
// from the handle's kernel layout like policy_pack_kernel does (a source that is nullptr reads as zeros); the writes are coalesced.
__global__ void __launch_bounds__(256) plant_pack_kernel(const double* __restrict__ x_bar, const double* __restrict__ u_bar,
                                                           const double* __restrict__ K, double* __restrict__ dst,
                                                           int B, int n, int m, int N, int steps, int layout) {
  const int W = n + m + m * n, M1 = N - 1;
  const size_t total = (size_t)steps * W * B;
  auto at = [&](const double* f, int rows, int len, int b, int r, int t) -> double {
    if (!f) return 0.0;
    if (layout == LAYOUT_TL) return f[((size_t)b * rows + r) * len + t];
    if (layout == LAYOUT_TM) return f[((size_t)b * len + t) * rows + r];
    return f[((size_t)t * rows + r) * B + b];
  };
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int b = (int)(e % B);
    const size_t jw = e / B;
    const int w = (int)(jw % W), t = (int)(jw / W);
    dst[e] = w < n ? at(x_bar, n, N, b, w, t) : (w < n + m ? at(u_bar, m, M1, b, w - n, t) : at(K, m * n, M1, b, w - n - m, t));
  }
}

// ... and rows_to_cols_kernel: a per-problem array, `width` doubles of problem b at src + b * stride (stride 0: one row for every
// problem), as (width, B)
__global__ void __launch_bounds__(256) rows_to_cols_kernel(const double* __restrict__ src, size_t stride, double* __restrict__ dst,
                                                             int width, int B) {
  const size_t total = (size_t)width * B;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t k = e / B, b = e - k * B;
    dst[e] = src[b * stride + k];
  }
}

// x0 <- the plants' states, on the device (dst may be the mapped host block of a tiny batch: host.hpp, host_inputs)
__global__ void __launch_bounds__(256) copy_doubles_kernel(const double* __restrict__ src, double* __restrict__ dst, size_t count) {
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < count; e += (size_t)gridDim.x * 256) dst[e] = src[e];
}

// Batched (R x C) -> (C x R) transposes with pitches, 32 x 32 tiles through LDS so that reads and writes are both coalesced: matrix
// z = (o, i), i < inner; element (r, c) is read at src[o src_outer + i src_inner + r src_r + c], written at dst[o dst_outer +
// i dst_inner + c dst_c + r].  The sample-minor <-> boundary conversions of mi_ilqr_policy_rollout.  grid = (ceil(C/32), ceil(R/32), <= Z).
__global__ void __launch_bounds__(256) transpose_tiles_kernel(const double* __restrict__ src, double* __restrict__ dst, int R, int C,
                                                                int Z, int inner, size_t src_outer, size_t src_inner, size_t src_r,
                                                                size_t dst_outer, size_t dst_inner, size_t dst_c) {
  __shared__ double tile[32][33];
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;          // 32 x 8 threads
  for (int z = blockIdx.z; z < Z; z += gridDim.z) {
    const int o = z / inner, i = z - o * inner;
    const double* s_ = src + (size_t)o * src_outer + (size_t)i * src_inner;
    double* d_ = dst + (size_t)o * dst_outer + (size_t)i * dst_inner;
    for (int j = ty; j < 32; j += 8) {
      const int r = r0 + j, c = c0 + tx;
      if (r < R && c < C) tile[j][tx] = s_[(size_t)r * src_r + c];
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
      const int c = c0 + j, r = r0 + tx;
      if (r < R && c < C) d_[(size_t)c * dst_c + r] = tile[tx][j];
    }
    __syncthreads();
  }
}

int transpose_tiles(mi_ilqr* h, const double* src, double* dst, int R, int C, size_t outer, int inner, size_t src_outer, size_t src_inner,
                    size_t src_r, size_t dst_outer, size_t dst_inner, size_t dst_c) {
  const size_t Z = outer * (size_t)inner;
  if (Z > 0x7fffffffull) return MI_ILQR_E_UNSUPPORTED;
  const dim3 grid((C + 31) / 32, (R + 31) / 32, (unsigned)std::min<size_t>(Z, 65535));
  if (grid.y > 65535) return MI_ILQR_E_UNSUPPORTED;
  hipLaunchKernelGGL(transpose_tiles_kernel, grid, dim3(256), 0, h->stream, src, dst, R, C, (int)Z, inner, src_outer, src_inner, src_r,
                     dst_outer, dst_inner, dst_c);
  HIPCHK(hipGetLastError());
  return MI_ILQR_OK;
}

// rows of the (rows,len) time-last view of a double field; 0 = not a trajectory array
int traj_rows(const mi_ilqr* h, int which, int* len) {
  const int n = h->n, m = h->m, N = h->N;
  switch (which) {
    case MI_F_X_BAR: case MI_F_X_TRIAL: *len = N; return n;
    case MI_F_U_BAR: case MI_F_U_TRIAL: case MI_F_KAPPA: *len = N - 1; return m;
    case MI_F_K: *len = N - 1; return m * n;
    case MI_F_FX: *len = N - 1; return n * n;
    case MI_F_FU: *len = N - 1; return n * m;
    case MI_F_DV: *len = N - 1; return 1;
  }
  *len = 0;
  return 0;
}

// Does this double field cross the boundary through a layout conversion (relayout), and with which rows and length?  The
// trajectory arrays of the handles whose kernel layout is not time-last - except single-row ones in the time-major layout, which
// are the same bytes either way.  A control sequence handed to mi_ilqr_set_initial has MI_F_U_BAR's shape.
bool needs_relayout(const mi_ilqr* h, int which, int* rows, int* len) {
  const int layout = layout_of(h);
  *rows = layout == LAYOUT_TL ? 0 : traj_rows(h, which, len);
  return *rows > 1 || (layout == LAYOUT_BM && *rows == 1);
}

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

// DevStats records of every enqueued solve that has none yet: ONE launch, a workgroup per pending ring slot.
int reduce_pending_stats(mi_ilqr* h) {
  long long first = h->stats_done;
  if (h->seq - first > mi_ilqr::kStatsRing) first = h->seq - mi_ilqr::kStatsRing;    // older slots were overwritten
  const int count = (int)(h->seq - first);
  if (count > 0) {
    hipLaunchKernelGGL(stats_kernel, dim3(count), dim3(256), 0, h->stream, h->iters_ring, h->status_ring, h->ls_ring, h->cost_ring,
                       h->B, h->d_ring, (int)(first % mi_ilqr::kStatsRing), (int)mi_ilqr::kStatsRing);
    HIPCHK(hipGetLastError());
  }
  h->stats_done = h->seq;
  return MI_ILQR_OK;
}

// Host -> device copy of a caller's (pageable) buffer, ordered on the handle's stream.  Small inputs go through
// the handle's page-locked staging block and an ASYNCHRONOUS copy: the call returns after a host memcpy, the
// kernels that follow on the stream see the data (a blocking hipMemcpy costs ~15-20 us each whatever its size).
// Large ones keep the runtime's own pipelined staging.
int stage_h2d(mi_ilqr* h, void* dst, const void* src, size_t bytes) {
  constexpr size_t kSmall = 256 * 1024;
  if (bytes > kSmall) {
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return MI_ILQR_OK;
  }
  if (!h->pin_in) {
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h->pin_in), 4 * kSmall, hipHostMallocDefault));
    HIPCHK(hipEventCreateWithFlags(&h->pin_ev, hipEventDisableTiming));
    h->pin_off = 0;
  }
  if (h->pin_off + bytes > 4 * kSmall) {          // the block is used as a ring; wrap once the copies in flight are done
    HIPCHK(hipEventSynchronize(h->pin_ev));
    h->pin_off = 0;
  }
  char* stage = h->pin_in + h->pin_off;
  std::memcpy(stage, src, bytes);
  HIPCHK(hipMemcpyAsync(dst, stage, bytes, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipEventRecord(h->pin_ev, h->stream));
  h->pin_off += (bytes + 255) & ~(size_t)255;
  return MI_ILQR_OK;
}

// The protocol of a per-problem array (host.hpp: RowStore).  store_upload: (B, width) rows from the host become the array's contents
// and the handle enters its per-problem mode.  Rows that equal what the device already holds are not sent.  Kernels already enqueued
// (mi_ilqr_solve_async) read the previous rows: stage_h2d copies on the handle's stream, behind them.  The mirror is committed only
// once every copy is enqueued; a failed allocation or copy leaves the mode - the device copies are undefined then, and the handle
// falls back to what it can vouch for - and returns the error.
void store_drop(RowStore& s) {
  s.synced = false;
  s.mirror.clear();
}

int store_upload(mi_ilqr* h, RowStore& s, const double* src) {
  const size_t B = h->B, cnt = B * s.width;
  if (s.synced && std::memcmp(s.mirror.data(), src, cnt * 8) == 0) return MI_ILQR_OK;
  store_drop(s);
  HIPCHK(hipSetDevice(h->d.device_id));
  int rc = MI_ILQR_OK;
  if (!s.rows) rc = dev_alloc(h, s.rows, cnt);
  if (rc == MI_ILQR_OK && s.batch_minor_copy && !s.cols) rc = dev_alloc(h, s.cols, cnt);
  if (rc == MI_ILQR_OK) rc = stage_h2d(h, s.rows, src, cnt * 8);
  if (rc == MI_ILQR_OK && s.batch_minor_copy) {
    std::vector<double> cols(cnt);
    for (size_t b = 0; b < B; ++b)
      for (size_t k = 0; k < s.width; ++k) cols[k * B + b] = src[b * s.width + k];
    rc = stage_h2d(h, s.cols, cols.data(), cnt * 8);
  }
  if (rc != MI_ILQR_OK) return rc;
  s.mirror.assign(src, src + cnt);
  s.synced = true;
  return MI_ILQR_OK;
}

// ... and the same with ONE row for every problem
int store_upload_broadcast(mi_ilqr* h, RowStore& s, const double* row) {
  std::vector<double> rows((size_t)h->B * s.width);
  for (size_t b = 0; b < (size_t)h->B; ++b) std::memcpy(rows.data() + b * s.width, row, s.width * 8);
  return store_upload(h, s, rows.data());
}

// mi_ilqr_get of a per-problem array: the mirror; in shared mode `shared_row` for every problem, or zeros (nullptr)
int store_read(const mi_ilqr* h, const RowStore& s, const double* shared_row, double* dst, size_t bytes) {
  if (s.width == 0) return MI_ILQR_E_UNSUPPORTED;
  if (bytes != (size_t)h->B * s.width * 8) return MI_ILQR_E_BAD_SHAPE;
  if (s.synced) std::memcpy(dst, s.mirror.data(), bytes);
  else if (!shared_row) std::memset(dst, 0, bytes);
  else for (size_t b = 0; b < (size_t)h->B; ++b) std::memcpy(dst + b * s.width, shared_row, s.width * 8);
  return MI_ILQR_OK;
}

// The selectors of mi_ilqr_get / mi_ilqr_device_ptr that are per-problem arrays: the store, and the row every problem reports in shared mode
struct RowField { RowStore* store; const double* shared_row; };
RowField row_field(mi_ilqr* h, int which) {
  switch (which) {
    case MI_F_X_NOM: return {&h->targets, shared_x_nom(h)};
    case MI_F_TARGET_STEP: return {&h->target_steps, nullptr};
    case MI_F_MODEL_PARAMS: return {&h->params, h->d.model_params};
    case MI_F_COST_MATRICES: return {&h->costs, h->h_costmat.data()};
    case MI_F_POLICY_NOISE: return {&h->policy_noise, nullptr};        // (not set: no noise, zeros)
    case MI_F_PLANT_STATE: return {&h->plant_state, nullptr};          // (mi_ilqr_get refuses it while the handle holds no plant)
    case MI_F_PLANT_PARAMS: return {&h->plant_params, h->d.model_params};   // (not set: the problem's model row, get_plant_field)
    case MI_F_PLANT_NOISE: return {&h->plant_noise, nullptr};
    case MI_F_POLICY_MC_DIST: return {&h->policy_mc_dist, nullptr};    // (not set: zeros)
    case MI_F_POLICY_MC_BOX: return {&h->mc_box, nullptr};             // (the same)
  }
  return {nullptr, nullptr};
}

// The lane-per-problem kernels' per-problem-cost instantiations on a handle with ONE target: its x_nom as (B, n) rows.
int refresh_lane_target_rows(mi_ilqr* h) {
  RowStore& s = h->lane_targets;      // (only ever one row repeated: the first says what all of them are, on every launch)
  if (s.synced && std::memcmp(s.mirror.data(), shared_x_nom(h), s.width * 8) == 0) return MI_ILQR_OK;
  return store_upload_broadcast(h, s, shared_x_nom(h));
}

struct Field { void* ptr; size_t bytes; bool is_int; };

Field field_of(mi_ilqr* h, int which) {
  const size_t n = h->n, m = h->m, N = h->N, B = h->B;
  switch (which) {
    case MI_F_X_BAR: return {h->x_bar, B * n * N * 8, false};
    case MI_F_U_BAR: return {h->u_bar, B * m * (N - 1) * 8, false};
    case MI_F_K: return {h->K, B * m * n * (N - 1) * 8, false};
    case MI_F_KAPPA: return {h->kappa, B * m * (N - 1) * 8, false};
    case MI_F_DV: return {h->dV, B * (N - 1) * 8, false};
    case MI_F_FX: return {h->fx, B * n * n * (N - 1) * 8, false};
    case MI_F_FU: return {h->fu, B * n * m * (N - 1) * 8, false};
    case MI_F_COST: return {h->cost, B * 8, false};
    case MI_F_X0: return {h->x0, B * n * 8, false};
    case MI_F_HIST: return {h->hist, B * (size_t)h->d.hist_cap * 4 * 8, false};
    case MI_F_ITER_CYCLES: return {h->iter_cyc, B * (size_t)h->d.hist_cap * 4 * 8, false};
    case MI_F_X_TRIAL: return {h->x_trial, B * n * N * 8, false};
    case MI_F_U_TRIAL: return {h->u_trial, B * m * (N - 1) * 8, false};
    case MI_F_TRIAL_COST: return {h->trial_cost, B * 2 * 8, false};
    case MI_I_ITERS: return {h->iters, B * 4, true};
    case MI_I_STATUS: return {h->status, B * 4, true};
    case MI_I_LS_TRIALS: return {h->ls_trials, B * 4, true};
    case MI_I_KP_COUNT: return {h->kp_count, B * 4, true};
    case MI_I_KP_LIST: return {h->kp_list, B * (N - 1) * 4, true};
    case MI_I64_STAGE_CYCLES: return {h->prof, B * 4 * 8, true};
    case MI_I64_CLUSTER_WORDS: return {h->cluster_sync, B * kSyncWords * 8, true};
  }
  return {nullptr, 0, false};
}

// The per-iteration records (MI_F_HIST, MI_F_ITER_CYCLES: hist_cap rows of 4 doubles per problem) may be read in part: any whole
// number of LEADING rows of the first problem - what a caller with one problem and a long log capacity wants after a short solve
// (the drop-in class keeps 4096 rows and reads the 64 first with the solve, the rest only when a solve took more iterations).
bool prefix_ok(int which, size_t bytes, size_t field_bytes) {
  return (which == MI_F_HIST || which == MI_F_ITER_CYCLES) && bytes > 0 && bytes < field_bytes && bytes % 32 == 0;
}

bool is_state_field(int which) {
  return which == MI_F_X_BAR || which == MI_F_K || which == MI_F_KAPPA || which == MI_F_DV || which == MI_F_FX || which == MI_F_FU;
}

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

}  // namespace

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
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (void* p : h->owned) (void)hipFree(p);
  if (h->host_records) (void)hipHostFree(h->host_records);
  if (h->h_ring) (void)hipHostFree(h->h_ring);
  if (h->pin_in) (void)hipHostFree(h->pin_in);
  for (int i = 0; i < mi_ilqr::kStatsRing; ++i) {
    if (h->ring_ev0[i]) (void)hipEventDestroy(h->ring_ev0[i]);
    if (h->ring_ev1[i]) (void)hipEventDestroy(h->ring_ev1[i]);
  }
  if (h->pin_ev) (void)hipEventDestroy(h->pin_ev);
  if (h->policy_ev0) (void)hipEventDestroy(h->policy_ev0);
  if (h->policy_ev1) (void)hipEventDestroy(h->policy_ev1);
  for (hipEvent_t e : h->mc_events) (void)hipEventDestroy(e);
  if (h->plant_ev0) (void)hipEventDestroy(h->plant_ev0);
  if (h->plant_ev1) (void)hipEventDestroy(h->plant_ev1);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

// Symmetric positive semi-definite (definite with `strict`)?  Cholesky of A + eps*I; the matrices are tiny.
static bool is_sym_psd(const double* A, int k, bool strict) {
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

// Per-problem targets (MI_F_X_NOM / MI_F_TARGET_STEP): the two arrays enter and leave their mode together.
static void drop_per_problem_targets(mi_ilqr* h) {
  store_drop(h->targets);
  store_drop(h->target_steps);
  h->target_steps_moving = false;
}

static int upload_target_rows(mi_ilqr* h, RowStore& s, const double* src) {
  const int rc = store_upload(h, s, src);
  if (rc != MI_ILQR_OK) drop_per_problem_targets(h);
  return rc;
}

static int set_target_field(mi_ilqr* h, int which, const double* src, size_t bytes) {
  const size_t cnt = (size_t)h->B * h->n;
  if (bytes != cnt * 8) return MI_ILQR_E_BAD_SHAPE;
  for (size_t i = 0; i < cnt; ++i) if (src[i] != src[i]) return MI_ILQR_E_BAD_ARG;
  int rc;
  if (!h->targets.synced) {     // entering the mode: the field the caller does not set starts from the shared x_nom broadcast / zero steps
    if (which == MI_F_X_NOM) rc = store_upload(h, h->target_steps, std::vector<double>(cnt, 0.0).data());
    else rc = store_upload_broadcast(h, h->targets, shared_x_nom(h));
    if (rc != MI_ILQR_OK) { drop_per_problem_targets(h); return rc; }
  }
  if ((rc = upload_target_rows(h, which == MI_F_X_NOM ? h->targets : h->target_steps, src)) != MI_ILQR_OK) return rc;
  if (which == MI_F_TARGET_STEP) {
    h->target_steps_moving = false;
    for (size_t i = 0; i < cnt; ++i) if (src[i] != 0.0) h->target_steps_moving = true;
  }
  return MI_ILQR_OK;
}

// mpc_run with per-problem targets: every row moves by its own step, once per re-solve - fp64 repeated addition, what the kernels do
static int advance_per_problem_targets(mi_ilqr* h, int32_t times) {
  std::vector<double> rows = h->targets.mirror;
  for (int32_t r = 0; r < times; ++r)
    for (size_t i = 0; i < rows.size(); ++i) rows[i] += h->target_steps.mirror[i];
  return upload_target_rows(h, h->targets, rows.data());
}

// Reference trajectories (MI_F_X_REF / MI_F_REF_CLOCK): (B, T, n) rows, T from the byte count; src == NULL with bytes == 0: no
// reference, clock 0 - the kernels get a null x_ref, as on a handle that never held one.  Workgroup-per-problem handles only; not
// beside a plant (the plant kernels know constant targets only).  A refused call changes nothing.
constexpr double kRefClockEnd = 0x1p30;       // clocks and reference lengths stay below: row indices are 32-bit in the kernels
static int set_reference(mi_ilqr* h, const double* src, size_t bytes) {
  if (!src && bytes == 0) { store_drop(h->reference); h->ref_T = 0; h->ref_clock = 0; return MI_ILQR_OK; }
  if (!h->large || h->plant_state.synced) return MI_ILQR_E_UNSUPPORTED;
  const size_t per_row = (size_t)h->B * h->n;
  if (bytes == 0 || bytes % (per_row * 8) != 0) return MI_ILQR_E_BAD_SHAPE;
  const size_t T = bytes / (per_row * 8), cnt = per_row * T;
  if ((double)T >= kRefClockEnd) return MI_ILQR_E_BAD_SHAPE;
  if (!src) return MI_ILQR_E_BAD_ARG;
  for (size_t i = 0; i < cnt; ++i) if (!std::isfinite(src[i])) return MI_ILQR_E_BAD_ARG;
  HIPCHK(hipSetDevice(h->d.device_id));
  int rc = MI_ILQR_OK;
  if (!h->ref_qn && (rc = dev_alloc(h, h->ref_qn, (size_t)h->B * (h->N - 1) * h->n)) != MI_ILQR_OK) return rc;
  RowStore& s = h->reference;
  if (s.width != T * (size_t)h->n) store_drop(s);           // (another length: nothing of the old rows can be kept)
  if (cnt > h->ref_cap) {                                  // a longer reference: a block of its own size (kernels in flight read the old one)
    HIPCHK(hipStreamSynchronize(h->stream));
    store_drop(s);
    h->ref_T = 0; h->ref_cap = 0;
    if ((rc = dev_free(h, s.rows)) != MI_ILQR_OK) return rc;
  }
  s.width = T * (size_t)h->n;
  if ((rc = store_upload(h, s, src)) != MI_ILQR_OK) { h->ref_T = 0; return rc; }
  if (cnt > h->ref_cap) h->ref_cap = cnt;
  h->ref_T = (int)T;
  return MI_ILQR_OK;
}

static int set_ref_clock(mi_ilqr* h, const double* src, size_t bytes) {
  if (!h->large) return MI_ILQR_E_UNSUPPORTED;
  if (bytes != 8) return MI_ILQR_E_BAD_SHAPE;
  if (!src) return MI_ILQR_E_BAD_ARG;
  const double c = *src;
  if (!(c >= 0.0 && c < kRefClockEnd && c == std::floor(c))) return MI_ILQR_E_BAD_ARG;
  h->ref_clock = (long long)c;
  return MI_ILQR_OK;
}

// Per-problem model parameters (MI_F_MODEL_PARAMS): (B, n_params) rows, problem b's plant in row b.  src == NULL with bytes == 0:
// back to the descriptor's parameters - the kernels read KArgs::params, as on a handle that never left them.
static int set_model_params(mi_ilqr* h, const double* src, size_t bytes) {
  const size_t cnt = (size_t)h->B * h->params.width;
  if (cnt == 0) return MI_ILQR_E_UNSUPPORTED;
  if (!src && bytes == 0) { store_drop(h->params); return MI_ILQR_OK; }
  if (bytes != cnt * 8) return MI_ILQR_E_BAD_SHAPE;
  if (!src) return MI_ILQR_E_BAD_ARG;
  for (size_t i = 0; i < cnt; ++i) if (!std::isfinite(src[i])) return MI_ILQR_E_BAD_ARG;
  return store_upload(h, h->params, src);
}

// The disturbances of mi_ilqr_policy_rollout.  MI_F_POLICY_NOISE: (B, n + m) rows sigma_x | sigma_u, standard deviations - finite
// and non-negative, zero on the padding controls; src == NULL with bytes == 0: no noise, the noise-free kernels again.
// MI_F_POLICY_STREAM: seed | first_sample | common as doubles holding integers.  A refused call changes nothing.
// (the same rows and rules serve the plant of the closed MPC loop: MI_F_PLANT_NOISE, a store of its own)
static int set_noise_rows(mi_ilqr* h, RowStore& store, const double* src, size_t bytes) {
  const size_t w = store.width, cnt = (size_t)h->B * w;
  if (!src && bytes == 0) { store_drop(store); return MI_ILQR_OK; }
  if (bytes != cnt * 8) return MI_ILQR_E_BAD_SHAPE;
  if (!src) return MI_ILQR_E_BAD_ARG;
  const int m_user = model_of(h->d.model_id)->p.m_user;
  const size_t first_pad = (size_t)h->n + (m_user > 0 ? (size_t)m_user : (size_t)h->m);
  for (size_t i = 0; i < cnt; ++i) {
    if (!std::isfinite(src[i]) || src[i] < 0.0) return MI_ILQR_E_BAD_ARG;
    if (i % w >= first_pad && src[i] != 0.0) return MI_ILQR_E_BAD_ARG;
  }
  return store_upload(h, store, src);
}

// The plant of the closed MPC loop (mi_ilqr_mpc_run; plant_advance.hpp).  MI_F_PLANT_STATE: (B, n) finite states - the handle holds
// a plant from now on, and every plant is running again; src == NULL with bytes == 0: no plant, mi_ilqr_mpc_run is the open loop.
// MI_F_PLANT_PARAMS: set_model_params' rules on the plants' own rows.  MI_F_PLANT_STREAM: seed | clock | common | feedback.
// A refused call changes nothing.
static int set_plant_state(mi_ilqr* h, const double* src, size_t bytes) {
  const size_t cnt = (size_t)h->B * h->n;
  if (!src && bytes == 0) { store_drop(h->plant_state); return MI_ILQR_OK; }
  if (h->reference.synced) return MI_ILQR_E_UNSUPPORTED;      // (the plant kernels know constant targets only)
  if (bytes != cnt * 8) return MI_ILQR_E_BAD_SHAPE;
  if (!src) return MI_ILQR_E_BAD_ARG;
  for (size_t i = 0; i < cnt; ++i) if (!std::isfinite(src[i])) return MI_ILQR_E_BAD_ARG;
  HIPCHK(hipSetDevice(h->d.device_id));
  int rc = h->plant_dead ? MI_ILQR_OK : dev_alloc(h, h->plant_dead, (size_t)h->B);
  if (rc != MI_ILQR_OK) return rc;
  HIPCHK(hipMemsetAsync(h->plant_dead, 0, (size_t)h->B * 8, h->stream));
  return store_upload(h, h->plant_state, src);
}

static int set_plant_params(mi_ilqr* h, const double* src, size_t bytes) {
  const size_t cnt = (size_t)h->B * h->plant_params.width;
  if (cnt == 0) return MI_ILQR_E_UNSUPPORTED;
  if (!src && bytes == 0) { store_drop(h->plant_params); return MI_ILQR_OK; }
  if (bytes != cnt * 8) return MI_ILQR_E_BAD_SHAPE;
  if (!src) return MI_ILQR_E_BAD_ARG;
  for (size_t i = 0; i < cnt; ++i) if (!std::isfinite(src[i])) return MI_ILQR_E_BAD_ARG;
  return store_upload(h, h->plant_params, src);
}

static int set_plant_stream(mi_ilqr* h, const double* src, size_t bytes) {
  if (bytes != 4 * 8) return MI_ILQR_E_BAD_SHAPE;
  if (!src) return MI_ILQR_E_BAD_ARG;
  const double seed = src[0], clock = src[1], common = src[2], feedback = src[3];
  if (!(seed >= 0.0 && seed < 0x1p53 && seed == std::floor(seed))) return MI_ILQR_E_BAD_ARG;
  if (!(clock >= 0.0 && clock < 0x1p32 && clock == std::floor(clock))) return MI_ILQR_E_BAD_ARG;
  if (!(common == 0.0 || common == 1.0) || !(feedback == 0.0 || feedback == 1.0)) return MI_ILQR_E_BAD_ARG;
  h->plant_seed = (unsigned long long)seed;
  h->plant_clock = (unsigned long long)clock;
  h->plant_common = common == 1.0;
  h->plant_feedback = feedback == 1.0;
  return MI_ILQR_OK;
}

static int set_policy_stream(mi_ilqr* h, const double* src, size_t bytes) {
  if (bytes != 3 * 8) return MI_ILQR_E_BAD_SHAPE;
  if (!src) return MI_ILQR_E_BAD_ARG;
  const double seed = src[0], first = src[1], common = src[2];
  // (the comparisons are false for a NaN; an integer below 2^53 is exact in a double)
  if (!(seed >= 0.0 && seed < 0x1p53 && seed == std::floor(seed))) return MI_ILQR_E_BAD_ARG;
  if (!(first >= 0.0 && first < 0x1p32 && first == std::floor(first))) return MI_ILQR_E_BAD_ARG;
  if (!(common == 0.0 || common == 1.0)) return MI_ILQR_E_BAD_ARG;
  h->policy_seed = (unsigned long long)seed;
  h->policy_first_sample = (uint32_t)first;
  h->policy_common = common == 1.0;
  return MI_ILQR_OK;
}

// The cost class of one set of matrices, cm = Q | R | Qf (mi_ilqr_set_cost and every row of MI_F_COST_MATRICES decide it here):
// `regular` - symmetric, Q and Qf positive semi-definite, R positive definite: the fast backward forms; otherwise the reference's
// recursion (exact_backward), and on the workgroup-per-problem kernels `asym` when a matrix is not symmetric.  May write cm: the
// n >= 33 kernels' round-off symmetrisation.  MI_ILQR_E_UNSUPPORTED: a non-finite entry the workgroup-per-problem kernels cannot take
// (mi_ilqr_set_cost only: the rows of MI_F_COST_MATRICES are finite when they get here - set_cost_rows refuses others up front,
// for every kernel family, with the MI_ILQR_E_BAD_ARG the header documents).
static int classify_cost(const mi_ilqr* h, double* cm, bool* regular_out, bool* asym_out) {
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
static void apply_cost_class(mi_ilqr* h) {
  h->exact_backward = h->costs.synced ? h->rows_exact_backward : h->shared_exact_backward;
  h->cost_asym = h->costs.synced ? h->rows_cost_asym : h->shared_cost_asym;
}

static void drop_per_problem_costs(mi_ilqr* h) {
  store_drop(h->costs);
  apply_cost_class(h);
}

// Per-problem cost matrices (MI_F_COST_MATRICES): (B, 2 n^2 + m^2) rows, row b = Q_b | R_b | Qf_b.  Every row is classified like
// mi_ilqr_set_cost classifies the shared matrices, and the handle runs the most general form a row needs.  What is stored (and
// mi_ilqr_get returns) is the rows as the kernels get them, i.e. after the n >= 33 round-off symmetrisation.  src == NULL with
// bytes == 0: back to the shared matrices.
static int set_cost_rows(mi_ilqr* h, const double* src, size_t bytes) {
  const size_t B = h->B, len = cost_len(h);
  if (!src && bytes == 0) { drop_per_problem_costs(h); return MI_ILQR_OK; }
  if (bytes != B * len * 8) return MI_ILQR_E_BAD_SHAPE;
  if (!src) return MI_ILQR_E_BAD_ARG;
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
  const int rc = stage_h2d(h, h->costmat, h->h_costmat.data(), h->h_costmat.size() * 8);    // Q | R | Qf | x_nom: one copy
  h->costmat_synced = rc == MI_ILQR_OK;
  return rc;
}

// tiny batches of the wave-per-problem kernels keep x0 / u_guess in page-locked host memory the kernels read directly (host.hpp:
// host_inputs): setting them is a memcpy once nothing on the stream can still be reading the old values - no copy engine, no
// broadcast kernel in front of the solve (C1: two ~5 us copies + one launch off the critical path of every Solve())
static int host_inputs_write(mi_ilqr* h, const double* x0, const double* u_guess, bool shared) {
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

int mi_ilqr_set_initial(mi_ilqr_t* h, const double* x0, const double* u_guess) {
  if (!h) return MI_ILQR_E_BAD_ARG;
  HIPCHK(hipSetDevice(h->d.device_id));
  if (h->host_inputs) return host_inputs_write(h, x0, u_guess, false);
  if (x0) { const int rc = stage_h2d(h, h->x0, x0, (size_t)h->B * h->n * 8); if (rc != MI_ILQR_OK) return rc; }
  if (u_guess) {
    const size_t cnt = (size_t)h->B * h->m * (h->N - 1);
    int rows = 0, len = 0;
    if (needs_relayout(h, MI_F_U_BAR, &rows, &len)) {
      int rc = ensure_scratch(h, cnt * 8);
      if (rc != MI_ILQR_OK) return rc;
      HIPCHK(hipStreamSynchronize(h->stream));
      HIPCHK(hipMemcpy(h->scratch, u_guess, cnt * 8, hipMemcpyHostToDevice));
      if ((rc = relayout(h, h->scratch, h->u_guess, rows, len, true)) != MI_ILQR_OK) return rc;
      HIPCHK(hipStreamSynchronize(h->stream));
    } else {
      const int rc = stage_h2d(h, h->u_guess, u_guess, cnt * 8);
      if (rc != MI_ILQR_OK) return rc;
    }
    h->u_pending = true;
    h->u_zero = false;
  }
  return MI_ILQR_OK;
}

int mi_ilqr_set_initial_shared(mi_ilqr_t* h, const double* x0, const double* u_guess_one) {
  if (!h) return MI_ILQR_E_BAD_ARG;
  HIPCHK(hipSetDevice(h->d.device_id));
  if (h->host_inputs) return host_inputs_write(h, x0, u_guess_one, true);
  if (x0) { const int rc = stage_h2d(h, h->x0, x0, (size_t)h->B * h->n * 8); if (rc != MI_ILQR_OK) return rc; }
  if (u_guess_one) {
    const size_t one = (size_t)h->m * (h->N - 1);
    int rc = h->u_one ? MI_ILQR_OK : dev_alloc(h, h->u_one, one);
    if (rc == MI_ILQR_OK) rc = stage_h2d(h, h->u_one, u_guess_one, one * 8);
    if (rc != MI_ILQR_OK) return rc;
    const size_t total = one * h->B;
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(broadcast_u_kernel, dim3(blocks), dim3(256), 0, h->stream, h->u_one, h->u_guess, h->B, h->m, h->N - 1, layout_of(h));
    HIPCHK(hipGetLastError());
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

// Whether a workgroup-per-problem handle has Limited<M> kernels: the mid-size layout (n <= 32), and kernels the model was built
// with (asked through its launch entry, which launches nothing for the probe).
static bool large_accepts_limits(mi_ilqr* h) {
  if (h->n > 32) return false;
  const KArgs a = make_args(h);
  return model_of(h->d.model_id)->p.launch(h, kModeProbeLimits, &a) == MI_ILQR_OK;
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
  if (!h->s2) {
    int rc = h->ulim ? MI_ILQR_OK : dev_alloc(h, h->ulim, (size_t)B * 2 * m);
    if (rc == MI_ILQR_OK) rc = dev_alloc(h, h->s2, (size_t)B);
    if (rc != MI_ILQR_OK) return rc;
    HIPCHK(hipMemsetAsync(h->s2, 0, (size_t)B * 8, h->stream));
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
  HIPCHK(hipStreamSynchronize(h->stream));
  return MI_ILQR_OK;
}

int mi_ilqr_solve_async(mi_ilqr_t* h) {
  if (!h) return MI_ILQR_E_BAD_ARG;
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
  return MI_ILQR_OK;
}

static void fill_stats(mi_ilqr* h, int slot, mi_ilqr_stats* st) {
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

int mi_ilqr_collect_stats(mi_ilqr_t* h, mi_ilqr_stats* st) {
  if (!h || !st) return MI_ILQR_E_BAD_ARG;
  HIPCHK(hipSetDevice(h->d.device_id));
  { const int rc = reduce_pending_stats(h); if (rc != MI_ILQR_OK) return rc; }
  HIPCHK(hipStreamSynchronize(h->stream));
  fill_stats(h, (int)(h->h_stats - h->h_ring), st);
  return MI_ILQR_OK;
}

int mi_ilqr_collect_stats_n(mi_ilqr_t* h, int32_t count, mi_ilqr_stats* st) {
  if (!h || !st || count < 1 || count > mi_ilqr::kStatsRing || count > h->seq) return MI_ILQR_E_BAD_ARG;
  HIPCHK(hipSetDevice(h->d.device_id));
  { const int rc = reduce_pending_stats(h); if (rc != MI_ILQR_OK) return rc; }
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int i = 0; i < count; ++i) fill_stats(h, (int)((h->seq - count + i) % mi_ilqr::kStatsRing), st + i);
  return MI_ILQR_OK;
}

int mi_ilqr_solve(mi_ilqr_t* h, mi_ilqr_stats* stats) {
  int rc = mi_ilqr_solve_async(h);
  if (rc != MI_ILQR_OK) return rc;
  if (stats) return mi_ilqr_collect_stats(h, stats);
  return mi_ilqr_synchronize(h);
}

static int upload_stage_in(mi_ilqr* h, const double* v) {
  if (!v) return MI_ILQR_E_BAD_ARG;
  HIPCHK(hipSetDevice(h->d.device_id));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(h->stage_in, v, (size_t)h->B * 8, hipMemcpyHostToDevice));
  return MI_ILQR_OK;
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

int mi_ilqr_policy_rollout(mi_ilqr_t* h, int32_t S, const double* x0, const double* params, double* cost, double* x_final,
                           int32_t* steps, double* X, double* U) {
  if (!h || S < 1 || !x0 || !cost) return MI_ILQR_E_BAD_ARG;
  if (h->reference.synced) return MI_ILQR_E_UNSUPPORTED;      // (the policy kernels cost a rollout against a constant target only)
  const Model* model = model_of(h->d.model_id);
  const size_t B = h->B, n = h->n, m = h->m, N = h->N, np = model->p.n_params, Sz = (size_t)S, W = n + m + m * n;
  if (params && np == 0) return MI_ILQR_E_UNSUPPORTED;
  if (params) for (size_t i = 0; i < B * Sz * np; ++i) if (!std::isfinite(params[i])) return MI_ILQR_E_BAD_ARG;
  const bool noisy = h->policy_noise.synced;
  if (noisy && (unsigned long long)h->policy_first_sample + (unsigned long long)S > 0x100000000ull) return MI_ILQR_E_BAD_ARG;   // (the sample counter is 32 bits)
  HIPCHK(hipSetDevice(h->d.device_id));
  // one block of the handle's grow-only scratch, in doubles: the policy's time-major copy | inputs as they arrive and sample-minor |
  // outputs sample-minor and in the boundary's layout
  size_t off = 0;
  auto take = [&](size_t count) { const size_t o = off; off += (count + 31) & ~(size_t)31; return o; };
  const size_t o_pol = take(B * (N - 1) * W), o_x0_in = take(B * Sz * n), o_x0 = take(B * n * Sz);
  const size_t o_p_in = take(params ? B * Sz * np : 0), o_p = take(params ? B * np * Sz : 0), o_prow = take(np ? np : 1);
  const size_t o_cost = take(B * Sz), o_steps = take((B * Sz + 1) / 2), o_xf = take(B * n * Sz), o_xf_out = take(B * Sz * n);
  const size_t o_X = take(X ? B * N * n * Sz : 0), o_X_out = take(X ? B * Sz * n * N : 0);
  const size_t o_U = take(U ? B * (N - 1) * m * Sz : 0), o_U_out = take(U ? B * Sz * m * (N - 1) : 0);
  int rc = ensure_scratch(h, off * 8);
  if (rc != MI_ILQR_OK) return rc;
  double* const sc = h->scratch;
  if (!h->policy_ev0) {
    HIPCHK(hipEventCreate(&h->policy_ev0));
    HIPCHK(hipEventCreate(&h->policy_ev1));
  }
  // the policy as the handle holds it now: a cold handle's x_bar and K read as zeros, a reset one's u_bar too, a pending initial
  // guess is the u_bar the next launch would start from - nothing of the handle is written
  const double* u_src = h->u_pending ? h->u_guess : (h->u_zero ? nullptr : h->u_bar);
  {
    const size_t total = B * (N - 1) * W;
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(policy_pack_kernel, dim3(blocks), dim3(256), 0, h->stream, h->cold ? nullptr : h->x_bar, u_src,
                       h->cold ? nullptr : h->K, sc + o_pol, (int)B, (int)n, (int)m, (int)N,
                       layout_of(h));
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemcpyAsync(sc + o_x0_in, x0, B * Sz * n * 8, hipMemcpyHostToDevice, h->stream));
  if ((rc = transpose_tiles(h, sc + o_x0_in, sc + o_x0, S, (int)n, B, 1, Sz * n, 0, n, n * Sz, 0, Sz)) != MI_ILQR_OK) return rc;
  if (params) {
    HIPCHK(hipMemcpyAsync(sc + o_p_in, params, B * Sz * np * 8, hipMemcpyHostToDevice, h->stream));
    if ((rc = transpose_tiles(h, sc + o_p_in, sc + o_p, S, (int)np, B, 1, Sz * np, 0, np, np * Sz, 0, Sz)) != MI_ILQR_OK) return rc;
  } else if (np && !h->params.synced) {
    if ((rc = stage_h2d(h, sc + o_prow, h->d.model_params, np * 8)) != MI_ILQR_OK) return rc;
  }
  PolicyArgs a{};
  a.policy = sc + o_pol; a.x0 = sc + o_x0; a.params = params ? sc + o_p : nullptr;
  // every per-problem array: its device rows with a row's stride, else the one shared row with stride 0
  auto rows_or = [](const RowStore& s, const double* shared_row, size_t* stride) {
    *stride = s.synced ? s.width : 0;
    return s.synced ? s.rows : shared_row;
  };
  a.param_rows = rows_or(h->params, sc + o_prow, &a.param_stride);
  a.cost = rows_or(h->costs, h->costmat, &a.cost_stride);
  a.x_nom = rows_or(h->targets, h->costmat + cost_len(h), &a.x_nom_stride);
  a.ulim = h->limited ? h->ulim : nullptr;
  a.noise = noisy ? h->policy_noise.rows : nullptr;
  a.seed = h->policy_seed; a.first_sample = h->policy_first_sample; a.common = h->policy_common ? 1 : 0;
  a.cost_out = sc + o_cost; a.x_final = sc + o_xf; a.steps = reinterpret_cast<int32_t*>(sc + o_steps);
  a.X = X ? sc + o_X : nullptr; a.U = U ? sc + o_U : nullptr;
  a.dt = h->d.dt; a.N = (int32_t)N; a.S = S; a.B = (int32_t)B; a.m_user = model->p.m_user > 0 ? model->p.m_user : (int32_t)m;
  h->policy_ran = h->policy_last_mc = false;
  if ((rc = model->p.launch(h, kModePolicyRollout, &a)) != MI_ILQR_OK) return rc;
  h->policy_ran = true;
  // sample-minor -> the boundary's layouts: x_final (B,S,n), X (B,S,n,N), U (B,S,m,N-1)
  HIPCHK(hipMemcpyAsync(cost, sc + o_cost, B * Sz * 8, hipMemcpyDeviceToHost, h->stream));
  if (steps) HIPCHK(hipMemcpyAsync(steps, sc + o_steps, B * Sz * 4, hipMemcpyDeviceToHost, h->stream));
  if (x_final) {
    if ((rc = transpose_tiles(h, sc + o_xf, sc + o_xf_out, (int)n, S, B, 1, n * Sz, 0, Sz, Sz * n, 0, n)) != MI_ILQR_OK) return rc;
    HIPCHK(hipMemcpyAsync(x_final, sc + o_xf_out, B * Sz * n * 8, hipMemcpyDeviceToHost, h->stream));
  }
  if (X) {
    if ((rc = transpose_tiles(h, sc + o_X, sc + o_X_out, (int)N, S, B, (int)n, N * n * Sz, Sz, n * Sz, Sz * n * N, N, n * N)) != MI_ILQR_OK) return rc;
    HIPCHK(hipMemcpyAsync(X, sc + o_X_out, B * Sz * n * N * 8, hipMemcpyDeviceToHost, h->stream));
  }
  if (U) {
    if ((rc = transpose_tiles(h, sc + o_U, sc + o_U_out, (int)N - 1, S, B, (int)m, (N - 1) * m * Sz, Sz, m * Sz, Sz * m * (N - 1), N - 1,
                              m * (N - 1))) != MI_ILQR_OK) return rc;
    HIPCHK(hipMemcpyAsync(U, sc + o_U_out, B * Sz * m * (N - 1) * 8, hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  return MI_ILQR_OK;
}

// Monte-Carlo on the device (include/mi_ilqr.h).  MI_F_POLICY_MC_DIST: (B, 3 n + 2 n_params) rows x0_mean | x0_spread | goal |
// p_mean | p_spread - means and spreads finite, spreads and goals non-negative, a goal may be +inf; src == NULL with bytes == 0
// clears the rows.  A refused call changes nothing.
static int set_mc_dist(mi_ilqr* h, const double* src, size_t bytes) {
  RowStore& s = h->policy_mc_dist;
  const size_t n = h->n, w = s.width, np = (w - 3 * n) / 2, cnt = (size_t)h->B * w;
  if (!src && bytes == 0) { store_drop(s); return MI_ILQR_OK; }
  if (bytes != cnt * 8) return MI_ILQR_E_BAD_SHAPE;
  if (!src) return MI_ILQR_E_BAD_ARG;
  for (size_t i = 0; i < cnt; ++i) {
    const size_t c = i % w;
    const double v = src[i];
    const bool goal = c >= 2 * n && c < 3 * n, spread = (c >= n && c < 2 * n) || c >= 3 * n + np;
    if (std::isnan(v) || (!goal && !std::isfinite(v)) || ((goal || spread) && v < 0.0)) return MI_ILQR_E_BAD_ARG;
  }
  return store_upload(h, s, src);
}

// MI_F_POLICY_MC_BOX: (B, 2 n) rows lo | hi, +-inf = unbounded; a NaN or lo > hi is refused; src == NULL with bytes == 0 clears the
// box.  MI_F_POLICY_MC_OBSERVE: one double, 0 .. 3 (bit 0 state envelopes, bit 1 control envelopes).  A refused call changes nothing.
static int set_mc_box(mi_ilqr* h, const double* src, size_t bytes) {
  RowStore& s = h->mc_box;
  const size_t n = h->n, cnt = (size_t)h->B * 2 * n;
  if (!src && bytes == 0) { store_drop(s); return MI_ILQR_OK; }
  if (bytes != cnt * 8) return MI_ILQR_E_BAD_SHAPE;
  if (!src) return MI_ILQR_E_BAD_ARG;
  for (size_t b = 0; b < (size_t)h->B; ++b)
    for (size_t i = 0; i < n; ++i) {
      const double lo = src[b * 2 * n + i], hi = src[b * 2 * n + n + i];
      if (!(lo <= hi)) return MI_ILQR_E_BAD_ARG;               // (a NaN on either side, or an inverted interval)
    }
  return store_upload(h, s, src);
}

static int set_mc_observe(mi_ilqr* h, const double* src, size_t bytes) {
  if (bytes != 8) return MI_ILQR_E_BAD_SHAPE;
  if (!src) return MI_ILQR_E_BAD_ARG;
  if (!(*src == 0.0 || *src == 1.0 || *src == 2.0 || *src == 3.0)) return MI_ILQR_E_BAD_ARG;
  h->mc_observe = (int32_t)*src;
  return MI_ILQR_OK;
}

// MI_F_POLICY_MC_RUN: v = S | x0_dist | p_dist | sample_params | samples.  Draws, rolls out and reduces S samples per problem on the
// handle's stream - passes over windows of sample groups, each one rollout kernel and one fold (policy_mc.hpp) - and synchronizes
// once.  Nothing of the handle's solver state is written; the staging memory is the grow-only scratch.
constexpr size_t kMcWindowBytes = 64u << 20;      // what the partials and the optional sample buffers of one pass may take
constexpr unsigned long long kMcEventPairs = 32;  // event pairs a handle keeps for the passes of a run
constexpr size_t kMcTrajWindowBytes = (size_t)1 << 30;   // ... and the trajectory windows of a run that observes envelopes or a box (at least one group)
static int run_policy_mc(mi_ilqr* h, const double* v, size_t bytes) {
  if (bytes != 5 * 8) return MI_ILQR_E_BAD_SHAPE;
  if (!v) return MI_ILQR_E_BAD_ARG;
  if (!(v[0] >= 1.0 && v[0] <= 0x1p32 && v[0] == std::floor(v[0]))) return MI_ILQR_E_BAD_ARG;
  for (int i = 1; i < 5; ++i) if (!(v[i] == 0.0 || v[i] == 1.0)) return MI_ILQR_E_BAD_ARG;
  if (h->reference.synced) return MI_ILQR_E_UNSUPPORTED;      // (the policy kernels cost a rollout against a constant target only)
  if (!h->policy_mc_dist.synced) return MI_ILQR_E_BAD_ARG;
  const unsigned long long S = (unsigned long long)v[0];
  if ((unsigned long long)h->policy_first_sample + S > 0x100000000ull) return MI_ILQR_E_BAD_ARG;   // (the sample counter is 32 bits)
  const Model* model = model_of(h->d.model_id);
  const size_t B = h->B, n = h->n, m = h->m, N = h->N, np = model->p.n_params, W = n + m + m * n, SW = n + np + 2;
  const bool sample_params = v[3] == 1.0, want_samples = v[4] == 1.0;
  if (sample_params && np == 0) return MI_ILQR_E_UNSUPPORTED;
  HIPCHK(hipSetDevice(h->d.device_id));
  // the window: as many groups of 64 samples per pass as the cap allows (MI_ILQR_MC_PASS_GROUPS forces it)
  const unsigned long long G = (S + 63) / 64;
  const size_t group_bytes = (size_t)kMcFields * B * 8 + (want_samples ? 2 * B * 64 * SW * 8 : 0);
  unsigned long long k = std::max<unsigned long long>(1, kMcWindowBytes / group_bytes);
  // what the run observes beside the cost (policy_env.hpp): the window's trajectories stay in the scratch, under a cap of their own
  const bool want_box = h->mc_box.synced, env_x = (h->mc_observe & 1) != 0, env_u = (h->mc_observe & 2) != 0;
  const bool keep_x = want_box || env_x, observing = keep_x || env_u;
  const size_t Rx = N * n, Ru = (N - 1) * m;
  if (observing) {
    const size_t traj_group_bytes = B * 64 * 8 * ((keep_x ? Rx : 0) + (env_u ? Ru : 0));
    k = std::min(k, std::max<unsigned long long>(1, kMcTrajWindowBytes / traj_group_bytes));
  }
  if (switches().mc_pass_groups > 0) k = (unsigned long long)switches().mc_pass_groups;
  k = std::min(std::min(k, G), std::max<unsigned long long>(1, 0x7fffffffull / B));
  const unsigned long long passes = (G + k - 1) / k;
  std::vector<double> samples;
  if (want_samples) {
    if (S > (unsigned long long)(SIZE_MAX / 8) / (B * SW)) return MI_ILQR_E_UNSUPPORTED;
    try { samples.resize(B * (size_t)S * SW); } catch (const std::bad_alloc&) { return MI_ILQR_E_UNSUPPORTED; }
  }
  size_t off = 0;
  auto take = [&](size_t count) { const size_t o = off; off += (count + 31) & ~(size_t)31; return o; };
  const size_t win_max = (size_t)k * 64;
  const size_t o_pol = take(B * (N - 1) * W), o_prow = take(np ? np : 1), o_part = take((size_t)k * kMcFields * B);
  const size_t o_smp = take(want_samples ? B * SW * win_max : 0), o_smp_out = take(want_samples ? B * win_max * SW : 0);
  const size_t o_X = take(keep_x ? B * Rx * win_max : 0), o_U = take(env_u ? B * Ru * win_max : 0);
  int rc = ensure_scratch(h, off * 8);
  if (rc != MI_ILQR_OK && observing) { (void)hipGetLastError(); return MI_ILQR_E_UNSUPPORTED; }   // (the windows did not fit: the last results stay)
  if (rc != MI_ILQR_OK) return rc;
  double* const sc = h->scratch;
  if (!h->mc_acc && (rc = dev_alloc(h, h->mc_acc, (size_t)kMcFields * B)) != MI_ILQR_OK) return rc;
  if (observing) {
    if (env_x && !h->env_acc_x) rc = dev_alloc(h, h->env_acc_x, B * Rx * 8);
    if (rc == MI_ILQR_OK && env_u && !h->env_acc_u) rc = dev_alloc(h, h->env_acc_u, B * Ru * 8);
    if (rc == MI_ILQR_OK && want_box && !h->box_counters) rc = dev_alloc(h, h->box_counters, B * (3 + N));
    if (rc != MI_ILQR_OK) { (void)hipGetLastError(); return MI_ILQR_E_UNSUPPORTED; }
    if (want_box) HIPCHK(hipMemsetAsync(h->box_counters, 0, B * (3 + N) * 8, h->stream));
  }
  // one start / stop pair per pass, at most kMcEventPairs of them: a run of more passes waits for the stream every kMcEventPairs
  // passes, adds their times up and uses the pairs again
  const size_t pairs = (size_t)std::min<unsigned long long>(passes, kMcEventPairs);
  while (h->mc_events.size() < 2 * pairs) {
    hipEvent_t e = nullptr;
    HIPCHK(hipEventCreate(&e));
    h->mc_events.push_back(e);
  }
  // the policy as the handle holds it now (mi_ilqr_policy_rollout's rules)
  const double* u_src = h->u_pending ? h->u_guess : (h->u_zero ? nullptr : h->u_bar);
  {
    const size_t total = B * (N - 1) * W;
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(policy_pack_kernel, dim3(blocks), dim3(256), 0, h->stream, h->cold ? nullptr : h->x_bar, u_src,
                       h->cold ? nullptr : h->K, sc + o_pol, (int)B, (int)n, (int)m, (int)N, layout_of(h));
    HIPCHK(hipGetLastError());
  }
  if (np && !h->params.synced && (rc = stage_h2d(h, sc + o_prow, h->d.model_params, np * 8)) != MI_ILQR_OK) return rc;
  PolicyMcArgs a{};
  auto rows_or = [](const RowStore& s, const double* shared_row, size_t* stride) {
    *stride = s.synced ? s.width : 0;
    return s.synced ? s.rows : shared_row;
  };
  a.r.policy = sc + o_pol;
  a.r.param_rows = rows_or(h->params, sc + o_prow, &a.r.param_stride);
  a.r.cost = rows_or(h->costs, h->costmat, &a.r.cost_stride);
  a.r.x_nom = rows_or(h->targets, h->costmat + cost_len(h), &a.r.x_nom_stride);
  a.r.ulim = h->limited ? h->ulim : nullptr;
  a.r.noise = h->policy_noise.synced ? h->policy_noise.rows : nullptr;
  a.r.seed = h->policy_seed; a.r.first_sample = h->policy_first_sample; a.r.common = h->policy_common ? 1 : 0;
  a.r.dt = h->d.dt; a.r.N = (int32_t)N; a.r.B = (int32_t)B; a.r.m_user = model->p.m_user > 0 ? model->p.m_user : (int32_t)m;
  a.dist = h->policy_mc_dist.rows; a.partials = sc + o_part; a.acc = h->mc_acc; a.samples = want_samples ? sc + o_smp : nullptr;
  a.S = S; a.x0_dist = (int32_t)v[1]; a.p_dist = (int32_t)v[2]; a.sample_params = sample_params ? 1 : 0;
  if (keep_x) a.r.X = sc + o_X;
  if (env_u) a.r.U = sc + o_U;
  std::vector<double> env_x_out, env_u_out, safety_out;
  std::vector<unsigned long long> box_out;
  if (observing) {
    try {
      if (env_x) env_x_out.resize(B * Rx * 8);
      if (env_u) env_u_out.resize(B * Ru * 8);
      if (want_box) { box_out.resize(B * (3 + N)); safety_out.resize(B * (3 + N)); }
    } catch (const std::bad_alloc&) { return MI_ILQR_E_UNSUPPORTED; }
  }
  // From here on copies into `samples` and `acc` may be queued on the stream: whatever fails, the stream is waited for before
  // the two go out of scope.
  std::vector<double> acc((size_t)kMcFields * B);
  double ms_sum = 0.0;
  auto timed = [&](unsigned long long used) -> int {          // the stream is idle: add the kernels of the pairs in use
    for (unsigned long long q = 0; q < used; ++q) {
      float ms = 0.0f;
      HIPCHK(hipEventElapsedTime(&ms, h->mc_events[2 * q], h->mc_events[2 * q + 1]));
      ms_sum += (double)ms;
    }
    return MI_ILQR_OK;
  };
  auto passes_and_copies = [&]() -> int {
    unsigned long long pass = 0;
    for (unsigned long long g0 = 0; g0 < G; g0 += k, ++pass) {
      const unsigned long long kg = std::min(k, G - g0), s0 = g0 * 64, slot = pass % kMcEventPairs;
      if (pass > 0 && slot == 0) {
        HIPCHK(hipStreamSynchronize(h->stream));
        if (const int rt = timed(kMcEventPairs); rt != MI_ILQR_OK) return rt;
      }
      const size_t win = (size_t)std::min<unsigned long long>(S - s0, kg * 64);
      a.group0 = (uint32_t)g0; a.groups = (int32_t)kg; a.win_samples = win; a.first_pass = pass == 0 ? 1 : 0;
      a.ev0 = h->mc_events[2 * slot]; a.ev1 = h->mc_events[2 * slot + 1];
      if (const int rl = model->p.launch(h, kModePolicyMC, &a); rl != MI_ILQR_OK) return rl;
      if (observing) {        // the window's trajectories, reduced before the next pass overwrites them
        const double g_first = (double)h->policy_first_sample + (double)s0;
        int re = MI_ILQR_OK;
        if (env_x) re = launch_policy_env(h, sc + o_X, h->env_acc_x, B, Rx, win, g_first, a.first_pass);
        if (re == MI_ILQR_OK && env_u) re = launch_policy_env(h, sc + o_U, h->env_acc_u, B, Ru, win, g_first, a.first_pass);
        if (re == MI_ILQR_OK && want_box)
          re = launch_policy_box(h, sc + o_X, h->mc_box.rows, a.r.x_nom, a.r.x_nom_stride, a.dist + 2 * n, h->policy_mc_dist.width,
                                 h->box_counters, B, (int)n, (int)N, win);
        if (re != MI_ILQR_OK) return re;
      }
      if (want_samples) {     // sample-minor (B, SW, win) -> (B, win, SW), then rows s0 .. s0 + win - 1 of every problem's block
        if (const int rt = transpose_tiles(h, sc + o_smp, sc + o_smp_out, (int)SW, (int)win, B, 1, SW * win, 0, win, win * SW, 0, SW);
            rt != MI_ILQR_OK) return rt;
        HIPCHK(hipMemcpy2DAsync(samples.data() + (size_t)s0 * SW, (size_t)S * SW * 8, sc + o_smp_out, win * SW * 8, win * SW * 8, B,
                                hipMemcpyDeviceToHost, h->stream));
      }
    }
    HIPCHK(hipMemcpyAsync(acc.data(), h->mc_acc, acc.size() * 8, hipMemcpyDeviceToHost, h->stream));
    if (env_x) HIPCHK(hipMemcpyAsync(env_x_out.data(), h->env_acc_x, env_x_out.size() * 8, hipMemcpyDeviceToHost, h->stream));
    if (env_u) HIPCHK(hipMemcpyAsync(env_u_out.data(), h->env_acc_u, env_u_out.size() * 8, hipMemcpyDeviceToHost, h->stream));
    if (want_box) HIPCHK(hipMemcpyAsync(box_out.data(), h->box_counters, box_out.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return timed((passes - 1) % kMcEventPairs + 1);
  };
  if ((rc = passes_and_copies()) != MI_ILQR_OK) {
    (void)hipStreamSynchronize(h->stream);
    return rc;
  }
  // (10, B) -> (B, 10); a problem without a counted sample: mean = M2 = NaN (min = +inf, max = -inf, argmin = argmax = -1 as folded)
  h->mc_stats.assign(B * kMcFields, 0.0);
  for (size_t b = 0; b < B; ++b) {
    double* row = h->mc_stats.data() + b * kMcFields;
    for (int f = 0; f < kMcFields; ++f) row[f] = acc[(size_t)f * B + b];
    if (row[1] == 0.0) row[3] = row[4] = std::nan("");
  }
  h->mc_samples.swap(samples);
  h->mc_env_x.swap(env_x_out);                 // (not observed: empty, and the selectors refuse)
  h->mc_env_u.swap(env_u_out);
  for (size_t i = 0; i < box_out.size(); ++i) safety_out[i] = (double)box_out[i];
  h->mc_safety.swap(safety_out);
  h->mc_ms = ms_sum;
  h->mc_passes = (int32_t)std::min<unsigned long long>(passes, 0x7fffffffull);
  h->policy_last_mc = true;
  return MI_ILQR_OK;
}

int mi_ilqr_mpc_shift(mi_ilqr_t* h, int32_t replan_steps) {
  if (!h) return MI_ILQR_E_BAD_ARG;
  if (replan_steps < 1 || replan_steps >= h->N - 1) return MI_ILQR_E_BAD_ARG;
  HIPCHK(hipSetDevice(h->d.device_id));
  int rc;
  if ((rc = materialize_zero_state(h)) != MI_ILQR_OK) return rc;
  if ((rc = materialize_u(h)) != MI_ILQR_OK) return rc;
  if (h->batch_minor)
    hipLaunchKernelGGL(mpc_shift_kernel_bm, dim3((h->B + 255) / 256), dim3(256), 0, h->stream, h->x_bar, h->u_bar, h->x0,
                       h->u_guess, h->B, h->n, h->m, h->N, (int)replan_steps);
  else if (h->large)
    hipLaunchKernelGGL(mpc_shift_kernel_tm, dim3(h->B), dim3(64), 0, h->stream, h->x_bar, h->u_bar, h->x0, h->u_guess,
                       h->B, h->n, h->m, h->N, (int)replan_steps);
  else
    hipLaunchKernelGGL(mpc_shift_kernel, dim3(h->B), dim3(64), 0, h->stream, h->x_bar, h->u_bar, h->x0, h->u_guess,
                       h->B, h->n, h->m, h->N, (int)replan_steps);
  HIPCHK(hipGetLastError());
  h->u_pending = true;
  return MI_ILQR_OK;
}

// host-loop form of the receding-horizon loop: the record the single-launch kernels write themselves (x0 | cost | iterations).
// Same policy as theirs: a problem whose re-solve fails (line search, internal, NOT_PD) gets that re-solve's row and none after
// it (`dead`: one flag per problem behind the log; the rows stay the zeros mi_ilqr_mpc_run fills the log with).
__global__ void __launch_bounds__(256) mpc_log_fill_kernel(const double* __restrict__ x0, const double* __restrict__ cost,
                                                           const int32_t* __restrict__ iters, const int32_t* __restrict__ status,
                                                           double* __restrict__ log, double* __restrict__ dead, int B, int n, int resolves, int r) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B || dead[b] != 0.0) return;
  double* lg = log + ((size_t)b * resolves + r) * (n + 2);
  for (int i = 0; i < n; ++i) lg[i] = x0[(size_t)b * n + i];
  lg[n] = cost[b];
  lg[n + 1] = (double)iters[b];
  if ((status[b] & ~MI_STATUS_FLAG_INDEFINITE) >= MI_STATUS_LINESEARCH_FAILED) dead[b] = 1.0;
}

// The closed loop's plant (a handle that holds MI_F_PLANT_STATE), the part of a mi_ilqr_mpc_run that does not change from one
// re-solve to the next, staged problem-minor in the handle's scratch: the plants' parameters, Q | R, the bounds, the sigmas.
// Offsets in doubles; `pol` and `x_nom` are filled before every launch (plant_advance).
struct PlantStage { size_t pol, prm, prow, cost, x_nom, ulim, noise; };

static int rows_to_cols(mi_ilqr* h, const double* src, size_t stride, double* dst, size_t width) {
  const size_t total = width * (size_t)h->B;
  if (total == 0) return MI_ILQR_OK;
  hipLaunchKernelGGL(rows_to_cols_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 8192)), dim3(256), 0, h->stream, src, stride, dst,
                     (int)width, h->B);
  HIPCHK(hipGetLastError());
  return MI_ILQR_OK;
}

static int plant_prepare(mi_ilqr* h, int32_t num_resolves, int32_t replan_steps, PlantStage* st) {
  const Model* model = model_of(h->d.model_id);
  const size_t B = h->B, n = h->n, m = h->m, np = model->p.n_params, W = n + m + m * n, C = n + m + 1;
  size_t off = 0;
  auto take = [&](size_t count) { const size_t o = off; off += (count + 31) & ~(size_t)31; return o; };
  st->pol = take((size_t)replan_steps * W * B); st->prm = take(np * B); st->prow = take(np); st->cost = take((n * n + m * m) * B);
  st->x_nom = take(n * B); st->ulim = take(2 * m * B); st->noise = take((n + m) * B);
  int rc = ensure_scratch(h, off * 8);
  if (rc != MI_ILQR_OK) return rc;
  const size_t need = (size_t)num_resolves * replan_steps * C * B;
  if (h->plant_log_cap < need) {                 // grow-only
    HIPCHK(hipStreamSynchronize(h->stream));
    h->plant_log_cap = 0;
    if ((rc = dev_free(h, h->plant_log)) != MI_ILQR_OK) return rc;
    if ((rc = dev_alloc(h, h->plant_log, need)) != MI_ILQR_OK) return rc;
    h->plant_log_cap = need;
  }
  if (!h->plant_ev0) {
    HIPCHK(hipEventCreate(&h->plant_ev0));
    HIPCHK(hipEventCreate(&h->plant_ev1));
  }
  double* const sc = h->scratch;
  // the plants' parameters: their own rows, else the problems' model rows, else the descriptor's row for every problem
  if (np) {
    const RowStore& own = h->plant_params.synced ? h->plant_params : h->params;
    if (own.synced) rc = rows_to_cols(h, own.rows, np, sc + st->prm, np);
    else if ((rc = stage_h2d(h, sc + st->prow, h->d.model_params, np * 8)) == MI_ILQR_OK) rc = rows_to_cols(h, sc + st->prow, 0, sc + st->prm, np);
    if (rc != MI_ILQR_OK) return rc;
  }
  if ((rc = rows_to_cols(h, h->costs.synced ? h->costs.rows : h->costmat, h->costs.synced ? h->costs.width : 0, sc + st->cost, n * n + m * m)) != MI_ILQR_OK) return rc;
  if (h->limited && (rc = rows_to_cols(h, h->ulim, 2 * m, sc + st->ulim, 2 * m)) != MI_ILQR_OK) return rc;
  if (h->plant_noise.synced && (rc = rows_to_cols(h, h->plant_noise.rows, n + m, sc + st->noise, n + m)) != MI_ILQR_OK) return rc;
  return MI_ILQR_OK;
}

// Step 1 of a closed-loop round: the plants advance `replan_steps` steps under the policy the handle holds now (a cold handle's x_bar
// and K read as zeros, a reset one's u_bar too, a pending guess is read from where it waits), with the target the plan was solved for.
static int plant_advance(mi_ilqr* h, const PlantStage& st, int32_t round, int32_t replan_steps, double* mpc_dead) {
  const Model* model = model_of(h->d.model_id);
  const size_t B = h->B, n = h->n, m = h->m, W = n + m + m * n, C = n + m + 1;
  double* const sc = h->scratch;
  const double* u_src = h->u_pending ? h->u_guess : (h->u_zero ? nullptr : h->u_bar);
  {
    const size_t total = (size_t)replan_steps * W * B;
    hipLaunchKernelGGL(plant_pack_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 8192)), dim3(256), 0, h->stream,
                       h->cold ? nullptr : h->x_bar, u_src, h->cold ? nullptr : h->K, sc + st.pol, (int)B, (int)n, (int)m, h->N, (int)replan_steps,
                       layout_of(h));
    HIPCHK(hipGetLastError());
  }
  int rc = rows_to_cols(h, h->targets.synced ? h->targets.rows : h->costmat + cost_len(h), h->targets.synced ? n : 0, sc + st.x_nom, n);
  if (rc != MI_ILQR_OK) return rc;
  PlantArgs a{};
  a.policy = sc + st.pol; a.params = sc + st.prm; a.cost = sc + st.cost; a.x_nom = sc + st.x_nom;
  a.ulim = h->limited ? sc + st.ulim : nullptr;
  a.noise = h->plant_noise.synced ? sc + st.noise : nullptr;
  a.x = h->plant_state.rows; a.dead = h->plant_dead; a.mpc_dead = mpc_dead;
  a.log = h->plant_log + (size_t)round * replan_steps * C * B;
  a.dt = h->d.dt; a.seed = h->plant_seed;
  a.clock = (uint32_t)(h->plant_clock + (unsigned long long)round * (unsigned long long)replan_steps);
  a.B = (int32_t)B; a.steps = replan_steps; a.m_user = model->p.m_user > 0 ? model->p.m_user : (int32_t)m;
  a.feedback = h->plant_feedback ? 1 : 0; a.common = h->plant_common ? 1 : 0;
  return model->p.launch(h, kModePlantAdvance, &a);
}

int mi_ilqr_mpc_run(mi_ilqr_t* h, int32_t num_resolves, int32_t replan_steps, const double* target_step, mi_ilqr_stats* stats) {
  if (!h) return MI_ILQR_E_BAD_ARG;
  if (num_resolves < 1 || replan_steps < 1 || replan_steps >= h->N - 1) return MI_ILQR_E_BAD_ARG;
  if (h->targets.synced && target_step) return MI_ILQR_E_BAD_ARG;   // the steps are the field MI_F_TARGET_STEP then
  const bool tracking = h->reference.synced;     // a reference trajectory: the window moves, replan_steps rows per re-solve
  if (tracking && target_step) return MI_ILQR_E_BAD_ARG;
  if (tracking && (double)h->ref_clock + (double)num_resolves * (double)replan_steps >= kRefClockEnd) return MI_ILQR_E_BAD_ARG;
  const bool plant = h->plant_state.synced;      // the closed loop: always the host-loop form, the plant kernel between its launches
  if (plant && h->plant_clock + (unsigned long long)num_resolves * (unsigned long long)replan_steps > 0x100000000ull) return MI_ILQR_E_BAD_ARG;   // (the step counter is 32 bits)
  HIPCHK(hipSetDevice(h->d.device_id));
  int rc;
  if (h->mpc_log_resolves < num_resolves) {
    HIPCHK(hipStreamSynchronize(h->stream));
    h->mpc_log_resolves = 0;
    if ((rc = dev_free(h, h->mpc_log)) != MI_ILQR_OK) return rc;
    if ((rc = dev_alloc(h, h->mpc_log, (size_t)h->B * num_resolves * (h->n + 2) + h->B)) != MI_ILQR_OK) return rc;
    h->mpc_log_resolves = num_resolves;
  }
  // rows a problem never reaches (it failed in an earlier re-solve: both forms of the loop stop logging it there) read as zeros
  double* const mpc_dead = h->mpc_log + (size_t)h->B * h->mpc_log_resolves * (h->n + 2);
  HIPCHK(hipMemsetAsync(h->mpc_log, 0, ((size_t)h->B * h->mpc_log_resolves * (h->n + 2) + h->B) * 8, h->stream));
  h->mpc_resolves = num_resolves; h->mpc_replan = replan_steps;     // (up front: a failing re-solve must not leave the log's shape stale)
  const bool large_on_device = h->large && (size_t)h->m * (h->N - 1) <= 8 * (size_t)kLargeThreads;
  if (plant || (h->large && !large_on_device) || h->batch_minor || (!h->large && (h->N > 512 || h->n > 8))) {
    // lane-per-problem path (and horizons the in-kernel shift does not cover): loop shift + solve on the host
    PlantStage stage{};
    if (plant) {
      if ((rc = plant_prepare(h, num_resolves, replan_steps, &stage)) != MI_ILQR_OK) return rc;
      h->plant_log_rows = 0; h->plant_ms = 0.0;
    }
    std::vector<double> xn(h->n);
    // x_nom from the host mirror: mi_ilqr_set_cost uploads asynchronously on the handle's stream, so a blocking
    // null-stream read of the device copy could still see the previous target
    if (target_step) std::memcpy(xn.data(), shared_x_nom(h), h->n * 8);
    mi_ilqr_stats acc; std::memset(&acc, 0, sizeof(acc)); acc.best_cost = INFINITY; acc.best_index = -1;
    const long long clock0 = h->ref_clock;       // (a run that fails leaves the reference's clock where it was)
    for (int r = 0; r < num_resolves; ++r) {
      if (plant && (rc = plant_advance(h, stage, r, replan_steps, mpc_dead)) != MI_ILQR_OK) return rc;
      if ((rc = mi_ilqr_mpc_shift(h, replan_steps)) != MI_ILQR_OK) { h->ref_clock = clock0; return rc; }
      if (plant) {                               // x0 <- the plant's state (a plant that has ended: the last state it held)
        const size_t cnt = (size_t)h->B * h->n;
        hipLaunchKernelGGL(copy_doubles_kernel, dim3((unsigned)std::min<size_t>((cnt + 255) / 256, 1024)), dim3(256), 0, h->stream,
                           h->plant_state.rows, h->x0, cnt);
        HIPCHK(hipGetLastError());
      }
      if (target_step) {
        for (int i = 0; i < h->n; ++i) xn[i] += target_step[i];
        if ((rc = mi_ilqr_set_cost(h, nullptr, nullptr, nullptr, xn.data())) != MI_ILQR_OK) return rc;
      }
      // (per-problem targets under a reference are kept but ignored: they do not move either)
      if (h->targets.synced && !tracking && (rc = advance_per_problem_targets(h, 1)) != MI_ILQR_OK) return rc;   // one (B, n) upload
      if (tracking) h->ref_clock += replan_steps;
      mi_ilqr_stats st;
      if ((rc = mi_ilqr_solve(h, &st)) != MI_ILQR_OK) { h->ref_clock = clock0; return rc; }
      hipLaunchKernelGGL(mpc_log_fill_kernel, dim3((h->B + 255) / 256), dim3(256), 0, h->stream, h->x0, h->cost, h->iters, h->status, h->mpc_log,
                         mpc_dead, h->B, h->n, num_resolves, r);
      HIPCHK(hipGetLastError());
      if (plant) {                               // (mi_ilqr_solve has synchronized: the plant kernel's events are complete)
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, h->plant_ev0, h->plant_ev1));
        h->plant_ms += (double)ms;
      }
      acc.total_iters += st.total_iters; acc.total_ls_trials += st.total_ls_trials; acc.kernel_ms += st.kernel_ms;
      acc.algorithmic_bytes += st.algorithmic_bytes;
      acc.n_converged = st.n_converged; acc.n_max_iters = st.n_max_iters; acc.n_ls_failed = st.n_ls_failed; acc.n_internal = st.n_internal; acc.n_not_pd = st.n_not_pd;
      if (st.max_iters_seen > acc.max_iters_seen) acc.max_iters_seen = st.max_iters_seen;
      acc.best_cost = st.best_cost; acc.best_index = st.best_index;
    }
    h->mpc_resolves = num_resolves; h->mpc_replan = replan_steps;
    if (plant) {                                 // the clock and the host mirror of the states follow the plants
      HIPCHK(hipMemcpyAsync(h->plant_state.mirror.data(), h->plant_state.rows, (size_t)h->B * h->n * 8, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));
      h->plant_clock += (unsigned long long)num_resolves * (unsigned long long)replan_steps;
      h->plant_log_rows = num_resolves * replan_steps;
    }
    if (stats) *stats = acc;
    return MI_ILQR_OK;
  }
  if ((rc = materialize_zero_state(h)) != MI_ILQR_OK) return rc;
  if ((rc = materialize_u(h)) != MI_ILQR_OK) return rc;
  h->mpc_resolves = num_resolves; h->mpc_replan = replan_steps;
  for (int i = 0; i < kMaxStateDim; ++i) h->mpc_target_step[i] = (target_step && i < h->n) ? target_step[i] : 0.0;
  rc = launch(h, MODE_MPC);
  if (rc != MI_ILQR_OK) return rc;
  if (tracking) h->ref_clock += (long long)num_resolves * replan_steps;   // (what the kernel's window moved by)
  if (!stats_in_kernel(h)) {
    hipLaunchKernelGGL(stats_kernel, dim3(1), dim3(256), 0, h->stream, h->iters_ring, h->status_ring, h->ls_ring, h->cost_ring,
                       h->B, h->d_ring, h->cur_slot, (int)mi_ilqr::kStatsRing);
    HIPCHK(hipGetLastError());
  }
  if (h->targets.synced && !tracking) {   // the rows the kernel moved, every problem's num_resolves times (a failed problem's included)
    HIPCHK(hipStreamSynchronize(h->stream));
    if ((rc = advance_per_problem_targets(h, num_resolves)) != MI_ILQR_OK) return rc;
  }
  if (target_step) {          // keep the handle's x_nom in step with what the kernel accumulated
    std::vector<double> xn(h->n);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(xn.data(), h->costmat + cost_len(h), h->n * 8, hipMemcpyDeviceToHost));
    for (int i = 0; i < h->n; ++i) xn[i] += num_resolves * target_step[i];
    HIPCHK(hipMemcpy(h->costmat + cost_len(h), xn.data(), h->n * 8, hipMemcpyHostToDevice));
    std::memcpy(h->h_costmat.data() + cost_len(h), xn.data(), h->n * 8);   // (the host mirror too)
  }
  if (stats) return mi_ilqr_collect_stats(h, stats);
  return mi_ilqr_synchronize(h);
}

int mi_ilqr_get_mpc_log(mi_ilqr_t* h, double* dst, size_t bytes) {
  if (!h || !dst || !h->mpc_log) return MI_ILQR_E_BAD_ARG;
  if (bytes != (size_t)h->B * h->mpc_resolves * (h->n + 2) * 8) return MI_ILQR_E_BAD_SHAPE;
  HIPCHK(hipSetDevice(h->d.device_id));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(dst, h->mpc_log, bytes, hipMemcpyDeviceToHost));
  return MI_ILQR_OK;
}

// mi_ilqr_get of the plant's selectors that are not plain mirrors (and of the reference trajectory's two: a (B, T, n) mirror whose
// length is its own, and the clock); kNotPlantField for every other selector
constexpr int kNotPlantField = 1;
static int get_plant_field(mi_ilqr* h, int which, double* dst, size_t bytes) {
  const size_t B = h->B;
  switch (which) {
    case MI_F_PLANT_STATE:                     // the mirror: mi_ilqr_mpc_run brings it up to date
      if (bytes != B * h->n * 8) return MI_ILQR_E_BAD_SHAPE;
      if (!h->plant_state.synced) return MI_ILQR_E_BAD_ARG;
      return store_read(h, h->plant_state, nullptr, dst, bytes);
    case MI_F_PLANT_PARAMS:                    // not set: problem b's model row
      if (!h->plant_params.synced && h->params.synced) return store_read(h, h->params, nullptr, dst, bytes);
      return store_read(h, h->plant_params, h->d.model_params, dst, bytes);
    case MI_F_PLANT_STREAM:
      if (bytes != 4 * 8) return MI_ILQR_E_BAD_SHAPE;
      dst[0] = (double)h->plant_seed; dst[1] = (double)h->plant_clock; dst[2] = h->plant_common ? 1.0 : 0.0; dst[3] = h->plant_feedback ? 1.0 : 0.0;
      return MI_ILQR_OK;
    case MI_F_X_REF:                           // the mirror (B, T, n); no reference: nothing to read
      if (!h->reference.synced) return MI_ILQR_E_BAD_ARG;
      if (bytes != h->reference.mirror.size() * 8) return MI_ILQR_E_BAD_SHAPE;
      std::memcpy(dst, h->reference.mirror.data(), bytes);
      return MI_ILQR_OK;
    case MI_F_REF_CLOCK:
      if (bytes != 8) return MI_ILQR_E_BAD_SHAPE;
      *dst = (double)h->ref_clock;
      return MI_ILQR_OK;
    case MI_F_PLANT_KERNEL_MS:
      if (bytes != 8) return MI_ILQR_E_BAD_SHAPE;
      if (h->plant_log_rows == 0) return MI_ILQR_E_BAD_ARG;
      *dst = h->plant_ms;
      return MI_ILQR_OK;
    case MI_F_PLANT_LOG: {                     // (rows, n + m + 1, B) on the device -> (B, rows, n + m + 1): one transpose, one copy
      const size_t cw = (size_t)h->plant_log_rows * (h->n + h->m + 1);
      if (h->plant_log_rows == 0) return MI_ILQR_E_BAD_ARG;
      if (bytes != B * cw * 8) return MI_ILQR_E_BAD_SHAPE;
      if (cw > 0x7fffffffull) return MI_ILQR_E_UNSUPPORTED;
      HIPCHK(hipSetDevice(h->d.device_id));
      int rc = ensure_scratch(h, bytes);
      if (rc != MI_ILQR_OK) return rc;
      if ((rc = transpose_tiles(h, h->plant_log, h->scratch, (int)cw, (int)B, 1, 1, 0, 0, B, 0, 0, cw)) != MI_ILQR_OK) return rc;
      HIPCHK(hipStreamSynchronize(h->stream));
      HIPCHK(hipMemcpy(dst, h->scratch, bytes, hipMemcpyDeviceToHost));
      return MI_ILQR_OK;
    }
  }
  return kNotPlantField;
}

int mi_ilqr_get(mi_ilqr_t* h, int which, double* dst, size_t bytes) {
  if (!h || !dst) return MI_ILQR_E_BAD_ARG;
  if (const int rc = get_plant_field(h, which, dst, bytes); rc != kNotPlantField) return rc;
  if (const RowField r = row_field(h, which); r.store) return store_read(h, *r.store, r.shared_row, dst, bytes);   // (host mirrors)
  if (which == MI_F_POLICY_STREAM) {
    if (bytes != 3 * 8) return MI_ILQR_E_BAD_SHAPE;
    dst[0] = (double)h->policy_seed; dst[1] = (double)h->policy_first_sample; dst[2] = h->policy_common ? 1.0 : 0.0;
    return MI_ILQR_OK;
  }
  if (which == MI_F_POLICY_MC_STATS || which == MI_F_POLICY_MC_SAMPLES) {      // the last run's results, host copies
    const std::vector<double>& r = which == MI_F_POLICY_MC_STATS ? h->mc_stats : h->mc_samples;
    if (r.empty()) return MI_ILQR_E_BAD_ARG;
    if (bytes != r.size() * 8) return MI_ILQR_E_BAD_SHAPE;
    std::memcpy(dst, r.data(), bytes);
    return MI_ILQR_OK;
  }
  if (which == MI_F_POLICY_MC_OBSERVE) {
    if (bytes != 8) return MI_ILQR_E_BAD_SHAPE;
    *dst = (double)h->mc_observe;
    return MI_ILQR_OK;
  }
  if (which == MI_F_POLICY_MC_ENVELOPE || which == MI_F_POLICY_MC_ENVELOPE_U || which == MI_F_POLICY_MC_SAFETY) {   // host copies too
    const std::vector<double>& r = which == MI_F_POLICY_MC_ENVELOPE ? h->mc_env_x : (which == MI_F_POLICY_MC_ENVELOPE_U ? h->mc_env_u : h->mc_safety);
    if (h->mc_stats.empty() || r.empty()) return MI_ILQR_E_BAD_ARG;      // (the last run did not produce them)
    if (bytes != r.size() * 8) return MI_ILQR_E_BAD_SHAPE;
    std::memcpy(dst, r.data(), bytes);
    return MI_ILQR_OK;
  }
  if (which == MI_F_POLICY_KERNEL_MS) {        // the rollout kernel of the last mi_ilqr_policy_rollout, from its own events
    if (bytes != 8) return MI_ILQR_E_BAD_SHAPE;
    if (h->policy_last_mc) { *dst = h->mc_ms; return MI_ILQR_OK; }      // (an on-device Monte-Carlo run: its rollout kernels, summed over the passes)
    if (!h->policy_ran) return MI_ILQR_E_BAD_ARG;
    float ms = 0.0f;
    HIPCHK(hipSetDevice(h->d.device_id));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipEventElapsedTime(&ms, h->policy_ev0, h->policy_ev1));
    *dst = (double)ms;
    return MI_ILQR_OK;
  }
  Field f = field_of(h, which);
  if (!f.ptr || f.is_int) return MI_ILQR_E_BAD_ARG;
  if (bytes != f.bytes && !prefix_ok(which, bytes, f.bytes)) return MI_ILQR_E_BAD_SHAPE;
  HIPCHK(hipSetDevice(h->d.device_id));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (h->cold && is_state_field(which)) { std::memset(dst, 0, bytes); return MI_ILQR_OK; }
  if (which == MI_F_U_BAR && h->u_zero && !h->u_pending) { std::memset(dst, 0, bytes); return MI_ILQR_OK; }
  const double* src = (h->u_pending && which == MI_F_U_BAR) ? h->u_guess : static_cast<const double*>(f.ptr);
  int rows = 0, len = 0;
  if (needs_relayout(h, which, &rows, &len)) {
    int rc = ensure_scratch(h, bytes);
    if (rc != MI_ILQR_OK) return rc;
    if ((rc = relayout(h, src, h->scratch, rows, len, false)) != MI_ILQR_OK) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(dst, h->scratch, bytes, hipMemcpyDeviceToHost));
    return MI_ILQR_OK;
  }
  HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDefault));            // (tiny batches keep some fields in mapped host memory: host.hpp)
  return MI_ILQR_OK;
}

int mi_ilqr_get_async(mi_ilqr_t* h, int which, void* dst, size_t bytes) {
  if (!h || !dst) return MI_ILQR_E_BAD_ARG;
  if (const int rc = get_plant_field(h, which, static_cast<double*>(dst), bytes); rc != kNotPlantField) return rc;   // (done when the call returns)
  if (const RowField r = row_field(h, which); r.store) {       // (host mirrors: the copy is done when the call returns)
    if (which == MI_F_X_NOM || which == MI_F_TARGET_STEP) {
      HIPCHK(hipSetDevice(h->d.device_id));
      HIPCHK(hipStreamSynchronize(h->stream));
    }
    return store_read(h, *r.store, r.shared_row, static_cast<double*>(dst), bytes);
  }
  Field f = field_of(h, which);
  if (!f.ptr) return MI_ILQR_E_BAD_ARG;
  if (bytes != f.bytes && !prefix_ok(which, bytes, f.bytes)) return MI_ILQR_E_BAD_SHAPE;
  HIPCHK(hipSetDevice(h->d.device_id));
  if (!f.is_int) {
    int rows = 0, len = 0;
    // fields that need a layout conversion (or are known-zero) take the blocking path
    if (needs_relayout(h, which, &rows, &len) || (h->cold && is_state_field(which)) ||
        (which == MI_F_U_BAR && h->u_zero && !h->u_pending))
      return mi_ilqr_get(h, which, static_cast<double*>(dst), bytes);
  }
  const void* src = (!f.is_int && h->u_pending && which == MI_F_U_BAR) ? h->u_guess : f.ptr;
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, h->stream));
  return MI_ILQR_OK;
}

int mi_ilqr_get_int(mi_ilqr_t* h, int which, int32_t* dst, size_t bytes) {
  if (!h || !dst) return MI_ILQR_E_BAD_ARG;
  if (which == MI_I64_CLUSTER_WORDS && (!h->cluster_sync || !h->last_clustered)) {
    // the header's promise: zeros when the last solve / MPC launch was not clustered (the device words would be an older launch's),
    // and for handles of the other kernel families, which have no such words
    if (bytes != (size_t)h->B * MI_ILQR_CLUSTER_WORDS * 8) return MI_ILQR_E_BAD_SHAPE;
    HIPCHK(hipSetDevice(h->d.device_id));
    HIPCHK(hipStreamSynchronize(h->stream));
    std::memset(dst, 0, bytes);
    return MI_ILQR_OK;
  }
  if (which == MI_I_POLICY_MC_PASSES) {          // the passes of the last on-device Monte-Carlo run (a host value)
    if (h->mc_stats.empty()) return MI_ILQR_E_BAD_ARG;
    if (bytes != 4) return MI_ILQR_E_BAD_SHAPE;
    *dst = h->mc_passes;
    return MI_ILQR_OK;
  }
  Field f = field_of(h, which);
  if (!f.ptr || !f.is_int) return MI_ILQR_E_BAD_ARG;
  if (bytes != f.bytes) return MI_ILQR_E_BAD_SHAPE;
  HIPCHK(hipSetDevice(h->d.device_id));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(dst, f.ptr, bytes, hipMemcpyDefault));
  return MI_ILQR_OK;
}

int mi_ilqr_set(mi_ilqr_t* h, int which, const double* src, size_t bytes) {
  if (h && which == MI_F_MODEL_PARAMS) return set_model_params(h, src, bytes);   // (src == NULL, bytes == 0: back to shared mode)
  if (h && which == MI_F_COST_MATRICES) return set_cost_rows(h, src, bytes);     // (the same)
  if (h && which == MI_F_POLICY_NOISE) return set_noise_rows(h, h->policy_noise, src, bytes);   // (src == NULL, bytes == 0: no noise)
  if (h && which == MI_F_POLICY_STREAM) return set_policy_stream(h, src, bytes);
  if (h && which == MI_F_POLICY_MC_DIST) return set_mc_dist(h, src, bytes);      // (src == NULL, bytes == 0: no sampler rows)
  if (h && which == MI_F_POLICY_MC_RUN) return run_policy_mc(h, src, bytes);     // (a command: runs the evaluation)
  if (h && which == MI_F_POLICY_MC_BOX) return set_mc_box(h, src, bytes);        // (src == NULL, bytes == 0: no box)
  if (h && which == MI_F_POLICY_MC_OBSERVE) return set_mc_observe(h, src, bytes);
  if (which == MI_F_POLICY_MC_ENVELOPE || which == MI_F_POLICY_MC_ENVELOPE_U || which == MI_F_POLICY_MC_SAFETY) return MI_ILQR_E_BAD_ARG;   // (read-only)
  if (h && which == MI_F_PLANT_STATE) return set_plant_state(h, src, bytes);     // (src == NULL, bytes == 0: no plant)
  if (h && which == MI_F_PLANT_PARAMS) return set_plant_params(h, src, bytes);   // (the same: the problems' model rows)
  if (h && which == MI_F_PLANT_NOISE) return set_noise_rows(h, h->plant_noise, src, bytes);
  if (h && which == MI_F_PLANT_STREAM) return set_plant_stream(h, src, bytes);
  if (h && which == MI_F_X_REF) return set_reference(h, src, bytes);             // (src == NULL, bytes == 0: no reference)
  if (h && which == MI_F_REF_CLOCK) return set_ref_clock(h, src, bytes);
  if (!h || !src) return MI_ILQR_E_BAD_ARG;
  if (which == MI_F_X_NOM || which == MI_F_TARGET_STEP) return set_target_field(h, which, src, bytes);
  Field f = field_of(h, which);
  if (!f.ptr || f.is_int) return MI_ILQR_E_BAD_ARG;
  if (bytes != f.bytes) return MI_ILQR_E_BAD_SHAPE;
  HIPCHK(hipSetDevice(h->d.device_id));
  if (is_state_field(which)) { int rc = materialize_zero_state(h); if (rc != MI_ILQR_OK) return rc; }
  HIPCHK(hipStreamSynchronize(h->stream));
  int rows = 0, len = 0;
  if (needs_relayout(h, which, &rows, &len)) {
    int rc = ensure_scratch(h, bytes);
    if (rc != MI_ILQR_OK) return rc;
    HIPCHK(hipMemcpy(h->scratch, src, bytes, hipMemcpyHostToDevice));
    if ((rc = relayout(h, h->scratch, static_cast<double*>(f.ptr), rows, len, true)) != MI_ILQR_OK) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
  } else {
    HIPCHK(hipMemcpy(f.ptr, src, bytes, hipMemcpyDefault));
  }
  if (which == MI_F_U_BAR) { h->u_pending = false; h->u_zero = false; }
  return MI_ILQR_OK;
}

int mi_ilqr_device_ptr(mi_ilqr_t* h, int which, void** ptr, size_t* bytes) {
  if (!h || !ptr) return MI_ILQR_E_BAD_ARG;
  if (const RowStore* s = row_field(h, which).store) {         // per-problem mode only: the (B, width) device rows
    if (!s->synced) return MI_ILQR_E_BAD_ARG;
    *ptr = s->rows;
    if (bytes) *bytes = s->mirror.size() * 8;
    return MI_ILQR_OK;
  }
  Field f = field_of(h, which);
  if (!f.ptr) return MI_ILQR_E_BAD_ARG;
  *ptr = f.ptr;
  if (bytes) *bytes = f.bytes;
  return MI_ILQR_OK;
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
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipEventElapsedTime(ms, h->ev0, h->ev1));
  return MI_ILQR_OK;
}

int mi_ilqr_get_cycles(mi_ilqr_t* h, int64_t* dst, size_t bytes) {
  if (!h || !dst) return MI_ILQR_E_BAD_ARG;
  if (bytes != (size_t)h->B * 4 * 8) return MI_ILQR_E_BAD_SHAPE;
  HIPCHK(hipSetDevice(h->d.device_id));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(dst, h->prof, bytes, hipMemcpyDefault));
  return MI_ILQR_OK;
}

int mi_ilqr_get_stream(mi_ilqr_t* h, void** hip_stream) {
  if (!h || !hip_stream) return MI_ILQR_E_BAD_ARG;
  *hip_stream = reinterpret_cast<void*>(h->stream);
  return MI_ILQR_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------
// The path's one collective: all-reduce(min) of the best costs over the ranks, RCCL over xGMI.
// librccl is bound at run time (dlopen), so libmi_ilqr.so has no link-time dependency on it; a
// process that already holds an RCCL (e.g. PyTorch's) shares that instance.
// ---------------------------------------------------------------------------------------------------
namespace {
struct RcclApi {
  // the few entry points used, with the types of rccl.h (ncclResult_t = int, ncclComm_t = opaque pointer,
  // ncclUniqueId = 128 bytes by value, ncclDataType_t / ncclRedOp_t = int enums whose values are taken from <rccl/rccl.h>)
  struct UniqueId { char internal[MI_ILQR_COMM_ID_BYTES]; };
  int (*GetUniqueId)(UniqueId*) = nullptr;
  int (*CommInitRank)(void**, int, UniqueId, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*CommCount)(void*, int*) = nullptr;
  int (*CommUserRank)(void*, int*) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  bool ok = false;
};
// the data type and reduction codes come from the header the library is compiled against - never from memory (round 2
// shipped ncclAvg = 4 under the name "min")
constexpr int kNcclFloat64 = (int)ncclFloat64, kNcclMin = (int)ncclMin;
static_assert(sizeof(ncclUniqueId) == MI_ILQR_COMM_ID_BYTES, "the communicator id crosses the C ABI as MI_ILQR_COMM_ID_BYTES bytes");
static_assert((int)ncclSuccess == 0, "RCCLCHK treats 0 as success");

const RcclApi& rccl() {
  static const RcclApi api = [] {
    RcclApi a;
    void* lib = nullptr;
    for (const char* name : {"librccl.so.1", "librccl.so"})            // an instance already in the process first
      if (!lib) lib = dlopen(name, RTLD_NOW | RTLD_NOLOAD);
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
      if (!lib) lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
    if (!lib) return a;
    a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(dlsym(lib, "ncclGetUniqueId"));
    a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(dlsym(lib, "ncclCommInitRank"));
    a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
    a.AllReduce = reinterpret_cast<decltype(a.AllReduce)>(dlsym(lib, "ncclAllReduce"));
    a.CommCount = reinterpret_cast<decltype(a.CommCount)>(dlsym(lib, "ncclCommCount"));
    a.CommUserRank = reinterpret_cast<decltype(a.CommUserRank)>(dlsym(lib, "ncclCommUserRank"));
    a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
    a.ok = a.GetUniqueId && a.CommInitRank && a.CommDestroy && a.AllReduce;
    return a;
  }();
  return api;
}
#define RCCLCHK(expr)                                                                               \
  do {                                                                                              \
    const int r_ = (expr);                                                                          \
    if (r_ != 0) {                                                                                  \
      std::fprintf(stderr, "mi_ilqr: %s failed: %s (%s:%d)\n", #expr,                               \
                   rccl().GetErrorString ? rccl().GetErrorString(r_) : "?", __FILE__, __LINE__);    \
      return MI_ILQR_E_RCCL;                                                                        \
    }                                                                                               \
  } while (0)
}  // namespace

struct mi_ilqr_comm {
  void* comm = nullptr;
  int rank = 0, world = 1, device = 0;
  hipStream_t stream = nullptr;     // the collective's own stream: it overlaps the solves of the handles
  hipEvent_t done = nullptr;
  double* d_buf = nullptr;          // MI_ILQR_COMM_MAX_COUNT doubles on the device
  double* h_buf = nullptr;          // pinned staging
  int in_flight = 0;                // count of the reduction started and not yet waited for
};

extern "C" {

int mi_ilqr_comm_unique_id(void* id_bytes) {
  if (!id_bytes) return MI_ILQR_E_BAD_ARG;
  if (!rccl().ok) return MI_ILQR_E_RCCL;
  RcclApi::UniqueId id;
  RCCLCHK(rccl().GetUniqueId(&id));
  std::memcpy(id_bytes, id.internal, MI_ILQR_COMM_ID_BYTES);
  return MI_ILQR_OK;
}

int mi_ilqr_comm_create(const void* id_bytes, int32_t rank, int32_t world, int32_t device_id, mi_ilqr_comm_t** out) {
  if (!id_bytes || !out || world < 1 || rank < 0 || rank >= world) return MI_ILQR_E_BAD_ARG;
  *out = nullptr;
  if (!rccl().ok) return MI_ILQR_E_RCCL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) return MI_ILQR_E_NO_DEVICE;
  HIPCHK(hipSetDevice(device_id));
  mi_ilqr_comm* c = new (std::nothrow) mi_ilqr_comm();
  if (!c) return MI_ILQR_E_BAD_ARG;
  c->rank = rank; c->world = world; c->device = device_id;
  RcclApi::UniqueId id;
  std::memcpy(id.internal, id_bytes, MI_ILQR_COMM_ID_BYTES);
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&c->done) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&c->d_buf), MI_ILQR_COMM_MAX_COUNT * 8) != hipSuccess ||
      hipHostMalloc(reinterpret_cast<void**>(&c->h_buf), MI_ILQR_COMM_MAX_COUNT * 8, hipHostMallocDefault) != hipSuccess) {
    mi_ilqr_comm_destroy(c);
    return MI_ILQR_E_HIP;
  }
  const int r = rccl().CommInitRank(&c->comm, world, id, rank);
  if (r != 0) {
    std::fprintf(stderr, "mi_ilqr: ncclCommInitRank failed: %s\n", rccl().GetErrorString ? rccl().GetErrorString(r) : "?");
    c->comm = nullptr;
    mi_ilqr_comm_destroy(c);
    return MI_ILQR_E_RCCL;
  }
  *out = c;
  return MI_ILQR_OK;
}

void mi_ilqr_comm_destroy(mi_ilqr_comm_t* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->comm && rccl().ok) (void)rccl().CommDestroy(c->comm);
  if (c->d_buf) (void)hipFree(c->d_buf);
  if (c->h_buf) (void)hipHostFree(c->h_buf);
  if (c->done) (void)hipEventDestroy(c->done);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int mi_ilqr_comm_count(mi_ilqr_comm_t* c, int32_t* ranks, int32_t* rank) {
  // what the COMMUNICATOR says (ncclCommCount / ncclCommUserRank), not what the caller passed to mi_ilqr_comm_create
  if (!c || !c->comm || !ranks) return MI_ILQR_E_BAD_ARG;
  if (!rccl().CommCount) return MI_ILQR_E_RCCL;
  int n = 0, r = -1;
  RCCLCHK(rccl().CommCount(c->comm, &n));
  if (rank && rccl().CommUserRank) RCCLCHK(rccl().CommUserRank(c->comm, &r));
  *ranks = n;
  if (rank) *rank = r;
  return MI_ILQR_OK;
}

int mi_ilqr_allreduce_min_start(mi_ilqr_comm_t* c, const double* values, int32_t count) {
  if (!c || !values || count < 1 || count > MI_ILQR_COMM_MAX_COUNT || c->in_flight) return MI_ILQR_E_BAD_ARG;
  HIPCHK(hipSetDevice(c->device));
  std::memcpy(c->h_buf, values, (size_t)count * 8);
  HIPCHK(hipMemcpyAsync(c->d_buf, c->h_buf, (size_t)count * 8, hipMemcpyHostToDevice, c->stream));
  RCCLCHK(rccl().AllReduce(c->d_buf, c->d_buf, (size_t)count, kNcclFloat64, kNcclMin, c->comm, c->stream));
  HIPCHK(hipMemcpyAsync(c->h_buf, c->d_buf, (size_t)count * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipEventRecord(c->done, c->stream));
  c->in_flight = count;
  return MI_ILQR_OK;
}

int mi_ilqr_allreduce_min_wait(mi_ilqr_comm_t* c, double* values, int32_t count) {
  if (!c || !values || count != c->in_flight || count < 1) return MI_ILQR_E_BAD_ARG;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipEventSynchronize(c->done));
  std::memcpy(values, c->h_buf, (size_t)count * 8);
  c->in_flight = 0;
  return MI_ILQR_OK;
}

int mi_ilqr_allreduce_min(mi_ilqr_comm_t* c, double* values, int32_t count) {
  const int rc = mi_ilqr_allreduce_min_start(c, values, count);
  if (rc != MI_ILQR_OK) return rc;
  return mi_ilqr_allreduce_min_wait(c, values, count);
}

}  // extern "C"
