// libmi_ilqr.so, host side - the policy: "the policy as the handle holds it now" staged once (pack_policy, fill_policy_args) for the
// calls that roll it out - mi_ilqr_policy_rollout, the on-device Monte-Carlo (MI_F_POLICY_MC_*: its setters and run_policy_mc) and,
// through pack_policy, the plant of the closed MPC loop (h_mpc.hip).  Nothing here writes the handle's solver state.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "host_internal.hpp"

using namespace mi;
using namespace mi_host;

namespace {     // the kernel: global, like every kernel of the host units - a name does not change with the unit

// The policy's rows t = x_bar_t | u_bar_t | K_t (m x n, row-major), W = n + m + m n doubles, for the first `steps` steps, gathered
// from the handle's kernel layout (LAYOUT_TL / TM / BM).  A source that is nullptr reads as zeros: the state of a cold handle, the
// controls of a reset one.  order PACK_TIME_MAJOR: (B, steps, W), what the rollout kernels read (policy_rollout.hpp);
// PACK_PROBLEM_MINOR: (steps, W, B), element e of problem b at e * B + b, what the plant reads (plant_advance.hpp: a lane is a
// problem) - the writes are coalesced either way.
__global__ void __launch_bounds__(256) policy_pack_kernel(const double* __restrict__ x_bar, const double* __restrict__ u_bar,
                                                            const double* __restrict__ K, double* __restrict__ dst,
                                                            int B, int n, int m, int N, int steps, int layout, int order,
                                                            const double* __restrict__ sel, int group, int cols) {
  // `cols` columns are written (B without groups).  Grouped (sel != nullptr: the (G, 3) selection rows on the device): column g is
  // the policy of problem g `group` + w_g, the group's winner - member 0 where the group has none
  const int W = n + m + m * n, M1 = N - 1;
  const size_t total = (size_t)cols * steps * W;
  auto at = [&](const double* f, int rows, int len, int b, int r, int t) -> double {
    if (!f) return 0.0;
    if (layout == LAYOUT_TL) return f[((size_t)b * rows + r) * len + t];
    if (layout == LAYOUT_TM) return f[((size_t)b * len + t) * rows + r];
    return f[((size_t)t * rows + r) * B + b];
  };
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    int b, w, t;
    if (order == PACK_PROBLEM_MINOR) { b = (int)(e % cols); const size_t tw = e / cols; w = (int)(tw % W); t = (int)(tw / W); }
    else { w = (int)(e % W); const size_t bt = e / W; t = (int)(bt % steps); b = (int)(bt / steps); }
    if (sel) { const double wg = sel[(size_t)b * 3]; b = b * group + (wg > 0.0 ? (int)wg : 0); }
    dst[e] = w < n ? at(x_bar, n, N, b, w, t) : (w < n + m ? at(u_bar, m, M1, b, w - n, t) : at(K, m * n, M1, b, w - n - m, t));
  }
}

}  // namespace

namespace mi_host {

// The controls of the policy as the handle holds it now: a pending initial guess is the u_bar the next launch would start from, a
// reset handle's u_bar reads as zeros (nullptr).
const double* policy_u_source(const mi_ilqr* h) { return h->u_pending ? h->u_guess : (h->u_zero ? nullptr : h->u_bar); }

namespace {

// What the two policy calls refuse alike.  `draws`: the samples the call takes from the handle's stream (a noise-free rollout: none).
int policy_call_refused(const mi_ilqr* h, unsigned long long draws) {
  if (h->reference.synced) return MI_ILQR_E_UNSUPPORTED;      // (the policy kernels cost a rollout against a constant target only)
  if ((unsigned long long)h->policy_first_sample + draws > 0x100000000ull) return MI_ILQR_E_BAD_ARG;   // (the sample counter is 32 bits)
  return MI_ILQR_OK;
}

}  // namespace

// The rollout kernels' arguments that come from the handle: the packed policy, every per-problem array - its device rows with a
// row's stride, else the one shared row with stride 0 (the descriptor's parameter row is staged into prow_scratch for that) - the
// bounds, the noise rows and their stream, dt, N, B, m_user.  The caller adds its inputs and outputs.
int fill_policy_args(mi_ilqr* h, const Model* model, const double* policy, double* prow_scratch, PolicyArgs& a) {
  const size_t np = model->p.n_params;
  if (np && !h->params.synced) {
    const int rc = stage_h2d(h, prow_scratch, h->d.model_params, np * 8);
    if (rc != MI_ILQR_OK) return rc;
  }
  auto rows_or = [](const RowStore& s, const double* shared_row, size_t* stride) {
    *stride = s.synced ? s.width : 0;
    return s.synced ? s.rows : shared_row;
  };
  a.policy = policy;
  a.param_rows = rows_or(h->params, prow_scratch, &a.param_stride);
  a.cost = rows_or(h->costs, h->costmat, &a.cost_stride);
  a.x_nom = rows_or(h->targets, h->costmat + cost_len(h), &a.x_nom_stride);
  a.ulim = h->limited ? h->ulim : nullptr;
  a.noise = h->policy_noise.synced ? h->policy_noise.rows : nullptr;
  a.seed = h->policy_seed; a.first_sample = h->policy_first_sample; a.common = h->policy_common ? 1 : 0;
  a.dt = h->d.dt; a.N = (int32_t)h->N; a.B = (int32_t)h->B; a.m_user = device_m_user(model, h);
  return MI_ILQR_OK;
}

namespace {

// MI_F_POLICY_MC_RUN, stage by stage: what the request asks for, the window plan, the scratch offsets (in doubles) and the host
// buffers the stream copies into.
struct McRun {
  unsigned long long S = 0, G = 0;
  McWindow w{};
  int32_t x0_dist = 0, p_dist = 0;
  bool sample_params = false, want_samples = false, want_box = false, env_x = false, env_u = false, keep_x = false, observing = false;
  size_t B = 0, n = 0, N = 0, np = 0, SW = 0, Rx = 0, Ru = 0;
  size_t o_pol = 0, o_prow = 0, o_part = 0, o_smp = 0, o_smp_out = 0, o_X = 0, o_U = 0, scratch_bytes = 0;
  std::vector<double> samples, env_x_out, env_u_out, safety_out, acc;
  std::vector<unsigned long long> box_out;
  double ms_sum = 0.0;
};

// v = S | x0_dist | p_dist | sample_params | samples
int mc_validate(const mi_ilqr* h, const double* v, size_t bytes, McRun& r) {
  if (bytes != 5 * 8) return MI_ILQR_E_BAD_SHAPE;
  if (!v) return MI_ILQR_E_BAD_ARG;
  if (!(v[0] >= 1.0 && v[0] <= 0x1p32 && v[0] == std::floor(v[0]))) return MI_ILQR_E_BAD_ARG;
  for (int i = 1; i < 5; ++i) if (!(v[i] == 0.0 || v[i] == 1.0)) return MI_ILQR_E_BAD_ARG;
  r.S = (unsigned long long)v[0];
  if (const int rc = policy_call_refused(h, r.S); rc != MI_ILQR_OK) return rc;
  if (!h->policy_mc_dist.synced) return MI_ILQR_E_BAD_ARG;
  r.np = model_of(h->d.model_id)->p.n_params;
  r.x0_dist = (int32_t)v[1]; r.p_dist = (int32_t)v[2]; r.sample_params = v[3] == 1.0; r.want_samples = v[4] == 1.0;
  if (r.sample_params && r.np == 0) return MI_ILQR_E_UNSUPPORTED;
  return MI_ILQR_OK;
}

// the window: as many groups of 64 samples per pass as the caps allow (mc_window.hpp), and where its arrays lie in the scratch
void mc_plan(const mi_ilqr* h, McRun& r) {
  const size_t B = r.B = h->B, n = r.n = h->n, m = h->m, N = r.N = h->N, W = n + m + m * n, SW = r.SW = n + r.np + 2;
  r.G = (r.S + 63) / 64;
  // what the run observes beside the cost (policy_env.hpp): the window's trajectories stay in the scratch, under a cap of their own
  r.want_box = h->mc_box.synced; r.env_x = (h->mc_observe & 1) != 0; r.env_u = (h->mc_observe & 2) != 0;
  r.keep_x = r.want_box || r.env_x; r.observing = r.keep_x || r.env_u;
  r.Rx = N * n; r.Ru = (N - 1) * m;
  const size_t group_bytes = (size_t)kMcFields * B * 8 + (r.want_samples ? 2 * B * 64 * SW * 8 : 0);
  const size_t traj_group_bytes = B * 64 * 8 * ((r.keep_x ? r.Rx : 0) + (r.env_u ? r.Ru : 0));
  r.w = mc_window(r.G, B, group_bytes, traj_group_bytes, switches().mc_pass_groups);
  ScratchPlan plan;
  const size_t win_max = (size_t)r.w.k * 64;
  r.o_pol = plan.take(B * (N - 1) * W); r.o_prow = plan.take(r.np ? r.np : 1); r.o_part = plan.take((size_t)r.w.k * kMcFields * B);
  r.o_smp = plan.take(r.want_samples ? B * SW * win_max : 0); r.o_smp_out = plan.take(r.want_samples ? B * win_max * SW : 0);
  r.o_X = plan.take(r.keep_x ? B * r.Rx * win_max : 0); r.o_U = plan.take(r.env_u ? B * r.Ru * win_max : 0);
  r.scratch_bytes = plan.bytes();
}

// the host buffers of the results, the scratch, the device accumulators and the events; a window or a result that does not fit is
// an answer (MI_ILQR_E_UNSUPPORTED), and the last results stay
int mc_allocate(mi_ilqr* h, McRun& r) {
  const size_t B = r.B, N = r.N;
  if (r.want_samples) {
    if (r.S > (unsigned long long)(SIZE_MAX / 8) / (B * r.SW)) return MI_ILQR_E_UNSUPPORTED;
    try { r.samples.resize(B * (size_t)r.S * r.SW); } catch (const std::bad_alloc&) { return MI_ILQR_E_UNSUPPORTED; }
  }
  int rc = ensure_scratch(h, r.scratch_bytes);
  if (rc != MI_ILQR_OK && r.observing) { (void)hipGetLastError(); return MI_ILQR_E_UNSUPPORTED; }   // (the windows did not fit)
  if (rc != MI_ILQR_OK) return rc;
  if (!h->mc_acc && (rc = dev_alloc(h, h->mc_acc, (size_t)kMcFields * B)) != MI_ILQR_OK) return rc;
  if (r.observing) {
    if (r.env_x && !h->env_acc_x) rc = dev_alloc(h, h->env_acc_x, B * r.Rx * 8);
    if (rc == MI_ILQR_OK && r.env_u && !h->env_acc_u) rc = dev_alloc(h, h->env_acc_u, B * r.Ru * 8);
    if (rc == MI_ILQR_OK && r.want_box && !h->box_counters) rc = dev_alloc(h, h->box_counters, B * (3 + N));
    if (rc != MI_ILQR_OK) { (void)hipGetLastError(); return MI_ILQR_E_UNSUPPORTED; }
    if (r.want_box) HIPCHK(hipMemsetAsync(h->box_counters, 0, B * (3 + N) * 8, h->stream));
    try {
      if (r.env_x) r.env_x_out.resize(B * r.Rx * 8);
      if (r.env_u) r.env_u_out.resize(B * r.Ru * 8);
      if (r.want_box) { r.box_out.resize(B * (3 + N)); r.safety_out.resize(B * (3 + N)); }
    } catch (const std::bad_alloc&) { return MI_ILQR_E_UNSUPPORTED; }
  }
  // one start / stop pair per pass, at most kMcEventPairs of them: a run of more passes waits for the stream every kMcEventPairs
  // passes, adds their times up and uses the pairs again
  const size_t pairs = (size_t)std::min<unsigned long long>(r.w.passes, kMcEventPairs);
  while (h->mc_events.size() < 2 * pairs) {
    hipEvent_t e = nullptr;
    HIPCHK(hipEventCreate(&e));
    h->mc_events.push_back(e);
  }
  r.acc.resize((size_t)kMcFields * B);
  return MI_ILQR_OK;
}

// the stream is idle: add the kernels of the event pairs in use
int mc_add_times(mi_ilqr* h, McRun& r, unsigned long long used) {
  for (unsigned long long q = 0; q < used; ++q) {
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, h->mc_events[2 * q], h->mc_events[2 * q + 1]));
    r.ms_sum += (double)ms;
  }
  return MI_ILQR_OK;
}

// Draws, rolls out and reduces the samples on the handle's stream - passes over windows of sample groups, each one rollout kernel and
// one fold (policy_mc.hpp) - copies the results into the run's host buffers and synchronizes once.
int mc_passes(mi_ilqr* h, McRun& r) {
  const Model* model = model_of(h->d.model_id);
  const size_t B = r.B, n = r.n, N = r.N, SW = r.SW;
  const unsigned long long S = r.S, G = r.G, k = r.w.k;
  double* const sc = h->scratch;
  int rc = pack_policy(h, sc + r.o_pol, (int)N - 1, PACK_TIME_MAJOR);
  if (rc != MI_ILQR_OK) return rc;
  PolicyMcArgs a{};
  if ((rc = fill_policy_args(h, model, sc + r.o_pol, sc + r.o_prow, a.r)) != MI_ILQR_OK) return rc;
  a.dist = h->policy_mc_dist.rows; a.partials = sc + r.o_part; a.acc = h->mc_acc; a.samples = r.want_samples ? sc + r.o_smp : nullptr;
  a.S = S; a.x0_dist = r.x0_dist; a.p_dist = r.p_dist; a.sample_params = r.sample_params ? 1 : 0;
  if (r.keep_x) a.r.X = sc + r.o_X;
  if (r.env_u) a.r.U = sc + r.o_U;
  unsigned long long pass = 0;
  for (unsigned long long g0 = 0; g0 < G; g0 += k, ++pass) {
    const unsigned long long kg = std::min(k, G - g0), s0 = g0 * 64, slot = pass % kMcEventPairs;
    if (pass > 0 && slot == 0) {
      HIPCHK(hipStreamSynchronize(h->stream));
      if ((rc = mc_add_times(h, r, kMcEventPairs)) != MI_ILQR_OK) return rc;
    }
    const size_t win = (size_t)std::min<unsigned long long>(S - s0, kg * 64);
    a.group0 = (uint32_t)g0; a.groups = (int32_t)kg; a.win_samples = win; a.first_pass = pass == 0 ? 1 : 0;
    a.ev0 = h->mc_events[2 * slot]; a.ev1 = h->mc_events[2 * slot + 1];
    if ((rc = model->p.launch(h, kModePolicyMC, &a)) != MI_ILQR_OK) return rc;
    if (r.observing) {        // the window's trajectories, reduced before the next pass overwrites them
      const double g_first = (double)h->policy_first_sample + (double)s0;
      if (r.env_x) rc = launch_policy_env(h, sc + r.o_X, h->env_acc_x, B, r.Rx, win, g_first, a.first_pass);
      if (rc == MI_ILQR_OK && r.env_u) rc = launch_policy_env(h, sc + r.o_U, h->env_acc_u, B, r.Ru, win, g_first, a.first_pass);
      if (rc == MI_ILQR_OK && r.want_box)
        rc = launch_policy_box(h, sc + r.o_X, h->mc_box.rows, a.r.x_nom, a.r.x_nom_stride, a.dist + 2 * n, h->policy_mc_dist.width,
                               h->box_counters, B, (int)n, (int)N, win);
      if (rc != MI_ILQR_OK) return rc;
    }
    if (r.want_samples) {     // sample-minor (B, SW, win) -> (B, win, SW), then rows s0 .. s0 + win - 1 of every problem's block
      if ((rc = transpose_tiles(h, sc + r.o_smp, sc + r.o_smp_out, (int)SW, (int)win, B, 1, SW * win, 0, win, win * SW, 0, SW)) != MI_ILQR_OK)
        return rc;
      HIPCHK(hipMemcpy2DAsync(r.samples.data() + (size_t)s0 * SW, (size_t)S * SW * 8, sc + r.o_smp_out, win * SW * 8, win * SW * 8, B,
                              hipMemcpyDeviceToHost, h->stream));
    }
  }
  HIPCHK(hipMemcpyAsync(r.acc.data(), h->mc_acc, r.acc.size() * 8, hipMemcpyDeviceToHost, h->stream));
  if (r.env_x) HIPCHK(hipMemcpyAsync(r.env_x_out.data(), h->env_acc_x, r.env_x_out.size() * 8, hipMemcpyDeviceToHost, h->stream));
  if (r.env_u) HIPCHK(hipMemcpyAsync(r.env_u_out.data(), h->env_acc_u, r.env_u_out.size() * 8, hipMemcpyDeviceToHost, h->stream));
  if (r.want_box) HIPCHK(hipMemcpyAsync(r.box_out.data(), h->box_counters, r.box_out.size() * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return mc_add_times(h, r, (r.w.passes - 1) % kMcEventPairs + 1);
}

// the run's results become the handle's last results (what the read-only selectors return)
void mc_publish(mi_ilqr* h, McRun& r) {
  const size_t B = r.B;
  // (10, B) -> (B, 10); a problem without a counted sample: mean = M2 = NaN (min = +inf, max = -inf, argmin = argmax = -1 as folded)
  h->mc_stats.assign(B * kMcFields, 0.0);
  for (size_t b = 0; b < B; ++b) {
    double* row = h->mc_stats.data() + b * kMcFields;
    for (int f = 0; f < kMcFields; ++f) row[f] = r.acc[(size_t)f * B + b];
    if (row[1] == 0.0) row[3] = row[4] = std::nan("");
  }
  h->mc_samples.swap(r.samples);
  h->mc_env_x.swap(r.env_x_out);               // (not observed: empty, and the selectors refuse)
  h->mc_env_u.swap(r.env_u_out);
  for (size_t i = 0; i < r.box_out.size(); ++i) r.safety_out[i] = (double)r.box_out[i];
  h->mc_safety.swap(r.safety_out);
  h->mc_ms = r.ms_sum;
  h->mc_passes = (int32_t)std::min<unsigned long long>(r.w.passes, 0x7fffffffull);
  h->policy_last_mc = true;
}

}  // namespace

int pack_policy(mi_ilqr* h, double* dst, int steps, int order, const double* sel, int K) {
  if (steps < 1 || steps > h->N - 1) return MI_ILQR_E_BAD_ARG;      // (the controls and gains have N - 1 columns)
  if (sel && (K < 1 || h->B % K != 0)) return MI_ILQR_E_BAD_ARG;
  const int cols = sel ? h->B / K : h->B;
  const size_t total = (size_t)cols * steps * (size_t)(h->n + h->m + h->m * h->n);
  const int blocks = (int)std::min<size_t>((total + 255) / 256, 8192);
  // a cold handle's x_bar and K read as zeros
  hipLaunchKernelGGL(policy_pack_kernel, dim3(blocks), dim3(256), 0, h->stream, h->cold ? nullptr : h->x_bar, policy_u_source(h),
                     h->cold ? nullptr : h->K, dst, h->B, h->n, h->m, h->N, steps, layout_of(h), order, sel, K, cols);
  HIPCHK(hipGetLastError());
  return MI_ILQR_OK;
}

// Monte-Carlo on the device (include/mi_ilqr.h).  MI_F_POLICY_MC_DIST: (B, 3 n + 2 n_params) rows x0_mean | x0_spread | goal |
// p_mean | p_spread - means and spreads finite, spreads and goals non-negative, a goal may be +inf; src == NULL with bytes == 0
// clears the rows.  A refused call changes nothing.
int set_mc_dist(mi_ilqr* h, const double* src, size_t bytes) {
  RowStore& s = h->policy_mc_dist;
  const size_t n = h->n, w = s.width, np = (w - 3 * n) / 2, cnt = (size_t)h->B * w;
  if (const int rc = rows_given(s, src, bytes, cnt); rc != kRowsGiven) return rc;
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
int set_mc_box(mi_ilqr* h, const double* src, size_t bytes) {
  RowStore& s = h->mc_box;
  const size_t n = h->n;
  if (const int rc = rows_given(s, src, bytes, (size_t)h->B * 2 * n); rc != kRowsGiven) return rc;
  for (size_t b = 0; b < (size_t)h->B; ++b)
    for (size_t i = 0; i < n; ++i) {
      const double lo = src[b * 2 * n + i], hi = src[b * 2 * n + n + i];
      if (!(lo <= hi)) return MI_ILQR_E_BAD_ARG;               // (a NaN on either side, or an inverted interval)
    }
  return store_upload(h, s, src);
}

int set_mc_observe(mi_ilqr* h, const double* src, size_t bytes) {
  if (bytes != 8) return MI_ILQR_E_BAD_SHAPE;
  if (!src) return MI_ILQR_E_BAD_ARG;
  if (!(*src == 0.0 || *src == 1.0 || *src == 2.0 || *src == 3.0)) return MI_ILQR_E_BAD_ARG;
  h->mc_observe = (int32_t)*src;
  return MI_ILQR_OK;
}

// MI_F_POLICY_MC_RUN: v = S | x0_dist | p_dist | sample_params | samples.  Nothing of the handle's solver state is written; the
// staging memory is the grow-only scratch.  A refused or failed run leaves the last results in place.
int run_policy_mc(mi_ilqr* h, const double* v, size_t bytes) {
  McRun r;
  int rc = mc_validate(h, v, bytes, r);
  if (rc != MI_ILQR_OK) return rc;
  HIPCHK(hipSetDevice(h->d.device_id));
  mc_plan(h, r);
  if ((rc = mc_allocate(h, r)) != MI_ILQR_OK) return rc;
  // From here on copies into the run's host buffers may be queued on the stream: whatever fails, the stream is waited for before
  // they go out of scope.
  if ((rc = mc_passes(h, r)) != MI_ILQR_OK) {
    (void)hipStreamSynchronize(h->stream);
    return rc;
  }
  mc_publish(h, r);
  return MI_ILQR_OK;
}

}  // namespace mi_host

extern "C" int mi_ilqr_policy_rollout(mi_ilqr_t* h, int32_t S, const double* x0, const double* params, double* cost, double* x_final,
                                      int32_t* steps, double* X, double* U) {
  if (!h || S < 1 || !x0 || !cost) return MI_ILQR_E_BAD_ARG;
  { const int rc = join_slots(h); if (rc != MI_ILQR_OK) return rc; }
  const Model* model = model_of(h->d.model_id);
  const size_t B = h->B, n = h->n, m = h->m, N = h->N, np = model->p.n_params, Sz = (size_t)S, W = n + m + m * n;
  // (the unsupported calls before the bad arguments, as ever: a refused call gets the code it always got)
  if (params && np == 0) return MI_ILQR_E_UNSUPPORTED;
  if (const int rc = policy_call_refused(h, h->policy_noise.synced ? (unsigned long long)S : 0); rc != MI_ILQR_OK) return rc;
  if (params) for (size_t i = 0; i < B * Sz * np; ++i) if (!std::isfinite(params[i])) return MI_ILQR_E_BAD_ARG;
  HIPCHK(hipSetDevice(h->d.device_id));
  // one block of the handle's grow-only scratch: the policy's time-major copy | inputs as they arrive and sample-minor |
  // outputs sample-minor and in the boundary's layout
  ScratchPlan plan;
  const size_t o_pol = plan.take(B * (N - 1) * W), o_x0_in = plan.take(B * Sz * n), o_x0 = plan.take(B * n * Sz);
  const size_t o_p_in = plan.take(params ? B * Sz * np : 0), o_p = plan.take(params ? B * np * Sz : 0), o_prow = plan.take(np ? np : 1);
  const size_t o_cost = plan.take(B * Sz), o_steps = plan.take((B * Sz + 1) / 2), o_xf = plan.take(B * n * Sz), o_xf_out = plan.take(B * Sz * n);
  const size_t o_X = plan.take(X ? B * N * n * Sz : 0), o_X_out = plan.take(X ? B * Sz * n * N : 0);
  const size_t o_U = plan.take(U ? B * (N - 1) * m * Sz : 0), o_U_out = plan.take(U ? B * Sz * m * (N - 1) : 0);
  int rc = ensure_scratch(h, plan.bytes());
  if (rc != MI_ILQR_OK) return rc;
  double* const sc = h->scratch;
  if (!h->policy_ev0) {
    HIPCHK(hipEventCreate(&h->policy_ev0));
    HIPCHK(hipEventCreate(&h->policy_ev1));
  }
  if ((rc = pack_policy(h, sc + o_pol, (int)N - 1, PACK_TIME_MAJOR)) != MI_ILQR_OK) return rc;
  HIPCHK(hipMemcpyAsync(sc + o_x0_in, x0, B * Sz * n * 8, hipMemcpyHostToDevice, h->stream));
  if ((rc = transpose_tiles(h, sc + o_x0_in, sc + o_x0, S, (int)n, B, 1, Sz * n, 0, n, n * Sz, 0, Sz)) != MI_ILQR_OK) return rc;
  if (params) {
    HIPCHK(hipMemcpyAsync(sc + o_p_in, params, B * Sz * np * 8, hipMemcpyHostToDevice, h->stream));
    if ((rc = transpose_tiles(h, sc + o_p_in, sc + o_p, S, (int)np, B, 1, Sz * np, 0, np, np * Sz, 0, Sz)) != MI_ILQR_OK) return rc;
  }
  PolicyArgs a{};
  if ((rc = fill_policy_args(h, model, sc + o_pol, sc + o_prow, a)) != MI_ILQR_OK) return rc;
  a.x0 = sc + o_x0; a.params = params ? sc + o_p : nullptr; a.S = S;
  a.cost_out = sc + o_cost; a.x_final = sc + o_xf; a.steps = reinterpret_cast<int32_t*>(sc + o_steps);
  a.X = X ? sc + o_X : nullptr; a.U = U ? sc + o_U : nullptr;
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
