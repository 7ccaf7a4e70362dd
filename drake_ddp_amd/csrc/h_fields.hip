// libmi_ilqr.so, host side - the fields: the table of the selectors that are plain device arrays, the setters that only validate and
// upload, and the boundary's generic entry points mi_ilqr_set / _get / _get_async / _get_int / _device_ptr, which send every other
// selector to the unit that owns it (the policy's: h_policy.hip, the plant's: h_mpc.hip, multi-start: h_seeds.hip).
#include <cmath>
#include <cstring>
#include <vector>

#include "host_internal.hpp"

using namespace mi;
using namespace mi_host;

namespace mi_host {

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

namespace {

bool is_state_field(int which) {
  return which == MI_F_X_BAR || which == MI_F_K || which == MI_F_KAPPA || which == MI_F_DV || which == MI_F_FX || which == MI_F_FU;
}

int set_target_field(mi_ilqr* h, int which, const double* src, size_t bytes) {
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

// Reference trajectories (MI_F_X_REF / MI_F_REF_CLOCK): (B, T, n) rows, T from the byte count; src == NULL with bytes == 0: no
// reference, clock 0 - the kernels get a null x_ref, as on a handle that never held one.  Workgroup-per-problem handles only; not
// beside a plant (the plant kernels know constant targets only).  A refused call changes nothing.
int set_reference(mi_ilqr* h, const double* src, size_t bytes) {
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

int set_ref_clock(mi_ilqr* h, const double* src, size_t bytes) {
  if (!h->large) return MI_ILQR_E_UNSUPPORTED;
  if (bytes != 8) return MI_ILQR_E_BAD_SHAPE;
  if (!src) return MI_ILQR_E_BAD_ARG;
  const double c = *src;
  if (!(c >= 0.0 && c < kRefClockEnd && c == std::floor(c))) return MI_ILQR_E_BAD_ARG;
  h->ref_clock = (long long)c;
  return MI_ILQR_OK;
}

// Per-problem model parameters (MI_F_MODEL_PARAMS): (B, n_params) rows, problem b's plant in row b.  src == NULL with bytes == 0:
// back to the descriptor's parameters - the kernels read KArgs::params, as on a handle that never left them.  MI_F_PLANT_PARAMS: the
// same rules on the plants' own rows (dropped: the problems' model rows again).
int set_param_rows(mi_ilqr* h, RowStore& store, const double* src, size_t bytes) {
  const size_t cnt = (size_t)h->B * store.width;
  if (cnt == 0) return MI_ILQR_E_UNSUPPORTED;
  if (const int rc = rows_given(store, src, bytes, cnt); rc != kRowsGiven) return rc;
  for (size_t i = 0; i < cnt; ++i) if (!std::isfinite(src[i])) return MI_ILQR_E_BAD_ARG;
  return store_upload(h, store, src);
}

// The disturbances of mi_ilqr_policy_rollout.  MI_F_POLICY_NOISE: (B, n + m) rows sigma_x | sigma_u, standard deviations - finite
// and non-negative, zero on the padding controls; src == NULL with bytes == 0: no noise, the noise-free kernels again.
// MI_F_POLICY_STREAM: seed | first_sample | common as doubles holding integers.  A refused call changes nothing.
// (the same rows and rules serve the plant of the closed MPC loop: MI_F_PLANT_NOISE, a store of its own)
int set_noise_rows(mi_ilqr* h, RowStore& store, const double* src, size_t bytes) {
  const size_t w = store.width, cnt = (size_t)h->B * w;
  if (const int rc = rows_given(store, src, bytes, cnt); rc != kRowsGiven) return rc;
  const size_t first_pad = (size_t)h->n + (size_t)device_m_user(model_of(h->d.model_id), h);
  for (size_t i = 0; i < cnt; ++i) {
    if (!std::isfinite(src[i]) || src[i] < 0.0) return MI_ILQR_E_BAD_ARG;
    if (i % w >= first_pad && src[i] != 0.0) return MI_ILQR_E_BAD_ARG;
  }
  return store_upload(h, store, src);
}

// The plant of the closed MPC loop (mi_ilqr_mpc_run; plant_advance.hpp).  MI_F_PLANT_STATE: (B, n) finite states - the handle holds
// a plant from now on, and every plant is running again; src == NULL with bytes == 0: no plant, mi_ilqr_mpc_run is the open loop.
// MI_F_PLANT_STREAM: seed | clock | common | feedback.
// A refused call changes nothing.
int set_plant_state(mi_ilqr* h, const double* src, size_t bytes) {
  const size_t cnt = (size_t)h->B * h->n;
  if ((src || bytes) && h->reference.synced) return MI_ILQR_E_UNSUPPORTED;      // (the plant kernels know constant targets only)
  if (const int rc = rows_given(h->plant_state, src, bytes, cnt); rc != kRowsGiven) return rc;
  for (size_t i = 0; i < cnt; ++i) if (!std::isfinite(src[i])) return MI_ILQR_E_BAD_ARG;
  HIPCHK(hipSetDevice(h->d.device_id));
  int rc = h->plant_dead ? MI_ILQR_OK : dev_alloc(h, h->plant_dead, (size_t)h->B);
  if (rc != MI_ILQR_OK) return rc;
  HIPCHK(hipMemsetAsync(h->plant_dead, 0, (size_t)h->B * 8, h->stream));
  return store_upload(h, h->plant_state, src);
}

int set_plant_stream(mi_ilqr* h, const double* src, size_t bytes) {
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

int set_policy_stream(mi_ilqr* h, const double* src, size_t bytes) {
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

// mi_ilqr_get of what the last Monte-Carlo run left on the host: the copy, or the refusal when that run (or no run) did not produce it
int copy_last_run(const mi_ilqr* h, const std::vector<double>& r, double* dst, size_t bytes) {
  if (h->mc_stats.empty() || r.empty()) return MI_ILQR_E_BAD_ARG;
  if (bytes != r.size() * 8) return MI_ILQR_E_BAD_SHAPE;
  std::memcpy(dst, r.data(), bytes);
  return MI_ILQR_OK;
}

}  // namespace
}  // namespace mi_host

extern "C" {

int mi_ilqr_get(mi_ilqr_t* h, int which, double* dst, size_t bytes) {
  if (!h || !dst) return MI_ILQR_E_BAD_ARG;
  { const int rc = join_slots(h); if (rc != MI_ILQR_OK) return rc; }      // (solve slots: what follows reads the current one, on its stream)
  if (const int rc = get_plant_field(h, which, dst, bytes); rc != kNotPlantField) return rc;
  if (const int rc = get_seeds_field(h, which, dst, bytes); rc != kNotSeedsField) return rc;      // (the last command's results, host copies)
  if (const int rc = get_fit_field(h, which, dst, bytes); rc != kNotFitField) return rc;          // (the same of parameter identification)
  if (const RowField r = row_field(h, which); r.store) return store_read(h, *r.store, r.shared_row, dst, bytes);   // (host mirrors)
  if (which == MI_F_POLICY_STREAM) {
    if (bytes != 3 * 8) return MI_ILQR_E_BAD_SHAPE;
    dst[0] = (double)h->policy_seed; dst[1] = (double)h->policy_first_sample; dst[2] = h->policy_common ? 1.0 : 0.0;
    return MI_ILQR_OK;
  }
  switch (which) {                               // the last run's results, host copies
    case MI_F_POLICY_MC_STATS: return copy_last_run(h, h->mc_stats, dst, bytes);
    case MI_F_POLICY_MC_SAMPLES: return copy_last_run(h, h->mc_samples, dst, bytes);
    case MI_F_POLICY_MC_ENVELOPE: return copy_last_run(h, h->mc_env_x, dst, bytes);
    case MI_F_POLICY_MC_ENVELOPE_U: return copy_last_run(h, h->mc_env_u, dst, bytes);
    case MI_F_POLICY_MC_SAFETY: return copy_last_run(h, h->mc_safety, dst, bytes);
  }
  if (which == MI_F_POLICY_MC_OBSERVE) {
    if (bytes != 8) return MI_ILQR_E_BAD_SHAPE;
    *dst = (double)h->mc_observe;
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
  { const int rc = join_slots(h); if (rc != MI_ILQR_OK) return rc; }
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
  { const int rc = join_slots(h); if (rc != MI_ILQR_OK) return rc; }
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
  if (!h) return MI_ILQR_E_BAD_ARG;
  { const int rc = join_slots(h); if (rc != MI_ILQR_OK) return rc; }      // (uploads and commands alike: on the current solve slot's stream, behind both)
  switch (which) {       // the selectors with rules of their own for src: most take src == NULL with bytes == 0 (back to shared mode / none)
    case MI_F_MODEL_PARAMS: return set_param_rows(h, h->params, src, bytes);
    case MI_F_COST_MATRICES: return set_cost_rows(h, src, bytes);
    case MI_F_POLICY_NOISE: return set_noise_rows(h, h->policy_noise, src, bytes);
    case MI_F_POLICY_STREAM: return set_policy_stream(h, src, bytes);
    case MI_F_POLICY_MC_DIST: return set_mc_dist(h, src, bytes);
    case MI_F_POLICY_MC_RUN: return run_policy_mc(h, src, bytes);            // (a command: runs the evaluation)
    case MI_F_POLICY_MC_BOX: return set_mc_box(h, src, bytes);
    case MI_F_POLICY_MC_OBSERVE: return set_mc_observe(h, src, bytes);
    case MI_F_POLICY_MC_ENVELOPE: case MI_F_POLICY_MC_ENVELOPE_U: case MI_F_POLICY_MC_SAFETY: return MI_ILQR_E_BAD_ARG;   // (read-only)
    case MI_F_SEEDS_SIGMA: return set_seeds_sigma(h, src, bytes);
    case MI_F_SEEDS_RUN: return run_seeds(h, src, bytes);                    // (a command: perturb / select / reseed / gather)
    case MI_F_SEEDS_BEST: case MI_F_SEEDS_X_BAR: case MI_F_SEEDS_U_BAR: case MI_F_SEEDS_COST: case MI_F_SEEDS_KERNEL_MS:
      return MI_ILQR_E_BAD_ARG;                                              // (read-only)
    case MI_F_PLANT_STATE: return set_plant_state(h, src, bytes);
    case MI_F_PLANT_PARAMS: return set_param_rows(h, h->plant_params, src, bytes);
    case MI_F_PLANT_NOISE: return set_noise_rows(h, h->plant_noise, src, bytes);
    case MI_F_PLANT_STREAM: return set_plant_stream(h, src, bytes);
    case MI_F_X_REF: return set_reference(h, src, bytes);
    case MI_F_REF_CLOCK: return set_ref_clock(h, src, bytes);
  }
  if (const int rc = set_fit_field(h, which, src, bytes); rc != kNotFitField) return rc;           // (MI_F_FIT_*: h_fit.hip)
  if (!src) return MI_ILQR_E_BAD_ARG;
  if (which == MI_F_X_NOM || which == MI_F_TARGET_STEP) return set_target_field(h, which, src, bytes);
  Field f = field_of(h, which);
  if (!f.ptr || f.is_int) return MI_ILQR_E_BAD_ARG;
  if (bytes != f.bytes) return MI_ILQR_E_BAD_SHAPE;
  HIPCHK(hipSetDevice(h->d.device_id));
  if (which == MI_F_X0) inputs_touched(h);
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
  // the state fields and x0 are those of the current solve slot (the solve enqueued last): ordered on its stream behind both, and
  // x0 possibly written through the pointer
  { const int rc = join_slots(h); if (rc != MI_ILQR_OK) return rc; }
  if (which == MI_F_X0) inputs_touched(h);
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

}  // extern "C"
