// libmi_ilqr.so, host side - parameter identification (include/mi_ilqr.h, "Parameter identification"; fit.hpp): the setters of
// MI_F_FIT_DATA / _WEIGHTS / _START / _BOUNDS, the command MI_F_FIT_RUN and what the read-only selectors return.  A run of I
// iterations is normal(theta0), I x {update, normal(trial)} and the closing update, all on the handle's stream with one event pair
// around them and one synchronisation at the end; the problems' records live in the handle's scratch for the length of the call.
// Nothing here reads or writes what a solve uses, except that apply = 1 ends in the upload MI_F_MODEL_PARAMS would make.
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "host_internal.hpp"

using namespace mi;
using namespace mi_host;

namespace mi_host {

namespace {

constexpr double kFitDefaultMu = 1e-3;
constexpr size_t kFitMaxT = (size_t)1 << 24;
constexpr int kFitResultExtra = 7;          // cost0 | cost | mu | iterations | accepted | status | count behind theta

bool whole(double x, double lo, double hi) { return x >= lo && x <= hi && x == std::floor(x); }   // (false for a NaN)

int set_fit_data(mi_ilqr* h, const double* src, size_t bytes) {
  if (!src && bytes == 0) { h->fit_T = 0; h->fit_weights.clear(); return MI_ILQR_OK; }
  const size_t per_row = (size_t)h->B * (2 * (size_t)h->n + h->m);
  if (bytes == 0 || bytes % (per_row * 8) != 0) return MI_ILQR_E_BAD_SHAPE;
  const size_t T = bytes / (per_row * 8), cnt = per_row * T;
  if (T >= kFitMaxT) return MI_ILQR_E_BAD_SHAPE;
  if (!src) return MI_ILQR_E_BAD_ARG;
  for (size_t i = 0; i < cnt; ++i) if (!std::isfinite(src[i])) return MI_ILQR_E_BAD_ARG;
  HIPCHK(hipSetDevice(h->d.device_id));
  int rc = MI_ILQR_OK;
  if (cnt > h->fit_data_cap) {                                   // grow-only; a run in flight has been waited for by then
    HIPCHK(hipStreamSynchronize(h->stream));
    h->fit_T = 0; h->fit_data_cap = 0;
    if ((rc = dev_free(h, h->fit_data)) != MI_ILQR_OK) return rc;
    if ((rc = dev_alloc(h, h->fit_data, cnt)) != MI_ILQR_OK) return rc;
    h->fit_data_cap = cnt;
  }
  h->fit_T = 0;
  if ((rc = stage_h2d(h, h->fit_data, src, cnt * 8)) != MI_ILQR_OK) return rc;
  h->fit_T = (int)T;
  h->fit_weights.clear();                                        // (the counts referred to the old T)
  return MI_ILQR_OK;
}

// the opening the three small setters share: NULL with 0 bytes drops the rows, then the size before the pointer
int small_rows(std::vector<double>& v, const double* src, size_t bytes, size_t cnt) {
  if (!src && bytes == 0) { v.clear(); return MI_ILQR_OK; }
  if (bytes != cnt * 8) return MI_ILQR_E_BAD_SHAPE;
  return src ? kRowsGiven : MI_ILQR_E_BAD_ARG;
}

int set_fit_weights(mi_ilqr* h, const double* src, size_t bytes) {
  const size_t B = h->B, n = h->n;
  if (const int rc = small_rows(h->fit_weights, src, bytes, B * (n + 1)); rc != kRowsGiven) return rc;
  if (h->fit_T < 1) return MI_ILQR_E_BAD_ARG;
  for (size_t b = 0; b < B; ++b) {
    const double* r = src + b * (n + 1);
    for (size_t i = 0; i < n; ++i) if (!std::isfinite(r[i]) || r[i] < 0.0) return MI_ILQR_E_BAD_ARG;
    if (!whole(r[n], 0.0, (double)h->fit_T)) return MI_ILQR_E_BAD_ARG;
  }
  h->fit_weights.assign(src, src + B * (n + 1));
  return MI_ILQR_OK;
}

int set_fit_start(mi_ilqr* h, const double* src, size_t bytes, size_t np) {
  const size_t B = h->B;
  if (const int rc = small_rows(h->fit_start, src, bytes, B * (np + 1)); rc != kRowsGiven) return rc;
  for (size_t i = 0; i < B * (np + 1); ++i) if (!std::isfinite(src[i])) return MI_ILQR_E_BAD_ARG;
  for (size_t b = 0; b < B; ++b) if (!(src[b * (np + 1) + np] > 0.0)) return MI_ILQR_E_BAD_ARG;
  h->fit_start.assign(src, src + B * (np + 1));
  return MI_ILQR_OK;
}

int set_fit_bounds(mi_ilqr* h, const double* src, size_t bytes, size_t np) {
  if (const int rc = small_rows(h->fit_bounds, src, bytes, 2 * np); rc != kRowsGiven) return rc;
  for (size_t k = 0; k < np; ++k) if (!(src[k] <= src[np + k])) return MI_ILQR_E_BAD_ARG;     // (a NaN compares false)
  h->fit_bounds.assign(src, src + 2 * np);
  return MI_ILQR_OK;
}

// v = iterations | ftol | fd_rel | fd_floor | apply | P | free[0 .. P-1]
struct FitRun { int32_t iterations = 0, P = 0; double ftol = 0.0, fd_rel = 0.0, fd_floor = 0.0; bool apply = false; int32_t free_idx[kFitMaxFree] = {}; };

int fit_validate(const double* v, size_t bytes, size_t np, FitRun& r) {
  if (bytes < 7 * 8 || bytes % 8 != 0 || bytes > (6 + (size_t)kFitMaxFree) * 8) return MI_ILQR_E_BAD_SHAPE;
  if (!v) return MI_ILQR_E_BAD_ARG;
  if (!whole(v[5], 1.0, (double)kFitMaxFree)) return MI_ILQR_E_BAD_ARG;
  r.P = (int32_t)v[5];
  if (bytes != (6 + (size_t)r.P) * 8) return MI_ILQR_E_BAD_SHAPE;
  if (!whole(v[0], 0.0, 0x1p20) || !(v[1] >= 0.0) || !std::isfinite(v[1]) || !(v[2] > 0.0) || !std::isfinite(v[2]) || !(v[3] > 0.0) ||
      !std::isfinite(v[3]) || !(v[4] == 0.0 || v[4] == 1.0))
    return MI_ILQR_E_BAD_ARG;
  for (int i = 0; i < r.P; ++i) {
    if (!whole(v[6 + i], 0.0, (double)np - 1.0) || (i > 0 && v[6 + i] <= v[5 + i])) return MI_ILQR_E_BAD_ARG;
    r.free_idx[i] = (int32_t)v[6 + i];
  }
  r.iterations = (int32_t)v[0]; r.ftol = v[1]; r.fd_rel = v[2]; r.fd_floor = v[3]; r.apply = v[4] == 1.0;
  return MI_ILQR_OK;
}

int run_fit(mi_ilqr* h, const double* v, size_t bytes) {
  const Model* model = model_of(h->d.model_id);
  const size_t B = h->B, n = h->n, np = model->p.n_params;
  FitRun r;
  int rc = fit_validate(v, bytes, np, r);
  if (rc != MI_ILQR_OK) return rc;
  if (h->fit_T < 1 || !h->fit_data) return MI_ILQR_E_BAD_ARG;
  const int P = r.P, L = fit_row_len(P), T = h->fit_T;
  int log2G = 1;
  while ((1 << log2G) < P + 1) ++log2G;
  const int per = 64 >> log2G, waves = (T + per - 1) / per;
  if ((unsigned long long)waves * B > 0x7fffffffull) return MI_ILQR_E_UNSUPPORTED;   // (the normal kernel's grid)

  // what the setters left, or the defaults
  std::vector<double> weights(h->fit_weights), bounds(h->fit_bounds), state(B * kFitStride, 0.0);
  if (weights.empty()) {
    weights.assign(B * (n + 1), 1.0);
    for (size_t b = 0; b < B; ++b) weights[b * (n + 1) + n] = (double)T;
  }
  for (size_t b = 0; b < B; ++b) if (weights[b * (n + 1) + n] > (double)T) return MI_ILQR_E_BAD_ARG;
  if (bounds.empty()) {
    bounds.assign(2 * np, std::numeric_limits<double>::infinity());
    for (size_t k = 0; k < np; ++k) bounds[k] = -bounds[k];
  }
  for (size_t b = 0; b < B; ++b) {
    double* st = state.data() + b * kFitStride;
    for (size_t k = 0; k < np; ++k) {
      st[kFitTheta + k] = st[kFitTrial + k] = !h->fit_start.empty() ? h->fit_start[b * (np + 1) + k]
                                                : (h->params.synced ? h->params.mirror[b * np + k] : h->d.model_params[k]);
    }
    st[kFitMu] = h->fit_start.empty() ? kFitDefaultMu : h->fit_start[b * (np + 1) + np];
    const bool empty = weights[b * (n + 1) + n] == 0.0;
    st[kFitStatus] = empty ? (double)MI_FIT_BAD_DATA : kFitRunning;
    st[kFitC] = st[kFitCost0] = empty ? std::numeric_limits<double>::infinity() : 0.0;
    st[kFitTrialOk] = 1.0;
  }

  HIPCHK(hipSetDevice(h->d.device_id));
  ScratchPlan plan;
  const size_t o_state = plan.take(B * kFitStride), o_part = plan.take(B * (size_t)waves * L), o_w = plan.take(B * (n + 1)), o_b = plan.take(2 * np);
  if ((rc = ensure_scratch(h, plan.bytes())) != MI_ILQR_OK) return rc;
  if (!h->fit_ev0) {
    HIPCHK(hipEventCreate(&h->fit_ev0));
    HIPCHK(hipEventCreate(&h->fit_ev1));
  }
  double* const sc = h->scratch;
  if ((rc = stage_h2d(h, sc + o_state, state.data(), state.size() * 8)) != MI_ILQR_OK) return rc;
  if ((rc = stage_h2d(h, sc + o_w, weights.data(), weights.size() * 8)) != MI_ILQR_OK) return rc;
  if ((rc = stage_h2d(h, sc + o_b, bounds.data(), bounds.size() * 8)) != MI_ILQR_OK) return rc;

  FitArgs a{};
  a.data = h->fit_data; a.weights = sc + o_w; a.state = sc + o_state; a.partial = sc + o_part;
  a.dt = h->d.dt; a.fd_rel = r.fd_rel; a.fd_floor = r.fd_floor;
  a.B = (int32_t)B; a.T = T; a.P = P; a.log2G = log2G; a.waves = waves;
  FitUpdateArgs u{};
  u.state = sc + o_state; u.partial = sc + o_part; u.bounds = sc + o_b; u.ftol = r.ftol;
  u.B = (int32_t)B; u.P = P; u.n_params = (int32_t)np; u.waves = waves;
  for (int i = 0; i < kFitMaxFree; ++i) a.free_idx[i] = u.free_idx[i] = i < P ? r.free_idx[i] : 0;
  // From here on the handle's stream carries the run: the start event rides on the first evaluation, the stop event on the closing decision.
  for (int i = 0; i <= r.iterations && rc == MI_ILQR_OK; ++i) {
    a.ev0 = i == 0 ? h->fit_ev0 : nullptr;
    a.ev1 = nullptr;
    if ((rc = model->p.launch(h, kModeFitNormal, &a)) != MI_ILQR_OK) break;
    u.first = i == 0; u.last = i == r.iterations;
    u.ev0 = nullptr;
    u.ev1 = u.last ? h->fit_ev1 : nullptr;
    rc = launch_fit_update(h, u);
  }
  if (rc != MI_ILQR_OK) {                                        // (a launch failed part-way: nothing of the handle has been written)
    (void)hipStreamSynchronize(h->stream);
    return rc;
  }
  HIPCHK(hipMemcpyAsync(state.data(), sc + o_state, state.size() * 8, hipMemcpyDeviceToHost, h->stream));
  if (hipStreamSynchronize(h->stream) != hipSuccess) { (void)hipDeviceSynchronize(); return MI_ILQR_E_HIP; }   // (a copy into a local was queued)
  float ms = 0.0f;
  HIPCHK(hipEventElapsedTime(&ms, h->fit_ev0, h->fit_ev1));

  const size_t RW = np + kFitResultExtra, NW = (size_t)P + (size_t)P * P;
  std::vector<double> result(B * RW), normal(B * NW, 0.0), rows(B * np);
  for (size_t b = 0; b < B; ++b) {
    const double* st = state.data() + b * kFitStride;
    double* o = result.data() + b * RW;
    for (size_t k = 0; k < np; ++k) o[k] = rows[b * np + k] = st[kFitTheta + k];
    o[np] = st[kFitCost0]; o[np + 1] = st[kFitC]; o[np + 2] = st[kFitMu]; o[np + 3] = st[kFitIters]; o[np + 4] = st[kFitAccepted];
    o[np + 5] = st[kFitStatus]; o[np + 6] = weights[b * (n + 1) + n];
    if (o[np + 6] == 0.0) continue;                              // (no rows: the record holds no normal equations)
    double* g = normal.data() + b * NW;
    const double* row = st + kFitC + 1;
    int q = P;
    for (int i = 0; i < P; ++i) g[i] = row[i];
    for (int i = 0; i < P; ++i)
      for (int j = i; j < P; ++j, ++q) g[P + i * P + j] = g[P + j * P + i] = row[q];
  }
  if (r.apply && (rc = store_upload(h, h->params, rows.data())) != MI_ILQR_OK) return rc;
  h->fit_ms = (double)ms;
  h->fit_result.swap(result);
  h->fit_normal.swap(normal);
  return MI_ILQR_OK;
}

int copy_rows(const std::vector<double>& r, double* dst, size_t bytes) {
  if (r.empty()) return MI_ILQR_E_BAD_ARG;
  if (bytes != r.size() * 8) return MI_ILQR_E_BAD_SHAPE;
  std::memcpy(dst, r.data(), bytes);
  return MI_ILQR_OK;
}

bool is_fit_field(int which) { return which >= MI_F_FIT_DATA && which <= MI_F_FIT_KERNEL_MS; }

}  // namespace

int set_fit_field(mi_ilqr* h, int which, const double* src, size_t bytes) {
  if (!is_fit_field(which)) return kNotFitField;
  const size_t np = model_of(h->d.model_id)->p.n_params;
  if (np == 0) return MI_ILQR_E_UNSUPPORTED;
  switch (which) {
    case MI_F_FIT_DATA: return set_fit_data(h, src, bytes);
    case MI_F_FIT_WEIGHTS: return set_fit_weights(h, src, bytes);
    case MI_F_FIT_START: return set_fit_start(h, src, bytes, np);
    case MI_F_FIT_BOUNDS: return set_fit_bounds(h, src, bytes, np);
    case MI_F_FIT_RUN: return run_fit(h, src, bytes);
  }
  return MI_ILQR_E_BAD_ARG;                                      // (read-only)
}

int get_fit_field(mi_ilqr* h, int which, double* dst, size_t bytes) {
  if (!is_fit_field(which)) return kNotFitField;
  if (model_of(h->d.model_id)->p.n_params == 0) return MI_ILQR_E_UNSUPPORTED;
  switch (which) {
    case MI_F_FIT_WEIGHTS: return copy_rows(h->fit_weights, dst, bytes);
    case MI_F_FIT_START: return copy_rows(h->fit_start, dst, bytes);
    case MI_F_FIT_BOUNDS: return copy_rows(h->fit_bounds, dst, bytes);
    case MI_F_FIT_RESULT: return copy_rows(h->fit_result, dst, bytes);
    case MI_F_FIT_NORMAL: return copy_rows(h->fit_normal, dst, bytes);
    case MI_F_FIT_KERNEL_MS:
      if (h->fit_result.empty()) return MI_ILQR_E_BAD_ARG;
      if (bytes != 8) return MI_ILQR_E_BAD_SHAPE;
      *dst = h->fit_ms;
      return MI_ILQR_OK;
  }
  return MI_ILQR_E_BAD_ARG;                                      // (the data stay on the device; the command is write-only)
}

}  // namespace mi_host
