// libmi_ilqr.so, host side - multi-start (include/mi_ilqr.h, "Multi-start"; seeds.hpp): the sigma rows of the perturbation, the command
// MI_F_SEEDS_RUN - perturb, select, reseed, select + gather on the handle's resident state, one launch of seeds_kernel each - and
// the host copies the read-only selectors return.  Select and gather write nothing of the solver's state; perturb and reseed leave
// the handle where mi_ilqr_reset followed by mi_ilqr_set_initial would: cold, with a pending guess.  The LONG form of the command
// (8 doubles: multi-start in the receding-horizon loop) is validated here and run by h_mpc.hip's mpc_run_seeds; its selection log and
// its kernels' time are kept here, behind the same selectors.
#include <cmath>
#include <cstring>
#include <vector>

#include "host_internal.hpp"

using namespace mi;
using namespace mi_host;

namespace mi_host {

namespace {

// v = K | op | seed | round | hold | reserved [| num_resolves | replan_steps: the long form], integers held in doubles (the
// comparisons are false for a NaN)
struct SeedsRun { int32_t K = 0, op = 0, hold = 1, num_resolves = 0, replan_steps = 0; unsigned long long seed = 0; uint32_t round = 0; };

int seeds_validate(const mi_ilqr* h, const double* v, size_t bytes, SeedsRun& r) {
  if (h->host_inputs) return MI_ILQR_E_UNSUPPORTED;              // (x0 and the guess live in host memory there: B <= 4, nothing to group)
  const bool long_form = bytes == 8 * 8;
  if (bytes != 6 * 8 && !long_form) return MI_ILQR_E_BAD_SHAPE;
  if (!v) return MI_ILQR_E_BAD_ARG;
  auto whole = [](double x, double lo, double end) { return x >= lo && x < end && x == std::floor(x); };
  if (!whole(v[0], 1.0, 0x1p31) || !whole(v[1], 0.0, 4.0) || !whole(v[2], 0.0, 0x1p53) || !whole(v[3], 0.0, 0x1p32) ||
      !whole(v[4], 1.0, 0x1p31) || v[5] != 0.0)
    return MI_ILQR_E_BAD_ARG;
  r.K = (int32_t)v[0]; r.op = (int32_t)v[1]; r.seed = (unsigned long long)v[2]; r.round = (uint32_t)v[3]; r.hold = (int32_t)v[4];
  if (h->B % r.K != 0) return MI_ILQR_E_BAD_ARG;
  if (long_form) {                                               // the receding-horizon loop: reseed is the one operation it joins with
    if (r.op != SEEDS_RESEED || !whole(v[6], 1.0, 0x1p31) || !whole(v[7], 1.0, (double)(h->N - 1))) return MI_ILQR_E_BAD_ARG;
    r.num_resolves = (int32_t)v[6]; r.replan_steps = (int32_t)v[7];
  }
  return MI_ILQR_OK;
}

int copy_result(const std::vector<double>& r, double* dst, size_t bytes) {
  if (r.empty()) return MI_ILQR_E_BAD_ARG;                       // (no select / no gather yet)
  if (bytes != r.size() * 8) return MI_ILQR_E_BAD_SHAPE;
  std::memcpy(dst, r.data(), bytes);
  return MI_ILQR_OK;
}

}  // namespace

// MI_F_SEEDS_SIGMA: (B, m) rows sigma_u, standard deviations - finite and non-negative, zero on the padding controls; src == NULL
// with bytes == 0 clears the rows (zeros).  A refused call changes nothing.
int set_seeds_sigma(mi_ilqr* h, const double* src, size_t bytes) {
  RowStore& s = h->seeds_sigma;
  const size_t w = s.width, cnt = (size_t)h->B * w;
  if (const int rc = rows_given(s, src, bytes, cnt); rc != kRowsGiven) return rc;
  const size_t first_pad = (size_t)device_m_user(model_of(h->d.model_id), h);
  for (size_t i = 0; i < cnt; ++i) {
    if (!std::isfinite(src[i]) || src[i] < 0.0) return MI_ILQR_E_BAD_ARG;
    if (i % w >= first_pad && src[i] != 0.0) return MI_ILQR_E_BAD_ARG;
  }
  return store_upload(h, s, src);
}

// MI_F_SEEDS_RUN.  The kernel runs on the handle's stream behind whatever is enqueued there, the call synchronizes once.  A refused
// command changes nothing; a select or gather leaves the solver's state alone.
int run_seeds(mi_ilqr* h, const double* v, size_t bytes) {
  const SlotHold hold(h);            // (solve slots: joined, and every launch below stays on the current one)
  if (hold.rc != MI_ILQR_OK) return hold.rc;
  if (bytes == 10 * 8) return run_mppi(h, v);                     // the sampling form: h_mppi.hip, the results kept behind the same selectors
  SeedsRun r;
  int rc = seeds_validate(h, v, bytes, r);
  if (rc != MI_ILQR_OK) return rc;
  if (r.num_resolves > 0) {                                      // the long form: the loop of h_mpc.hip, the results kept here
    std::vector<double> log;
    double ms = 0.0;
    if ((rc = mpc_run_seeds(h, SeedsMpcRun{r.K, r.hold, r.num_resolves, r.replan_steps, r.seed, r.round}, log, ms)) != MI_ILQR_OK) return rc;
    h->seeds_best.swap(log);
    h->seeds_x.clear(); h->seeds_u.clear(); h->seeds_cost.clear();   // (the last command that selected was no gather)
    h->seeds_ms = ms;
    h->seeds_ran = true;
    return MI_ILQR_OK;
  }
  const size_t B = h->B, n = h->n, m = h->m, N = h->N, G = B / (size_t)r.K;
  HIPCHK(hipSetDevice(h->d.device_id));
  if (!h->seeds_best_dev && (rc = dev_alloc(h, h->seeds_best_dev, B * 3)) != MI_ILQR_OK) return rc;
  if (!h->seeds_ev0) {
    HIPCHK(hipEventCreate(&h->seeds_ev0));
    HIPCHK(hipEventCreate(&h->seeds_ev1));
  }
  ScratchPlan plan;                                              // the gather's staging arrays, in the grow-only scratch
  const bool gather = r.op == SEEDS_GATHER, writes = r.op == SEEDS_PERTURB || r.op == SEEDS_RESEED;
  const size_t o_x = plan.take(gather ? G * n * N : 0), o_u = plan.take(gather ? G * m * (N - 1) : 0), o_c = plan.take(gather ? G : 0);
  if (gather && (rc = ensure_scratch(h, plan.bytes())) != MI_ILQR_OK) return rc;
  SeedsArgs a{};
  a.u_src = policy_u_source(h); a.u_dst = h->u_guess;
  a.sigma = h->seeds_sigma.synced ? h->seeds_sigma.rows : nullptr;
  a.cost = h->cost; a.status = h->status; a.best = h->seeds_best_dev;
  a.x_bar = h->cold ? nullptr : h->x_bar;
  if (gather) { a.gx = h->scratch + o_x; a.gu = h->scratch + o_u; a.gc = h->scratch + o_c; }
  a.seed = r.seed; a.round = r.round;
  a.B = (int32_t)B; a.K = r.K; a.n = (int32_t)n; a.m = (int32_t)m; a.m_user = device_m_user(model_of(h->d.model_id), h);
  a.N = (int32_t)N; a.layout = layout_of(h); a.op = r.op; a.hold = r.hold;
  a.ev0 = h->seeds_ev0; a.ev1 = h->seeds_ev1;
  h->seeds_ran = false;
  if ((rc = launch_seeds(h, a)) != MI_ILQR_OK) return rc;
  if (writes) {                                                  // the guesses are in u_guess: the next solve starts cold from them
    h->cold = true;
    h->u_pending = true;
    h->u_zero = false;
  }
  std::vector<double> best, gx, gu, gc;
  if (r.op != SEEDS_PERTURB) {
    best.resize(G * 3);
    HIPCHK(hipMemcpyAsync(best.data(), h->seeds_best_dev, best.size() * 8, hipMemcpyDeviceToHost, h->stream));
  }
  if (gather) {
    gx.resize(G * n * N); gu.resize(G * m * (N - 1)); gc.resize(G);
    HIPCHK(hipMemcpyAsync(gx.data(), a.gx, gx.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(gu.data(), a.gu, gu.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(gc.data(), a.gc, gc.size() * 8, hipMemcpyDeviceToHost, h->stream));
  }
  if (hipStreamSynchronize(h->stream) != hipSuccess) { (void)hipDeviceSynchronize(); return MI_ILQR_E_HIP; }   // (copies into locals were queued)
  float ms = 0.0f;
  HIPCHK(hipEventElapsedTime(&ms, h->seeds_ev0, h->seeds_ev1));
  h->seeds_ms = (double)ms;
  h->seeds_ran = true;
  if (r.op != SEEDS_PERTURB) {                                   // a select: the rows, and the gather's results only when it was one
    h->seeds_best.swap(best);
    h->seeds_x.swap(gx); h->seeds_u.swap(gu); h->seeds_cost.swap(gc);
  }
  return MI_ILQR_OK;
}

// mi_ilqr_get of the multi-start selectors; kNotSeedsField for every other one
int get_seeds_field(mi_ilqr* h, int which, double* dst, size_t bytes) {
  switch (which) {
    case MI_F_SEEDS_RUN: return MI_ILQR_E_BAD_ARG;              // (write-only)
    case MI_F_SEEDS_BEST: return copy_result(h->seeds_best, dst, bytes);
    case MI_F_SEEDS_X_BAR: return copy_result(h->seeds_x, dst, bytes);
    case MI_F_SEEDS_U_BAR: return copy_result(h->seeds_u, dst, bytes);
    case MI_F_SEEDS_COST: return copy_result(h->seeds_cost, dst, bytes);
    case MI_F_SEEDS_KERNEL_MS:
      if (!h->seeds_ran) return MI_ILQR_E_BAD_ARG;
      if (bytes != 8) return MI_ILQR_E_BAD_SHAPE;
      *dst = h->seeds_ms;
      return MI_ILQR_OK;
  }
  return kNotSeedsField;
}

}  // namespace mi_host
