// libmi_ilqr.so, host side - sampling-based MPC (include/mi_ilqr.h, "Sampling-based MPC"; mppi.hpp): the sampling form of
// MI_F_SEEDS_RUN, 10 doubles, which h_seeds.hip hands over.  The iteration loop never leaves the device: the nominal is staged once,
// every iteration is one sampled rollout and one update, a closing rollout of the final nominal alone and the hand-over follow, all
// on the handle's stream with one event pair around them and one synchronisation at the end.  The results go where the multi-start
// commands keep theirs (h->seeds_best / seeds_cost / seeds_u), behind the same read-only selectors.
#include <cmath>
#include <vector>

#include "host_internal.hpp"

using namespace mi;
using namespace mi_host;

namespace mi_host {

namespace {

// v = S | op | seed | first_sample | hold | reserved = 0 | iterations | shift | temperature | reserved = 0; S <= 2^31 - 64: the
// rollout rounds S up to whole waves in 32-bit arithmetic
struct MppiRun { int32_t S = 0, hold = 1, iterations = 0, shift = 0; unsigned long long seed = 0; uint32_t first_sample = 0; double temperature = 0.0; };

int mppi_validate(const mi_ilqr* h, const double* v, MppiRun& r) {
  if (h->reference.synced) return MI_ILQR_E_UNSUPPORTED;         // (the rollout costs against a constant target only, like the policy calls)
  if (h->host_inputs) return MI_ILQR_E_UNSUPPORTED;              // (x0 and the guess live in host memory there, like the seed commands)
  if (!v) return MI_ILQR_E_BAD_ARG;
  auto whole = [](double x, double lo, double end) { return x >= lo && x < end && x == std::floor(x); };   // (false for a NaN)
  if (!whole(v[0], 1.0, 0x1p31 - 63.0) || v[1] != (double)SEEDS_RESEED || !whole(v[2], 0.0, 0x1p53) || !whole(v[3], 0.0, 0x1p32) ||
      !whole(v[4], 1.0, 0x1p31) || v[5] != 0.0 || !whole(v[6], 1.0, 0x1p31) || !whole(v[7], 0.0, (double)(h->N - 1)) || !(v[8] >= 0.0) ||
      v[9] != 0.0)
    return MI_ILQR_E_BAD_ARG;
  if (v[3] + v[6] * v[0] > 0x1p32) return MI_ILQR_E_BAD_ARG;     // (the sample counter is 32 bits; a product too large to be exact is far above the bound)
  r.S = (int32_t)v[0]; r.seed = (unsigned long long)v[2]; r.first_sample = (uint32_t)v[3]; r.hold = (int32_t)v[4];
  r.iterations = (int32_t)v[6]; r.shift = (int32_t)v[7]; r.temperature = v[8];
  return MI_ILQR_OK;
}

}  // namespace

int run_mppi(mi_ilqr* h, const double* v) {
  MppiRun r;
  int rc = mppi_validate(h, v, r);
  if (rc != MI_ILQR_OK) return rc;
  const Model* model = model_of(h->d.model_id);
  const size_t B = h->B, m = h->m, N = h->N, np = model->p.n_params, S = (size_t)r.S, I = (size_t)r.iterations, plan_len = B * (N - 1) * m;
  if ((S + 63) / 64 * B > 0x7fffffffull) return MI_ILQR_E_UNSUPPORTED;   // (the rollout's grid)
  HIPCHK(hipSetDevice(h->d.device_id));
  ScratchPlan plan;
  const size_t o_nom[2] = {plan.take(plan_len), plan.take(plan_len)}, o_cost = plan.take(B * S), o_cost1 = plan.take(B), o_prow = plan.take(np ? np : 1);
  const size_t o_tl = plan.take(plan_len), o_best = plan.take(I * B * 3), o_log = plan.take((I + 1) * B * 2);
  if ((rc = ensure_scratch(h, plan.bytes())) != MI_ILQR_OK) return rc;
  if (!h->seeds_ev0) {
    HIPCHK(hipEventCreate(&h->seeds_ev0));
    HIPCHK(hipEventCreate(&h->seeds_ev1));
  }
  std::vector<double> best(I * B * 3), costlog((I + 1) * B * 2), tl(plan_len);
  double* const sc = h->scratch;
  const int layout = layout_of(h);
  MppiArgs a{};
  if ((rc = fill_policy_args(h, model, nullptr, sc + o_prow, a.r)) != MI_ILQR_OK) return rc;
  const double* sigma = h->seeds_sigma.synced ? h->seeds_sigma.rows : nullptr;
  a.x0 = h->x0; a.seed = r.seed; a.hold = r.hold;
  MppiUpdateArgs u{};
  u.sigma = sigma; u.ulim = a.r.ulim; u.seed = r.seed; u.temperature = r.temperature;
  u.B = (int32_t)B; u.S = r.S; u.m = (int32_t)m; u.m_user = a.r.m_user; u.N = (int32_t)N; u.hold = r.hold;
  // From here on the handle's stream carries the run: the start event rides on the staging copy, the stop event on the hand-over.
  h->seeds_ran = false;
  if ((rc = launch_mppi_stage(h, policy_u_source(h), sc + o_nom[0], (int)B, (int)m, (int)N, layout, h->seeds_ev0)) != MI_ILQR_OK) return rc;
  int cur = 0;
  for (size_t i = 0; i < I && rc == MI_ILQR_OK; ++i, cur ^= 1) {
    const uint32_t sample0 = (uint32_t)((unsigned long long)r.first_sample + i * S);
    a.nominal = sc + o_nom[cur]; a.sigma = sigma; a.cost_out = sc + o_cost; a.S = r.S; a.sample0 = sample0;
    if ((rc = model->p.launch(h, kModeSampledRollout, &a)) != MI_ILQR_OK) break;
    u.nom_in = sc + o_nom[cur]; u.nom_out = sc + o_nom[cur ^ 1]; u.cost = sc + o_cost; u.sample0 = sample0;
    u.best = sc + o_best + i * B * 3; u.costlog = sc + o_log + i * B * 2;
    rc = launch_mppi_update(h, u);
  }
  if (rc == MI_ILQR_OK) {                                        // the closing rollout: the final nominal alone
    a.nominal = sc + o_nom[cur]; a.sigma = nullptr; a.cost_out = sc + o_cost1; a.S = 1; a.sample0 = 0;
    rc = model->p.launch(h, kModeSampledRollout, &a);
  }
  if (rc == MI_ILQR_OK)
    rc = launch_mppi_handover(h, sc + o_nom[cur], h->u_guess, sc + o_tl, sc + o_cost1, sc + o_log + I * B * 2, (int)B, (int)m, (int)N, layout,
                              r.shift, h->seeds_ev1);
  if (rc != MI_ILQR_OK) {                                        // (a launch failed part-way: nothing of the handle has been written yet)
    (void)hipStreamSynchronize(h->stream);
    return rc;
  }
  // the final nominal is in u_guess: the next solve starts cold from it, as after mi_ilqr_reset + mi_ilqr_set_initial
  h->cold = true;
  h->u_pending = true;
  h->u_zero = false;
  HIPCHK(hipMemcpyAsync(best.data(), sc + o_best, best.size() * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(costlog.data(), sc + o_log, costlog.size() * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(tl.data(), sc + o_tl, tl.size() * 8, hipMemcpyDeviceToHost, h->stream));
  if (hipStreamSynchronize(h->stream) != hipSuccess) { (void)hipDeviceSynchronize(); return MI_ILQR_E_HIP; }   // (copies into locals were queued)
  float ms = 0.0f;
  HIPCHK(hipEventElapsedTime(&ms, h->seeds_ev0, h->seeds_ev1));
  h->seeds_ms = (double)ms;
  h->seeds_ran = true;
  h->seeds_best.swap(best);
  h->seeds_cost.swap(costlog);
  h->seeds_u.swap(tl);
  h->seeds_x.clear();                                            // (no state trajectory: MI_F_SEEDS_X_BAR answers MI_ILQR_E_BAD_ARG)
  return MI_ILQR_OK;
}

}  // namespace mi_host
