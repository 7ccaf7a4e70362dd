// libmi_ilqr.so, host side - the receding-horizon loop: the shift between re-solves, mi_ilqr_mpc_run in its host-loop and
// single-launch forms with its log, the plant of the closed loop (plant_advance.hpp) with what mi_ilqr_get reads of it, and the
// host loop with the seeds of a group joined between its re-solves (mpc_run_seeds: the long form of MI_F_SEEDS_RUN).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "host_internal.hpp"
#include "lds_layout.hpp"    // kLargeThreads

using namespace mi;
using namespace mi_host;

namespace {     // the kernels: global, like every kernel of the host units - a name does not change with the unit

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

// The closed loop's plant (plant_advance.hpp: a lane is a problem) reads everything PROBLEM-MINOR, element e of problem b at
// e * B + b: the policy's first columns (h_policy.hip: pack_policy), and through rows_to_cols_kernel a per-problem array, `width`
// doubles of problem b at src + b * stride (stride 0: one row for every problem), as (width, B)
__global__ void __launch_bounds__(256) rows_to_cols_kernel(const double* __restrict__ src, size_t stride, double* __restrict__ dst,
                                                             int width, int B) {
  const size_t total = (size_t)width * B;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t k = e / B, b = e - k * B;
    dst[e] = src[b * stride + k];
  }
}

// `width` doubles of row g at src + g * stride -> dst (G, width) dense: the groups' plants out of member 0's rows
__global__ void __launch_bounds__(256) gather_rows_kernel(const double* __restrict__ src, size_t stride, double* __restrict__ dst, int width, int G) {
  const size_t total = (size_t)width * G;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t g = e / width, i = e - g * width;
    dst[e] = src[g * stride + i];
  }
}

// the grouped plant log (rows, G) -> the (rows, B) one the selector reads: every member reports its group's plant
__global__ void __launch_bounds__(256) expand_cols_kernel(const double* __restrict__ src, double* __restrict__ dst, size_t rows, int B, int K) {
  const size_t total = rows * (size_t)B, G = (size_t)(B / K);
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t r = e / B, b = e - r * B;
    dst[e] = src[r * G + b / K];
  }
}

// x0 <- the plants' states, on the device (dst may be the mapped host block of a tiny batch: host.hpp, host_inputs)
__global__ void __launch_bounds__(256) copy_doubles_kernel(const double* __restrict__ src, double* __restrict__ dst, size_t count) {
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < count; e += (size_t)gridDim.x * 256) dst[e] = src[e];
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

}  // namespace

namespace mi_host {

namespace {

// mpc_run with per-problem targets: every row moves by its own step, once per re-solve - fp64 repeated addition, what the kernels do
int advance_per_problem_targets(mi_ilqr* h, int32_t times) {
  std::vector<double> rows = h->targets.mirror;
  for (int32_t r = 0; r < times; ++r)
    for (size_t i = 0; i < rows.size(); ++i) rows[i] += h->target_steps.mirror[i];
  return upload_target_rows(h, h->targets, rows.data());
}

// The closed loop's plant (a handle that holds MI_F_PLANT_STATE), the part of a mi_ilqr_mpc_run that does not change from one
// re-solve to the next, staged problem-minor in the handle's scratch: the plants' parameters, Q | R, the bounds, the sigmas.
// Offsets in doubles; `pol` and `x_nom` are filled before every launch (plant_advance).
// Grouped (the long form of MI_F_SEEDS_RUN, K members per group, one plant per group - member 0's): everything is staged for G = B / K
// columns, column g from problem g K; gx / gdead / gmdead: the plants' compact (G, n) states and (G,) flags, glog: the run's log
// (rows, n + m + 1, G) behind the (rows, n + m + 1, B) one the selector reads.
struct PlantStage { size_t pol, prm, prow, cost, x_nom, ulim, noise, gx = 0, gdead = 0, gmdead = 0; int K = 1; double* glog = nullptr; };

int rows_to_cols(mi_ilqr* h, const double* src, size_t stride, double* dst, size_t width, size_t cols = 0) {
  if (cols == 0) cols = (size_t)h->B;             // (grouped plants: G columns, column g from member 0's row - stride K x the row width)
  const size_t total = width * cols;
  if (total == 0) return MI_ILQR_OK;
  hipLaunchKernelGGL(rows_to_cols_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 8192)), dim3(256), 0, h->stream, src, stride, dst,
                     (int)width, (int)cols);
  HIPCHK(hipGetLastError());
  return MI_ILQR_OK;
}

int plant_prepare(mi_ilqr* h, int32_t num_resolves, int32_t replan_steps, PlantStage* st, int K = 0) {
  const Model* model = model_of(h->d.model_id);
  const bool grouped = K > 0;
  const size_t gk = grouped ? (size_t)K : 1, B = (size_t)h->B / gk, n = h->n, m = h->m, np = model->p.n_params, W = n + m + m * n, C = n + m + 1;
  ScratchPlan plan;
  st->pol = plan.take((size_t)replan_steps * W * B); st->prm = plan.take(np * B); st->prow = plan.take(np); st->cost = plan.take((n * n + m * m) * B);
  st->x_nom = plan.take(n * B); st->ulim = plan.take(2 * m * B); st->noise = plan.take((n + m) * B);
  st->K = (int)gk;
  if (grouped) { st->gx = plan.take(n * B); st->gdead = plan.take(B); st->gmdead = plan.take(B); }
  int rc = ensure_scratch(h, plan.bytes());
  if (rc != MI_ILQR_OK) return rc;
  const size_t need = (size_t)num_resolves * replan_steps * C * (grouped ? (size_t)h->B + B : B);
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
    if (own.synced) rc = rows_to_cols(h, own.rows, np * gk, sc + st->prm, np, B);
    else if ((rc = stage_h2d(h, sc + st->prow, h->d.model_params, np * 8)) == MI_ILQR_OK) rc = rows_to_cols(h, sc + st->prow, 0, sc + st->prm, np, B);
    if (rc != MI_ILQR_OK) return rc;
  }
  if ((rc = rows_to_cols(h, h->costs.synced ? h->costs.rows : h->costmat, h->costs.synced ? h->costs.width * gk : 0, sc + st->cost, n * n + m * m, B)) != MI_ILQR_OK) return rc;
  if (h->limited && (rc = rows_to_cols(h, h->ulim, 2 * m * gk, sc + st->ulim, 2 * m, B)) != MI_ILQR_OK) return rc;
  if (h->plant_noise.synced && (rc = rows_to_cols(h, h->plant_noise.rows, (n + m) * gk, sc + st->noise, n + m, B)) != MI_ILQR_OK) return rc;
  if (grouped) {                                 // the groups' plants: member 0's state and flag, compact (a (G, w) gather is rows_to_cols of w = 1 .. per row)
    st->glog = h->plant_log + (size_t)num_resolves * replan_steps * C * (size_t)h->B;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)std::min<size_t>((n * B + 255) / 256, 1024)), dim3(256), 0, h->stream, h->plant_state.rows,
                       n * gk, sc + st->gx, (int)n, (int)B);
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)std::min<size_t>((B + 255) / 256, 1024)), dim3(256), 0, h->stream, h->plant_dead, gk, sc + st->gdead,
                       1, (int)B);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(sc + st->gmdead, 0, B * 8, h->stream));
  }
  return MI_ILQR_OK;
}

// Step 1 of a closed-loop round: the plants advance `replan_steps` steps under the policy the handle holds now (a cold handle's x_bar
// and K read as zeros, a reset one's u_bar too, a pending guess is read from where it waits), with the target the plan was solved for.
int plant_advance(mi_ilqr* h, const PlantStage& st, int32_t round, int32_t replan_steps, double* mpc_dead, const double* sel = nullptr) {
  const Model* model = model_of(h->d.model_id);
  const bool grouped = sel != nullptr;           // (G lanes on the compact arrays, each under its group's winner's policy)
  const size_t gk = (size_t)st.K, B = (size_t)h->B / gk, n = h->n, m = h->m, C = n + m + 1;
  double* const sc = h->scratch;
  int rc = pack_policy(h, sc + st.pol, replan_steps, PACK_PROBLEM_MINOR, sel, st.K);
  if (rc != MI_ILQR_OK) return rc;
  rc = rows_to_cols(h, h->targets.synced ? h->targets.rows : h->costmat + cost_len(h), h->targets.synced ? n * gk : 0, sc + st.x_nom, n, B);
  if (rc != MI_ILQR_OK) return rc;
  PlantArgs a{};
  a.policy = sc + st.pol; a.params = sc + st.prm; a.cost = sc + st.cost; a.x_nom = sc + st.x_nom;
  a.ulim = h->limited ? sc + st.ulim : nullptr;
  a.noise = h->plant_noise.synced ? sc + st.noise : nullptr;
  a.x = h->plant_state.rows; a.dead = h->plant_dead; a.mpc_dead = mpc_dead;
  a.log = h->plant_log + (size_t)round * replan_steps * C * B;
  if (grouped) { a.x = sc + st.gx; a.dead = sc + st.gdead; a.mpc_dead = sc + st.gmdead; a.log = st.glog + (size_t)round * replan_steps * C * B; }
  a.dt = h->d.dt; a.seed = h->plant_seed;
  a.clock = (uint32_t)(h->plant_clock + (unsigned long long)round * (unsigned long long)replan_steps);
  a.B = (int32_t)B; a.steps = replan_steps; a.m_user = device_m_user(model, h);
  a.feedback = h->plant_feedback ? 1 : 0; a.common = h->plant_common ? 1 : 0;
  return model->p.launch(h, kModePlantAdvance, &a);
}

// (re)allocate the MPC log for `num_resolves` rows per problem - grow-only, the `dead` flags behind it - and zero it: rows a problem
// never reaches read as zeros.  The same steps as the block at the top of mi_ilqr_mpc_run, which keeps its own copy (that function
// is left as it was): a change to the log's layout or to the `dead` flags behind it goes into BOTH.
int mpc_log_begin(mi_ilqr* h, int32_t num_resolves, double** dead) {
  int rc;
  if (h->mpc_log_resolves < num_resolves) {
    HIPCHK(hipStreamSynchronize(h->stream));
    h->mpc_log_resolves = 0;
    if ((rc = dev_free(h, h->mpc_log)) != MI_ILQR_OK) return rc;
    if ((rc = dev_alloc(h, h->mpc_log, (size_t)h->B * num_resolves * (h->n + 2) + h->B)) != MI_ILQR_OK) return rc;
    h->mpc_log_resolves = num_resolves;
  }
  *dead = h->mpc_log + (size_t)h->B * h->mpc_log_resolves * (h->n + 2);
  HIPCHK(hipMemsetAsync(h->mpc_log, 0, ((size_t)h->B * h->mpc_log_resolves * (h->n + 2) + h->B) * 8, h->stream));
  return MI_ILQR_OK;
}

}  // namespace

// The long form of MI_F_SEEDS_RUN (include/mi_ilqr.h: "Multi-start in the receding-horizon loop"): num_resolves x { join the seeds of
// every group - one launch of seeds_mpc_join_kernel: select, the shifted winner and its predicted state to every member -; move the
// targets; solve; log }, then one more select.  The host-loop form of mi_ilqr_mpc_run with the join in the place of the shift; that
// function itself is untouched.  K > 1: a member starts from another problem's plan, so its own gains and nominal trajectory mean
// nothing to it and the re-solve is COLD from the guess, as after the short form's reseed.  K = 1: every member continues its own
// plan and the re-solve is warm - the loop is bitwise mi_ilqr_mpc_shift + mi_ilqr_solve.  With a plant: one plant per group, advanced
// under the winner's policy between a select of its own and the join (plant_prepare / plant_advance, grouped).
int mpc_run_seeds(mi_ilqr* h, const SeedsMpcRun& r, std::vector<double>& best, double& join_ms) {
  const int32_t R = r.num_resolves, rp = r.replan_steps;
  if (h->cold) return MI_ILQR_E_BAD_ARG;          // nothing solved: no cost, no status and no plan to select on
  const bool plant = h->plant_state.synced;       // the closed loop: one plant per group, member 0's, under the winner's policy
  if (plant && h->reference.synced) return MI_ILQR_E_UNSUPPORTED;   // (the plant kernels know constant targets only)
  if (plant && h->plant_clock + (unsigned long long)R * (unsigned long long)rp > 0x100000000ull) return MI_ILQR_E_BAD_ARG;   // (the step counter is 32 bits)
  if ((double)r.round + (double)R > 0x1p32) return MI_ILQR_E_BAD_ARG;   // (round + r is the 32-bit counter word of re-solve r)
  const bool tracking = h->reference.synced;
  if (tracking && (double)h->ref_clock + (double)R * (double)rp >= kRefClockEnd) return MI_ILQR_E_BAD_ARG;
  HIPCHK(hipSetDevice(h->d.device_id));
  const size_t B = h->B, G = B / (size_t)r.K, rows = ((size_t)R + 1) * G * 3;
  int rc;
  if (h->seeds_log_cap < rows) {                  // grow-only
    HIPCHK(hipStreamSynchronize(h->stream));
    h->seeds_log_cap = 0;
    if ((rc = dev_free(h, h->seeds_log_dev)) != MI_ILQR_OK) return rc;
    if ((rc = dev_alloc(h, h->seeds_log_dev, rows)) != MI_ILQR_OK) return rc;
    h->seeds_log_cap = rows;
  }
  if (!h->seeds_ev0) {
    HIPCHK(hipEventCreate(&h->seeds_ev0));
    HIPCHK(hipEventCreate(&h->seeds_ev1));
  }
  double* mpc_dead = nullptr;
  if ((rc = mpc_log_begin(h, R, &mpc_dead)) != MI_ILQR_OK) return rc;
  h->mpc_resolves = R; h->mpc_replan = rp;        // (up front: a failing re-solve must not leave the log's shape stale)
  const long long clock0 = h->ref_clock;         // (a run that fails leaves the reference's clock where it was)
  double ms_sum = 0.0;
  PlantStage stage{};
  const size_t n = h->n, C = n + h->m + 1;
  if (plant) {
    if ((rc = plant_prepare(h, R, rp, &stage, r.K)) != MI_ILQR_OK) return rc;
    h->plant_log_rows = 0; h->plant_ms = 0.0;
  }
  SeedsJoinArgs a{};
  a.u_bar = h->u_bar; a.x_bar = h->x_bar; a.u_guess = h->u_guess; a.x0 = h->x0;
  a.cost = h->cost; a.status = h->status; a.mpc_dead = mpc_dead;
  a.seed = r.seed;
  a.B = (int32_t)B; a.K = r.K; a.n = h->n; a.m = h->m; a.m_user = device_m_user(model_of(h->d.model_id), h);
  a.N = h->N; a.layout = layout_of(h); a.hold = r.hold; a.replan = rp;
  a.ev0 = h->seeds_ev0; a.ev1 = h->seeds_ev1;
  for (int32_t i = 0; i < R; ++i) {
    if ((rc = materialize_u(h)) != MI_ILQR_OK) { h->ref_clock = clock0; return rc; }   // a pending guess is the plan: source u_bar, destination u_guess
    a.sigma = h->seeds_sigma.synced ? h->seeds_sigma.rows : nullptr;
    a.cost = h->cost; a.status = h->status;       // (the last solve's slot of the statistics ring)
    a.best = h->seeds_log_dev + (size_t)i * G * 3;
    a.round = r.round + (uint32_t)i;
    if (plant) {
      // the selection first, on its own (the join repeats it: the same costs and statuses, the same row), then the groups' plants
      // advance under their winners' policies - a group without a winner under member 0's - with the target the plan was solved for
      SeedsArgs s{};
      s.cost = h->cost; s.status = h->status; s.best = a.best;
      s.B = (int32_t)B; s.K = r.K; s.n = h->n; s.m = h->m; s.m_user = a.m_user; s.N = h->N; s.layout = a.layout; s.op = SEEDS_SELECT; s.hold = 1;
      if ((rc = launch_seeds(h, s)) != MI_ILQR_OK) return rc;
      if ((rc = plant_advance(h, stage, i, rp, nullptr, a.best)) != MI_ILQR_OK) return rc;
      a.plant_x = h->scratch + stage.gx; a.plant_ended = h->scratch + stage.gdead;
      a.plant_rows = h->plant_state.rows; a.plant_dead = h->plant_dead;
    }
    if ((rc = launch_seeds_mpc_join(h, a)) != MI_ILQR_OK) { h->ref_clock = clock0; return rc; }
    if (r.K > 1) h->cold = true;
    h->u_pending = true;
    h->u_zero = false;
    // (per-problem targets under a reference are kept but ignored: they do not move either)
    if (h->targets.synced && !tracking && (rc = advance_per_problem_targets(h, 1)) != MI_ILQR_OK) { h->ref_clock = clock0; return rc; }
    if (tracking) h->ref_clock += rp;
    if ((rc = mi_ilqr_solve(h, nullptr)) != MI_ILQR_OK) { h->ref_clock = clock0; return rc; }
    hipLaunchKernelGGL(mpc_log_fill_kernel, dim3((h->B + 255) / 256), dim3(256), 0, h->stream, h->x0, h->cost, h->iters, h->status, h->mpc_log,
                       mpc_dead, h->B, h->n, R, i);
    HIPCHK(hipGetLastError());
    float ms = 0.0f;                              // (mi_ilqr_solve has synchronized: the join kernel's events are complete)
    HIPCHK(hipEventElapsedTime(&ms, h->seeds_ev0, h->seeds_ev1));
    ms_sum += (double)ms;
    if (plant) {
      HIPCHK(hipEventElapsedTime(&ms, h->plant_ev0, h->plant_ev1));
      h->plant_ms += (double)ms;
    }
  }
  if (plant) {                                    // the log every member reads, the clock and the host mirror of the states follow the plants
    const size_t lrows = (size_t)R * rp * C, cnt = lrows * B;
    hipLaunchKernelGGL(expand_cols_kernel, dim3((unsigned)std::min<size_t>((cnt + 255) / 256, 8192)), dim3(256), 0, h->stream, stage.glog, h->plant_log,
                       lrows, (int)B, r.K);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h->plant_state.mirror.data(), h->plant_state.rows, B * n * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->plant_clock += (unsigned long long)R * (unsigned long long)rp;
    h->plant_log_rows = R * rp;
  }
  SeedsArgs s{};                                  // row R: the selection on the last re-solve
  s.cost = h->cost; s.status = h->status; s.best = h->seeds_log_dev + (size_t)R * G * 3;
  s.B = (int32_t)B; s.K = r.K; s.n = h->n; s.m = h->m; s.m_user = a.m_user; s.N = h->N; s.layout = a.layout; s.op = SEEDS_SELECT; s.hold = 1;
  if ((rc = launch_seeds(h, s)) != MI_ILQR_OK) return rc;
  std::vector<double> log(rows);
  HIPCHK(hipMemcpyAsync(log.data(), h->seeds_log_dev, rows * 8, hipMemcpyDeviceToHost, h->stream));
  if (hipStreamSynchronize(h->stream) != hipSuccess) { (void)hipDeviceSynchronize(); return MI_ILQR_E_HIP; }   // (a copy into a local was queued)
  best.swap(log);
  join_ms = ms_sum;
  return MI_ILQR_OK;
}

// mi_ilqr_get of the plant's selectors that are not plain mirrors (and of the reference trajectory's two: a (B, T, n) mirror whose
// length is its own, and the clock); kNotPlantField for every other selector
int get_plant_field(mi_ilqr* h, int which, double* dst, size_t bytes) {
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

}  // namespace mi_host

extern "C" {

int mi_ilqr_mpc_shift(mi_ilqr_t* h, int32_t replan_steps) {
  if (!h) return MI_ILQR_E_BAD_ARG;
  if (replan_steps < 1 || replan_steps >= h->N - 1) return MI_ILQR_E_BAD_ARG;
  HIPCHK(hipSetDevice(h->d.device_id));
  const SlotHold hold(h);            // (solve slots: joined, and every launch below stays on the current one)
  if (hold.rc != MI_ILQR_OK) return hold.rc;
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

int mi_ilqr_mpc_run(mi_ilqr_t* h, int32_t num_resolves, int32_t replan_steps, const double* target_step, mi_ilqr_stats* stats) {
  if (!h) return MI_ILQR_E_BAD_ARG;
  if (num_resolves < 1 || replan_steps < 1 || replan_steps >= h->N - 1) return MI_ILQR_E_BAD_ARG;
  const SlotHold hold(h);            // (solve slots: joined, and every launch below stays on the current one)
  if (hold.rc != MI_ILQR_OK) return hold.rc;
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
  if (!stats_in_kernel(h) && (rc = reduce_stats(h, h->cur_slot, 1)) != MI_ILQR_OK) return rc;
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
  { const int rc = join_slots(h); if (rc != MI_ILQR_OK) return rc; }
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(dst, h->mpc_log, bytes, hipMemcpyDeviceToHost));
  return MI_ILQR_OK;
}

}  // extern "C"
