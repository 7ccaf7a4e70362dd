// What the host units of libmi_ilqr.so share (mi_ilqr.hip and the h_<concern>.hip units): declared once here, defined
// in the unit named above each group, all of it hidden from the dynamic symbol table.  Host units only: no k_*.hip unit, no
// launch_*.hpp, no family header and not the plugin template includes this header, and it includes no family header.
// The calls go one way: h_memory.hip calls nothing of the others; mi_ilqr.hip (the core) calls h_memory.hip, and of h_fields.hip the
// field table alone; h_policy.hip, h_mpc.hip, h_seeds.hip, h_mppi.hip and h_fit.hip call the core and h_memory.hip (the plant its policy's pack, the seeds
// its rule for the controls a launch starts from, and - the one call between two of them - h_seeds.hip hands the long form of its
// command to the loop in h_mpc.hip); h_fields.hip, the boundary's selectors, calls all of them.  h_comm.hip stands alone.
#pragma once
#include "host.hpp"
#include "mc_window.hpp"

namespace mi_host {

// ---- mi_ilqr.hip: the model table, the launch of a kernel mode, the lazily-zero state
// One record per model id: the plugin record (n, m, parameters and their defaults, family, LDS bytes, launch entry) - filled in
// for the built-in models by the table, by mi_ilqr_register_model for those registered at run time - and the clustering policy.
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
MI_INTERNAL const Model* model_of(int id);
MI_INTERNAL int launch(mi_ilqr* h, int mode);
MI_INTERNAL int materialize_zero_state(mi_ilqr* h);
MI_INTERNAL int materialize_u(mi_ilqr* h);
MI_INTERNAL int reduce_stats(mi_ilqr* h, int first_slot, int count);     // DevStats records of `count` ring slots: one launch
MI_INTERNAL int set_cost_rows(mi_ilqr* h, const double* src, size_t bytes);   // MI_F_COST_MATRICES (classified like mi_ilqr_set_cost's)

// Solve slots (host.hpp: SolveSlot).  Only mi_ilqr_solve_async puts a launch on the other slot, and only a cold
// MODE_SOLVE launch of the wave-per-problem kernels; only mi_ilqr_set_initial(_shared) writes on the other slot's stream.  Every
// other entry point that reads or writes solver state, or hands out a pointer or the stream, calls join_slots first: the current
// slot's stream then waits - on the device, never the host - for what the other slot's stream still holds, and the entry point
// works on the current slot as if there were one.  Two flag tests when there is nothing to join.
MI_INTERNAL int join_slots_now(mi_ilqr* h);
MI_INTERNAL inline int join_slots(mi_ilqr* h) { return (!h->other_pending && h->fork_needed) ? MI_ILQR_OK : join_slots_now(h); }
// ... and call this once the host has waited for the current stream behind a join: nothing of the handle is in flight
MI_INTERNAL inline void slots_idle(mi_ilqr* h) { h->inflight = 0; h->fork_needed = false; }
// An entry point that may WRITE x0 / u_guess in place (through the handle's aliases: kernels of the MPC, multi-start and sampling
// loops, mi_ilqr_set, a caller holding mi_ilqr_device_ptr's pointer): the copy the aliases name is the only one to vouch for.
MI_INTERNAL inline void inputs_touched(mi_ilqr* h) {
  h->in_x0.version[1 - h->in_x0.latest] = -1;
  h->in_u.version[1 - h->in_u.latest] = -1;
}
// The entry points that enqueue solves of their own (the MPC, multi-start and sampling loops) or launch behind the policy: joined,
// and every launch until the end of the scope stays on the current slot.
struct MI_INTERNAL SlotHold {
  explicit SlotHold(mi_ilqr* h_) : h(h_), rc(join_slots(h_)) { ++h->hold; inputs_touched(h); }
  ~SlotHold() { --h->hold; }
  SlotHold(const SlotHold&) = delete;
  SlotHold& operator=(const SlotHold&) = delete;
  mi_ilqr* h;
  int rc;
};

// costmat and its host mirror are Q | R | Qf | x_nom: the length of the matrices, and the shared x_nom (host mirror) behind them
MI_INTERNAL inline size_t cost_len(const mi_ilqr* h) { return 2 * (size_t)h->n * h->n + (size_t)h->m * h->m; }
MI_INTERNAL inline const double* shared_x_nom(const mi_ilqr* h) { return h->h_costmat.data() + cost_len(h); }
// the controls the caller sees: m_user .. m - 1 are padding (a model without padding declares 0)
MI_INTERNAL inline int32_t device_m_user(const Model* model, const mi_ilqr* h) { return model->p.m_user > 0 ? model->p.m_user : (int32_t)h->m; }
constexpr double kRefClockEnd = 0x1p30;       // clocks and reference lengths stay below: row indices are 32-bit in the kernels

// One block of the handle's grow-only scratch carved into arrays: offsets in doubles, every array on a 32-double boundary.
struct MI_INTERNAL ScratchPlan {
  size_t take(size_t count) { const size_t o = off; off += (count + 31) & ~(size_t)31; return o; }
  size_t bytes() const { return off * 8; }
  size_t off = 0;
};

// ---- h_memory.hip: the owner of device memory, the layout conversions, the RowStore protocol
// The handle's device memory: every allocation is recorded in h->owned, which is what mi_ilqr_destroy frees - a buffer allocated on
// first use, or by a create that fails half-way, needs no line of its own there.  dev_free releases one early (buffers that are re-grown).
MI_INTERNAL int dev_alloc_bytes(mi_ilqr* h, void** p, size_t bytes, bool zero);
MI_INTERNAL int dev_free_ptr(mi_ilqr* h, void* p);
template <class T>
MI_INTERNAL int dev_alloc(mi_ilqr* h, T*& p, size_t count, bool zero = false) {
  void* q = nullptr;
  const int rc = dev_alloc_bytes(h, &q, count * sizeof(T), zero);
  if (rc == MI_ILQR_OK) p = static_cast<T*>(q);
  return rc;
}
template <class T>
MI_INTERNAL int dev_free(mi_ilqr* h, T*& p) {
  void* q = p;
  p = nullptr;
  return dev_free_ptr(h, q);
}
MI_INTERNAL int ensure_scratch(mi_ilqr* h, size_t bytes);
MI_INTERNAL int stage_h2d(mi_ilqr* h, void* dst, const void* src, size_t bytes);

// Layouts of a (B, rows, len) trajectory array: TL time-last [b][row][t] (the reference's, SURVEY F5 - what
// crosses the C ABI); TM time-major [b][t][row] (workgroup-per-problem kernels); BM batch-minor
// [t][row][b] (lane-per-problem kernels).  The conversions run on the DEVICE, between the field and a
// staging buffer; the host copy is then one linear transfer.
enum { LAYOUT_TL = 0, LAYOUT_TM = 1, LAYOUT_BM = 2 };
MI_INTERNAL inline int layout_of(const mi_ilqr* h) { return h->batch_minor ? LAYOUT_BM : (h->large ? LAYOUT_TM : LAYOUT_TL); }
MI_INTERNAL bool needs_relayout(const mi_ilqr* h, int which, int* rows, int* len);
MI_INTERNAL int relayout(mi_ilqr* h, const double* src, double* dst, int rows, int len, bool to_kernel_layout);
MI_INTERNAL int broadcast_u(mi_ilqr* h, const double* one, double* dst);
MI_INTERNAL int transpose_tiles(mi_ilqr* h, const double* src, double* dst, int R, int C, size_t outer, int inner, size_t src_outer,
                                size_t src_inner, size_t src_r, size_t dst_outer, size_t dst_inner, size_t dst_c);

MI_INTERNAL void store_drop(RowStore& s);
MI_INTERNAL int store_upload(mi_ilqr* h, RowStore& s, const double* src);
MI_INTERNAL int store_upload_broadcast(mi_ilqr* h, RowStore& s, const double* row);
MI_INTERNAL int store_read(const mi_ilqr* h, const RowStore& s, const double* shared_row, double* dst, size_t bytes);
// The selectors of mi_ilqr_get / mi_ilqr_device_ptr that are per-problem arrays: the store, and the row every problem reports in shared mode
struct RowField { RowStore* store; const double* shared_row; };
MI_INTERNAL RowField row_field(mi_ilqr* h, int which);
MI_INTERNAL int refresh_lane_target_rows(mi_ilqr* h);
MI_INTERNAL void drop_per_problem_targets(mi_ilqr* h);
MI_INTERNAL int upload_target_rows(mi_ilqr* h, RowStore& s, const double* src);
// the opening every per-problem setter shares: src == NULL with bytes == 0 drops the rows (MI_ILQR_OK), then the size
// (MI_ILQR_E_BAD_SHAPE) before the pointer (MI_ILQR_E_BAD_ARG); kRowsGiven: `cnt` doubles are there, the setter's own checks follow
constexpr int kRowsGiven = 1;
MI_INTERNAL inline int rows_given(RowStore& s, const double* src, size_t bytes, size_t cnt) {
  if (!src && bytes == 0) { store_drop(s); return MI_ILQR_OK; }
  if (bytes != cnt * 8) return MI_ILQR_E_BAD_SHAPE;
  return src ? kRowsGiven : MI_ILQR_E_BAD_ARG;
}

// ---- h_fields.hip: the table of the selectors that are plain device arrays
struct Field { void* ptr; size_t bytes; bool is_int; };
MI_INTERNAL Field field_of(mi_ilqr* h, int which);
MI_INTERNAL bool prefix_ok(int which, size_t bytes, size_t field_bytes);

// ---- h_policy.hip: the policy as the handle holds it now, the Monte-Carlo selectors of mi_ilqr_set
// pack_policy: the first `steps` rows t of x_bar_t | u_bar_t | K_t (W = n + m + m n doubles) gathered from the handle's kernel
// layout into dst, (B, steps, W) or (steps, W, B) - nothing of the handle is written
enum { PACK_TIME_MAJOR = 0, PACK_PROBLEM_MINOR = 1 };
// sel != nullptr (the (G, 3) selection rows of multi-start, on the device): G = B / K columns, column g the policy of its group's winner
MI_INTERNAL int pack_policy(mi_ilqr* h, double* dst, int steps, int order, const double* sel = nullptr, int K = 1);
MI_INTERNAL const double* policy_u_source(const mi_ilqr* h);      // the controls the next launch would start from; nullptr: zeros
// the rollout kernels' arguments that come from the handle (every per-problem array or the shared row, bounds, noise, dt, N, B, m_user)
MI_INTERNAL int fill_policy_args(mi_ilqr* h, const Model* model, const double* policy, double* prow_scratch, PolicyArgs& a);
MI_INTERNAL int set_mc_dist(mi_ilqr* h, const double* src, size_t bytes);
MI_INTERNAL int set_mc_box(mi_ilqr* h, const double* src, size_t bytes);
MI_INTERNAL int set_mc_observe(mi_ilqr* h, const double* src, size_t bytes);
MI_INTERNAL int run_policy_mc(mi_ilqr* h, const double* v, size_t bytes);

// ---- h_seeds.hip: multi-start (MI_F_SEEDS_*) - the sigma rows, the command and what the read-only selectors return
MI_INTERNAL int set_seeds_sigma(mi_ilqr* h, const double* src, size_t bytes);
MI_INTERNAL int run_seeds(mi_ilqr* h, const double* v, size_t bytes);
constexpr int kNotSeedsField = 1;
MI_INTERNAL int get_seeds_field(mi_ilqr* h, int which, double* dst, size_t bytes);

// ---- h_mppi.hip: the sampling form of MI_F_SEEDS_RUN (10 doubles), which h_seeds.hip hands over before it looks at anything else
MI_INTERNAL int run_mppi(mi_ilqr* h, const double* v);

// ---- h_fit.hip: parameter identification (MI_F_FIT_*) - the setters and the command behind mi_ilqr_set, the results behind
// mi_ilqr_get; kNotFitField for every other selector.  Calls the core (the model table) and h_memory.hip, like h_mppi.hip.
constexpr int kNotFitField = 1;
MI_INTERNAL int set_fit_field(mi_ilqr* h, int which, const double* src, size_t bytes);
MI_INTERNAL int get_fit_field(mi_ilqr* h, int which, double* dst, size_t bytes);

// ---- h_mpc.hip: mi_ilqr_get of the plant's and the reference's selectors; kNotPlantField for every other one
constexpr int kNotPlantField = 1;
MI_INTERNAL int get_plant_field(mi_ilqr* h, int which, double* dst, size_t bytes);
// ... and the receding-horizon loop with the seeds of a group joined between its re-solves: the long form of MI_F_SEEDS_RUN, which
// h_seeds.hip validates and hands over (the loop belongs to the unit that owns the MPC log and the targets' clocks).  On success
// `best` holds the (num_resolves + 1, G, 3) selection log and `join_ms` the join kernels' events, summed.
struct SeedsMpcRun { int32_t K = 0, hold = 1, num_resolves = 0, replan_steps = 0; unsigned long long seed = 0; uint32_t round = 0; };
MI_INTERNAL int mpc_run_seeds(mi_ilqr* h, const SeedsMpcRun& r, std::vector<double>& best, double& join_ms);

}  // namespace mi_host
