// Launch templates of the lane-per-problem ("throughput") kernels (ilqr_batch.hpp); included by k_batch.hip (built-in
// small-state models) and by the family-0 plugin units (drake_ddp_amd/plugin.py).
#pragma once
#include "host.hpp"
#include "ilqr_batch.hpp"

namespace mi_host {
template <class M, int JAC, bool KP, bool PT, bool PP, bool PC = false>
int launch_batch_one(mi_ilqr* h, const KArgs& a) {
  return launch_timed(h, ilqr_batch_kernel<M, JAC, KP, PT, PP, PC>, dim3((h->B + 63) / 64), dim3(64), 0, a);
}

// per-problem model parameters (KArgs::param_cols): PP instantiations
template <class M, int JAC, bool KP, bool PT>
int launch_batch_pp(mi_ilqr* h, const KArgs& a) {
  if (a.param_cols != nullptr) return launch_batch_one<M, JAC, KP, PT, true>(h, a);
  return launch_batch_one<M, JAC, KP, PT, false>(h, a);
}

// per-problem cost matrices (KArgs::cost_cols): PC instantiations.  Always with PT - make_args gives such a launch target rows in
// any case (the shared target broadcast when the handle has none of its own) - so PC adds two kernels per (JAC, KP), not four.
template <class M, int JAC, bool KP>
int launch_batch_pc(mi_ilqr* h, const KArgs& a) {
  if (a.x_nom_rows == nullptr) return MI_ILQR_E_BAD_ARG;     // (make_args always pairs the two)
  if (a.param_cols != nullptr) return launch_batch_one<M, JAC, KP, true, true, true>(h, a);
  return launch_batch_one<M, JAC, KP, true, false, true>(h, a);
}

template <class M>
int launch_batch(mi_ilqr* h, int mode, const KArgs& a) {
  if (mode != MODE_SOLVE) return MI_ILQR_E_UNSUPPORTED;    // stage-level entries: latency kernels only
  // key-point configurations other than setInterval / 1 (KArgs::bm_scratch), per-problem targets (KArgs::x_nom_rows), per-problem
  // model parameters (KArgs::param_cols) and per-problem cost matrices (KArgs::cost_cols) take instantiations of their own: the
  // regular kernels' code does not change
  return with_jac(h, [&](auto jac) {
    constexpr int JAC = decltype(jac)::value;
    const bool kp = a.bm_scratch != nullptr;
    if (a.cost_cols != nullptr) return kp ? launch_batch_pc<M, JAC, true>(h, a) : launch_batch_pc<M, JAC, false>(h, a);
    if (a.x_nom_rows != nullptr) return kp ? launch_batch_pp<M, JAC, true, true>(h, a) : launch_batch_pp<M, JAC, false, true>(h, a);
    return kp ? launch_batch_pp<M, JAC, true, false>(h, a) : launch_batch_pp<M, JAC, false, false>(h, a);
  });
}

// Handles with control limits: the Limited<M> lane-per-problem kernels (k_batch_lim.hip, the plugin units).
template <class M>
int launch_batch_limited(mi_ilqr* h, int mode, const KArgs& a) { return launch_batch<Limited<M>>(h, mode, a); }

}  // namespace mi_host
