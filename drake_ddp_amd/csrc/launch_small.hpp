// Launch templates of the wave-per-problem kernels (ilqr_small.hpp); included by the k_<model>.hip units.
#pragma once
#include "host.hpp"
#include "ilqr_small.hpp"

namespace mi_host {
template <class M, int JAC, int MODE>
int launch_one(mi_ilqr* h, const KArgs& a) {
  auto kern = ilqr_small_kernel<M, JAC, MODE>;
  static bool lds_ok[kMaxDevices] = {};
  { const int rc = allow_max_lds(kern, lds_ok, h->d.device_id); if (rc != MI_ILQR_OK) return rc; }
  const int waves = (a.helpers > 0 && (MODE == MODE_SOLVE || MODE == MODE_MPC)) ? 1 + a.helpers : 1;
  return launch_timed(h, kern, dim3(h->B), dim3(64 * waves), h->lds, a);
}

// every kernel mode, in the handle's Jacobian mode
template <class M>
int launch_modes(mi_ilqr* h, int mode, const KArgs& a) {
  return with_jac(h, [&](auto jac) {
    return with_any_mode(mode, [&](auto md) { return launch_one<M, decltype(jac)::value, decltype(md)::value>(h, a); });
  });
}

// the modes that run a backward pass, for the model forms that only change that pass (ExactCost, LongHorizon): MODE_BACKWARD in its
// central-difference form only
template <class M>
int launch_backward_forms(mi_ilqr* h, int mode, const KArgs& a) {
  return with_mode<MODE_SOLVE, MODE_MPC, MODE_BACKWARD>(mode, [&](auto md) {
    constexpr int MODE = decltype(md)::value;
    if constexpr (MODE == MODE_BACKWARD) return launch_one<M, MI_JAC_FD_CENTRAL, MODE>(h, a);
    else return with_jac(h, [&](auto jac) { return launch_one<M, decltype(jac)::value, MODE>(h, a); });
  });
}

template <class M>
int launch_jac(mi_ilqr* h, int mode, const KArgs& a) {
  if constexpr (M::n >= 3 && M::n <= 4 && M::m == 1) {
    if (mode == MODE_SOLVE || mode == MODE_MPC || mode == MODE_BACKWARD) {
      // cost matrices outside the symmetric-PSD class: the kernels whose backward pass is the reference's recursion
      if (h->exact_backward) return launch_backward_forms<ExactCost<M>>(h, mode, a);
      // two or more steps per lane: the kernels whose backward pass is the time-parallel scan (ilqr_small.hpp: LongHorizon)
      if (h->N > 128) return launch_backward_forms<LongHorizon<M>>(h, mode, a);
    }
  }
  return launch_modes<M>(h, mode, a);
}

// Handles with control limits (mi_ilqr_set_control_limits): the Limited<M> kernels - sequential rollout with the clamp, the
// box-QP backward pass - for every mode.  Instantiated apart from launch_jac (k_<model>_lim.hip, the plugin units) so that
// the parallel build keeps its shape.
template <class M>
int launch_limited(mi_ilqr* h, int mode, const KArgs& a) { return launch_modes<Limited<M>>(h, mode, a); }

}  // namespace mi_host
