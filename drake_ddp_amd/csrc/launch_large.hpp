// Launch templates of the workgroup-per-problem kernels (ilqr_large.hpp); included by the k_<model>.hip units.
#pragma once
#include "host.hpp"
#include "ilqr_large.hpp"

namespace mi_host {
template <class M, int JAC, int MODE, bool PIV = false>
int launch_one_large(mi_ilqr* h, const KArgs& a) {
  auto kern = ilqr_large_kernel<M, JAC, MODE, PIV>;
  static bool lds_ok[kMaxDevices] = {};
  { const int rc = allow_max_lds(kern, lds_ok, h->d.device_id); if (rc != MI_ILQR_OK) return rc; }
  const int cluster = (MODE == MODE_SOLVE || MODE == MODE_MPC) ? (a.cluster & 0xff) : 1;
  if (MODE == MODE_SOLVE || MODE == MODE_MPC) h->last_clustered = cluster > 1;
  if (cluster > 1) HIPCHK(hipMemsetAsync(h->cluster_sync, 0, (size_t)h->B * kSyncWords * sizeof(unsigned long long), h->stream));
  // clusters: 8 G ceil(B / 8) workgroups, a cluster's members congruent mod 8 = on one XCD (ilqr_large_kernel: XCD-aware placement)
  const unsigned grid = cluster > 1 ? (((a.cluster >> 8) & 3) ? 8u * (unsigned)cluster * (unsigned)((h->B + 7) / 8) : (unsigned)(h->B * cluster)) : (unsigned)h->B;
  return launch_timed(h, kern, dim3(grid), dim3(kLargeThreads), h->lds, a);
}

// Which models get BOTH forms of the kernels with a backward pass (ilqr_large.hpp: PIV) - with and without the pivoted-inverse cold
// path: those that declare kPivSplit (models.hpp: Synth36, Quad3D, PlanarQuad).  Same-box A/B, cycles per iteration of the bench's
// MPC loops without | with the ~150 cold instructions in the kernel: 36-state chain 429 k | 451 k (its LINE SEARCH 74 k | 85 k - the
// register allocation of the phases around the backward pass, not the pass), 3-D quadruped 682 k | 695 k, planar quadruped + 2.5 %
// it/s without.  The default (on_indefinite = 0, symmetric costs) is what the benchmarks run, so these get the lean form for it.
// Every other model keeps the ONE form that carries the path: the arm + ball is no faster without it (130 k | 134 k cycles per
// trial the other way round), plugin models would pay twice the kernels per build - the (34, 12) chain's lean form does not even
// compile with this hipcc ("Illegal instruction detected: V_CMP_NE_U32 0, $src_shared_base").
// The planar quadruped's lean MPC kernel was MISCOMPILED when it was first built (round 5, first session: another x_1 from bitwise
// the same x_0, u_0, non-deterministically; eight tests of the GPU suite caught it) and left out; the round's last session found
// the mechanism of this hipcc's miscompiles of these kernels (a VGPR spill copy placed in a zero-EXEC block prologue: DESIGN
// section 8, tools/check_exec_spill.py), rebuilt the form on the current sources - the checker finds no such site in it, the
// 50 planar-quadruped tests of the GPU suite pass on it - and adopted it.
template <class M>
constexpr bool kPivSplit = HasPivSplit<M>::value;

template <class M, int JAC, bool PIV, int... MODES>
int launch_large_modes(mi_ilqr* h, int mode, const KArgs& a) {
  return with_mode<MODES...>(mode, [&](auto md) { return launch_one_large<M, JAC, decltype(md)::value, PIV>(h, a); });
}

template <class M>
int launch_jac_large(mi_ilqr* h, int mode, const KArgs& a) {
  const bool backward = mode == MODE_SOLVE || mode == MODE_BACKWARD || mode == MODE_MPC;
  const bool piv = a.pd_continue || a.cost_asym || !kPivSplit<M>;
  return with_jac(h, [&](auto jac) {
    constexpr int JAC = decltype(jac)::value;
    if (backward && piv) return launch_large_modes<M, JAC, true, MODE_SOLVE, MODE_BACKWARD, MODE_MPC>(h, mode, a);
    if constexpr (kPivSplit<M>) if (backward) return launch_large_modes<M, JAC, false, MODE_SOLVE, MODE_BACKWARD, MODE_MPC>(h, mode, a);
    return launch_large_modes<M, JAC, false, MODE_ROLLOUT, MODE_FORWARD, MODE_LINEARIZE>(h, mode, a);
  });
}

// Handles with control limits (mi_ilqr_set_control_limits; the mid-size family, n <= 32): the Limited<M> kernels - the clamped
// rollouts and the box-QP backward pass (mid_backward_limited) - for every mode.  The backward pass has no pivoted-inverse path, so
// there is one form (PIV = false).  Instantiated apart from launch_jac_large (k_<model>_lim.hip, the plugin units built with limits).
template <class M>
int launch_jac_large_limited(mi_ilqr* h, int mode, const KArgs& a) {
  static_assert(LLay<M::n, M::m>::kMid, "control limits: the mid-size family only");
  return with_jac(h, [&](auto jac) {
    return launch_large_modes<Limited<M>, decltype(jac)::value, false, MODE_SOLVE, MODE_BACKWARD, MODE_MPC, MODE_ROLLOUT, MODE_FORWARD,
                              MODE_LINEARIZE>(h, mode, a);
  });
}

}  // namespace mi_host
