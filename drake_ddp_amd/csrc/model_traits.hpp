// The model interface of the kernels.  A model type M (a struct of models.hpp, or the one drake_ddp_amd/plugin.py generates) declares
// `static constexpr int n, m, n_params` and `template <class T> __device__ static void step(const T* x, const T* u, T* xn, const
// double* p, double dt)`, and MAY declare the `static constexpr` members below; the kernels detect them through the traits of this
// header and nowhere else.  (A model with none of the four step members is rolled out dof by dof: `nq` and `dof<T>(i, x, u, qn, vn,
// p, dt)`, Synth36.)  wave = the wave-per-problem kernels (ilqr_small.hpp), wg = the workgroup-per-problem kernels (ilqr_large.hpp).
//
// member [trait]                         type, default  declared by                   read by: what it selects
// -------------------------------------  -------------  ----------------------------  -------------------------------------------------
// kNewtonRollout [NewtonMeasured]        bool, false    Pendulum                      wave, n = 2: rollout_newton_impl (dynamics_hold).  The
//     remainder of the time-parallel rollout was MEASURED on the model: its guard re-steps a lane's last step only.  Every other n = 2
//     model (plugins) takes that rollout too, with every step of the chunk re-stepped.
// kHasStepPool [HasStepPool]             bool, false    CartPoleT<WALL> (= WALL)      wave: rollout_step, PoolOf.  The plain-double rollout
//     calls M::step_pooled with an M::StepPool that its caller keeps in vector registers across the loop.
// kScanBackward [UsesScanBackward]       bool, false    LongHorizon<M>                wave, n = 3..4, m = 1: backward, ilqr_small_kernel.  The
//     time-parallel scan instead of the sequential MFMA sweep; the kernel keeps an LDS image of the cost constants for it.
// kExactBackward [UsesExactBackward]     bool, false    ExactCost<M>                  wave: backward.  The reference's scalar recursion.
// kLimited [UsesLimits]                  bool, false    Limited<M>                    every family: rollout_step, LimitRegs, ilqr_small_kernel;
//     ilqr_batch_kernel (ilqr_batch.hpp); large_rollout, mid_rollout4, ls_expected, ilqr_large_kernel.  Clamped controls in every
//     rollout, the box-QP backward pass, no Newton rollout.
// kChainCooperative [IsChainModel]       bool, false    PlanarQuad                    wg: large_rollout - one lane per chain of the tree
//     (kChains, chain_up / base_solve / chain_down); ilqr_large_kernel - large_jac_at_tree, odd strides of the LDS trajectory copy.
// kLegCooperative [IsLegModel]           bool, false    Quad3D                        wg: large_rollout - one lane per leg (kLegs, rotation /
//     leg / trunk), the legs' wrenches summed over the 16-lane row; ilqr_large_kernel - large_jac_at_legs.
// kTrigCooperative [IsTrigModel]         bool, false    Arm27, Arm27C                 wg: large_rollout, mid_rollout4.  The sines / cosines of
//     kJoints (<= 8) angles on 2 kJoints lanes at once, the rest of the step (M::core) on every lane of the row.  Bitwise M::step.
// kWholeStep [IsWholeStepModel]          bool, false    Arm27, Arm27C, plugins (f. 1) wg: large_rollout, mid_rollout4.  ONE lane advances the
//     dynamics with M::step and carries x_t in registers.  plugin.py emits the member for family 1.
// kCanFail [CanFail]                     bool, false    PlanarQuad, Quad3D            wg: large_rollout.  A step M::infeasible_velocity flags
//     makes the trial's cost +inf (ilqr.py:315-323); such a model gets no mid_rollout4 (kSpecRollout).
// kEarlyLeaderBlocks [EarlyLeaderBlocks] int, 0         PlanarQuad (1)                wg: ilqr_large_kernel (early linearization).  Blocks at
//     the END of the horizon that the leader linearizes itself once the trial is accepted: models whose helpers cannot keep up with the
//     rollout (an item is two passes over the tree, ~78 k cycles) - the last block comes out last anyway, the leader is free by then.
// kMaxAffected [HasSparsity]             int, absent    Synth36 (3)                   wg: ilqr_large_kernel - large_jac_at_sparse, only the
//     dofs M::affected(col, idx) lists are evaluated per Jacobian column.  PRESENCE selects; the value only sizes idx.
// kPivSplit [HasPivSplit]                bool, false    Synth36, PlanarQuad, Quad3D   wg, host: launch_jac_large (launch_large.hpp).  Two
//     forms of the kernels with a backward pass, with and without the pivoted-inverse cold path; the measurements are there.
//
// Where members combine, as the `if constexpr` chains have it (the first that holds wins):
//   * step of large_rollout: kChainCooperative, kLegCooperative, kTrigCooperative, kWholeStep, else dof by dof.  Arm27 and Arm27C
//     declare the last two: they take the trig step, and kWholeStep changes nothing for them (the carried state and kSpecRollout
//     ask for either).  mid_rollout4 (under kSpecRollout only): kTrigCooperative, else the whole step.
//   * linearization (ilqr_large_kernel: jac, jac_list): kMaxAffected, kChainCooperative, kLegCooperative, else large_jac_at - whole
//     M::step evaluations per (key-point, column) item; kTrigCooperative and kWholeStep are not consulted there.
//   * the chain and the leg step call M::infeasible_velocity with or without kCanFail; kCanFail decides whether the flag reaches the cost.
//   * backward pass, wave: kLimited (ilqr_small_kernel calls backward_limited, not backward), kExactBackward, then kScanBackward
//     (n = 3..4, m = 1 only).  The host never nests the wrappers (launch_small.hpp).
#pragma once

namespace mi {

// THE detection: Name<M>::value is `absent` for a model that does not declare `member`, else `present`.  Three shapes - bool member,
// default false: (bool, false, M::member);  int member, default d: (int, d, M::member);  member present: (bool, false, true).
#define MI_MODEL_TRAIT(Name, member, type, absent, present)                                 \
  template <class M, class = void> struct Name { static constexpr type value = absent; }; \
  template <class M> struct Name<M, decltype((void)M::member)> { static constexpr type value = present; }
MI_MODEL_TRAIT(NewtonMeasured, kNewtonRollout, bool, false, M::kNewtonRollout);
MI_MODEL_TRAIT(HasStepPool, kHasStepPool, bool, false, M::kHasStepPool);
MI_MODEL_TRAIT(UsesScanBackward, kScanBackward, bool, false, M::kScanBackward);
MI_MODEL_TRAIT(UsesExactBackward, kExactBackward, bool, false, M::kExactBackward);
MI_MODEL_TRAIT(UsesLimits, kLimited, bool, false, M::kLimited);
MI_MODEL_TRAIT(IsChainModel, kChainCooperative, bool, false, M::kChainCooperative);
MI_MODEL_TRAIT(IsLegModel, kLegCooperative, bool, false, M::kLegCooperative);
MI_MODEL_TRAIT(IsTrigModel, kTrigCooperative, bool, false, M::kTrigCooperative);
MI_MODEL_TRAIT(IsWholeStepModel, kWholeStep, bool, false, M::kWholeStep);
MI_MODEL_TRAIT(CanFail, kCanFail, bool, false, M::kCanFail);
MI_MODEL_TRAIT(EarlyLeaderBlocks, kEarlyLeaderBlocks, int, 0, M::kEarlyLeaderBlocks);
MI_MODEL_TRAIT(HasSparsity, kMaxAffected, bool, false, true);
MI_MODEL_TRAIT(HasPivSplit, kPivSplit, bool, false, M::kPivSplit);
#undef MI_MODEL_TRAIT

// The same model with the kernels' backward pass run as the time-parallel scan.  For n = 3..4 the scan
// pays from two steps per lane on (N > 128) and its register appetite must not touch the kernels of
// short horizons, so the host picks this instantiation by horizon (launch_small.hpp: launch_jac).
template <class M>
struct LongHorizon : M { static constexpr bool kScanBackward = true; };
// The same model with the kernels' backward pass run as the reference's scalar recursion verbatim
// (cost matrices the MFMA / scan forms do not cover: asymmetric or indefinite Q, Qf, R).
template <class M>
struct ExactCost : M { static constexpr bool kExactBackward = true; };
// The same model with box control limits u_min <= u <= u_max (mi_ilqr_set_control_limits): every rollout clamps its controls,
// the backward pass solves a box QP per step (backward_limited).  Both are sequential in time - the n = 2 Newton rollout and
// the Riccati scans have no form that carries an active set - so the host picks this instantiation for limited handles only,
// like LongHorizon<M> / ExactCost<M>, and the regular kernels carry neither its code nor its registers.
template <class M>
struct Limited : M { static constexpr bool kLimited = true; };

// Constants derived from the traits alone.  (kSpecRollout - which models get mid_rollout4 - also reads LLay<n, m>::kMid
// (lds_layout.hpp) and stays in ilqr_large.hpp.)  kLxFromRollout: the rollout leaves lx_t, lu_t of the accepted trial in the backward pass's
// cost-gradient area (not chain models: their linearization uses that area as a cache).  kEarlyLin: early linearization is possible.
template <class M>
constexpr bool kLxFromRollout = !IsChainModel<M>::value;
template <class M>
constexpr bool kEarlyLin = M::m * 16 <= 192;                 // (the fourth wave holds no control-law lanes: no prefetch loads on it)

}  // namespace mi
