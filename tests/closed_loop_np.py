"""NumPy statement of step 1 of a closed-loop MPC round (include/mi_ilqr.h: "Closed-loop MPC"; csrc/plant_advance.hpp): the plant of
one problem advanced `steps` = replan_steps steps under the policy of the previous solve.  The per-step arithmetic is that of
tests/policy_rollout_np.py / tests/policy_noise_np.py, the normals are policy_noise_np's with the counter (0, k, b, j): sample 0 of a
policy rollout at step t = k, k the plant clock.

    u_k     = u_bar[:, j] - K[:, :, j] (x_k - x_bar[:, j])      [u_bar[:, j] with feedback off]   [clamped]      j = k - clock
    x_{k+1} = f(x_k, u_k + sigma_u o xi^u_k) + sigma_x o xi^x_k
    l_k     = (x_k - x_nom)' Q (x_k - x_nom) + u_k' R u_k

A plant ENDS at a step the model declares infeasible or whose result is not finite: it keeps x_k, the row of that step is
x_k | NaN | NaN, later rows are NaN."""
import numpy as np

import policy_noise_np as PN
from oracle import models_np as M


def plant_segment(model, x, x_bar, u_bar, K, Q, R, x_nom, steps, sigma_x=None, sigma_u=None, zx=None, zu=None, feedback=True,
                  u_min=None, u_max=None):
    """One plant: x (n,), the policy x_bar (n, >= steps), u_bar (m, >= steps), K (m, n, >= steps); zx (steps, n), zu (steps, m) the
    normals (sigma_x None: no noise).  -> x_final (n,), steps completed, X (n, steps), U (m, steps), l (steps,)."""
    n, m = x_bar.shape[0], u_bar.shape[0]
    bad = M.INFEASIBLE_FUNCS.get(model.model_id)
    X, U, L = np.full((n, steps), np.nan), np.full((m, steps), np.nan), np.full(steps, np.nan)
    x = np.array(x, dtype=float).reshape(n)
    done = 0
    alive = bool(np.isfinite(x).all())
    for t in range(steps):
        if not alive:
            break
        X[:, t] = x
        u = u_bar[:, t] - K[:, :, t] @ (x - x_bar[:, t]) if feedback else np.array(u_bar[:, t], dtype=float)
        if u_min is not None:
            u = np.clip(u, u_min, u_max)
        with np.errstate(all="ignore"):
            if sigma_x is None:
                xn = model.step_unchecked(x, u)
            else:
                xn = model.step_unchecked(x, u + sigma_u * zu[t]) + sigma_x * zx[t]
        if not np.isfinite(xn).all() or (bad is not None and bad(list(xn), model.params)):
            alive = False
            break
        dx = x - x_nom
        L[t] = dx @ Q @ dx + u @ R @ u
        U[:, t] = u
        x = xn
        done += 1
    return x, done, X, U, L


def plant_normals(seed, common, b, clock, steps, n, m, shift=0.0):
    """zx (steps, n), zu (steps, m) of problem b from plant clock `clock` on; `shift` is added to every normal."""
    k = clock + np.arange(steps)
    return (PN.state_normals(seed, 0, common, b, 0, k, n) + shift, PN.control_normals(seed, 0, common, b, 0, k, m) + shift)


def advance(make_model, x, params, x_bar, u_bar, K, Q, R, x_nom, steps, sigma=None, seed=0, clock=0, common=False, feedback=True,
            u_min=None, u_max=None, shift=0.0):
    """The batched form: x (B, n), params (B, n_params) rows, make_model(row) -> Model, the policy x_bar (B, n, N), u_bar (B, m, N-1),
    K (B, m, n, N-1) - its first `steps` columns are used -, Q, R (k, k) or (B, k, k), x_nom (n,) or (B, n), sigma None or
    (B, n + m) = sigma_x | sigma_u, u_min / u_max None, (m,) or (B, m).
    -> x_final (B, n), steps completed (B,) int32, X (B, n, steps), U (B, m, steps), l (B, steps)."""
    B, n = x.shape
    m = u_bar.shape[1]
    row = lambda a, b, nd: a if a is None or np.ndim(a) == nd else a[b]   # noqa: E731
    xf, done = np.empty((B, n)), np.empty(B, dtype=np.int32)
    X, U, L = np.empty((B, n, steps)), np.empty((B, m, steps)), np.empty((B, steps))
    for b in range(B):
        sx = su = zx = zu = None
        if sigma is not None and np.any(sigma[b] != 0.0):         # (a problem whose sigmas are all zero: the noise-free step)
            sx, su = sigma[b, :n], sigma[b, n:]
            zx, zu = plant_normals(seed, common, b, clock, steps, n, m, shift)
        xf[b], done[b], X[b], U[b], L[b] = plant_segment(make_model(params[b]), x[b], x_bar[b], u_bar[b], K[b], row(Q, b, 2), row(R, b, 2),
                                                        row(x_nom, b, 1), steps, sx, su, zx, zu, feedback, row(u_min, b, 1), row(u_max, b, 1))
    return xf, done, X, U, L
