"""NumPy statement of mi_ilqr_policy_rollout (include/mi_ilqr.h): one sample rolled out under a time-varying feedback policy.

    u_t = u_bar[:, t] - eps kappa[:, t] - K[:, :, t] (x_t - x_bar[:, t])           ilqr.py:313 (the device entry has eps = 0)
    u_t = clip(u_t, u_min, u_max)                                                  control-limited handles only
    x_{t+1} = f(x_t, u_t)
    L += (x_t - x_nom)' Q (x_t - x_nom) + u_t' R u_t                               ilqr.py:325
    L += (x_{N-1} - x_nom)' Qf (x_{N-1} - x_nom)                                   ilqr.py:327

A sample ENDS at a step the model declares infeasible (oracle.models_np.INFEASIBLE_FUNCS) or whose result is not finite, and
before its first step when x0 is not finite: cost = +inf, `steps` = steps completed, x_final = the last state it held, X keeps
steps + 1 columns and U steps columns, the rest is NaN.  `eps` and `kappa` exist only to tie this function to the reference's
line-search rollout (tests/test_policy_rollout_oracle.py)."""
import numpy as np

from oracle import models_np as M


def rollout_sample(model, x0, x_bar, u_bar, K, Q, R, Qf, x_nom, u_min=None, u_max=None, eps=0.0, kappa=None):
    """-> cost, x_final (n,), steps, X (n, N), U (m, N-1) for one sample on `model` (oracle.models_np.Model)."""
    n, N = x_bar.shape
    m = u_bar.shape[0]
    bad = M.INFEASIBLE_FUNCS.get(model.model_id)
    X, U = np.full((n, N), np.nan), np.full((m, N - 1), np.nan)
    x = np.array(x0, dtype=float).reshape(n)
    X[:, 0] = x
    L, steps = 0.0, 0
    alive = bool(np.isfinite(x).all())
    for t in range(N - 1):
        if not alive:
            break
        u = u_bar[:, t] - K[:, :, t] @ (x - x_bar[:, t])
        if kappa is not None:
            u = u_bar[:, t] - eps * kappa[:, t] - K[:, :, t] @ (x - x_bar[:, t])
        if u_min is not None:
            u = np.clip(u, u_min, u_max)
        with np.errstate(all="ignore"):
            xn = model.step_unchecked(x, u)
        if not np.isfinite(xn).all() or (bad is not None and bad(list(xn), model.params)):
            alive = False
            break
        dx = x - x_nom
        L += dx @ Q @ dx + u @ R @ u
        U[:, t] = u
        X[:, t + 1] = xn
        x = xn
        steps += 1
    if alive:
        dx = x - x_nom
        L += dx @ Qf @ dx
    else:
        L = np.inf
    return L, x, steps, X, U


def rollout(make_model, x0, params, x_bar, u_bar, K, Q, R, Qf, x_nom, u_min=None, u_max=None):
    """The batched form: x0 (B,S,n); params (B,S,n_params), or (B,n_params) rows; make_model(params_row) -> Model; x_bar (B,n,N),
    u_bar (B,m,N-1), K (B,m,n,N-1); Q, R, Qf (k,k) or (B,k,k); x_nom (n,) or (B,n); u_min / u_max None, (m,) or (B,m).
    -> cost (B,S), x_final (B,S,n), steps (B,S) int32, X (B,S,n,N), U (B,S,m,N-1)."""
    B, S, n = x0.shape
    N, m = x_bar.shape[2], u_bar.shape[1]
    row = lambda a, b, nd: a if a is None or np.ndim(a) == nd else a[b]
    cost, xf, steps = np.empty((B, S)), np.empty((B, S, n)), np.empty((B, S), dtype=np.int32)
    X, U = np.empty((B, S, n, N)), np.empty((B, S, m, N - 1))
    for b in range(B):
        shared = make_model(params[b]) if np.ndim(params) == 2 else None
        for s in range(S):
            model = shared if shared is not None else make_model(params[b, s])
            cost[b, s], xf[b, s], steps[b, s], X[b, s], U[b, s] = rollout_sample(
                model, x0[b, s], x_bar[b], u_bar[b], K[b], row(Q, b, 2), row(R, b, 2), row(Qf, b, 2), row(x_nom, b, 1),
                row(u_min, b, 1), row(u_max, b, 1))
    return cost, xf, steps, X, U
