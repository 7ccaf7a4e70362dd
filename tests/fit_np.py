"""NumPy statement of parameter identification on the device (include/mi_ilqr.h: "Parameter identification"; csrc/fit.hpp) on top of
oracle/models_np.py's steps; a plugin's step goes through Model.custom.

    residual : r_j = x_next_j - f(x_j, u_j; theta)
    Jacobian : J_j[:, i] = (f(.; theta + h e_k) - f(.; theta - h e_k)) / (2 h), k = free[i], h = fd_rel max(|theta_k|, fd_floor)
    normal   : c = sum_j r_j' W r_j, g = sum_j J_j' W r_j, H = sum_j J_j' W J_j over the first `count` rows
    trial    : (H + mu D) delta = g by Cholesky, D_ii = H_ii where H_ii > 0 else 1; theta' = clip(theta + delta) on the free entries,
               by comparisons; a pivot that is not positive or not finite: a rejected trial
    accept   : c(theta') finite and < c(theta): theta <- theta', the normal equations those of theta', mu <- max(mu / 10, 1e-12);
               CONVERGED when c - c' <= ftol c or c' == 0.  Else STALLED when mu is at 1e12 already, else mu <- min(10 mu, 1e12)
    end      : MAX_ITERS after `iterations` trials; BAD_DATA for count == 0 (cost +inf) or c(theta0) not finite: theta untouched
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONVERGED, MAX_ITERS, STALLED, BAD_DATA = 0, 1, 2, 3
MU_MIN, MU_MAX = 1e-12, 1e12


def predict(model, theta, x, u):
    """f(x_j, u_j; theta) for every row: (T, n)."""
    with np.errstate(all="ignore"):
        return np.array([model._f(list(xj), list(uj), theta, model.dt) for xj, uj in zip(x, u)], dtype=float).reshape(len(x), model.n)


def normal(model, theta, x, u, x_next, w, free, fd_rel=1e-6, fd_floor=1e-8):
    """The normal equations at theta over the rows given -> (c, g (P,), H (P, P))."""
    theta = np.array(theta, dtype=float)
    P = len(free)
    with np.errstate(all="ignore"):
        r = x_next - predict(model, theta, x, u)
        J = np.empty((len(x), model.n, P))
        for i, k in enumerate(free):
            h = fd_rel * max(abs(theta[k]), fd_floor)
            tp, tm = theta.copy(), theta.copy()
            tp[k] += h
            tm[k] -= h
            J[:, :, i] = (predict(model, tp, x, u) - predict(model, tm, x, u)) / (2.0 * h)
        c = float(np.sum(w * r * r))
        g = np.einsum("jni,n,jn->i", J, w, r)
        H = np.einsum("jni,n,jnk->ik", J, w, J)
    return c, g, H


def cholesky_solve(A, g):
    """delta with A delta = g, or None when a pivot is not positive or not finite."""
    P = len(g)
    Lm = np.zeros((P, P))
    with np.errstate(all="ignore"):
        for j in range(P):
            s = A[j, j] - Lm[j, :j] @ Lm[j, :j]
            if not (s > 0.0) or not np.isfinite(s):
                return None
            Lm[j, j] = np.sqrt(s)
            for i in range(j + 1, P):
                Lm[i, j] = (A[i, j] - Lm[i, :j] @ Lm[j, :j]) / Lm[j, j]
        y = np.zeros(P)
        for i in range(P):
            y[i] = (g[i] - Lm[i, :i] @ y[:i]) / Lm[i, i]
        for i in range(P - 1, -1, -1):
            y[i] = (y[i] - Lm[i + 1:, i] @ y[i + 1:]) / Lm[i, i]
    return y


def clip(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def fit(model, x, u, x_next, theta0, free, count=None, weights=None, damping=1e-3, bounds=None, iterations=20, ftol=1e-12, fd_rel=1e-6,
        fd_floor=1e-8):
    """One problem: x, x_next (T, n), u (T, m).  -> dict: params, cost0, cost, damping, iterations, accepted, status, gradient,
    normal_matrix, and the log `trials`: (cost of the trial or None when its factorisation failed, accepted) per trial."""
    free = list(free)
    P = len(free)
    theta = np.array(theta0, dtype=float)
    count = len(x) if count is None else int(count)
    w = np.ones(model.n) if weights is None else np.asarray(weights, dtype=float)
    lo, hi = (np.full(theta.size, -np.inf), np.full(theta.size, np.inf)) if bounds is None else (np.asarray(bounds[0], float), np.asarray(bounds[1], float))
    out = dict(params=theta, damping=float(damping), iterations=0, accepted=0, trials=[], gradient=np.zeros(P), normal_matrix=np.zeros((P, P)))
    if count == 0:
        out.update(cost0=np.inf, cost=np.inf, status=BAD_DATA)
        return out
    x, u, x_next = x[:count], u[:count], x_next[:count]
    ev = lambda th: normal(model, th, x, u, x_next, w, free, fd_rel, fd_floor)   # noqa: E731
    c, g, H = ev(theta)
    out.update(cost0=c, cost=c, gradient=g, normal_matrix=H)
    if not np.isfinite(c):
        out["status"] = BAD_DATA
        return out
    mu, status = float(damping), MAX_ITERS
    for _ in range(int(iterations)):
        out["iterations"] += 1
        d = np.diag(H).copy()
        A = H + mu * np.diag(np.where(d > 0.0, d, 1.0))
        delta = cholesky_solve(A, g)
        accepted = False
        cn = None
        if delta is not None:
            trial = theta.copy()
            for i, k in enumerate(free):
                trial[k] = clip(theta[k] + delta[i], lo[k], hi[k])
            cn, gn, Hn = ev(trial)
            accepted = bool(np.isfinite(cn) and cn < c)
        out["trials"].append((cn, accepted))
        if accepted:
            done = (c - cn <= ftol * c) or cn == 0.0
            theta, c, g, H = trial, cn, gn, Hn
            mu = max(mu / 10.0, MU_MIN)
            out["accepted"] += 1
            if done:
                status = CONVERGED
                break
        else:
            if mu >= MU_MAX:
                status = STALLED
                break
            mu = min(10.0 * mu, MU_MAX)
    out.update(params=theta, cost=c, damping=mu, status=status, gradient=g, normal_matrix=H)
    return out
