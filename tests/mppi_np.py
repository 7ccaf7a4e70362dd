"""NumPy statement of sampling-based MPC on the device (include/mi_ilqr.h: "Sampling-based MPC"; csrc/mppi.hpp) on top of
tests/policy_noise_np.py's Philox4x32-10 and Box-Muller and oracle/models_np.py's steps.

    key      = (seed mod 2^32, seed div 2^32)
    counter  = (g, t div hold, b, 1024 + k / 4), normal k mod 4 of the block;  g = first_sample + i S + s the global sample number
    applied  : v_s[k, t] = clip(u[k, t] + sigma[b, k] z) - a rounded product, a rounded sum; sample 0 (the elite slot) and sigma = 0:
               clip(u[k, t]) bit for bit; the clip by comparisons, on a limited handle only
    rollout  : open loop from x0 with v_s; cost = sum_t (x_t - x_nom)' Q (x_t - x_nom) + v_t' R v_t + the terminal term; +inf for a
               sample that meets an infeasible step, a non-finite state or a non-finite cost
    update   : L_min the least finite cost, ties to the lowest s; e_s = exp(-(L_s - L_min) / temperature) (temperature = 0: 1 for the
               argmin, 0 else) over the finite samples; Z = sum e_s and Q = sum (e_s / Z)^2 SEQUENTIALLY IN s = 0, 1, .. S - 1 from 0.0;
               u_new = w_0 v_0 + w_1 v_1 + .. sequentially in s, w_s = e_s / Z: the first finite sample's product starts the sum;
               non-finite samples are skipped; clipped again; no finite sample: u stays
    log      : argmin | L_min | finite (none finite: -1 | +inf | 0); nominal cost (sample 0's) | ESS = 1 / Q (none finite: NaN); a
               closing rollout of the final nominal alone gives row I of the nominal cost
    end      : u_guess[t] = u[min(t + shift, N - 2)]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import policy_noise_np as PN  # noqa: E402
from oracle import models_np as M  # noqa: E402

MPPI_BLOCK = 1024


def normals(seed, g, b, steps, m, hold=1):
    """z (len(g), m, steps) of problem b for the global sample numbers g: a function of (seed, g, t div hold, b, k) alone."""
    g = np.asarray(g, dtype=np.uint64).reshape(-1)
    t = (np.arange(steps) // int(hold)).astype(np.uint64)
    z = PN._stream(seed, 0, False, b, g[:, None], t[None, :], m, MPPI_BLOCK)          # (G, steps, m)
    return np.ascontiguousarray(z.transpose(0, 2, 1))


def clip(v, lo, hi):
    """By comparisons (a NaN stays one); lo, hi (m,) or None."""
    if lo is None:
        return v
    lo, hi = np.asarray(lo, dtype=float).reshape(-1, 1), np.asarray(hi, dtype=float).reshape(-1, 1)
    return np.where(v < lo, lo, np.where(v > hi, hi, v))


def applied(u, sigma, z, lo=None, hi=None):
    """u (m, steps), sigma (m,), z (S, m, steps) -> v (S, m, steps); sample 0 is the elite slot."""
    s = np.asarray(sigma, dtype=float).reshape(1, -1, 1)
    v = np.where(s != 0.0, u[None] + s * z, u[None])
    v[0] = u
    return np.stack([clip(vs, lo, hi) for vs in v])


def rollout_cost(model, x0, v, Q, R, Qf, x_nom):
    """The cost of the open-loop rollout of v (m, steps) from x0; +inf for a sample that ends early or whose cost is not finite."""
    bad = M.INFEASIBLE_FUNCS.get(model.model_id)
    x = np.array(x0, dtype=float).reshape(-1)
    if not np.isfinite(x).all():
        return np.inf
    L = 0.0
    with np.errstate(all="ignore"):
        for t in range(v.shape[1]):
            xn = model.step_unchecked(x, v[:, t])
            if not np.isfinite(xn).all() or (bad is not None and bad(list(xn), model.params)):
                return np.inf
            dx = x - x_nom
            L += dx @ Q @ dx + v[:, t] @ R @ v[:, t]
            x = xn
        dx = x - x_nom
        L += dx @ Qf @ dx
    return float(L) if np.isfinite(L) else np.inf


def update(u, v, L, temperature, lo=None, hi=None):
    """u (m, steps), v (S, m, steps), L (S,) -> (u_new, argmin, L_min, finite, ess)."""
    S = L.size
    fin = np.isfinite(L)
    if not fin.any():
        return u.copy(), -1, np.inf, 0, np.nan
    best, Lmin = -1, np.inf
    for s in range(S):
        if fin[s] and (best < 0 or L[s] < Lmin):               # (strict: of equal costs the first stays)
            best, Lmin = s, L[s]
    with np.errstate(all="ignore"):
        e = (np.arange(S) == best).astype(float) if temperature == 0.0 else np.exp(-(L - Lmin) / temperature)
    Z = 0.0
    for s in range(S):
        if fin[s]:
            Z = Z + e[s]
    Qs, acc = 0.0, None
    for s in range(S):
        if fin[s]:
            w = e[s] / Z
            Qs = Qs + w * w
            p = w * v[s]
            acc = p if acc is None else acc + p
    return clip(acc, lo, hi), best, float(Lmin), int(fin.sum()), 1.0 / Qs


def shift_plan(u, shift):
    """u (.., m, N-1) -> u_guess[.., t] = u[.., min(t + shift, N - 2)]."""
    steps = u.shape[-1]
    return u[..., np.minimum(np.arange(steps) + int(shift), steps - 1)]


def run(models, x0, u, sigma, Q, R, Qf, x_nom, S, iterations, temperature, seed=0, first_sample=0, hold=1, shift=0, u_min=None, u_max=None,
        z_shift=0.0):
    """models: one oracle model per problem (its parameters inside); x0 (B, n), u (B, m, N-1), sigma (B, m); Q, R, Qf, x_nom shared or
    with a leading batch axis; u_min / u_max (B, m) or None.  z_shift is added to every normal (the statement's own sensitivity to
    the last digits of the normals).  -> dict: u (B, m, N-1), u_guess, best_sample / best_cost / finite / ess (I, B),
    nominal_cost (I + 1, B), costs (I, B, S)."""
    u = np.array(u, dtype=float)
    B, m, steps = u.shape
    sigma = np.broadcast_to(np.asarray(sigma, dtype=float), (B, m))
    row = lambda a, b, nd: a if np.ndim(a) == nd else a[b]   # noqa: E731
    out = dict(best_sample=np.empty((iterations, B), dtype=np.int64), best_cost=np.empty((iterations, B)),
               finite=np.empty((iterations, B), dtype=np.int64), ess=np.empty((iterations, B)), nominal_cost=np.empty((iterations + 1, B)),
               costs=np.empty((iterations, B, S)))
    for b in range(B):
        lo, hi = (None, None) if u_min is None else (u_min[b], u_max[b])
        Qb, Rb, Qfb, xb = row(Q, b, 2), row(R, b, 2), row(Qf, b, 2), row(x_nom, b, 1)
        for i in range(iterations):
            z = normals(seed, first_sample + i * S + np.arange(S), b, steps, m, hold) + z_shift
            v = applied(u[b], sigma[b], z, lo, hi)
            L = np.array([rollout_cost(models[b], x0[b], v[s], Qb, Rb, Qfb, xb) for s in range(S)])
            out["costs"][i, b] = L
            out["nominal_cost"][i, b] = L[0]
            u[b], out["best_sample"][i, b], out["best_cost"][i, b], out["finite"][i, b], out["ess"][i, b] = update(u[b], v, L, temperature, lo, hi)
        out["nominal_cost"][iterations, b] = rollout_cost(models[b], x0[b], clip(u[b], lo, hi), Qb, Rb, Qfb, xb)
    out["u"] = u
    out["u_guess"] = shift_plan(u, shift)
    return out
