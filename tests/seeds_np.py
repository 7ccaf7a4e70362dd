"""NumPy statement of the multi-start operations (include/mi_ilqr.h: "Multi-start"; csrc/seeds.hpp) on top of tests/policy_noise_np.py's
Philox4x32-10 and Box-Muller.  A batch of B problems is G = B / K groups of K consecutive problems.

    key     = (seed mod 2^32, seed div 2^32)
    counter = (round, t div hold, b, 768 + j / 4), normal j mod 4 of the block
    perturb : u[b, j, t] = base[b, j, t] + sigma[b, j] z(b, t div hold, j) for the members k >= 1; member 0 and sigma = 0: base itself
    select  : eligible = status & ~16 in {CONVERGED, MAX_ITERS} and cost finite; the eligible member of least cost, ties to the lowest
              index -> winner | cost | eligible; none eligible: -1 | +inf | 0
    reseed  : the winner's slot its own u_bar; the others the winner's u_bar + the noise; no winner: perturb around each member's own
              u_bar with non-finite entries read as 0
    gather  : the winners' x_bar, u_bar, cost; no winner: NaN rows, +inf
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import policy_noise_np as PN  # noqa: E402

SEEDS_BLOCK = 768
STATUS_CONVERGED, STATUS_MAX_ITERS, FLAG_INDEFINITE = 0, 1, 16


def noise(seed, round, B, steps, m, hold=1, b0=0):   # noqa: A002
    """(B, m, steps): z[b, j, t] of problems b0 .. b0 + B - 1, a function of (seed, round, b0 + b, t div hold, j) alone."""
    b = np.arange(b0, b0 + B, dtype=np.uint64)
    t = (np.arange(steps) // int(hold)).astype(np.uint64)
    z = PN._stream(seed, round, False, b[:, None, None], np.zeros((B, 1), dtype=np.uint64), t[None, :], m, SEEDS_BLOCK)   # (B, steps, m)
    return np.ascontiguousarray(z.transpose(0, 2, 1))


def normals(seed, round, b, steps, m, hold=1):   # noqa: A002
    """z of problem b: (m, steps)."""
    return noise(seed, round, 1, steps, m, hold, b0=b)[0]


def _add(base, sigma, z):
    """base + sigma z where sigma != 0 (a rounded product, a rounded sum), base itself - bit for bit - where sigma = 0."""
    s = np.broadcast_to(np.asarray(sigma, dtype=np.float64)[:, :, None], base.shape)
    return np.where(s != 0.0, base + s * z, base)


def perturb(base, K, sigma, seed=0, round=0, hold=1):   # noqa: A002
    """base (B, m, N-1), sigma (B, m) -> the guesses (B, m, N-1)."""
    base = np.asarray(base, dtype=np.float64)
    B, m, steps = base.shape
    assert K >= 1 and B % K == 0 and hold >= 1
    s = np.array(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (B, m)))
    s[::K] = 0.0                                             # member 0: the elite slot
    return _add(base, s, noise(seed, round, B, steps, m, hold))


def eligible(cost, status):
    st = np.asarray(status).astype(np.int64) & ~FLAG_INDEFINITE
    return ((st == STATUS_CONVERGED) | (st == STATUS_MAX_ITERS)) & np.isfinite(np.asarray(cost, dtype=np.float64))


def select(cost, status, K):
    """-> (G, 3) rows winner | cost | eligible."""
    cost = np.asarray(cost, dtype=np.float64)
    B = cost.size
    assert K >= 1 and B % K == 0
    ok = eligible(cost, status).reshape(B // K, K)
    c = cost.reshape(B // K, K)
    out = np.empty((B // K, 3))
    for g in range(B // K):
        win, best = -1, np.inf
        for k in range(K):
            if ok[g, k] and (win < 0 or c[g, k] < best):     # (strict: of equal costs the first stays)
                win, best = k, c[g, k]
        out[g] = (win, best, ok[g].sum())
    return out


def reseed(u_bar, cost, status, K, sigma, seed=0, round=0, hold=1):   # noqa: A002
    """-> (guesses (B, m, N-1), the (G, 3) selection)."""
    u_bar = np.asarray(u_bar, dtype=np.float64)
    B, m, steps = u_bar.shape
    best = select(cost, status, K)
    s = np.array(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (B, m)))
    base = np.empty_like(u_bar)
    for g in range(B // K):
        w, rows = int(best[g, 0]), slice(g * K, (g + 1) * K)
        if w >= 0:
            base[rows] = u_bar[g * K + w]
            s[g * K + w] = 0.0
        else:
            base[rows] = np.where(np.isfinite(u_bar[rows]), u_bar[rows], 0.0)
            s[g * K] = 0.0
    return _add(base, s, noise(seed, round, B, steps, m, hold)), best


def gather(x_bar, u_bar, cost, status, K):
    """-> (x (G, n, N), u (G, m, N-1), cost (G,), the (G, 3) selection)."""
    x_bar, u_bar, cost = (np.asarray(a, dtype=np.float64) for a in (x_bar, u_bar, cost))
    best = select(cost, status, K)
    G = best.shape[0]
    x, u, c = np.full((G,) + x_bar.shape[1:], np.nan), np.full((G,) + u_bar.shape[1:], np.nan), np.full(G, np.inf)
    for g in range(G):
        w = int(best[g, 0])
        if w >= 0:
            x[g], u[g], c[g] = x_bar[g * K + w], u_bar[g * K + w], cost[g * K + w]
    return x, u, c, best
