"""NumPy statement of the join between two re-solves of the multi-start receding-horizon loop (include/mi_ilqr.h: "Multi-start in the
receding-horizon loop"; csrc/seeds.hpp: seeds_mpc_join_kernel), on top of tests/seeds_np.py:

    shift : u[b, j, t] <- u_bar[b, j, min(t + r, N - 2)]                        (mi_ilqr_mpc_shift)
    join  : seeds_np.reseed applied to the shifted plans - the winner's slot its own shifted plan, the other members of its group
            the winner's shifted plan + sigma z; no winner: each member's own shifted plan, non-finite entries read as 0, member 0
            unperturbed - and x0[gK + k] <- x_bar[gK + w][:, r], each member's own x_bar[:, r] in a group without a winner.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import seeds_np as SN  # noqa: E402


def shift(u_bar, replan):
    """(B, m, N-1) -> the plans moved `replan` steps ahead, the last column held."""
    u_bar = np.asarray(u_bar, dtype=np.float64)
    steps = u_bar.shape[2]
    return u_bar[:, :, np.minimum(np.arange(steps) + int(replan), steps - 1)]


def join(x_bar, u_bar, cost, status, K, replan, sigma, seed=0, round=0, hold=1):   # noqa: A002
    """x_bar (B, n, N), u_bar (B, m, N-1) -> (x0 (B, n), u_guess (B, m, N-1), the (G, 3) selection).  Written out element by
    element, independently of seeds_np.reseed (tests/test_mpc_seeds_abi.py holds the two against each other)."""
    x_bar, u_bar = np.asarray(x_bar, dtype=np.float64), np.asarray(u_bar, dtype=np.float64)
    B, m, steps = u_bar.shape
    assert K >= 1 and B % K == 0 and 1 <= replan < steps and hold >= 1
    s = np.array(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (B, m)))
    best = SN.select(cost, status, K)
    z = SN.noise(seed, round, B, steps, m, hold)
    src = np.minimum(np.arange(steps) + int(replan), steps - 1)
    x0, u = np.empty((B, x_bar.shape[1])), np.empty_like(u_bar)
    for g in range(B // K):
        w = int(best[g, 0])
        for k in range(K):
            b = g * K + k
            sb = g * K + w if w >= 0 else b
            x0[b] = x_bar[sb, :, replan]
            base = u_bar[sb][:, src]
            if w < 0:
                base = np.where(np.isfinite(base), base, 0.0)
            elite = k == (w if w >= 0 else 0)
            for j in range(m):
                u[b, j] = base[j] if (elite or s[b, j] == 0.0) else base[j] + s[b, j] * z[b, j]
    return x0, u, best
