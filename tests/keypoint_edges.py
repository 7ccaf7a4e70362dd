"""The edge configurations of the three key-point methods (ilqr.py:417-593), shared by the CPU and GPU key-point tests.

Each configuration makes the list independent of round-off: jerk thresholds of +-inf (or a crafted trajectory whose jerks
are +-1, against 0), interpolation-error thresholds of 0 and +inf, and spacings at and beyond the horizon.  A tuple is
(method, minN, maxN, jerk_threshold, iterative_error_threshold), as utils_derivs_interpolation.derivs_interpolation takes it.
"""
import numpy as np

INF = float("inf")


def edge_configs(N):
    """label -> key-point configuration, at horizon N (N >= 6)."""
    return {
        # t = 0 twice ([0, 0, 1, 2, ...]), then every step
        "aj_min1_neginf": ("adaptiveJerk", 1, N + 5, -INF, 0.0),
        # every step from the counter alone, t = 0 twice again
        "aj_max1": ("adaptiveJerk", 3, 1, INF, 0.0),
        # minN > maxN: the counter always reaches maxN first - every second step
        "aj_min_gt_max": ("adaptiveJerk", 6, 2, -INF, 0.0),
        # nothing triggers: the single key-point [N - 2]
        "aj_single": ("adaptiveJerk", 1, N + 5, INF, 0.0),
        # a key-point wherever the counter has reached minN on a positive jerk (alternating +-1, see crafted_x_bar), or at maxN
        "aj_alternating": ("adaptiveJerk", 2, 7, 0.0, 0.0),
        # every step (the default): the lane-per-problem kernels' KP = false instantiation
        "si_every_step": ("setInterval", 1, 0, 0.0, 0.0),
        "si_n_minus_3": ("setInterval", N - 3, 0, 0.0, 0.0),
        "si_n_minus_2": ("setInterval", N - 2, 0, 0.0, 0.0),
        "si_n_minus_1": ("setInterval", N - 1, 0, 0.0, 0.0),
        "si_n_plus_5": ("setInterval", N + 5, 0, 0.0, 0.0),
        # (N - 2) a multiple of minN, and not
        "si_divides": ("setInterval", _divisor(N - 2), 0, 0.0, 0.0),
        "si_remainder": ("setInterval", _non_divisor(N - 2), 0, 0.0, 0.0),
        # the root bin is never tested: the empty list, 0 % derivatives
        "ie_empty": ("iterativeError", N - 2, 0, 0.0, 0.0),
        "ie_empty_wide": ("iterativeError", N + 5, 0, 0.0, 0.0),
        # every bin splits down to width 1 (deepest bisection)
        "ie_zero": ("iterativeError", 1, 0, 0.0, 0.0),
        # the root bin is tested once and never split: [0, (N - 2) / 2, N - 2]
        "ie_inf": ("iterativeError", 1, 0, 0.0, INF),
    }


def short_configs():
    """Horizons N = 2 .. 5 (the jerk loop runs N - 3 < 3 times, or not at all)."""
    return {
        "aj_min1_neginf": ("adaptiveJerk", 1, 50, -INF, 0.0),
        "aj_max1": ("adaptiveJerk", 3, 1, INF, 0.0),
        "aj_single": ("adaptiveJerk", 1, 50, INF, 0.0),
        "si_1": ("setInterval", 1, 0, 0.0, 0.0),
        "si_2": ("setInterval", 2, 0, 0.0, 0.0),
        "ie_zero": ("iterativeError", 1, 0, 0.0, 0.0),
    }


def _divisor(k):
    for d in range(3, k):
        if k % d == 0:
            return d
    return 1


def _non_divisor(k):
    for d in range(3, k):
        if k % d != 0:
            return d
    return k + 1


def expected_list(cfg, N):
    """The list the reference builds where it does not depend on the trajectory (None where it does)."""
    method, minN, maxN, jthr, ethr = cfg
    if method == "setInterval":
        kp = list(range(0, N - 1, minN))
        kp[-1] = N - 2
        return kp
    if method == "adaptiveJerk":
        if not np.isinf(jthr):
            return None
        kp, since = [0], 0
        for t in range(N - 3):
            since += 1
            if since >= minN and jthr < 0:
                kp.append(t); since = 0
            if since >= maxN:
                kp.append(t); since = 0
        kp[-1] = N - 2
        return kp
    if minN >= N - 2:
        return []
    if ethr == INF:
        return sorted({0, (N - 2) // 2, N - 2})
    if ethr == 0.0 and minN == 1:
        return list(range(N - 1))
    return None


def crafted_x_bar(x0, N, rng, amp=0.05):
    """(B, n, N) trajectories near the states x0 (B, n), different per problem, whose 'velocity' rows (dof .. 2 dof - 1 with
    dof = int(n / 2), ilqr.py:469-486) carry a smooth part plus c (-1)^(t + phase): every jerk of every row is then
    4 c (+-1) + O(1e-16) - with c = 1/4 exactly +-1, far from the threshold 0 of "aj_alternating"."""
    B, n = x0.shape
    dof = n // 2
    t = np.arange(N)
    x = x0[:, :, None] + amp * np.cumsum(rng.standard_normal((B, n, N)), axis=2) / np.sqrt(N)
    phase = rng.integers(0, 2, B)
    for b in range(B):
        sign = (-1.0) ** (t + phase[b])
        for i in range(dof, 2 * dof):
            x[b, i] = x0[b, i] + 0.01 * rng.standard_normal() * t / N + 0.25 * sign
    return x


def fx_sentinel(B, n, N):
    """A finite value per (problem, row, element) that no Jacobian reproduces: 1000 + t + b / 4 + element / 1024."""
    b = np.arange(B)[:, None, None, None]
    e = np.arange(n * n).reshape(1, n, n, 1)
    t = np.arange(N - 1)[None, None, None, :]
    return 1000.0 + t + 0.25 * b + e / 1024.0


def fu_sentinel(B, n, m, N):
    b = np.arange(B)[:, None, None, None]
    e = np.arange(n * m).reshape(1, n, m, 1)
    t = np.arange(N - 1)[None, None, None, :]
    return -2000.0 - t - 0.25 * b - e / 1024.0


def benign_sentinels(B, n, m, N):
    """Sentinels for a backward pass to run through: fx_t = 0.9 I + s_t, fu_t = s_t with s_t a small positive constant per
    row and problem (a contraction: the value function stays finite whatever rows stay stale)."""
    s = 0.05 * (np.arange(N - 1)[None, :] + 1.0) / N + 1e-3 * np.arange(B)[:, None]       # (B, N-1)
    fx = np.broadcast_to(s[:, None, None, :] / n, (B, n, n, N - 1)) + 0.9 * np.eye(n)[None, :, :, None]
    fu = np.broadcast_to(s[:, None, None, :], (B, n, m, N - 1)).copy()
    return np.ascontiguousarray(fx), fu


def iterations_before_roundoff(cost_history, rel=1e-7):
    """How many leading iterations of a solve are decided above round-off: the count before the first iteration whose accepted
    improvement is below `rel` of the cost (iteration 0 always counts).  There the line search compares two costs that agree to
    ~1e-9 relative - the Jacobians' round-off (central differences, libm) decides it, and no two implementations need share
    that decision.  Such an iteration comes when a solve lands on its optimum in a Newton step: at once on a single key-point
    [N - 2] or N = 2 (one control that moves, control-affine models), after three iterations on a short pendulum.  Solves are
    compared with max_iters set to this count."""
    L = np.asarray(cost_history, float)
    for i in range(1, L.size):
        if abs(L[i - 1] - L[i]) < rel * abs(L[i - 1]):
            return i
    return int(L.size)
