"""NumPy statement of the on-device Monte-Carlo (include/mi_ilqr.h: "Monte-Carlo on the device"; csrc/policy_mc.hpp): the draws
of the start states and the parameters, built on policy_noise_np's Philox4x32-10 and Box-Muller, and the MIRROR of the device's
reduction - per group of 64 samples the butterfly over lane distance 1 .. 32 of Chan's merge, then the left fold over the groups -
in plain float64, one operation per line of the header's formula.

    counter = (first_sample + s, 0, common ? 0 : b, block)      block = 512 + i / 4 for x0 component i, 768 + j / 4 for parameter j
    normal:  d = the Box-Muller normal of word pair (i mod 4);   uniform: d = (w + 1/2) 2^-31 - 1, w = word i mod 4
    value = mean + spread d                                      (a spread of zero: the mean's bits)
"""
import numpy as np

import policy_noise_np as PN

X0_BLOCK, PARAM_BLOCK = 512, 768
FIELDS = ("n", "counted", "success", "mean", "m2", "min", "max", "argmin", "argmax", "steps_total")
EPS = np.finfo(np.float64).eps


def words(seed, first_sample, common, b, s, count, first_block):
    """The Philox words behind `count` components for the samples s (integer array): (len(s), 4 * blocks) uint64."""
    seed = int(seed)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    s = np.asarray(s, dtype=np.uint64)
    blocks = (count + 3) // 4
    ctr = np.zeros(s.shape + (blocks, 4), dtype=np.uint64)
    ctr[..., 0] = (np.uint64(first_sample) + s)[..., None]
    ctr[..., 2] = np.uint64(0 if common else b)
    ctr[..., 3] = np.uint64(first_block) + np.arange(blocks, dtype=np.uint64)
    assert int(ctr[..., 0].max(initial=0)) < 2 ** 32
    return PN.philox4x32_10(ctr, key).reshape(s.shape + (4 * blocks,))


def unit_draws(dist, seed, first_sample, common, b, s, count, first_block):
    """d of the header for `count` components: (len(s), count) float64."""
    w = words(seed, first_sample, common, b, s, count, first_block)
    if dist == "uniform":
        return ((w.astype(np.float64) + 0.5) * 2.0 ** -31 - 1.0)[..., :count]
    assert dist == "normal"
    z = np.empty(w.shape)
    z[..., 0::4], z[..., 1::4] = PN.box_muller(w[..., 0::4], w[..., 1::4])
    z[..., 2::4], z[..., 3::4] = PN.box_muller(w[..., 2::4], w[..., 3::4])
    return z[..., :count]


def draw(dist, mean, spread, seed, first_sample, common, b, s, first_block):
    """mean + spread o d for the samples s of problem b: (len(s), len(mean)); a spread of zero returns the mean's bits."""
    mean, spread = np.asarray(mean, dtype=np.float64), np.asarray(spread, dtype=np.float64)
    d = unit_draws(dist, seed, first_sample, common, b, s, mean.size, first_block)
    return np.where(spread == 0.0, mean, mean + spread * d)


def draw_x0(dist, mean, spread, seed, first_sample, common, b, s):
    return draw(dist, mean, spread, seed, first_sample, common, b, s, X0_BLOCK)


def draw_params(dist, mean, spread, seed, first_sample, common, b, s):
    return draw(dist, mean, spread, seed, first_sample, common, b, s, PARAM_BLOCK)


# ---------------------------------------------------------------- the mirror reduction
EMPTY = (0.0, 0.0, 0.0)                                  # (count, mean, M2)


def merge(A, B):
    """Chan's merge of (count, mean, M2), A the operand of the lower sample numbers; a count-0 operand returns the other's bits."""
    nA, mA, qA = A
    nB, mB, qB = B
    if nB == 0.0:
        return A
    if nA == 0.0:
        return B
    n = nA + nB
    delta = mB - mA
    w = nB / n
    q = (nA * nB) / n
    return (n, mA + delta * w, (qA + qB) + (delta * delta) * q)


def group_moments(cost, counted):
    """One group (up to 64 samples, in lane order): the butterfly - since both partners compute merge(lower, upper), lane 0's result is
    the balanced tree over the 64 lanes."""
    lanes = [EMPTY] * 64
    for i, (c, ok) in enumerate(zip(cost, counted)):
        if ok:
            lanes[i] = (1.0, float(c), 0.0)
    while len(lanes) > 1:                                # lane distance 1, 2, 4, 8, 16, 32
        lanes = [merge(lanes[2 * k], lanes[2 * k + 1]) for k in range(len(lanes) // 2)]
    return lanes[0]


def mirror_moments(cost, counted, acc=EMPTY):
    """The device's (count, mean, M2) of one problem's samples (1-D arrays, sample order): groups of 64, folded left to right into acc."""
    cost, counted = np.asarray(cost, dtype=np.float64), np.asarray(counted, dtype=bool)
    for g0 in range(0, cost.size, 64):
        acc = merge(acc, group_moments(cost[g0:g0 + 64], counted[g0:g0 + 64]))
    return acc


def stats(cost, steps, N, first_sample=0, success=None):
    """The ten numbers of one problem from its samples' cost and steps (1-D): a dict over FIELDS.  success: boolean per sample (goal
    test), None: all true.  counted = 0: mean = m2 = NaN, min = +inf, max = -inf, argmin = argmax = -1."""
    cost, steps = np.asarray(cost, dtype=np.float64), np.asarray(steps)
    counted = (steps == N - 1) & np.isfinite(cost)
    n, mean, m2 = mirror_moments(cost, counted)
    out = dict(n=cost.size, counted=int(counted.sum()), steps_total=int(steps.astype(np.int64).sum()))
    out["success"] = int((counted & (True if success is None else np.asarray(success, dtype=bool))).sum())
    assert n == out["counted"]
    if out["counted"] == 0:
        out.update(mean=np.nan, m2=np.nan, min=np.inf, max=-np.inf, argmin=-1, argmax=-1)
        return out
    c = np.where(counted, cost, np.nan)
    out.update(mean=mean, m2=m2, min=float(np.nanmin(c)), max=float(np.nanmax(c)),
               argmin=first_sample + int(np.nanargmin(c)), argmax=first_sample + int(np.nanargmax(c)))      # (the first of equals: the lower g)
    return out


def merge_stats(a, b):
    """PolicyStats.merge for two dicts of `stats` (a: the earlier window)."""
    A = EMPTY if a["counted"] == 0 else (float(a["counted"]), a["mean"], a["m2"])
    B = EMPTY if b["counted"] == 0 else (float(b["counted"]), b["mean"], b["m2"])
    n, mean, m2 = merge(A, B)
    out = {k: a[k] + b[k] for k in ("n", "counted", "success", "steps_total")}
    if n == 0.0:
        mean = m2 = np.nan
    lo, hi = b["min"] < a["min"], b["max"] > a["max"]
    out.update(mean=mean, m2=m2, min=b["min"] if lo else a["min"], max=b["max"] if hi else a["max"],
               argmin=b["argmin"] if lo else a["argmin"], argmax=b["argmax"] if hi else a["argmax"])
    return out


def moment_bounds(cost, counted, mean):
    """What the device's mean and M2 may differ from the mirror's by (issue / tests/test_gpu_policy_mc.py's docstring): with G the
    groups folded, 8 eps (6 + G) max|c| for the mean and 8 eps (6 + G) (sum (c - mean)^2 + S max|c| |mean|) for M2."""
    cost, counted = np.asarray(cost, dtype=np.float64), np.asarray(counted, dtype=bool)
    G = (cost.size + 63) // 64
    c = cost[counted]
    cmax = float(np.max(np.abs(c))) if c.size else 0.0
    k = 8.0 * EPS * (6 + G)
    return k * cmax, k * (float(np.sum((c - mean) ** 2)) + cost.size * cmax * abs(mean))


def two_pass_longdouble(cost, counted):
    """(mean, M2) of the counted costs, two passes in np.longdouble: the yardstick the bound is checked against."""
    c = np.asarray(cost, dtype=np.float64)[np.asarray(counted, dtype=bool)].astype(np.longdouble)
    mean = c.sum() / c.size
    return mean, ((c - mean) ** 2).sum()
