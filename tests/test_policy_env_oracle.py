"""The NumPy mirror of the envelope fold and the box rules (tests/policy_env_np.py) against an independent statement: a two-pass
np.longdouble mean / variance, exact counts and extrema, window independence bit for bit, the merge of two halves, and the box rules
on hand-made trajectories.  Also drake_ddp_amd.ilqr's finalisation and merges (PolicyEnvelope, PolicySafety), which must say the
same as the mirror's.  CPU only.

Bounds of the moments (policy_env_np.moment_bounds): the fold sums the shifted data d = v - K recursively, S terms, so by the
standard bound of recursive summation  |mean - ref| <= 2 S eps max|d| + eps |K|  and  |M2 - ref| <= 4 S eps sum d^2."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import policy_env_np as EN  # noqa: E402


def _rows(seed=5):
    """Random rows with NaN tails, S <= 300: scales from 1e-3 to 1e3, offsets far from zero, a constant row, an empty row, an inf."""
    rng = np.random.default_rng(seed)
    out = []
    for S in (1, 2, 63, 64, 65, 130, 300):
        for scale, off in ((1.0, 0.0), (1e-3, 1e3), (1e3, -7.0), (1e-6, 1.0)):
            v = off + scale * rng.standard_normal(S)
            v[rng.random(S) < 0.2] = np.nan
            out.append(v)
    out.append(np.full(70, 2.5))
    out.append(np.full(70, np.nan))
    w = rng.standard_normal(100)
    w[3], w[50] = np.inf, -np.inf
    out.append(w)
    out.append(np.concatenate([np.full(5, np.nan), rng.standard_normal(60), np.full(35, np.nan)]))
    return out


def test_the_fold_against_two_passes_in_extended_precision():
    worst = [0.0, 0.0]
    for v in _rows():
        f = EN.finalise(EN.fold(v, first_sample=11))
        cnt, mean, m2 = EN.two_pass(v)
        fin = np.isfinite(v)
        assert f["count"] == cnt == fin.sum()
        if cnt == 0:
            assert np.isnan(f["mean"]) and np.isnan(f["m2"]) and f["min"] == np.inf and f["max"] == -np.inf
            assert f["argmin"] == -1 and f["argmax"] == -1
            continue
        b_mean, b_m2 = EN.moment_bounds(v)
        e_mean, e_m2 = abs(float(np.longdouble(f["mean"]) - mean)), abs(float(np.longdouble(f["m2"]) - m2))
        assert e_mean <= b_mean and e_m2 <= b_m2, (v.size, e_mean, b_mean, e_m2, b_m2)
        if b_mean > 0:
            worst = [max(worst[0], e_mean / b_mean), max(worst[1], e_m2 / b_m2 if b_m2 else 0.0)]
        x = np.where(fin, v, np.nan)
        assert f["min"] == np.nanmin(x) and f["max"] == np.nanmax(x)
        assert f["argmin"] == 11 + int(np.nanargmin(x)) and f["argmax"] == 11 + int(np.nanargmax(x))      # (the first occurrence)
    print("fold vs two-pass: worst error / bound: mean %.3f, M2 %.3f" % tuple(worst))


def test_ties_keep_the_lower_sample_number_and_empty_rows_read_empty():
    v = np.array([np.nan, 3.0, 1.0, 3.0, 1.0, np.nan, 1.0, 3.0])
    acc = EN.fold(v, first_sample=100)
    assert acc.tolist() == [6.0, 3.0, -6.0, 12.0, 1.0, 3.0, 102.0, 101.0]
    assert EN.fold(np.full(4, np.nan)).tolist() == [0.0, 0.0, 0.0, 0.0, np.inf, -np.inf, -1.0, -1.0] == EN.empty().tolist()
    assert EN.fold(np.zeros(0)).tolist() == EN.empty().tolist()
    f = EN.finalise(acc)
    assert f["mean"] == 3.0 + (-6.0) / 6.0 and f["m2"] == 12.0 - 36.0 / 6.0


def test_the_fold_does_not_depend_on_the_window():
    for v in _rows(9):
        one = EN.fold(v, first_sample=3)
        for w in (1, 64, 65, max(1, v.size)):
            got = EN.fold_windows(v, w, first_sample=3)
            assert got.tobytes() == one.tobytes(), (v.size, w)
    V = np.stack([r for r in _rows(9) if r.size == 130])                             # vectorised over rows: the same bits per row
    assert EN.fold(V, 3).tobytes() == np.stack([EN.fold(r, 3) for r in V]).tobytes()


def test_merge_of_two_halves_against_one_fold():
    from drake_ddp_amd.ilqr import PolicyEnvelope
    for v in _rows(13):
        if v.size < 2:
            continue
        h = v.size // 2
        one = EN.finalise(EN.fold(v, first_sample=7))
        a, b = EN.fold(v[:h], first_sample=7), EN.fold(v[h:], first_sample=7 + h)
        m = EN.merge(EN.finalise(a), EN.finalise(b))
        pe = PolicyEnvelope.from_raw(a[None]).merge(PolicyEnvelope.from_raw(b[None]))
        for k in EN.FIELDS:                                                          # the package's merge is the mirror's
            assert np.array_equal(np.asarray(getattr(pe, k))[0], m[k], equal_nan=True), k
        for k in ("count", "min", "max", "argmin", "argmax"):
            assert m[k] == one[k], k
        if one["count"] == 0:
            assert np.isnan(m["mean"]) and np.isnan(m["m2"])
            continue
        b_mean, b_m2 = EN.moment_bounds(v)
        cnt, mean, m2 = EN.two_pass(v)
        # The merge works on FINALISED halves: their means are rounded at the size of the values, eps |mean| each, not of the shifted
        # data, and that error reaches M2 through delta^2 q - at most 4 eps max|v| |delta| q.  For rows whose offset is of the size
        # of their spread the term is far inside the fold's bound and the fold's bounds are asserted as they are; for the rows far
        # from zero (offset / spread = 1e6) it is what a merge of finalised halves can promise, and it is added.
        fin = v[np.isfinite(v)]
        far = np.abs(fin).max() > 100.0 * (np.ptp(fin) + np.finfo(float).tiny)
        fa, fb = EN.finalise(a), EN.finalise(b)
        extra = 0.0
        if far and fa["count"] and fb["count"]:
            q = float(fa["count"]) * float(fb["count"]) / float(one["count"])
            extra = 4.0 * np.finfo(float).eps * np.abs(fin).max() * abs(float(fb["mean"] - fa["mean"])) * q
        assert abs(float(np.longdouble(m["mean"]) - mean)) <= b_mean and abs(float(np.longdouble(m["m2"]) - m2)) <= b_m2 + extra
    e = EN.finalise(EN.empty())
    f = EN.finalise(EN.fold(np.array([1.0, 2.0, 4.0])))
    for x, y in ((e, f), (f, e)):                                                    # a count-0 side leaves the other's bits
        m = EN.merge(x, y)
        assert all(np.array_equal(m[k], f[k]) for k in EN.FIELDS)


def test_the_packages_finalisation_is_the_mirrors():
    from drake_ddp_amd.ilqr import PolicyEnvelope
    acc = np.stack([EN.fold(v, 2) for v in _rows(21) if v.size == 130] + [EN.empty()])
    pe, f = PolicyEnvelope.from_raw(acc), EN.finalise(acc)
    for k in EN.FIELDS:
        assert np.array_equal(getattr(pe, k), f[k], equal_nan=True) and getattr(pe, k).dtype == f[k].dtype, k
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(pe.var, np.where(f["count"] > 1, f["m2"] / (f["count"] - 1), np.nan), equal_nan=True)


def test_the_box_rules_on_hand_made_trajectories():
    nan, inf = np.nan, np.inf
    N, n = 4, 2
    lo, hi = np.array([-1.0, -inf]), np.array([1.0, 5.0])
    x_nom, goal = np.zeros(2), np.array([0.5, inf])
    X = np.zeros((7, N, n))
    X[0, 0, 0] = 2.0                       # starts outside: exit at t = 0
    X[1, 2:, :] = nan                      # a NaN tail: did not run, never outside
    X[2, 1, 0], X[2, 2, 0] = -1.5, 0.0     # leaves at t = 1 and returns: exit at 1, once
    X[3, :, 1] = -1e300                    # an unbounded side: inside
    X[4, 3, 0] = 1.0                       # exactly on a bound at the last step: inside - and outside the goal (|1 - 0| > 0.5)
    X[5, 2, 1], X[5, 3, 0] = 6.0, -3.0     # outside twice through different components: exit at 2
    X[6, 1, 1] = 5.0                       # on the upper bound: inside
    ran, safe, succ, exits = EN.box(X, lo, hi, x_nom, goal)
    assert (ran, safe, succ) == (6, 3, 2) and exits.tolist() == [1, 1, 1, 0]
    X[1, 1, 0] = 9.0                       # the sample that ends leaves the box before it does: an exit, still not ran
    ran, safe, succ, exits = EN.box(X, lo, hi, x_nom, goal)
    assert (ran, safe, succ) == (6, 3, 2) and exits.tolist() == [1, 2, 1, 0]
    ran, safe, succ, exits = EN.box(X, np.full(2, -inf), np.full(2, inf), x_nom, np.full(2, inf))      # no box at all
    assert (ran, safe, succ) == (6, 6, 6) and exits.sum() == 0


def test_safety_merge_and_survival():
    from drake_ddp_amd.ilqr import PolicySafety
    a = PolicySafety.from_rows(np.array([10, 10]), np.array([[9.0, 7, 6, 1, 0, 2], [10.0, 10, 10, 0, 0, 0]]))
    b = PolicySafety.from_rows(np.array([6, 6]), np.array([[6.0, 5, 5, 0, 1, 0], [5.0, 4, 4, 1, 0, 0]]))
    m = a.merge(b)
    assert m.n.tolist() == [16, 16] and m.ran.tolist() == [15, 15] and m.safe.tolist() == [12, 14] and m.safe_success.tolist() == [11, 14]
    assert m.exits.tolist() == [[1, 1, 2], [1, 0, 0]] and m.exits.dtype == np.int64
    assert np.array_equal(m.survival, 1.0 - np.cumsum(m.exits, axis=1) / 16.0)


def test_check_mc_observe():
    from drake_ddp_amd.ilqr import check_mc_observe as chk
    B, n = 3, 2
    assert chk(False, False, None, B, n) == (0, None)
    assert chk(True, False, None, B, n)[0] == 1 and chk(False, True, None, B, n)[0] == 2 and chk(True, True, None, B, n)[0] == 3
    bits, box = chk(False, False, ([-1.0, -np.inf], None), B, n)
    assert bits == 0 and box.shape == (B, 4) and box.flags["C_CONTIGUOUS"] and np.array_equal(box[1], [-1.0, -np.inf, np.inf, np.inf])
    per = np.arange(B * n, dtype=float).reshape(B, n)
    assert np.array_equal(chk(True, True, (per, per), B, n)[1], np.hstack([per, per]))          # lo == hi is a box
    for bad in ((1.0, 2.0, 3.0), 1.0, "ab", ([0.0, 0.0],), ([0.0, 0.0, 0.0], None), (np.zeros((B + 1, n)), None), (None, np.zeros((1, n))),
                ([np.nan, 0.0], None), ([1.0, 0.0], [0.0, 0.0]), (["x", 0.0], None)):
        with pytest.raises(ValueError, match="RolloutPolicyStats"):
            chk(False, False, bad, B, n)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="RolloutPolicyStats: envelope"):
            chk(bad, False, None, B, n)
        with pytest.raises(ValueError, match="RolloutPolicyStats: controls"):
            chk(False, bad, None, B, n)
