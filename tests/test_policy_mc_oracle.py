"""The on-device Monte-Carlo without a device: the NumPy statement (tests/policy_mc_np.py) of the draws - uniform exactly, normal by
its moments, independent of the disturbances' blocks - and of the reduction: the mirror of the device's butterfly-then-fold order
against a two-pass extended-precision mean / M2 within the bound the GPU tests use, merge of two windows against one call, and the
count-0 identity bit for bit.  CPU only."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import policy_mc_np as MC  # noqa: E402
import policy_noise_np as PN  # noqa: E402

SEED = PN.TEST_SEED


# ---------------------------------------------------------------- the draws
@pytest.mark.parametrize("first_block", [MC.X0_BLOCK, MC.PARAM_BLOCK])
def test_uniform_draws_are_exact_and_inside_the_open_interval(first_block):
    s = np.arange(4096)
    w = MC.words(SEED, 0, False, 1, s, 10, first_block)
    d = MC.unit_draws("uniform", SEED, 0, False, 1, s, 10, first_block)
    assert d.shape == (4096, 10)
    # exactly (w + 1/2) 2^-31 - 1: in integers, (d + 1) 2^32 = 2 w + 1
    assert np.array_equal(((d + 1.0) * 2.0 ** 32).astype(np.uint64), 2 * w[:, :10] + 1)
    assert d.min() > -1.0 and d.max() < 1.0
    # the extreme words stay inside
    for word, want in ((0, 2.0 ** -32 - 1.0), (2 ** 32 - 1, 1.0 - 2.0 ** -32)):
        v = (np.float64(word) + 0.5) * 2.0 ** -31 - 1.0
        assert v == want and -1.0 < v < 1.0
    assert abs(d.mean()) <= 5.0 / np.sqrt(3.0 * d.size) and abs(d.var() - 1.0 / 3.0) <= 5.0 * np.sqrt(4.0 / 45.0 / d.size)
    # x0 = mean + spread d lies in mean +- spread; a spread of zero returns the mean's bits (-0.0 included)
    mean, spread = np.array([1.0, -2.0, -0.0, 5.0]), np.array([0.5, 0.0, 0.0, 1e-3])
    x = MC.draw("uniform", mean, spread, SEED, 0, False, 0, s, first_block)
    assert np.all(np.abs(x - mean) <= spread)
    assert np.all(x[:, 1] == -2.0) and np.all(np.signbit(x[:, 2])) and not np.all(x[:, 0] == 1.0)


def test_normal_draws_have_the_moments_of_a_normal_stream():
    """(S, 1, C): samples x one 'step' x components, the form policy_noise_np.assert_moments takes (its step axis has one entry, so that
    correlation is taken over the other two)."""
    s = np.arange(8192)
    for first_block in (MC.X0_BLOCK, MC.PARAM_BLOCK):
        z = MC.unit_draws("normal", SEED, 0, False, 0, s, 40, first_block)
        zz = np.stack([z[0::2], z[1::2]], axis=1)                  # (S/2, 2, C): neighbouring samples as the middle axis
        PN.assert_moments(zz)


def test_the_draw_depends_on_seed_problem_sample_and_component_only():
    s = np.arange(130)
    a = MC.unit_draws("normal", SEED, 0, False, 1, s, 6, MC.X0_BLOCK)
    assert np.array_equal(MC.unit_draws("normal", SEED, 64, False, 1, np.arange(66), 6, MC.X0_BLOCK), a[64:])     # a window
    assert np.array_equal(MC.unit_draws("normal", SEED, 0, False, 1, s, 3, MC.X0_BLOCK), a[:, :3])                 # not on the model's n
    assert np.all(MC.unit_draws("normal", SEED, 0, False, 0, s, 6, MC.X0_BLOCK) != a)                              # the problem
    assert np.array_equal(MC.unit_draws("normal", SEED, 0, True, 0, s, 6, MC.X0_BLOCK),
                          MC.unit_draws("normal", SEED, 0, True, 1, s, 6, MC.X0_BLOCK))                            # common
    for other in (SEED + 1, SEED + 2 ** 32):
        assert np.all(MC.unit_draws("normal", other, 0, False, 1, s, 6, MC.X0_BLOCK) != a)
    top = MC.unit_draws("uniform", SEED, 2 ** 32 - 3, False, 1, np.arange(3), 6, MC.X0_BLOCK)                       # the last sample numbers
    assert np.isfinite(top).all()


def test_the_draws_blocks_are_not_the_disturbances():
    """Blocks 512.. and 768.. against the noise's 0.. and 256.. for the same (seed, b, g) at step 0: different words, everywhere."""
    s = np.arange(256)
    for b in (0, 1):
        x0 = MC.words(SEED, 0, False, b, s, 40, MC.X0_BLOCK)
        pr = MC.words(SEED, 0, False, b, s, 16, MC.PARAM_BLOCK)
        nx = MC.words(SEED, 0, False, b, s, 40, 0)
        nu = MC.words(SEED, 0, False, b, s, 16, PN.CONTROL_BLOCK)
        assert not np.any(x0 == nx) and not np.any(x0[:, :16] == nu) and not np.any(pr == nx[:, :16]) and not np.any(pr == nu)
        assert not np.any(x0[:, :16] == pr)
    assert MC.X0_BLOCK > 9 and MC.PARAM_BLOCK > PN.CONTROL_BLOCK + 3 and MC.X0_BLOCK + 9 < MC.PARAM_BLOCK
    # the normals of the noise are the words of t = 0 .. N-2 in blocks 0 .. 9 / 256 .. 259: the state stream at step 0 IS block 0's
    z = PN.state_normals(SEED, 0, False, 1, s, np.zeros_like(s), 4)
    assert np.array_equal(z, np.stack(PN.box_muller(*MC.words(SEED, 0, False, 1, s, 4, 0)[:, :2].T) +
                                      PN.box_muller(*MC.words(SEED, 0, False, 1, s, 4, 0)[:, 2:].T), axis=1))


# ---------------------------------------------------------------- the mirror reduction
def _cost_sets():
    """Costs like the ones the GPU tests reduce - positive, within a decade or two, S in {1, 64, 65, 130}, some samples uncounted -
    and an adversarial set: a large offset with a small spread, at a few thousand samples."""
    rng = np.random.default_rng(21)
    out = []
    for S in (1, 2, 64, 65, 130):
        out.append(("like S=%d" % S, 30.0 * np.exp(rng.standard_normal(S)), np.ones(S, dtype=bool)))
    c = 5.0 + rng.random(130)
    out.append(("ragged, a third uncounted", c, rng.random(130) > 1.0 / 3.0))
    out.append(("offset 1e9, spread 1e-3", 1e9 + 1e-3 * rng.standard_normal(4097), np.ones(4097, dtype=bool)))
    out.append(("offset -1e12, spread 1", -1e12 + rng.standard_normal(1000), rng.random(1000) > 0.1))
    out.append(("all equal", np.full(130, 0.1), np.ones(130, dtype=bool)))
    return out


@pytest.mark.parametrize("case", _cost_sets(), ids=lambda c: c[0])
def test_the_mirror_stays_within_the_bound_of_a_two_pass_extended_precision_reduction(case):
    """This checks the BOUND (policy_mc_np.moment_bounds), not the device: the mirror is one of the evaluation orders the bound has to
    cover, and the two-pass np.longdouble figures stand for the exact ones."""
    _, cost, counted = case
    n, mean, m2 = MC.mirror_moments(cost, counted)
    assert n == counted.sum()
    ref_mean, ref_m2 = MC.two_pass_longdouble(cost, counted)
    b_mean, b_m2 = MC.moment_bounds(cost, counted, float(ref_mean))
    assert abs(np.longdouble(mean) - ref_mean) <= b_mean, (float(abs(mean - ref_mean)), b_mean)
    assert abs(np.longdouble(m2) - ref_m2) <= b_m2, (float(abs(m2 - ref_m2)), b_m2)
    assert m2 >= 0.0
    print("%s: |mean - ref| / bound %.3f, |M2 - ref| / bound %.3f" % (case[0], float(abs(mean - ref_mean)) / b_mean if b_mean else 0.0,
                                                                       float(abs(m2 - ref_m2)) / b_m2 if b_m2 else 0.0))


def test_merge_of_two_windows_agrees_with_one_call():
    rng = np.random.default_rng(22)
    N = 9
    for S, cut in ((130, 64), (130, 70), (4097, 1000), (65, 1)):
        cost = 1e6 + 10.0 * rng.standard_normal(S)
        steps = np.where(rng.random(S) > 0.2, N - 1, 3)
        cost = np.where(steps == N - 1, cost, np.inf)
        cost[S // 2] = cost[0] = cost[:cut].min() - 1.0 if cut > 1 else cost[0]           # a tie of the minimum across the cut
        cost = np.where(steps == N - 1, cost, np.inf)
        one = MC.stats(cost, steps, N, first_sample=100)
        two = MC.merge_stats(MC.stats(cost[:cut], steps[:cut], N, first_sample=100), MC.stats(cost[cut:], steps[cut:], N, first_sample=100 + cut))
        for k in ("n", "counted", "success", "steps_total", "min", "max", "argmin", "argmax"):
            assert one[k] == two[k], (k, one[k], two[k])
        counted = (steps == N - 1)
        b_mean, b_m2 = MC.moment_bounds(cost, counted, one["mean"])
        assert abs(one["mean"] - two["mean"]) <= 2.0 * b_mean and abs(one["m2"] - two["m2"]) <= 2.0 * b_m2      # (each within the bound of the exact)
    # no counted sample on one side or on both
    dead = MC.stats(np.full(5, np.inf), np.zeros(5, dtype=int), N, first_sample=7)
    assert dead["counted"] == 0 and np.isnan(dead["mean"]) and np.isnan(dead["m2"]) and dead["min"] == np.inf and dead["max"] == -np.inf
    assert dead["argmin"] == dead["argmax"] == -1 and dead["steps_total"] == 0
    live = MC.stats(np.array([3.0, 1.0, 2.0]), np.full(3, N - 1), N, first_sample=12)
    for m in (MC.merge_stats(dead, live), MC.merge_stats(live, dead)):
        assert all(m[k] == live[k] for k in ("counted", "mean", "m2", "min", "max", "argmin", "argmax")) and m["n"] == 8
    both = MC.merge_stats(dead, dead)
    assert both["counted"] == 0 and np.isnan(both["mean"]) and both["argmin"] == -1


def test_the_count_zero_identity_holds_bit_for_bit():
    vals = [(3.0, 0.1 + 0.2, 1e-17), (1.0, -0.0, 0.0), (64.0, 1e300, 5e-324), (2.0, np.nextafter(1.0, 2.0), 7.0)]
    for v in vals:
        for got in (MC.merge(v, MC.EMPTY), MC.merge(MC.EMPTY, v)):
            assert all(np.float64(a).tobytes() == np.float64(b).tobytes() for a, b in zip(got, v)), (got, v)
    assert MC.merge(MC.EMPTY, MC.EMPTY) == MC.EMPTY
    # a group whose only counted sample sits in any lane: that sample's cost, M2 exactly 0
    for lane in (0, 1, 31, 63):
        cost, counted = np.full(64, 123.456), np.zeros(64, dtype=bool)
        counted[lane] = True
        assert MC.group_moments(cost, counted) == (1.0, 123.456, 0.0)
    # ... and the same through PolicyStats.merge
    from drake_ddp_amd.ilqr import PolicyStats
    i = lambda v: np.array([v], dtype=np.int64)   # noqa: E731
    f = lambda v: np.array([v], dtype=np.float64)   # noqa: E731
    a = PolicyStats(i(5), i(3), i(2), f(0.1 + 0.2), f(1e-17), f(0.25), f(0.375), i(9), i(11), i(40))
    e = PolicyStats(i(4), i(0), i(0), f(np.nan), f(np.nan), f(np.inf), f(-np.inf), i(-1), i(-1), i(6))
    for m in (a.merge(e), e.merge(a)):
        assert m.mean.tobytes() == a.mean.tobytes() and m.m2.tobytes() == a.m2.tobytes() and m.n[0] == 9 and m.counted[0] == 3
        assert m.min[0] == 0.25 and m.max[0] == 0.375 and m.argmin[0] == 9 and m.argmax[0] == 11 and m.steps_total[0] == 46
    ee = e.merge(e)
    assert np.isnan(ee.mean[0]) and ee.argmin[0] == -1 and ee.counted[0] == 0 and np.isnan(ee.var[0]) and ee.success_rate[0] == 0.0


def test_policy_stats_merge_is_the_mirrors_merge():
    from drake_ddp_amd.ilqr import PolicyStats
    rng = np.random.default_rng(23)
    N, S, cut = 5, 200, 77
    cost = 40.0 + rng.standard_normal((2, S))
    steps = np.full((2, S), N - 1)
    steps[1, ::3] = 1
    cost[1, ::3] = np.inf

    def ps(sl, first):
        d = [MC.stats(cost[b, sl], steps[b, sl], N, first_sample=first) for b in range(2)]
        col = lambda k, t: np.array([r[k] for r in d], dtype=t)   # noqa: E731
        return PolicyStats(*(col(k, np.float64 if k in ("mean", "m2", "min", "max") else np.int64) for k in MC.FIELDS)), d
    (a, da), (b_, db) = ps(slice(0, cut), 0), ps(slice(cut, S), cut)
    m = a.merge(b_)
    for b in range(2):
        want = MC.merge_stats(da[b], db[b])
        for k in MC.FIELDS:
            assert getattr(m, k)[b] == want[k], (b, k)
    assert np.allclose(m.var, m.m2 / (m.counted - 1)) and np.array_equal(m.success_rate, m.success / m.n)
