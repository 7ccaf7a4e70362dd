"""The multi-start spec against itself (tests/seeds_np.py; include/mi_ilqr.h: "Multi-start"): what a normal depends on, what hold does,
the elite slot, the tie rule, the eligibility rule and the no-winner fallback.  CPU only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import policy_noise_np as PN  # noqa: E402
import seeds_np as SN  # noqa: E402

SEED = PN.TEST_SEED
B, M, STEPS = 12, 5, 21


def _base(rng):
    return rng.uniform(-1.0, 1.0, (B, M, STEPS))


def test_the_counter_is_round_step_problem_block():
    """Normal j of step t of problem b is Box-Muller normal j mod 4 of the Philox block at (round, t, b, 768 + j / 4) under the key of
    the seed - stated once more here with the cipher itself."""
    z = SN.normals(SEED, 7, 3, STEPS, M)
    key = np.array([SEED & 0xFFFFFFFF, SEED >> 32], dtype=np.uint64)
    for t in (0, 5, STEPS - 1):
        for j in range(M):
            w = PN.philox4x32_10(np.array([7, t, 3, 768 + j // 4], dtype=np.uint64), key)
            pair = PN.box_muller(w[2 * ((j % 4) // 2)], w[2 * ((j % 4) // 2) + 1])
            assert z[j, t] == pair[j % 2], (t, j)
    assert not np.array_equal(z, SN.normals(SEED, 8, 3, STEPS, M)) and not np.array_equal(z, SN.normals(SEED + 1, 7, 3, STEPS, M))
    assert not np.array_equal(z, SN.normals(SEED, 7, 4, STEPS, M))
    PN.assert_moments(SN.noise(SEED, 0, 64, 40, 8).transpose(0, 2, 1))


def test_the_noise_does_not_depend_on_K():
    rng = np.random.default_rng(0)
    base, sigma = _base(rng), rng.uniform(0.1, 0.5, (B, M))
    runs = {K: SN.perturb(base, K, sigma, SEED, 2) for K in (1, 2, 3, 4, 6, 12)}
    for K, u in runs.items():
        elite = np.arange(B) % K == 0
        assert np.array_equal(u[elite], base[elite]), K                      # member 0 is untouched, bit for bit
        assert np.array_equal(u[~elite], runs[12][~elite]), K                # every other member: the same numbers whatever K
        assert K == 1 or not np.array_equal(u[~elite], base[~elite])
    assert np.array_equal(runs[1], base)                                     # K = 1: every problem is its group's elite


def test_the_noise_does_not_depend_on_how_the_batch_is_split():
    """Problems b0 .. b0 + B' - 1 drawn on their own are the rows of the whole batch: the counter holds the problem number."""
    whole = SN.noise(SEED, 1, B, STEPS, M, hold=3)
    for b0, nb in ((0, 5), (5, 7), (11, 1)):
        assert np.array_equal(SN.noise(SEED, 1, nb, STEPS, M, hold=3, b0=b0), whole[b0:b0 + nb])


def test_hold_repeats_a_value_over_exactly_hold_steps():
    for hold in (1, 2, 5, STEPS, STEPS + 3):
        z = SN.noise(SEED, 0, 3, STEPS, M, hold)
        one = SN.noise(SEED, 0, 3, STEPS, M, 1)
        for t in range(STEPS):
            assert np.array_equal(z[:, :, t], one[:, :, t // hold]), (hold, t)   # the value of step t div hold of the unheld stream
        changes = np.nonzero(np.any(z[:, :, 1:] != z[:, :, :-1], axis=(0, 1)))[0] + 1
        assert changes.tolist() == list(range(hold, STEPS, hold)), hold          # ... and it changes at every multiple of hold, only there


def test_sigma_zero_and_padding_rows_are_the_base_bit_for_bit():
    rng = np.random.default_rng(1)
    base = _base(rng)
    base[2, 1, 3] = -0.0                                                     # (base + 0 z would lose the sign)
    sigma = rng.uniform(0.1, 0.5, (B, M))
    sigma[:, 1] = 0.0
    sigma[4] = 0.0
    u = SN.perturb(base, 3, sigma, SEED)
    assert np.array_equal(u[:, 1], base[:, 1]) and np.array_equal(u[4], base[4]) and np.signbit(u[2, 1, 3])
    z = SN.noise(SEED, 0, B, STEPS, M)
    moved = (sigma != 0.0) & (np.arange(B) % 3 != 0)[:, None]
    assert np.array_equal(u[moved], (base + sigma[:, :, None] * z)[moved])


def test_the_tie_rule_and_the_eligibility_rule():
    C, X, L, I, P = SN.STATUS_CONVERGED, SN.STATUS_MAX_ITERS, 2, 3, 5        # converged, max_iters, line search failed, internal, not PD
    F = SN.FLAG_INDEFINITE
    cost = np.array([3.0, 1.0, 1.0, 2.0,      1.0, 0.5, 0.25, 9.0,      np.nan, np.inf, -np.inf, 1.0,      np.nan, np.inf, 4.0, 4.0])
    stat = np.array([C, C, X, C,              C, L, I, P,               C, C, C, L,                        C, C, X | F, C | F])
    best = SN.select(cost, stat, 4)
    assert best.tolist() == [[1.0, 1.0, 4.0],                                # equal costs: the lowest index
                             [0.0, 1.0, 1.0],                                # cheaper members with a failed status do not count
                             [-1.0, np.inf, 0.0],                            # NaN, +inf, -inf and a failed status: nobody
                             [2.0, 4.0, 2.0]]                                # the indefinite flag is masked off; NaN and +inf skipped
    assert SN.select(cost, stat, 1)[:, 0].tolist() == [0, 0, 0, 0, 0, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0]
    whole = SN.select(cost, stat, 16)
    assert whole.tolist() == [[1.0, 1.0, 7.0]]
    assert SN.select(np.array([-0.0, 0.0, 0.0, -0.0]), np.zeros(4, dtype=np.int32), 4)[0, 0] == 0.0   # -0 == +0: a tie


def test_reseed_and_its_fallback():
    rng = np.random.default_rng(2)
    K = 4
    u_bar = _base(rng)
    u_bar[9, 0, 2], u_bar[10, 3, 0], u_bar[8, 1, 1] = np.nan, np.inf, -np.inf
    sigma = rng.uniform(0.1, 0.5, (B, M))
    cost = np.array([5.0, 2.0, 7.0, 2.0,    1.0, 3.0, 3.0, 3.0,    np.nan, np.inf, np.nan, np.inf])
    stat = np.zeros(B, dtype=np.int32)
    u, best = SN.reseed(u_bar, cost, stat, K, sigma, SEED, round=1, hold=2)
    assert best[:, 0].tolist() == [1.0, 0.0, -1.0]
    z = SN.noise(SEED, 1, B, STEPS, M, hold=2)
    assert np.array_equal(u[1], u_bar[1]) and np.array_equal(u[4], u_bar[4])                 # the winners' slots: their own controls
    for b, w in ((0, 1), (2, 1), (3, 1), (5, 4), (6, 4), (7, 4)):
        assert np.array_equal(u[b], u_bar[w] + sigma[b][:, None] * z[b]), b                  # the others: the winner's + their own noise
    clean = np.where(np.isfinite(u_bar), u_bar, 0.0)
    assert np.array_equal(u[8], clean[8]) and u[8, 1, 1] == 0.0                              # no winner: member 0 its own, non-finite -> 0
    for b in (9, 10, 11):
        assert np.array_equal(u[b], clean[b] + sigma[b][:, None] * z[b]) and np.isfinite(u[b]).all(), b
    x_bar = rng.uniform(-1.0, 1.0, (B, 3, STEPS + 1))
    gx, gu, gc, gb = SN.gather(x_bar, u_bar, cost, stat, K)
    assert np.array_equal(gb, best)
    assert np.array_equal(gx[0], x_bar[1]) and np.array_equal(gu[1], u_bar[4]) and gc.tolist() == [2.0, 1.0, np.inf]
    assert np.isnan(gx[2]).all() and np.isnan(gu[2]).all()
