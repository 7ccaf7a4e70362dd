"""Multi-start on the device (BatchedIterativeLQR.PerturbInitialGuess / SelectBest / ReseedFromBest / GatherBest / SolveMultiStart;
MI_F_SEEDS_*; csrc/seeds.hpp) against the NumPy statement of the four operations (tests/seeds_np.py), on one handle per kernel
layout: the wave-per-problem pendulum (time last), the lane-per-problem pendulum (batch minor), the 36-state chain (time major)
and the chainx plugin with a padding control.  Horizons with N - 1 no multiple of 64 (N = 9, 70), K = 1 and 3 on B = 9, and groups
of 65 and 130 members: more than one wave, more than one trip of the strided loop.

A perturbed entry is base + sigma z with a rounded product and a rounded sum on both sides, so the device and the spec differ by
sigma |z_device - z_spec|: the bound is policy_noise_np.NORMAL_TOL - what tests/test_gpu_policy_noise.py holds a device normal to -
times sigma.  The test data keep |base + sigma z| below 8 and sigma at 0.25 or 0.5: the two roundings of the sum where the normals
differ (2^-51 at most) stay below a tenth of that bound, inside the factor 4 NORMAL_TOL already leaves."""
import functools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "plugins"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import policy_noise_np as PN  # noqa: E402
import seeds_np as SN  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = PN.TEST_SEED
B = 9
FAMILIES = ("pendulum", "pendulum_throughput", "synth36")          # time last, batch minor, time major


def _problem(name, N):
    from drake_ddp_amd import workloads as W
    if name.startswith("pendulum"):
        return dict(W.pendulum_problem(), N=N), W.pendulum_batch_x0, np.zeros((1, N - 1)), "throughput" if name.endswith("throughput") else "auto"
    return W.synth36_problem(N), W.synth36_batch_x0, W.synth36_u_guess(N), "auto"


def _solver(name, N, batch=B, **kw):
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    from drake_ddp_amd.models import ModelSystem
    p, x0, ug, mode = _problem(name, N)
    s = BatchedIterativeLQR(ModelSystem(p["model_id"], p["dt"]), N, batch, delta=p["delta"], beta=p["beta"], gamma=p["gamma"], device=0,
                            kernel_mode=mode, **kw)
    s.SetTargetState(p["x_nom"]); s.SetRunningCost(p["Q"], p["R"]); s.SetTerminalCost(p["Qf"])
    s.SetInitialState(x0(batch))
    return s, ug


def _solve(s):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # (a problem stopped at max_iters is an outcome here, not a failure)
        s.Solve()
    return _state(s)


def _state(s):
    return dict(x=np.array(s.x_bar), u=np.array(s.u_bar), cost=np.array(s.cost), it=np.array(s.iterations), st=np.array(s.status))


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("x", "u", "cost", "it", "st"))


def _sigma(rng, batch, m):
    """(B, m) rows of 0, 0.25 and 0.5, every value present."""
    s = rng.choice([0.0, 0.25, 0.5], size=(batch, m))
    s.flat[:3] = (0.0, 0.25, 0.5)
    return s


def _check_noise(got, want, exact, sigma):
    """`exact` (B, m) marks the rows that must be bitwise the spec's; the others agree to NORMAL_TOL sigma.  -> the worst ratio."""
    ex = np.broadcast_to(exact[:, :, None], got.shape)
    assert np.array_equal(got[ex], want[ex])
    bound = np.broadcast_to((PN.NORMAL_TOL * sigma)[:, :, None], got.shape)
    err = np.abs(got - want)
    assert np.all(err[~ex] <= bound[~ex]), float(np.max(err[~ex] / bound[~ex]))
    assert np.abs(want).max() < 8.0
    return float(np.max(err[~ex] / bound[~ex])) if (~ex).any() else 0.0


def _set_cost(s, cost):
    from drake_ddp_amd import _capi
    s._set(_capi.F_COST, np.asarray(cost, dtype=np.float64), (s.B,))


# ---------------------------------------------------------------- 1. perturb against the spec
@pytest.mark.parametrize("N", [9, 70])
@pytest.mark.parametrize("name", FAMILIES)
def test_perturb_against_the_spec(name, N):
    """The pending guess read back through MI_F_U_BAR against tests/seeds_np.py, K = 1 and 3, hold = 1 and 4; then the two other
    bases: zeros on a reset handle, u_bar on a solved one."""
    s, _ = _solver(name, N)
    m = s.m
    rng = np.random.default_rng(N)
    worst = 0.0
    for K, hold, rnd in ((1, 1, 0), (3, 1, 3), (3, 4, 2 ** 32 - 1)):
        base, sigma = rng.uniform(-1.0, 1.0, (B, m, N - 1)), _sigma(rng, B, m)
        s.Reset(); s.SetInitialGuess(base)
        s.PerturbInitialGuess(K, sigma, seed=SEED, round=rnd, hold=hold)
        got = np.array(s.u_bar)
        exact = (sigma == 0.0) | (np.arange(B) % K == 0)[:, None]
        worst = max(worst, _check_noise(got, SN.perturb(base, K, sigma, SEED, rnd, hold), exact, sigma))
        assert np.array_equal(got[::K], base[::K])                              # member 0: the base
        s.PerturbInitialGuess(K, sigma, seed=SEED, round=rnd, hold=hold)       # again: the base is now the pending guess, in place
        again = np.array(s.u_bar)
        assert np.array_equal(again[exact], base[exact]) and (K == 1 or not np.array_equal(again, got))
    sigma = np.full((B, m), 0.5)
    s.Reset()
    s.PerturbInitialGuess(3, sigma, seed=SEED)                                # a reset handle: zeros
    exact = np.broadcast_to((np.arange(B) % 3 == 0)[:, None], (B, m))
    worst = max(worst, _check_noise(np.array(s.u_bar), SN.perturb(np.zeros((B, m, N - 1)), 3, sigma, SEED), exact, sigma))
    if N == 9:
        s.Reset(); s.SetInitialGuess(_problem(name, N)[2])
        u = np.clip(_solve(s)["u"], -4.0, 4.0)                                # (the data stay inside the bound's premise)
        s.set_state(u_bar=u)
        s.PerturbInitialGuess(3, 0.25, seed=SEED + 1, round=1)                # a solved handle: its u_bar
        want = SN.perturb(u, 3, np.full((B, m), 0.25), SEED + 1, 1)
        worst = max(worst, _check_noise(np.array(s.u_bar), want, exact, np.full((B, m), 0.25)))
    print("seeds perturb %s N=%d: worst error / (NORMAL_TOL sigma) = %.3f; kernel %.4f ms" % (name, N, worst, s.seeds_kernel_ms()))


@pytest.mark.parametrize("name,K", [("pendulum", 65), ("pendulum", 130), ("pendulum_throughput", 130), ("synth36", 65)])
def test_perturb_and_select_on_groups_wider_than_a_wave(name, K):
    """G = 2 groups of 65 and of 130 members: the strided loop over the members, the butterfly inside the wave and the step
    through LDS across the waves all carry candidates; costs doctored to ties, NaN and infinities."""
    N, batch = 9, 2 * K
    s, ug = _solver(name, N, batch)
    s.SetInitialGuess(ug)
    st = _solve(s)
    rng = np.random.default_rng(K)
    base, sigma = rng.uniform(-1.0, 1.0, (batch, s.m, N - 1)), _sigma(rng, batch, s.m)
    for trial in range(4):
        cost = rng.integers(0, 12, batch).astype(float)                        # many ties
        cost[rng.integers(0, batch, 20)] = (np.nan, np.inf, -np.inf, -1.0)[trial]
        if trial == 3:
            cost[K:] = np.inf; cost[K + 7] = np.nan                            # a whole group without a winner
            cost[:K] = 5.0; cost[K - 1] = 4.0; cost[K - 2] = 4.0               # the winner in the last wave, a tie beside it
        _set_cost(s, cost)
        sel = s.SelectBest(K)
        want = SN.select(cost, st["st"], K)
        assert np.array_equal(sel.winner, want[:, 0]) and np.array_equal(sel.cost, want[:, 1]) and np.array_equal(sel.eligible, want[:, 2]), trial
        for K2 in (1, 2, 5):                              # ... and the same costs in narrower groups
            w2 = SN.select(cost, st["st"], K2)
            s2 = s.SelectBest(K2)
            assert np.array_equal(s2.winner, w2[:, 0]) and np.array_equal(s2.cost, w2[:, 1]) and np.array_equal(s2.eligible, w2[:, 2]), (trial, K2)
    assert want.tolist()[1] == [-1.0, np.inf, 0.0] and want[0, 0] == K - 2
    s.SetInitialGuess(base)
    s.PerturbInitialGuess(K, sigma, seed=SEED, round=5, hold=3)
    exact = (sigma == 0.0) | (np.arange(batch) % K == 0)[:, None]
    _check_noise(np.array(s.u_bar), SN.perturb(base, K, sigma, SEED, 5, 3), exact, sigma)


@functools.lru_cache(maxsize=None)
def _padded():
    import models as PM
    return PM.build_chainx(16, 3, 5)(0.02)


def test_padding_controls_get_no_noise():
    """The chainx plugin with n = 37 > 32 and m = 3: four device controls.  The caller's rows are perturbed like any, the padding row
    stays an exact zero, and a sigma on it is refused."""
    from drake_ddp_amd import _capi
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    sys_ = _padded()
    n, m, N = sys_.n, sys_.m, 12
    assert m == 3 and sys_.m_dev == 4
    s = BatchedIterativeLQR(sys_, N, B, delta=1e-3, beta=0.6, gamma=0.0, device=0, max_iters=3)
    s.SetTargetState(np.zeros(n)); s.SetRunningCost(0.02 * np.eye(n), 0.002 * np.eye(m)); s.SetTerminalCost(5.0 * np.eye(n))
    rng = np.random.default_rng(4)
    s.SetInitialState(0.3 * rng.standard_normal((B, n)))
    base, sigma = rng.uniform(-1.0, 1.0, (B, m, N - 1)), _sigma(rng, B, m)
    s.SetInitialGuess(base)
    s.PerturbInitialGuess(3, sigma, seed=SEED, hold=2)
    exact = (sigma == 0.0) | (np.arange(B) % 3 == 0)[:, None]
    _check_noise(np.array(s.u_bar), SN.perturb(base, 3, sigma, SEED, 0, 2), exact, sigma)
    raw = np.empty((B, 4, N - 1))
    assert s._lib.mi_ilqr_get(s._h, _capi.F_U_BAR, _capi.ptr(raw), raw.nbytes) == _capi.OK
    assert np.all(raw[:, 3] == 0.0) and not np.signbit(raw[:, 3]).any()
    rows = np.zeros((B, 4)); rows[:, :3] = sigma
    assert s._lib.mi_ilqr_set(s._h, _capi.F_SEEDS_SIGMA, _capi.ptr(rows), rows.nbytes) == _capi.OK
    back = np.empty((B, 4))
    assert s._lib.mi_ilqr_get(s._h, _capi.F_SEEDS_SIGMA, _capi.ptr(back), back.nbytes) == _capi.OK and np.array_equal(back, rows)
    bad = rows.copy(); bad[2, 3] = 1e-3
    assert s._lib.mi_ilqr_set(s._h, _capi.F_SEEDS_SIGMA, _capi.ptr(bad), bad.nbytes) == _capi.E_BAD_ARG
    user = np.zeros((B, 3))                                                    # (a row has the DEVICE's number of controls)
    assert s._lib.mi_ilqr_set(s._h, _capi.F_SEEDS_SIGMA, _capi.ptr(user), user.nbytes) == _capi.E_BAD_SHAPE
    st = _solve(s)                                                             # ... and the gather cuts the padding row off
    x, u, c, sel = s.GatherBest(3)
    pick = np.arange(3) * 3 + sel.winner
    assert u.shape == (3, m, N - 1) and np.array_equal(u, st["u"][pick]) and np.array_equal(x, st["x"][pick]) and np.array_equal(c, st["cost"][pick])


# ---------------------------------------------------------------- 2. identity
@pytest.mark.parametrize("name,N", [("pendulum", 70), ("pendulum_throughput", 70), ("synth36", 9)])
def test_sigma_zero_is_the_plain_solve(name, N):
    """PerturbInitialGuess with sigma = 0, then Solve, against SetInitialGuess(base) + Solve on a twin handle: x_bar, u_bar, cost,
    iterations and status, bitwise - with the guess pending and with the base taken from a solved handle's u_bar."""
    s, ug = _solver(name, N)
    twin, _ = _solver(name, N)
    rng = np.random.default_rng(7)
    base = np.broadcast_to(ug, (B, s.m, N - 1)) + 0.01 * rng.standard_normal((B, s.m, N - 1))
    s.SetInitialGuess(base); twin.SetInitialGuess(base)
    s.PerturbInitialGuess(3, 0.0, seed=SEED)
    assert np.array_equal(np.array(s.u_bar), base)
    a, b = _solve(s), _solve(twin)
    assert _same(a, b), name
    s.PerturbInitialGuess(3, np.zeros(s.m), seed=SEED, round=1)              # warm: the base is u_bar, the solve after it is cold
    twin.Reset(); twin.SetInitialGuess(b["u"])
    assert _same(_solve(s), _solve(twin)), name


# ---------------------------------------------------------------- 3. selection
def _sel_eq(sel, want):
    return np.array_equal(sel.winner, want[:, 0]) and np.array_equal(sel.cost, want[:, 1]) and np.array_equal(sel.eligible, want[:, 2])


@pytest.mark.parametrize("name,N", [("pendulum", 70), ("pendulum_throughput", 70), ("synth36", 9)])
def test_select_on_solver_output_and_doctored_costs(name, N):
    s, ug = _solver(name, N)
    s.SetInitialGuess(ug)
    st = _solve(s)
    assert np.isin(st["st"], (0, 1)).all() and len(set(st["cost"].tolist())) == B
    for K in (1, 3, 9):
        sel = s.SelectBest(K)
        assert _sel_eq(sel, SN.select(st["cost"], st["st"], K)), K
        assert np.array_equal(sel.problem, np.arange(B // K) * K + sel.winner)
    cost = np.array([2.0, 1.0, 1.0,   np.inf, np.nan, 3.0,   np.nan, np.inf, -np.inf])
    _set_cost(s, cost)
    sel = s.SelectBest(3)
    assert sel.winner.tolist() == [1, 2, -1] and sel.cost.tolist() == [1.0, 3.0, np.inf] and sel.eligible.tolist() == [3, 1, 0]
    assert _sel_eq(sel, SN.select(cost, st["st"], 3)) and _sel_eq(s.SelectBest(9), SN.select(cost, st["st"], 9))
    assert _same(_state(s), dict(st, cost=cost))                              # a select writes nothing


def test_max_iters_members_are_eligible_and_a_failed_line_search_is_not():
    """max_iters = 1: every problem stops with MAX_ITERS and stays eligible.  The ineligible-by-status case reuses the recipe of
    tests/test_gpu_properties.py::test_a_poisoned_problem_fails_alone - a NaN in one problem's x0 ends it with LINESEARCH_FAILED - and
    gives that member the group's lowest (finite) cost: it still does not win."""
    from drake_ddp_amd import _capi, workloads as W
    s, ug = _solver("pendulum", 70, max_iters=1)
    s.SetInitialGuess(ug)
    st = _solve(s)
    assert (st["st"] == _capi.STATUS_MAX_ITERS).all()
    sel = s.SelectBest(3)
    assert (sel.eligible == 3).all() and _sel_eq(sel, SN.select(st["cost"], st["st"], 3))
    t, ug = _solver("pendulum", 70)
    x0 = W.pendulum_batch_x0(B); x0[4, 0] = np.nan
    t.SetInitialState(x0); t.SetInitialGuess(ug)
    st = _solve(t)
    assert st["st"][4] == _capi.STATUS_LINESEARCH_FAILED and np.isin(np.delete(st["st"], 4), (0, 1)).all()
    cost = st["cost"].copy(); cost[4] = 1e-6
    _set_cost(t, cost)
    sel = t.SelectBest(3)
    assert sel.winner[1] in (0, 2) and sel.eligible.tolist() == [3, 2, 3] and _sel_eq(sel, SN.select(cost, st["st"], 3))


# ---------------------------------------------------------------- 4. reseed
@pytest.mark.parametrize("name,N", [("pendulum", 70), ("pendulum_throughput", 70), ("synth36", 9)])
def test_reseed_from_the_best(name, N):
    """Group 0 has a tie, group 1 a winner in its last slot, group 2 no winner and non-finite controls: the fallback.  Then the
    solve after the reseed against a reset twin handle given the same guesses, bitwise."""
    K = 3
    s, ug = _solver(name, N)
    s.SetInitialGuess(ug)
    st = _solve(s)
    u = np.clip(st["u"], -4.0, 4.0)
    u[6, 0, 1], u[7, -1, -1], u[8, 0, 0] = np.nan, np.inf, -np.inf
    s.set_state(u_bar=u)
    cost = np.array([2.0, 1.0, 1.0,   5.0, np.nan, 3.0,   np.nan, np.inf, np.nan])
    _set_cost(s, cost)
    sigma = _sigma(np.random.default_rng(11), B, s.m)
    sigma[2] = 0.5
    sel = s.ReseedFromBest(K, sigma, seed=SEED, round=1, hold=2)
    want, best = SN.reseed(u, cost, st["st"], K, sigma, SEED, 1, 2)
    assert _sel_eq(sel, best) and sel.winner.tolist() == [1, 2, -1]
    got = np.array(s.u_bar)                                                    # (the pending guesses)
    exact = sigma == 0.0
    exact[[1, 5, 6]] = True                                                    # the winners' slots, the fallback's member 0
    _check_noise(got, want, exact, sigma)
    assert np.array_equal(got[1], u[1]) and np.array_equal(got[5], u[5])       # bitwise their own u_bar
    assert np.isfinite(got).all() and got[6, 0, 1] == 0.0 and np.array_equal(got[6], np.where(np.isfinite(u[6]), u[6], 0.0))
    assert not np.array_equal(got[2], u[1])
    after = _solve(s)
    twin, _ = _solver(name, N)
    twin.SetInitialGuess(got)
    assert _same(after, _solve(twin)), name
    u2 = np.clip(after["u"], -4.0, 4.0)
    s.set_state(u_bar=u2)
    s.ReseedFromBest(K, sigma, seed=SEED, round=2)                            # (real costs and statuses now)
    s.ReseedFromBest(K, sigma, seed=SEED, round=2)                            # with the guesses pending: every member reads the winner's slot in place
    want2, _ = SN.reseed(SN.reseed(u2, after["cost"], after["st"], K, sigma, SEED, 2)[0], after["cost"], after["st"], K, sigma, SEED, 2)
    win = (np.arange(B // K) * K + SN.select(after["cost"], after["st"], K)[:, 0]).astype(int)
    exact = sigma == 0.0
    exact[win] = True
    _check_noise(np.array(s.u_bar), want2, exact, sigma)
    assert np.array_equal(np.array(s.u_bar)[win], u2[win])


# ---------------------------------------------------------------- 5. gather
@pytest.mark.parametrize("name,N", [("pendulum", 70), ("pendulum_throughput", 70), ("synth36", 9)])
def test_gather_and_no_side_effects(name, N):
    s, ug = _solver(name, N)
    twin, _ = _solver(name, N)
    s.SetInitialGuess(ug); twin.SetInitialGuess(ug)
    st = _solve(s)
    assert _same(st, _solve(twin))
    for K in (1, 3):
        x, u, c, sel = s.GatherBest(K)
        pick = np.arange(B // K) * K + sel.winner
        assert _sel_eq(sel, SN.select(st["cost"], st["st"], K))
        assert np.array_equal(x, st["x"][pick]) and np.array_equal(u, st["u"][pick]) and np.array_equal(c, st["cost"][pick]), K
    s.SelectBest(3)
    assert _same(_state(s), st)
    assert _same(_solve(s), _solve(twin)), name                               # the warm solve after select and gather: the twin's
    cost = np.array(s.cost)
    cost[3:6] = (np.nan, np.inf, np.nan)
    _set_cost(s, cost)
    now = _state(s)
    x, u, c, sel = s.GatherBest(3)
    wx, wu, wc, wb = SN.gather(now["x"], now["u"], cost, now["st"], 3)
    assert sel.winner[1] == -1 and np.isnan(x[1]).all() and np.isnan(u[1]).all() and c[1] == np.inf
    assert np.array_equal(x, wx, equal_nan=True) and np.array_equal(u, wu, equal_nan=True) and np.array_equal(c, wc) and _sel_eq(sel, wb)


# ---------------------------------------------------------------- 6. best of K never loses
def test_best_of_k_never_loses():
    """Pendulum swing-up, G = 8 random starts x K = 4 seeds, two rounds.  Round 0: member 0 is the unperturbed start, so its cost is
    bitwise the cost of the same start solved alone, and the group's best is <= it - by construction, no tolerance.  Round 1: the
    winner's slot is re-solved cold from its own converged controls; the line search only accepts a lower cost, so the re-solve
    can end above the cost it started from only by the rounding of its first rollout.  That is held to the reference's own one-ulp
    spread, the rule of tests/test_gpu_tracking.py: the C oracle re-solves each winner from the same controls with x0 moved by
    one ulp up and down, and ten times the largest change of its cost is the slack of that group (printed beside the excess)."""
    from drake_ddp_amd import workloads as W
    from oracle import c_oracle, models_np as M
    G, K, N = 8, 4, 70
    p = dict(W.pendulum_problem(), N=N)
    x0 = np.repeat(W.pendulum_batch_x0(G, seed=5), K, axis=0)
    s, ug = _solver("pendulum", N, G * K)
    alone, _ = _solver("pendulum", N, G)
    s.SetInitialState(x0); alone.SetInitialState(x0[::K])
    s.SetInitialGuess(ug); alone.SetInitialGuess(ug)
    ref = _solve(alone)
    s.PerturbInitialGuess(K, 0.5, seed=SEED, hold=10)
    r0 = _solve(s)
    assert np.array_equal(r0["cost"][::K], ref["cost"]) and np.array_equal(r0["u"][::K], ref["u"]) and np.array_equal(r0["it"][::K], ref["it"])
    sel0 = s.ReseedFromBest(K, 0.25, seed=SEED, round=1, hold=10)
    assert (sel0.winner >= 0).all() and np.all(sel0.cost <= r0["cost"][::K])          # no tolerance
    assert np.array_equal(sel0.cost, r0["cost"][sel0.problem])
    r1 = _solve(s)
    x, u, c, sel1 = s.GatherBest(K)
    model = M.Model(p["model_id"], p["dt"])
    uw, xw = r0["u"][sel0.problem], x0[sel0.problem]
    base = c_oracle.solve_batch(model, p, xw, uw, want_arrays=False)["cost"]
    spread = np.zeros(G)
    for d in (np.inf, -np.inf):
        spread = np.maximum(spread, np.abs(c_oracle.solve_batch(model, p, np.nextafter(xw, d), uw, want_arrays=False)["cost"] - base))
    excess = sel1.cost - sel0.cost
    print("best-of-K: improved on member 0 in %d of %d groups (round 0), on round 0 in %d (round 1); largest excess %.3e, slack %s"
          % (int((sel0.cost < r0["cost"][::K]).sum()), G, int((excess < 0).sum()), float(excess.max()), (10.0 * spread).tolist()))
    assert np.all(excess <= 10.0 * spread), (excess.tolist(), spread.tolist())
    assert np.array_equal(c, sel1.cost) and np.array_equal(c, r1["cost"][sel1.problem])
    # ... and the loop as one call gives the same winners
    t, _ = _solver("pendulum", N, G * K)
    t.SetInitialState(x0); t.SetInitialGuess(ug)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        x2, u2, c2, sels = t.SolveMultiStart(K, 2, 0.5, seed=SEED, hold=10, shrink=0.5)
    assert len(sels) == 2 and np.array_equal(sels[0].winner, sel0.winner) and np.array_equal(sels[0].cost, sel0.cost)
    assert np.array_equal(c2, c) and np.array_equal(x2, x) and np.array_equal(u2, u) and np.array_equal(sels[1].winner, sel1.winner)


# ---------------------------------------------------------------- 7. refusals
def test_refusals_leave_the_handle_alone():
    from drake_ddp_amd import _capi
    s, ug = _solver("pendulum", 70)
    twin, _ = _solver("pendulum", 70)
    lib, h = s._lib, s._h
    run = lambda *v: lib.mi_ilqr_set(h, _capi.F_SEEDS_RUN, _capi.ptr(np.array(v, dtype=np.float64)), 8 * len(v))   # noqa: E731
    out = np.empty(B * 2 * 70)
    for which, cnt in ((_capi.F_SEEDS_BEST, 9), (_capi.F_SEEDS_X_BAR, 3 * 2 * 70), (_capi.F_SEEDS_U_BAR, 3 * 69), (_capi.F_SEEDS_COST, 3),
                       (_capi.F_SEEDS_KERNEL_MS, 1)):
        assert lib.mi_ilqr_get(h, which, _capi.ptr(out), cnt * 8) == _capi.E_BAD_ARG, which        # nothing selected, nothing run yet
    s.SetInitialGuess(ug); twin.SetInitialGuess(ug)
    s._push_problem()
    assert run(2, 0, 0, 0, 1, 0) == _capi.E_BAD_ARG                            # K does not divide B
    assert run(0, 0, 0, 0, 1, 0) == _capi.E_BAD_ARG and run(-3, 0, 0, 0, 1, 0) == _capi.E_BAD_ARG and run(1.5, 0, 0, 0, 1, 0) == _capi.E_BAD_ARG
    assert run(3, 0, 0, 0, 0, 0) == _capi.E_BAD_ARG                            # hold = 0
    assert run(3, 4, 0, 0, 1, 0) == _capi.E_BAD_ARG and run(3, -1, 0, 0, 1, 0) == _capi.E_BAD_ARG   # unknown op
    assert run(3, 0, -1, 0, 1, 0) == _capi.E_BAD_ARG and run(3, 0, 0, 2.0 ** 32, 1, 0) == _capi.E_BAD_ARG
    assert run(3, 0, 0, 0, 1, 1) == _capi.E_BAD_ARG and run(3, 0, np.nan, 0, 1, 0) == _capi.E_BAD_ARG
    assert run(3, 0, 0, 0, 1) == _capi.E_BAD_SHAPE
    assert lib.mi_ilqr_set(h, _capi.F_SEEDS_RUN, None, 48) == _capi.E_BAD_ARG
    for bad in (-0.1, np.nan, np.inf):
        rows = np.full((B, 1), 0.1); rows[4, 0] = bad
        assert lib.mi_ilqr_set(h, _capi.F_SEEDS_SIGMA, _capi.ptr(rows), rows.nbytes) == _capi.E_BAD_ARG, bad
    assert lib.mi_ilqr_set(h, _capi.F_SEEDS_SIGMA, _capi.ptr(np.zeros(B + 1)), (B + 1) * 8) == _capi.E_BAD_SHAPE
    for which in (_capi.F_SEEDS_BEST, _capi.F_SEEDS_X_BAR, _capi.F_SEEDS_U_BAR, _capi.F_SEEDS_COST, _capi.F_SEEDS_KERNEL_MS):
        assert lib.mi_ilqr_set(h, which, _capi.ptr(out), 8) == _capi.E_BAD_ARG                      # read-only
    assert lib.mi_ilqr_get(h, _capi.F_SEEDS_RUN, _capi.ptr(out), 48) == _capi.E_BAD_ARG             # write-only
    assert lib.mi_ilqr_get(h, _capi.F_SEEDS_BEST, _capi.ptr(out), 72) == _capi.E_BAD_ARG            # (still nothing selected)
    back = np.ones((B, 1))
    assert lib.mi_ilqr_get(h, _capi.F_SEEDS_SIGMA, _capi.ptr(back), back.nbytes) == _capi.OK and np.all(back == 0.0)   # no rows were taken
    for K, kw in ((2, {}), (3, {"hold": 0}), (3, {"sigma_u": -1.0})):          # the class decides the same before the library sees it
        with pytest.raises(ValueError):
            s.PerturbInitialGuess(K, kw.pop("sigma_u", 0.1), **kw)
    assert _same(_solve(s), _solve(twin))                                      # the handle solves as if nothing had been asked
    assert run(3, 1, 0, 0, 1, 0) == _capi.OK
    assert lib.mi_ilqr_get(h, _capi.F_SEEDS_BEST, _capi.ptr(out), 64) == _capi.E_BAD_SHAPE
    assert lib.mi_ilqr_get(h, _capi.F_SEEDS_BEST, _capi.ptr(out), 72) == _capi.OK
    assert lib.mi_ilqr_get(h, _capi.F_SEEDS_COST, _capi.ptr(out), 24) == _capi.E_BAD_ARG            # a select is no gather
    ms = np.empty(1)
    assert lib.mi_ilqr_get(h, _capi.F_SEEDS_KERNEL_MS, _capi.ptr(ms), 8) == _capi.OK and 0.0 < ms[0] < 100.0
    small, ug3 = _solver("pendulum", 70, 3)                                    # B <= 4, wave per problem: the inputs live in host memory
    small.SetInitialGuess(ug3)
    ref3, _ = _solver("pendulum", 70, 3)
    ref3.SetInitialGuess(ug3)
    small._push_problem()
    v = np.array([3, 0, 0, 0, 1, 0], dtype=np.float64)
    for op in range(4):
        v[1] = op
        assert small._lib.mi_ilqr_set(small._h, _capi.F_SEEDS_RUN, _capi.ptr(v), 48) == _capi.E_UNSUPPORTED
    with pytest.raises(ValueError, match="host"):
        small.SelectBest(3)
    assert _same(_solve(small), _solve(ref3))


# ---------------------------------------------------------------- 8. the example
def test_the_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "multistart_pendulum.py"), "--groups", "8", "--seeds", "4",
                        "--rounds", "2", "--steps", "70"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "multistart_pendulum: OK", r.stdout[-3000:]
    assert any("strictly below member 0" in ln for ln in lines) and sum(ln.startswith("round ") for ln in lines) == 2
