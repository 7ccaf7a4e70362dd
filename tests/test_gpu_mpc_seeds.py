"""Multi-start in the receding-horizon loop (BatchedIterativeLQR.MPCRunMultiStart; the long form of MI_F_SEEDS_RUN;
csrc/seeds.hpp: seeds_mpc_join_kernel) against the same loop written out with the pieces the library already has, on a twin handle
in the same state and BIT FOR BIT: per re-solve MPCShift, ReseedFromBest at round + r, the winner's x_bar[:, replan_steps] read back
and handed to every member of its group (each member's own in a group without a winner), solve_resident.  The handles are those of
tests/test_gpu_seeds.py - pendulum (time last), pendulum_throughput (batch minor), synth36 (time major), the chainx plugin with a
padding control.  B = 9, K = 3, N = 12, replan_steps 2, three re-solves unless a case says otherwise: N - 1 = 11 is no multiple of a
hold of 5 or 3, and the shift moves the window boundaries of the noise against the plan's."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "plugins"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import seeds_np as SN  # noqa: E402
from test_gpu_seeds import B, FAMILIES, SEED, _padded, _same, _set_cost, _sigma, _solve, _solver, _state  # noqa: E402

pytestmark = pytest.mark.gpu

N, K, REPLAN, R = 12, 3, 2, 3


def _run(s, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # (a problem stopped at max_iters is an outcome here, not a failure)
        return s.MPCRunMultiStart(*a, **kw)


def _set_x0(s, x0):
    """x0 alone, straight to the handle: a pending guess and the targets stay what they are."""
    from drake_ddp_amd import _capi
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    _capi.check(s._lib.mi_ilqr_set_initial(s._h, _capi.ptr(x0), None), "mi_ilqr_set_initial")


def _pieces_round(t, k, sigma, seed, rnd, hold, replan):
    """One round of the loop by its pieces on `t` -> (the selection it used, the x0 it gave)."""
    x = np.array(t.x_bar)
    t.MPCShift(replan)
    sel = t.ReseedFromBest(k, sigma, seed=seed, round=rnd, hold=hold)
    src = np.where(np.repeat(sel.winner, k) >= 0, np.repeat(sel.problem, k), np.arange(t.B))
    x0 = np.ascontiguousarray(x[src][:, :, replan])
    _set_x0(t, x0)
    t.solve_resident()
    return sel, x0


def _sel_same(a, b):
    return np.array_equal(a.winner, b.winner) and np.array_equal(a.cost, b.cost) and np.array_equal(a.eligible, b.eligible)


def _sel_is(sel, rows):
    return np.array_equal(sel.winner, rows[:, 0]) and np.array_equal(sel.cost, rows[:, 1]) and np.array_equal(sel.eligible, rows[:, 2])


def _against_the_pieces(make, k, rounds, replan, hold, sigma, doctor=None, rnd0=4):
    """Three handles in one state (`make` -> a solved solver): `one` runs MPCRunMultiStart(k, rounds, ..) once, `split` runs it
    `rounds` times for one re-solve with `round` advanced by hand, `twin` runs the pieces.  After every round split == twin in
    x_bar, u_bar, cost, iterations, status, the MPC log row and both selections; at the end one == twin, its log the rows gathered."""
    one, split, twin = make(), make(), make()
    first = _state(one)
    assert _same(first, _state(split)) and _same(first, _state(twin))
    if doctor is not None:
        for s in (one, split, twin):
            _set_cost(s, doctor(first["cost"]))
    rows, sels, failed = [], [], []
    for r in range(rounds):
        sel, x0 = _pieces_round(twin, k, sigma, SEED, rnd0 + r, hold, replan)
        got = _run(split, k, 1, replan, sigma, seed=SEED, round=rnd0 + r, hold=hold)
        now = _state(twin)
        assert _same(_state(split), now), r
        assert len(got) == 2 and _sel_same(got[0], sel) and _sel_is(got[1], SN.select(now["cost"], now["st"], k)), r
        row = np.concatenate([x0, now["cost"][:, None], now["it"][:, None].astype(float)], axis=1)
        assert np.array_equal(split.mpc_log[:, 0, :], row, equal_nan=True), r
        rows.append(row); sels.append(sel); failed.append((now["st"] & ~16) >= 2)
        assert split.seeds_kernel_ms() > 0.0
    got = _run(one, k, rounds, replan, sigma, seed=SEED, round=rnd0, hold=hold)
    now = _state(twin)
    assert _same(_state(one), now)
    assert len(got) == rounds + 1 and all(_sel_same(a, b) for a, b in zip(got, sels)) and _sel_is(got[-1], SN.select(now["cost"], now["st"], k))
    log = one.mpc_log
    dead = np.zeros(one.B, dtype=bool)                            # the log's rule: a failed re-solve is a problem's last row - until the
    for r in range(rounds):                                       # join replaces it from its group's winner
        dead &= np.repeat(sels[r].winner < 0, k)
        assert np.array_equal(log[:, r, :], np.where(dead[:, None], 0.0, rows[r]), equal_nan=True), r
        dead |= failed[r]
    assert int(one.stats.n_converged) + int(one.stats.n_max_iters) + int(one.stats.n_ls_failed) + int(one.stats.n_internal) + int(one.stats.n_not_pd) == one.B
    return one, twin, sels, got


def _make(name, n_steps=N, batch=B, **kw):
    def make():
        s, ug = _solver(name, n_steps, batch, **kw)
        s.SetInitialGuess(ug)
        _solve(s)
        return s
    return make


def _winner_not_member_0(cost):
    c = cost.copy()
    c[5] = 0.5 * c[3:6].min()                                     # group 1: its last member wins the first round
    c[0] = c[1] = 0.5 * c[0:3].min()                              # group 0: a tie, member 0 keeps it
    return c


# ---------------------------------------------------------------- 1. a round is its pieces
@pytest.mark.parametrize("name", FAMILIES)
def test_a_round_is_its_pieces(name):
    make = _make(name)
    m = make().m
    sigma = _sigma(np.random.default_rng(21), B, m)
    one, twin, sels, got = _against_the_pieces(make, K, R, REPLAN, 1, sigma, _winner_not_member_0)
    assert sels[0].winner[1] == 2 and sels[0].winner[0] == 0
    assert np.array_equal(one.mpc_winner_log(got)[:, -1, -2], got[-1].cost)          # the winners' costs, through the helper


# ---------------------------------------------------------------- 2. the noise shared over a window and a block changes no bit
@pytest.mark.parametrize("name,hold", [("pendulum", 5), ("pendulum_throughput", 5), ("synth36", 5), ("synth36", 1)])
def test_noise_sharing_changes_no_bit(name, hold):
    """hold = 5 on N - 1 = 11 steps: three windows, the last one short; synth36 has m = 12 controls, three Philox blocks."""
    make = _make(name)
    sigma = _sigma(np.random.default_rng(22), B, make().m)
    _against_the_pieces(make, K, 2, REPLAN, hold, sigma, _winner_not_member_0)


def test_noise_sharing_with_a_padding_control():
    """The chainx plugin of tests/test_gpu_seeds.py: m = 3, four device controls - one block, its last control padding -, hold = 3."""
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    sys_ = _padded()
    n, m = sys_.n, sys_.m
    assert m == 3 and sys_.m_dev == 4

    def make():
        s = BatchedIterativeLQR(sys_, N, B, delta=1e-3, beta=0.6, gamma=0.0, device=0, max_iters=3)
        s.SetTargetState(np.zeros(n)); s.SetRunningCost(0.02 * np.eye(n), 0.002 * np.eye(m)); s.SetTerminalCost(5.0 * np.eye(n))
        rng = np.random.default_rng(4)
        s.SetInitialState(0.3 * rng.standard_normal((B, n)))
        s.SetInitialGuess(rng.uniform(-1.0, 1.0, (B, m, N - 1)))
        _solve(s)
        return s
    sigma = _sigma(np.random.default_rng(23), B, m)
    one, _, _, _ = _against_the_pieces(make, K, 2, REPLAN, 3, sigma, _winner_not_member_0)
    from drake_ddp_amd import _capi
    raw = np.empty((B, 4, N - 1))
    assert one._lib.mi_ilqr_get(one._h, _capi.F_U_BAR, _capi.ptr(raw), raw.nbytes) == _capi.OK and np.all(raw[:, 3] == 0.0)


# ---------------------------------------------------------------- 3. groups wider than the workgroup
@pytest.mark.parametrize("name", ["pendulum", "pendulum_throughput"])
def test_groups_wider_than_a_workgroup(name):
    """K = 300 > 256 members, G = 2, N = 8: the strided select, tiles that cross members, one round."""
    make = _make(name, 8, 600)
    sigma = _sigma(np.random.default_rng(24), 600, 1)

    def doctor(cost):
        c = cost.copy()
        c[299] = 0.5 * c[:300].min(); c[300 + 257] = 0.5 * c[300:].min()
        return c
    _, _, sels, _ = _against_the_pieces(make, 300, 1, 2, 2, sigma, doctor)
    assert sels[0].winner.tolist() == [299, 257]


# ---------------------------------------------------------------- 4. no winner, and a failed seed replaced
def test_no_winner_and_revival():
    """A NaN in x0 ends a problem with LINESEARCH_FAILED (the recipe of tests/test_gpu_seeds.py).  Group 2 fails whole: no winner, the
    fallback - each member's own shifted plan and own predicted state, whatever the failed solve left there -, bitwise the pieces,
    which take the fallback too.  In group 1 one member failed: it is reseeded from the winner, solves, and logs every re-solve.
    (Whether the fallback's members recover is the solver's business: the selections after it are held against the pieces', and
    mpc_winner_log is NaN exactly where a selection names nobody.)"""
    from drake_ddp_amd import _capi, workloads as W

    def make():
        s, ug = _solver("pendulum", N)
        x0 = W.pendulum_batch_x0(B)
        x0[4, 0] = np.nan; x0[6:9, 1] = np.nan
        s.SetInitialState(x0); s.SetInitialGuess(ug)
        _solve(s)
        return s
    st = _state(make())["st"]
    assert (st[[4, 6, 7, 8]] == _capi.STATUS_LINESEARCH_FAILED).all() and np.isin(np.delete(st, [4, 6, 7, 8]), (0, 1)).all()
    sigma = np.full((B, 1), 0.25)
    one, twin, sels, got = _against_the_pieces(make, K, 2, REPLAN, 1, sigma)
    assert got[0].winner[2] == -1 and got[0].eligible.tolist() == [3, 2, 0] and got[0].winner[1] in (0, 2)
    assert got[0].cost[2] == np.inf
    log = one.mpc_log
    assert np.isfinite(log[4]).all() and (log[4, :, :2] != 0.0).any(axis=1).all()     # the replaced seed: both re-solves, finite
    assert np.array_equal(log[4, 0, :2], log[got[0].problem[1], 0, :2])                # ... from the winner's predicted state
    wl = one.mpc_winner_log(got)
    for r in range(2):
        assert np.array_equal(np.isnan(wl[:, r]).all(axis=1), got[r + 1].winner < 0) and np.isfinite(wl[got[r + 1].winner >= 0, r]).all()


def test_a_seed_that_fails_in_the_run_is_replaced_and_logs_again():
    """Member 4's target step is +inf: its cost is not finite from the first re-solve on, every re-solve of it fails.  It is replaced
    from its group's winner before the next re-solve, so its `dead` flag is cleared and it logs that re-solve too - with the
    winner's predicted state as x0.  Without a group (K = 1) the same problem logs the re-solve in which it fails and none after."""
    from drake_ddp_amd import _capi
    make = _make("pendulum")
    step = np.zeros((B, 2)); step[4, 0] = np.inf
    sigma = np.full((B, 1), 0.25)
    s = make()
    x = np.array(s.x_bar)
    got = _run(s, K, 2, REPLAN, sigma, seed=SEED, target_step=step)
    assert s.status[4] >= _capi.STATUS_LINESEARCH_FAILED and [g.eligible[1] for g in got] == [3, 2, 2]
    log = s.mpc_log
    w = got[1].problem[1]
    assert w in (3, 5) and np.array_equal(log[4, 0, :2], x[got[0].problem[1], :, REPLAN])
    assert (log[4, 1, :2] != 0.0).any() and np.array_equal(log[4, 1, :2], log[w, 1, :2])        # the second row: written, the winner's state
    alone = make()
    _run(alone, 1, 2, REPLAN, sigma, seed=SEED, target_step=step)
    assert (alone.mpc_log[4, 0, :2] != 0.0).any() and np.all(alone.mpc_log[4, 1, :] == 0.0)


# ---------------------------------------------------------------- 5. K = 1 is the plain loop
@pytest.mark.parametrize("name", FAMILIES)
def test_k_one_is_the_plain_loop(name):
    """MPCRunMultiStart(1, R, r, sigma) against R x { MPCShift; solve_resident } - warm re-solves, no member is perturbed - and
    against the open-loop MPCRun(R, r) where that one loops on the host."""
    make = _make(name)
    a, b = make(), make()
    got = _run(a, 1, R, REPLAN, 0.5, seed=SEED)
    costs = []
    for _ in range(R):
        b.MPCShift(REPLAN)
        b.solve_resident()
        costs.append(np.array(b.cost))
    assert _same(_state(a), _state(b)) and np.array_equal(a.mpc_log[:, :, -2], np.stack(costs, axis=1))
    assert all((g.winner == 0).all() for g in got) and np.array_equal(got[-1].cost, costs[-1])
    if name == "pendulum_throughput":                              # (the lane-per-problem kernels: mi_ilqr_mpc_run's host loop)
        c = make()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            c.MPCRun(R, REPLAN)
        assert _same(_state(a), _state(c)) and np.array_equal(a.mpc_log, c.mpc_log)


# ---------------------------------------------------------------- 7. a reference trajectory: the clock, and the run split
def _tracking_split_check():
    """arm27, B = 4, K = 2, under a reference: one call of three re-solves against three calls of one, bitwise; target_clock moves
    by R r, and a refused run leaves it."""
    import test_gpu_tracking as T
    p, batch, x0, ug, ref = T._case("arm27")

    def begin():
        s = T._start(T._solver(p, batch), x0, ug)
        s.SetTargetTrajectory(ref, clock=0)
        s.Solve()
        return s
    sigma = np.full(ug.shape[0], 0.05)
    a, b = begin(), begin()
    got = _run(a, 2, 3, 2, sigma, seed=SEED, round=7, hold=2)
    assert a.target_clock == 6
    log = a.mpc_log
    for i in range(3):
        one = _run(b, 2, 1, 2, sigma, seed=SEED, round=7 + i, hold=2)
        assert b.target_clock == 2 * (i + 1) and _sel_same(one[0], got[i]) and _sel_same(one[1], got[i + 1]), i
        assert np.array_equal(b.mpc_log[:, 0, :], log[:, i, :]), i
    ra, rb = T._result(a), T._result(b)
    for k in ("x_bar", "u_bar", "K", "kappa", "dV_coeff", "cost", "status"):
        assert np.array_equal(ra[k], rb[k]), k
    with pytest.raises(ValueError, match="target_step must be None"):
        a.MPCRunMultiStart(2, 1, 2, sigma, target_step=np.zeros(a.n))
    assert a.target_clock == 6


def test_splitting_a_run_under_a_reference_trajectory():
    script = ("import sys; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests'); "
              "import test_gpu_mpc_seeds as M; M._tracking_split_check()")
    r = subprocess.run([sys.executable, "-c", script, ROOT], capture_output=True, text=True, timeout=300, env=dict(os.environ, MI_ILQR_SPEC="2"))
    assert r.returncode == 0, r.stderr[-3000:]


def test_per_problem_target_steps_move_once_per_re_solve():
    """target_step (n,) is turned into rows; the targets end R steps further, and the run is bitwise the pieces with the rows moved
    by hand before every solve."""
    make = _make("pendulum")
    a, b = make(), make()
    step = np.array([0.01, 0.0])
    sigma = np.full((B, 1), 0.25)
    xn = np.broadcast_to(np.asarray(a.x_nom, dtype=np.float64), (B, 2)).copy()
    got = _run(a, K, 2, REPLAN, sigma, seed=SEED, target_step=step)
    assert np.array_equal(np.asarray(a.x_nom), (xn + step) + step)
    for r in range(2):
        x = np.array(b.x_bar)
        b.MPCShift(REPLAN)
        sel = b.ReseedFromBest(K, sigma, seed=SEED, round=r)
        _set_x0(b, x[np.repeat(sel.problem, K)][:, :, REPLAN])
        xn = xn + step
        b.SetTargetStateResident(xn)
        b.solve_resident()
        assert _sel_same(sel, got[r])
    assert _same(_state(a), _state(b))


# ---------------------------------------------------------------- 5b, 6, 7: the closed loop, one plant per group
def _cl_case(name, batch=B, n_steps=N):
    """A case of tests/test_gpu_closed_loop.py (its problem, starts, sigmas and the oracle's model factory); synth36 added here."""
    import test_gpu_closed_loop as CLT
    if name != "synth36":
        return CLT._case(name, batch, n_steps)
    from drake_ddp_amd import workloads as W
    from oracle import models_np as M
    c = CLT._Case()
    c.name, c.B, c.N, c.mode, c.system = name, batch, n_steps, "auto", None
    c.p, c.x0, c.ug, c.sig = W.synth36_problem(n_steps), W.synth36_batch_x0(batch), W.synth36_u_guess(n_steps), (1e-3, 1e-2)
    c.make_model = lambda row: M.Model(c.p["model_id"], c.p["dt"], row)   # noqa: E731
    c.base = np.tile(np.asarray(M.DEFAULT_PARAMS[c.p["model_id"]], dtype=float), (batch, 1))
    c.n, c.m = c.x0.shape[1], c.ug.shape[0]
    return c


def _plant_setup(c):
    """Plant states off the controller's, plant parameters +-10 %, noise on: (x, params, sigma (B, n + m))."""
    import test_gpu_closed_loop as CLT
    rng = np.random.default_rng(31)
    x = c.x0 + 0.02 * rng.standard_normal(c.x0.shape)
    params = c.base * (1.0 + 0.1 * rng.uniform(-1.0, 1.0, c.base.shape))
    return x, params, CLT._sigma(c)


def _with_plant(c, x, params, sigma, seed):
    import test_gpu_closed_loop as CLT
    s = CLT._solved(c)
    s.SetPlant(x, params, state_noise=sigma[:, :c.n], control_noise=sigma[:, c.n:], seed=seed)
    return s


def _plant_same(a, b):
    la, lb = a.plant_log, b.plant_log
    return (np.array_equal(la.X, lb.X, equal_nan=True) and np.array_equal(la.U, lb.U, equal_nan=True) and
            np.array_equal(la.stage_cost, lb.stage_cost, equal_nan=True) and np.array_equal(la.steps, lb.steps) and
            np.array_equal(a.plant_state, b.plant_state) and a.plant_clock == b.plant_clock)


@pytest.mark.parametrize("name", FAMILIES)
def test_k_one_with_a_plant_is_the_closed_loop_mpc_run(name):
    """MPCRunMultiStart(1, R, r, sigma) on a solver that holds a plant against the closed-loop MPCRun(R, r): noise on, plant
    parameters off the model's - state, MPC log, plant log, plant state and clock, bitwise."""
    c = _cl_case(name)
    x, params, sigma = _plant_setup(c)
    a, b = _with_plant(c, x, params, sigma, SEED), _with_plant(c, x, params, sigma, SEED)
    got = _run(a, 1, R, REPLAN, 0.5, seed=SEED)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        b.MPCRun(R, REPLAN)
    assert _same(_state(a), _state(b)) and np.array_equal(a.mpc_log, b.mpc_log) and _plant_same(a, b)
    assert a.plant_clock == R * REPLAN and len(got) == R + 1 and a.plant_kernel_ms() > 0.0


@pytest.mark.parametrize("name", ["pendulum", "synth36"])
def test_closed_loop_one_plant_per_group(name):
    """B = 9, K = 3, plant parameters +-10 %, noise on, three rounds of one re-solve.  Per round: from the device's own plant state
    at the start of the segment, the group's segment of plant_log matches closed_loop_np.advance under the WINNER's policy (read
    from the twin) with member 0's plant parameters, sigmas and problem index g for the normals - to the rule of
    tests/test_gpu_closed_loop.py: 1e-9 relative + 10 x the oracle's own spread, that spread asserted small first; the re-solve is
    bitwise the twin's MPCShift, ReseedFromBest, SetInitialState(the plant state, to every member), solve_resident; every member's
    plant row and plant log is its group's."""
    import test_gpu_closed_loop as CLT
    import test_gpu_policy_rollout as TP
    c = _cl_case(name)
    G = B // K
    x, params, sigma = _plant_setup(c)
    a, twin = _with_plant(c, x, params, sigma, SEED), CLT._solved(c)
    cg = _cl_case(name, G)                                        # the oracle's batch: the G plants
    sig_u = _sigma(np.random.default_rng(32), B, c.m)
    cost = _winner_not_member_0(np.array(a.cost))
    _set_cost(a, cost); _set_cost(twin, cost)
    for r in range(3):
        sel = twin.SelectBest(K)
        pick = np.where(sel.winner >= 0, sel.problem, np.arange(G) * K)
        pol = tuple(f[pick] for f in CLT._policy(twin))
        start, clock = np.array(a.plant_state), a.plant_clock
        assert clock == r * REPLAN              # (round 0: the rows are SetPlant's, one per problem - the group's plant is member 0's)
        assert r == 0 or np.array_equal(start.reshape(G, K, -1), np.repeat(start[::K, None, :], K, axis=1))
        got = _run(a, K, 1, REPLAN, sig_u, seed=SEED, round=r, hold=2)
        assert _sel_same(got[0], sel) and (r > 0 or sel.winner[1] == 2)
        lg, now = a.plant_log, np.array(a.plant_state)
        for f in (lg.X, lg.U, lg.stage_cost, lg.steps, now):      # every member reports its group's plant
            assert np.array_equal(f.reshape((G, K) + f.shape[1:]), np.repeat(f[::K, None], K, axis=1), equal_nan=True)
        ref, sp, L, spl = CLT._oracle_with_spread(cg, start[::K], params[::K], pol, REPLAN, sigma[::K], SEED, clock)
        done = (~np.isnan(lg.U[::K]).any(axis=1)).sum(axis=1)
        rec = CLT._R(CLT._as_rollout(now[::K], done, lg.X[::K, :, :-1], lg.U[::K], lg.stage_cost[::K]))
        TP._compare(rec, ref, sp, 1)
        assert np.all(np.abs(lg.stage_cost[::K] - L) <= 1e-9 * np.abs(L).max(axis=1, keepdims=True) + 10.0 * spl)
        twin.MPCShift(REPLAN)
        assert _sel_same(twin.ReseedFromBest(K, sig_u, seed=SEED, round=r, hold=2), sel)
        _set_x0(twin, now)
        twin.solve_resident()
        assert _same(_state(a), _state(twin)), r
        assert np.array_equal(a.mpc_log[:, 0, :c.n], now)


@pytest.mark.parametrize("name", ["pendulum", "pendulum_throughput", "synth36"])
def test_splitting_a_closed_loop_run(name):
    """One call of three re-solves against three calls of one with `round` advanced by hand, on solvers that hold a plant."""
    c = _cl_case(name)
    x, params, sigma = _plant_setup(c)
    a, b = _with_plant(c, x, params, sigma, SEED), _with_plant(c, x, params, sigma, SEED)
    sig_u = _sigma(np.random.default_rng(33), B, c.m)
    got = _run(a, K, R, REPLAN, sig_u, seed=SEED, round=9)
    la, log = a.plant_log, a.mpc_log
    for i in range(R):
        one = _run(b, K, 1, REPLAN, sig_u, seed=SEED, round=9 + i)
        assert _sel_same(one[0], got[i]) and _sel_same(one[1], got[i + 1]) and b.plant_clock == (i + 1) * REPLAN, i
        lb, rows = b.plant_log, slice(i * REPLAN, (i + 1) * REPLAN)
        assert np.array_equal(lb.U, la.U[:, :, rows], equal_nan=True) and np.array_equal(lb.X[:, :, :-1], la.X[:, :, rows], equal_nan=True), i
        assert np.array_equal(lb.stage_cost, la.stage_cost[:, rows], equal_nan=True) and np.array_equal(b.mpc_log[:, 0, :], log[:, i, :]), i
    assert _same(_state(a), _state(b)) and np.array_equal(a.plant_state, b.plant_state) and a.plant_clock == b.plant_clock == R * REPLAN


# ---------------------------------------------------------------- 8. refusals
def test_refusals_leave_the_handle_alone():
    from drake_ddp_amd import _capi
    s, ug = _solver("pendulum", N)
    twin, _ = _solver("pendulum", N)
    lib, h = s._lib, s._h
    run = lambda *v: lib.mi_ilqr_set(h, _capi.F_SEEDS_RUN, _capi.ptr(np.array(v, dtype=np.float64)), 8 * len(v))   # noqa: E731
    s.SetInitialGuess(ug); twin.SetInitialGuess(ug)
    s._push_problem()
    assert run(3, 2, 0, 0, 1, 0, 2, 2) == _capi.E_BAD_ARG                      # a cold handle: nothing to select on
    with pytest.raises(ValueError, match="MPCRunMultiStart: the solver holds no solve"):
        s.MPCRunMultiStart(3, 2, 2, 0.1)
    assert _same(_solve(s), _solve(twin))                                      # ... and it solves as if nothing had been asked
    for op in (0, 1, 3, 4, -1):
        assert run(3, op, 0, 0, 1, 0, 2, 2) == _capi.E_BAD_ARG, op            # only RESEED has a long form
    for nr in (0, -1, 1.5, np.nan, 2.0 ** 31):
        assert run(3, 2, 0, 0, 1, 0, nr, 2) == _capi.E_BAD_ARG, nr
    for rp in (0, N - 1, N, 0.5, np.inf):
        assert run(3, 2, 0, 0, 1, 0, 2, rp) == _capi.E_BAD_ARG, rp
    assert run(3, 2, 0, 2.0 ** 32 - 1, 1, 0, 2, 2) == _capi.E_BAD_ARG          # round + num_resolves passes 2^32
    assert run(3, 2, 0, 0, 1, 1, 2, 2) == _capi.E_BAD_ARG and run(3, 2, 0, 0, 0, 0, 2, 2) == _capi.E_BAD_ARG   # reserved, hold
    assert run(2, 2, 0, 0, 1, 0, 2, 2) == _capi.E_BAD_ARG                      # K does not divide B
    assert run(3, 2, 0, 0, 1, 0, 2) == _capi.E_BAD_SHAPE and run(3, 2, 0, 0, 1, 0, 2, 2, 0) == _capi.E_BAD_SHAPE   # 7 and 9 doubles
    assert lib.mi_ilqr_set(h, _capi.F_SEEDS_RUN, None, 64) == _capi.E_BAD_ARG
    out = np.empty(64)
    assert lib.mi_ilqr_get(h, _capi.F_SEEDS_BEST, _capi.ptr(out), 72) == _capi.E_BAD_ARG   # nothing was selected
    with pytest.raises(ValueError, match="K must divide"):
        s.MPCRunMultiStart(2, 2, 2, 0.1)
    assert _same(_solve(s), _solve(twin))                                      # warm, after every refusal: the twin's warm solve
    assert run(3, 2, 0, 0, 1, 0, 2, 2) == _capi.OK
    assert lib.mi_ilqr_get(h, _capi.F_SEEDS_BEST, _capi.ptr(out), 72) == _capi.E_BAD_SHAPE
    assert lib.mi_ilqr_get(h, _capi.F_SEEDS_BEST, _capi.ptr(out), 3 * 3 * 3 * 8) == _capi.OK
    assert lib.mi_ilqr_get(h, _capi.F_SEEDS_COST, _capi.ptr(out), 24) == _capi.E_BAD_ARG   # the run was no gather
    ms = np.empty(1)
    assert lib.mi_ilqr_get(h, _capi.F_SEEDS_KERNEL_MS, _capi.ptr(ms), 8) == _capi.OK and 0.0 < ms[0] < 100.0
    small, ug3 = _solver("pendulum", N, 3)                                     # B <= 4, wave per problem: the inputs live in host memory
    ref3, _ = _solver("pendulum", N, 3)
    small.SetInitialGuess(ug3); ref3.SetInitialGuess(ug3)
    assert _same(_solve(small), _solve(ref3))
    v = np.array([3, 2, 0, 0, 1, 0, 2, 2], dtype=np.float64)
    assert small._lib.mi_ilqr_set(small._h, _capi.F_SEEDS_RUN, _capi.ptr(v), 64) == _capi.E_UNSUPPORTED
    with pytest.raises(ValueError, match="MPCRunMultiStart: not on this solver"):
        small.MPCRunMultiStart(3, 2, 2, 0.1)
    assert _same(_solve(small), _solve(ref3))


# ---------------------------------------------------------------- 9. the example
def test_the_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "mpc_multistart_pendulum.py"), "--groups", "8", "--seeds", "4",
                        "--resolves", "4", "--steps", "40"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "mpc_multistart_pendulum: OK", r.stdout[-3000:]
    assert any("within the goal" in ln for ln in lines)
