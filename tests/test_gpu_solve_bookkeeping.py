"""The n = 2 solve kernels' bookkeeping and their cold first iteration, against the C oracle.

Every iteration of a solve leaves one row in the log (cost, eps, trials, key-point share) and one in the stopwatch log:
the rows of a solve are [0, min(iterations, hist_cap)), in order, whatever the exit of the iteration loop, and nothing
is written beyond them - in the device MPC loop after every re-solve.  The first iteration of a cold solve builds its
guess for the time-parallel rollout from u_bar alone (the rest of the solver state is zero there): same iterations,
trials and results as the oracle's plain rollout at every horizon that path takes or just does not take.

Tolerances: those of tests/test_gpu_parity.py for central differences (cost rel 1e-8, x / u abs 1e-6, K rel 1e-6);
eps, trial counts, iteration counts and status are exact.  Two set-ups differ from the workload's on purpose: the one-step
horizon N = 2 is compared after two iterations (its third gains ~1e-13, and the line search that finds it compares costs one
ulp apart), and the 70-row solve uses dt = 0.3 (at dt = 0.01 every pendulum solve stalls at round-off within 18 iterations).
"""
import numpy as np
import pytest

from common import rel_err
from test_gpu_parity import TOL, make_solver

pytestmark = pytest.mark.gpu

FD = TOL["fd"]


def _pendulum(N, **kw):
    from drake_ddp_amd import workloads as W
    return dict(W.pendulum_problem(), N=N, **kw)


def _oracle(prob, x0, ug, hist_cap=64, max_iters=100000):
    from oracle import c_oracle, models_np as M
    return c_oracle.solve_batch(M.Model(prob["model_id"], prob["dt"]), prob, x0, ug, fd_h=1e-5, hist_cap=hist_cap, max_iters=max_iters)


def _check_rows(h, r, b, rows, what):
    """history rows [0, rows) of problem b against the oracle's iteration log: cost | eps | trials, and 100 % key-points"""
    ho = r["hist"][b, :rows]
    assert np.array_equal(h[b, :rows, 1], ho[:, 1]), (what, b, "eps")
    assert np.array_equal(h[b, :rows, 2], ho[:, 2]), (what, b, "trials")
    assert rel_err(h[b, :rows, 0], ho[:, 0]) < FD["L"], (what, b, "cost")
    assert np.array_equal(h[b, :rows, 3], np.full(rows, 100.0)), (what, b, "key-point share")


def _check_results(s, r, what):
    assert np.array_equal(s.iterations, r["iters"]), (what, s.iterations, r["iters"])
    assert np.array_equal(s.ls_trials, r["ls"]), (what, s.ls_trials, r["ls"])
    assert np.array_equal(s.status, r["status"]), (what, s.status, r["status"])
    for b in range(len(r["iters"])):
        assert abs(s.cost[b] - r["cost"][b]) <= FD["L"] * abs(r["cost"][b]), (what, b)
        assert np.max(np.abs(s.x_bar[b] - r["x_bar"][b])) < FD["xu"] * max(1.0, np.abs(r["x_bar"][b]).max()), (what, b)
        assert np.max(np.abs(s.u_bar[b] - r["u_bar"][b])) < FD["xu"] * max(1.0, np.abs(r["u_bar"][b]).max()), (what, b)
        assert rel_err(s.K[b], r["K"][b]) < FD["K"], (what, b)


@pytest.mark.parametrize("N", [3, 6, 66])
@pytest.mark.parametrize("hist_cap", [1, 3, 8])
def test_history_rows_vs_oracle_and_nothing_beyond_them(N, hist_cap):
    """Two cold solves on one handle: the first from far away (more iterations), the second from beside the target
    (fewer).  Each solve's rows [0, min(iterations, hist_cap)) are the oracle's; the rows from there on are, bit for
    bit, what the first solve left - in `history` and in `iteration_cycles`."""
    B = 3
    rng = np.random.default_rng(100 * N + hist_cap)
    prob = _pendulum(N)
    far = np.stack([rng.uniform(-3 * np.pi, 3 * np.pi, B), rng.uniform(-1, 1, B)], axis=1)
    near = np.stack([np.pi + rng.uniform(-1e-3, 1e-3, B), rng.uniform(-1e-3, 1e-3, B)], axis=1)
    ug_far, ug_near = 5.0 * rng.uniform(-1, 1, (B, 1, N - 1)), np.zeros((B, 1, N - 1))
    r_far, r_near = _oracle(prob, far, ug_far), _oracle(prob, near, ug_near)
    assert (r_near["iters"] < r_far["iters"]).all() and (r_near["iters"] >= 1).all()   # (the inputs: rows of the first solve do stay behind)
    s = make_solver(prob, B=B, jac="fd", fd_step=1e-5, hist_cap=hist_cap)
    s.SetInitialState(far); s.SetInitialGuess(ug_far)
    s.Solve()
    h_far, c_far = s.history.copy(), s.iteration_cycles.copy()
    assert h_far.shape == (B, hist_cap, 4)
    _check_results(s, r_far, "far")
    for b in range(B):
        rows = min(int(r_far["iters"][b]), hist_cap)
        _check_rows(h_far, r_far, b, rows, "far")
        assert not h_far[b, rows:].any() and not c_far[b, rows:].any()          # a new handle's log is zeros
        assert (c_far[b, :rows, 3] > 0).all()
    s.Reset()
    s.SetInitialState(near); s.SetInitialGuess(ug_near)
    s.Solve()
    h, c = s.history, s.iteration_cycles
    _check_results(s, r_near, "near")
    for b in range(B):
        rows = min(int(r_near["iters"][b]), hist_cap)
        _check_rows(h, r_near, b, rows, "near")
        assert np.array_equal(h[b, rows:], h_far[b, rows:]), (b, "history rows beyond the solve's own were written")
        assert np.array_equal(c[b, rows:], c_far[b, rows:]), (b, "stopwatch rows beyond the solve's own were written")


def test_seventy_rows_all_present_and_in_order():
    """delta = 0 and a cap of 70 iterations, 70 log rows, written one per iteration by lane 0 of the problem's wave.
    (dt = 0.3: the pendulum's step is then nonlinear enough that these two problems - picked with the C oracle from a
    seeded batch - still gain more than 1e-6 of their cost per iteration beyond the 70th; at the workload's dt = 0.01
    every solve stalls at round-off within 18 iterations.)"""
    from drake_ddp_amd import _capi
    B, N, CAP = 2, 9, 70
    rng = np.random.default_rng(11)
    x0 = np.stack([rng.uniform(-3 * np.pi, 3 * np.pi, 64), rng.uniform(-1, 1, 64)], axis=1)[[13, 23]]
    ug = rng.uniform(-1, 1, (64, 1, N - 1))[[13, 23]]
    prob = _pendulum(N, delta=0.0, dt=0.3)
    r = _oracle(prob, x0, ug, hist_cap=CAP, max_iters=CAP)
    assert (r["iters"] == CAP).all() and (r["status"] == _capi.STATUS_MAX_ITERS).all()
    s = make_solver(prob, B=B, jac="fd", fd_step=1e-5, hist_cap=CAP, max_iters=CAP)
    s.SetInitialState(x0); s.SetInitialGuess(ug)
    with pytest.warns(RuntimeWarning, match="stopped at max_iters"):
        s.Solve()
    assert np.array_equal(s.iterations, [CAP, CAP]) and (s.status == _capi.STATUS_MAX_ITERS).all()
    h, c = s.history, s.iteration_cycles
    for b in range(B):
        # all rows, each in its place: gamma = 0 accepts a trial only if it lowers the cost, so the log's costs fall strictly -
        # two rows exchanged, one missing (zeros) or one written twice would break that; the first row is the oracle's (the
        # later ones follow it only to ~1e-8: at dt = 0.3 the backtracking iterations amplify the round-off of the first)
        assert (np.diff(h[b, :, 0]) < 0).all(), (b, np.nonzero(np.diff(h[b, :, 0]) >= 0)[0])
        assert (h[b, :, 1] > 0).all() and (h[b, :, 1] <= 1).all() and (h[b, :, 2] >= 1).all()
        assert np.array_equal(h[b, :, 2], np.round(h[b, :, 2])) and h[b, :, 2].sum() == s.ls_trials[b]
        assert np.array_equal(h[b, :, 3], np.full(CAP, 100.0))
        _check_rows(h, r, b, 1, "first row")
        assert abs(h[b, -1, 0] - s.cost[b]) == 0.0                               # the last row is the last iteration
        # stopwatches: forward | derivatives | backward | iteration, in cycles
        assert np.isfinite(c[b]).all() and (c[b] >= 0).all()
        assert (c[b, :, 3:4] >= c[b, :, 0:3]).all() and (c[b, :, 3] > 0).all()
        assert np.array_equal(c[b, :, 3], c[b, :, 0] + c[b, :, 1] + c[b, :, 2])  # (integers below 2^53: exact)


def test_device_mpc_loop_leaves_the_host_loop_s_log():
    """MPCRun(3, 1) against MPCShift + Solve three times on a second solver: after every re-solve the log holds that
    re-solve's rows over what was there before - so at the end both hold the same array."""
    B, N = 2, 9
    rng = np.random.default_rng(5)
    prob = _pendulum(N)
    x0 = np.stack([rng.uniform(-np.pi, np.pi, B), rng.uniform(-1, 1, B)], axis=1)
    ug = rng.uniform(-1, 1, (B, 1, N - 1))
    dev, host = (make_solver(prob, B=B, jac="fd", fd_step=1e-5, hist_cap=8) for _ in range(2))
    for s in (dev, host):
        s.SetInitialState(x0); s.SetInitialGuess(ug)
        s.Solve()
    assert np.array_equal(dev.history, host.history)
    dev.MPCRun(3, 1)
    its = []
    for _ in range(3):
        host.MPCShift(1)
        host.solve_resident()
        its.append(host.iterations.copy())
    assert np.array_equal(dev.mpc_log[:, :, -1].astype(int), np.stack(its, axis=1))
    assert np.array_equal(dev.iterations, np.sum(its, axis=0))
    assert np.array_equal(dev.history, host.history)
    assert (dev.history[:, 0, 2] >= 1).all()
    assert np.array_equal(dev.x_bar, host.x_bar) and np.array_equal(dev.cost, host.cost)


@pytest.mark.parametrize("N", [2, 3, 5, 257, 258])
def test_cold_first_iteration_vs_oracle(N):
    """Cold solves from a random nonzero u_guess, |theta_0| up to 3 pi: one step, partial chunks of the four-steps-per-lane
    rollout, the last horizon it takes (257) and the first it does not (258).
    (N = 2 after TWO iterations: a one-step problem is solved to the last bit by then, its third iteration gains ~1e-13 and
    the line search that finds it compares costs one ulp apart - the oracle itself gives up on one problem in five there.)"""
    import warnings
    B = 4
    cap = 2 if N == 2 else 1000
    rng = np.random.default_rng(7000 + N)
    prob = _pendulum(N)
    x0 = np.stack([rng.uniform(-3 * np.pi, 3 * np.pi, B), rng.uniform(-1, 1, B)], axis=1)
    ug = rng.uniform(-2, 2, (B, 1, N - 1))
    ug[np.abs(ug) < 1e-3] = 1e-3
    r = _oracle(prob, x0, ug, hist_cap=64, max_iters=cap)
    s = make_solver(prob, B=B, jac="fd", fd_step=1e-5, hist_cap=64, max_iters=cap)
    s.SetInitialState(x0); s.SetInitialGuess(ug)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # (N = 2: "stopped at max_iters")
        s.Solve()
    _check_results(s, r, "solve")
    h = s.history
    c = s.iteration_cycles
    for b in range(B):
        assert r["iters"][b] >= 2
        _check_rows(h, r, b, min(int(r["iters"][b]), 64), "solve")
        if N == 258:
            # no time-parallel rollout at this horizon, so no rollout that linearizes on the way: every iteration has a
            # linearization span of its own (where a rollout did linearize, that column is exactly zero)
            assert (c[b, :r["iters"][b], 1] > 0).all()


@pytest.mark.parametrize("N", [3, 5, 257, 258])
def test_device_mpc_loop_on_a_cold_handle(N):
    """MPCRun(2, 1) on a handle that has never solved, against MPCShift + Solve twice on a second such handle, and the first
    re-solve against the oracle (zero solver state: it starts at x_bar[:, 1] = 0 from u_guess shifted by one step).
    TODAY THIS DOES NOT TAKE THE COLD FORM OF THE ROLLOUT: the host writes the zero state to memory before the MPC launch
    and clears the handle's cold flag, so the kernel's `cold_start` is false in every MPC launch and the first iteration is
    the sequential rollout.  The kernel's condition still names the MPC mode; should the host ever launch it cold, this is
    the test that holds the coarse guess to the same results."""
    from drake_ddp_amd.workloads import mpc_shift
    B = 4
    rng = np.random.default_rng(7100 + N)
    prob = _pendulum(N)
    x0 = np.stack([rng.uniform(-3 * np.pi, 3 * np.pi, B), rng.uniform(-1, 1, B)], axis=1)
    ug = rng.uniform(-2, 2, (B, 1, N - 1))
    dev, host = (make_solver(prob, B=B, jac="fd", fd_step=1e-5, hist_cap=64) for _ in range(2))
    for s in (dev, host):
        s.SetInitialState(x0); s.SetInitialGuess(ug)
        s._push_problem()                                        # (what Solve() does first; MPCRun starts from the handle's inputs)
    dev.MPCRun(2, 1)
    its, ls, hists = [], [], []
    for _ in range(2):
        host.MPCShift(1)
        host.solve_resident()
        its.append(host.iterations.copy()); ls.append(host.ls_trials.copy()); hists.append(host.history.copy())
    log = dev.mpc_log
    assert np.array_equal(log[:, :, -1].astype(int), np.stack(its, axis=1))
    assert np.array_equal(dev.iterations, np.sum(its, axis=0)) and np.array_equal(dev.ls_trials, np.sum(ls, axis=0))
    assert np.array_equal(dev.status, host.status)
    assert np.array_equal(dev.history, host.history)
    for b in range(B):
        assert abs(dev.cost[b] - host.cost[b]) <= FD["L"] * abs(host.cost[b])
        assert np.max(np.abs(dev.x_bar[b] - host.x_bar[b])) < FD["xu"] * max(1.0, np.abs(host.x_bar[b]).max())
        assert np.max(np.abs(dev.u_bar[b] - host.u_bar[b])) < FD["xu"] * max(1.0, np.abs(host.u_bar[b]).max())
        assert rel_err(dev.K[b], host.K[b]) < FD["K"]
    _, ug1 = mpc_shift(np.zeros((B, 2, N)), ug, 1)
    r1 = _oracle(prob, np.zeros((B, 2)), ug1, hist_cap=64)
    assert np.array_equal(its[0], r1["iters"]) and np.array_equal(ls[0], r1["ls"])
    assert rel_err(log[:, 0, -2], r1["cost"]) < FD["L"]
    for b in range(B):
        _check_rows(hists[0], r1, b, min(int(r1["iters"][b]), 64), "first re-solve")


def test_acrobot_log_vs_oracle():
    """n = 4: the same log from the kernels that hold four states."""
    from drake_ddp_amd import workloads as W
    B, N = 2, 8
    prob = dict(W.acrobot_problem(), N=N)
    x0 = W.acrobot_batch_x0(B)
    ug = np.random.default_rng(9).uniform(-1, 1, (B, 1, N - 1))
    r = _oracle(prob, x0, ug, hist_cap=16)
    s = make_solver(prob, B=B, jac="fd", fd_step=1e-5, hist_cap=16)
    s.SetInitialState(x0); s.SetInitialGuess(ug)
    s.Solve()
    _check_results(s, r, "acrobot")
    h, c = s.history, s.iteration_cycles
    for b in range(B):
        rows = min(int(r["iters"][b]), 16)
        assert rows >= 1
        _check_rows(h, r, b, rows, "acrobot")
        assert not h[b, rows:].any() and not c[b, rows:].any()
        assert (c[b, :rows, 3] >= c[b, :rows, :3].max(axis=1)).all() and (c[b, :rows, 3] > 0).all()
