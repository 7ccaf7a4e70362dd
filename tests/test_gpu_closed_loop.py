"""Closed-loop MPC on the device (SetPlant + MPCRun; MI_F_PLANT_*; csrc/plant_advance.hpp: one lane per problem) against the NumPy
statement of the plant (tests/closed_loop_np.py), against the pieces it is composed of (MPCShift, an x0 upload, solve_resident),
against itself (one call of R rounds = R calls of one) and against the policy-rollout kernel; failing plants, clearing, and the
selectors through ctypes.  One model per solver layout: pendulum (wave-per-problem), pendulum with kernel_mode="throughput"
(batch-minor), acrobot, the 3-D quadruped (time-major workgroup kernels) and the (37, 3) chainx plugin with four device controls.

Tolerance against the oracle: the rule of tests/test_gpu_policy_rollout.py (_compare) - 1e-9 relative + 10 x the oracle's own spread,
the largest change of the oracle under a one-ulp perturbation of the plant's state in both directions and under every normal moved
by +-4e-14 (policy_noise_np.NORMAL_TOL); that spread is asserted below 1e-6 relative with the oracle alone first
(_assert_spread_small).  Everything that compares the device with itself is bitwise."""
import functools
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "plugins"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import closed_loop_np as CL  # noqa: E402
import policy_noise_np as PN  # noqa: E402
import test_gpu_policy_rollout as TP  # noqa: E402  (its solver factory, its comparison rule)

pytestmark = pytest.mark.gpu

SEED = PN.TEST_SEED + 5


class _Case:
    pass


@functools.lru_cache(maxsize=None)
def _chainx():
    return TP._plugins()[0]


def _case(name, B, N):
    """The problem, B starts, the guess, the kernel mode, the system, the oracle's model factory and the sigmas' sizes."""
    from drake_ddp_amd import workloads as W
    from oracle import models_np as M
    c = _Case()
    c.name, c.B, c.N, c.mode, c.system = name, B, N, "auto", None
    if name in ("pendulum", "pendulum_throughput"):
        c.p, c.x0, c.ug = dict(W.pendulum_problem(), N=N), W.pendulum_batch_x0(B), np.zeros((1, N - 1))
        c.mode = "throughput" if name.endswith("throughput") else "auto"
        c.sig = (3e-3, 1e-2)
    elif name == "acrobot":
        c.p, c.x0, c.ug, c.sig = W.acrobot_problem(N), W.acrobot_batch_x0(B), np.zeros((1, N - 1)), (2e-3, 1e-2)
    elif name == "quad3d":
        c.p, c.x0, c.ug, c.sig = W.quad3d_problem(N), W.quad3d_batch_x0(B), W.quad3d_u_guess(N), (1e-3, 5e-2)
    elif name == "planar_quad":
        c.p, c.x0, c.ug, c.sig = W.planar_quad_problem(N), W.planar_quad_batch_x0(B), W.planar_quad_u_guess(N), (1e-3, 5e-2)
    else:
        import plugin_steps as PS
        nq, m, ne, dt = 16, 3, 5, 0.02
        n = 2 * nq + ne
        c.system = _chainx()(dt)
        assert c.system.m == m and c.system.m_dev == 4
        c.p = dict(model_id=c.system.model_id, dt=dt, N=N, delta=1e-3, beta=0.6, gamma=0.0, Q=dt * np.eye(n), R=dt * 0.1 * np.eye(m),
                   Qf=5.0 * np.eye(n), x_nom=np.zeros(n))
        c.x0, c.ug, c.sig = 0.3 * np.random.default_rng(8).standard_normal((B, n)), np.zeros((m, N - 1)), (1e-3, 1e-2)
        c.make_model = lambda row: M.Model.custom(n, m, PS.chainx_step(nq, m, ne), row, dt)   # noqa: E731
        c.base = np.tile(c.system.params, (B, 1))
    if c.system is None:
        c.make_model = lambda row: M.Model(c.p["model_id"], c.p["dt"], row)   # noqa: E731
        c.base = np.tile(np.asarray(M.DEFAULT_PARAMS[c.p["model_id"]], dtype=float), (B, 1))
    c.n, c.m = c.x0.shape[1], c.ug.shape[0]
    return c


def _solved(c, max_iters=3, **kw):
    """A solver of the case with a policy on it: `max_iters` iLQR iterations from the case's own starts."""
    s = TP._solver(c.p, system=c.system, batch=c.B, max_iters=max_iters, kernel_mode=c.mode, **kw)
    for k, v in getattr(c, "setup", {}).items():
        getattr(s, k)(*v)
    s.SetInitialState(c.x0); s.SetInitialGuess(c.ug)
    TP._solve(s)
    return s


def _run(s, resolves, replan):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # (max_iters = 3: "not converged" is expected)
        return s.MPCRun(resolves, replan)


def _policy(s):
    return np.array(s.x_bar), np.array(s.u_bar), np.array(s.K)


def _sigma(c, rng=None):
    """(B, n + m) rows, a different multiple per problem; the 3-D quadruped's attitude quaternion gets no noise of its own."""
    sx, su = np.full(c.n, c.sig[0]), np.full(c.m, c.sig[1])
    if c.name == "quad3d":
        sx[:4] = 0.0
    return np.tile(np.concatenate([sx, su]), (c.B, 1)) * np.array([1.0, 0.5, 2.0])[np.arange(c.B) % 3][:, None]


def _as_rollout(xf, done, X, U, L):
    """The plant's record in the form of the policy rollouts' (cost, x_final, steps, X, U) with S = 1: what TP._compare takes."""
    steps = L.shape[1]
    with np.errstate(invalid="ignore"):
        cost = np.where(done == steps, L.sum(axis=1), np.inf)
    return (cost[:, None], xf[:, None, :], done.astype(np.int32)[:, None], np.concatenate([X, xf[:, :, None]], axis=2)[:, None], U[:, None])


class _R:
    def __init__(self, t):
        self.cost, self.x_final, self.steps, self.X, self.U = t


def _device_record(s, rows=slice(None)):
    """The same form from plant_log (its rows `rows`) and plant_state."""
    lg = s.plant_log
    L = lg.stage_cost[:, rows]
    done = (~np.isnan(lg.U[:, :, rows]).any(axis=1)).sum(axis=1)
    return _R(_as_rollout(np.array(s.plant_state), done, lg.X[:, :, :-1][:, :, rows], lg.U[:, :, rows], L)), L


def _oracle_with_spread(c, x, params, pol, steps, sigma, seed, clock, feedback=True, lo=None, hi=None, Q=None, x_nom=None):
    Q = c.p["Q"] if Q is None else Q
    x_nom = c.p["x_nom"] if x_nom is None else x_nom
    run = lambda x_, shift: CL.advance(c.make_model, x_, params, pol[0], pol[1], pol[2], Q, c.p["R"], x_nom, steps, sigma, seed, clock,   # noqa: E731
                                       False, feedback, lo, hi, shift)
    raw = run(x, 0.0)
    ref = _as_rollout(*raw)
    sp = [np.zeros(ref[0].shape) for _ in range(3)]
    spl = np.zeros(raw[4].shape)
    alts = [run(np.nextafter(x, np.inf), 0.0), run(np.nextafter(x, -np.inf), 0.0)]
    if sigma is not None:
        alts += [run(x, PN.NORMAL_TOL), run(x, -PN.NORMAL_TOL)]
    for a in alts:
        alt = _as_rollout(*a)
        with np.errstate(invalid="ignore"):
            sp[0] = np.fmax(sp[0], np.abs(alt[0] - ref[0]))
            sp[1] = np.fmax(sp[1], np.nanmax(np.abs(alt[3] - ref[3]), axis=(2, 3)))
            sp[2] = np.fmax(sp[2], np.nanmax(np.abs(alt[4] - ref[4]), axis=(2, 3)))
            spl = np.fmax(spl, np.abs(a[4] - raw[4]))
    TP._assert_spread_small(ref, sp)
    return ref, sp, raw[4], spl


def _check_segment(s, c, x, params, pol, steps, sigma, seed, clock, rows=slice(None), report=None, **kw):
    """plant_log (its rows `rows`) and plant_state after a segment of `steps` steps from the state x and the policy `pol`."""
    ref, sp, L, spl = _oracle_with_spread(c, x, params, pol, steps, sigma, seed, clock, **kw)
    r, Ld = _device_record(s, rows)
    TP._compare(r, ref, sp, 1, report=report)
    assert np.all(np.abs(Ld - L) <= 1e-9 * np.abs(L).max(axis=1, keepdims=True) + 10.0 * spl)      # the stage costs, entry by entry (relative to the problem's largest)
    return ref


# ---------------------------------------------------------------- 1. the plant segment against the oracle
SHAPES = [("pendulum", 1, 3, 1, 1), ("pendulum", 65, 8, 6, 1), ("pendulum", 3, 8, 2, 3), ("pendulum_throughput", 65, 8, 6, 1),
          ("pendulum_throughput", 3, 3, 1, 3), ("acrobot", 3, 8, 3, 1), ("acrobot", 65, 6, 4, 3), ("quad3d", 3, 8, 6, 1), ("quad3d", 65, 5, 2, 1),
          ("chainx", 3, 12, 4, 1)]


@pytest.mark.parametrize("name,B,N,replan,resolves", SHAPES, ids=["%s-B%d-N%d-r%d-R%d" % s_ for s_ in SHAPES])
def test_the_plant_segment_against_the_oracle(name, B, N, replan, resolves):
    """Offset states, perturbed parameters and noise; every round of the run on its own: the policy and the plant's state are read
    before it, plant_log and plant_state after it."""
    c = _case(name, B, N)
    s = _solved(c)
    rng = np.random.default_rng(40)
    pol = _policy(s)
    x = pol[0][:, :, 0] + 10.0 * c.sig[0] * rng.standard_normal((B, c.n))
    params = c.base * rng.uniform(0.9, 1.1, c.base.shape)
    sigma = _sigma(c)
    s.SetPlant(x, params, state_noise=sigma[:, :c.n], control_noise=sigma[:, c.n:], seed=SEED, clock=7)
    assert np.array_equal(s.plant_state, x) and s.plant_clock == 7
    for r in range(resolves):
        _run(s, 1, replan)
        assert s.plant_clock == 7 + (r + 1) * replan
        lg = s.plant_log
        assert lg.X.shape == (B, c.n, replan + 1) and lg.U.shape == (B, c.m, replan) and lg.stage_cost.shape == (B, replan) and lg.steps.shape == (B,)
        assert np.array_equal(lg.X[:, :, 0], x) and np.array_equal(lg.X[:, :, -1], s.plant_state) and np.all(lg.steps == replan)
        _check_segment(s, c, x, params, pol, replan, sigma, SEED, 7 + r * replan, report="%s round %d" % (name, r))
        assert np.array_equal(s.mpc_log[:, 0, :c.n], s.plant_state)
        x, pol = np.array(s.plant_state), _policy(s)
    assert s.plant_kernel_ms() > 0.0


@pytest.mark.parametrize("variant", ["feedback_off", "no_noise", "limits", "per_problem_costs_and_targets"])
def test_the_variants_of_the_plant_step(variant):
    B, N, replan = 3, 8, 4
    c = _case("pendulum", B, N)
    rng = np.random.default_rng(41)
    kw, okw, sigma = {}, {}, _sigma(c)
    if variant == "limits":
        lo, hi = np.array([[-0.4], [-0.2], [-1.0]]), np.array([[0.3], [0.5], [0.1]])
        kw = dict(control_limits="enforce")
        c.setup = {"SetControlLimits": (lo, hi)}
        okw = dict(lo=lo, hi=hi)
    if variant == "per_problem_costs_and_targets":
        A = rng.standard_normal((B, 2, 2))
        Q = np.einsum("bij,bkj->bik", A, A) + c.p["Q"]
        x_nom = c.p["x_nom"][None, :] + 0.3 * rng.standard_normal((B, 2))
        c.setup = {"SetRunningCost": (Q, c.p["R"]), "SetTargetState": (x_nom,)}
        okw = dict(Q=Q, x_nom=x_nom)
    s = _solved(c, **kw)
    pol = _policy(s)
    x = pol[0][:, :, 0] + (1.5 if variant == "limits" else 0.05) * rng.standard_normal((B, 2))     # (limits: far enough out that the feedback saturates)
    params = c.base * rng.uniform(0.9, 1.1, c.base.shape)
    if variant == "no_noise":
        sigma = None
        s.SetPlant(x, params)
    else:
        s.SetPlant(x, params, state_noise=sigma[:, :2], control_noise=sigma[:, 2:], seed=SEED, feedback=variant != "feedback_off")
    _run(s, 1, replan)
    _check_segment(s, c, x, params, pol, replan, sigma, SEED, 0, report="pendulum %s" % variant, feedback=variant != "feedback_off", **okw)
    U = s.plant_log.U
    if variant == "feedback_off":
        assert np.array_equal(U, pol[1][:, :, :replan])                # u_bar alone, whatever the state's offset
    if variant == "limits":
        assert np.all(U >= lo[:, :, None]) and np.all(U <= hi[:, :, None]) and (np.any(U == lo[:, :, None]) or np.any(U == hi[:, :, None]))


# ---------------------------------------------------------------- 2. composition, bitwise
COMPOSE = [("pendulum", 3, 8, 2), ("pendulum", 65, 3, 1), ("pendulum_throughput", 65, 8, 6), ("acrobot", 3, 8, 3), ("quad3d", 3, 8, 6), ("chainx", 3, 12, 4)]


def _plant_kwargs(c, noise=True):
    sigma = _sigma(c)
    return dict(state_noise=sigma[:, :c.n], control_noise=sigma[:, c.n:], seed=SEED) if noise else {}


@pytest.mark.parametrize("name,B,N,replan", COMPOSE, ids=["%s-B%d-N%d-r%d" % s_ for s_ in COMPOSE])
def test_a_round_is_shift_plant_state_and_solve(name, B, N, replan):
    from drake_ddp_amd import _capi
    c = _case(name, B, N)
    a, t = _solved(c), _solved(c)
    rng = np.random.default_rng(42)
    x = np.array(a.x_bar)[:, :, 0] + 10.0 * c.sig[0] * rng.standard_normal((B, c.n))
    a.SetPlant(x, c.base * rng.uniform(0.9, 1.1, c.base.shape), **_plant_kwargs(c))
    _run(a, 1, replan)
    xp = np.ascontiguousarray(a.plant_state)
    assert not np.array_equal(xp, x) and np.isfinite(xp).all()
    t.MPCShift(replan)
    assert t._lib.mi_ilqr_set(t._h, _capi.F_X0, _capi.ptr(xp), xp.nbytes) == _capi.OK
    t.solve_resident()
    for f in ("x_bar", "u_bar", "K", "cost", "iterations", "status"):
        assert np.array_equal(getattr(a, f), getattr(t, f)), f
    assert np.array_equal(a.mpc_log[:, 0, :c.n], xp)
    assert np.array_equal(np.array(a.x_bar)[:, :, 0], xp)              # the re-solve did start from the plant's state


# ---------------------------------------------------------------- 3. one call of R rounds against R calls of one
@pytest.mark.parametrize("name,B,N,replan", [("pendulum", 65, 8, 2), ("pendulum_throughput", 3, 8, 6), ("quad3d", 3, 8, 2)])
def test_one_call_of_three_is_three_calls_of_one(name, B, N, replan):
    c = _case(name, B, N)
    a, t = _solved(c), _solved(c)
    rng = np.random.default_rng(43)
    x = np.array(a.x_bar)[:, :, 0] + 10.0 * c.sig[0] * rng.standard_normal((B, c.n))
    params = c.base * rng.uniform(0.9, 1.1, c.base.shape)
    for s in (a, t):
        s.SetPlant(x, params, **_plant_kwargs(c))
    _run(a, 3, replan)
    logs, mpc = [], []
    for _ in range(3):
        _run(t, 1, replan)
        logs.append(t.plant_log)
        mpc.append(t.mpc_log)
    assert a.plant_clock == t.plant_clock == 3 * replan
    for f in ("x_bar", "u_bar", "K", "cost", "iterations", "status", "plant_state"):
        assert np.array_equal(getattr(a, f), getattr(t, f)), f
    lg = a.plant_log
    assert np.array_equal(lg.X[:, :, :-1], np.concatenate([l_.X[:, :, :-1] for l_ in logs], axis=2)) and np.array_equal(lg.X[:, :, -1], logs[-1].X[:, :, -1])
    assert np.array_equal(lg.U, np.concatenate([l_.U for l_ in logs], axis=2))
    assert np.array_equal(lg.stage_cost, np.concatenate([l_.stage_cost for l_ in logs], axis=1)) and np.all(lg.steps == 3 * replan)
    assert np.array_equal(a.mpc_log, np.concatenate(mpc, axis=1))
    # the noise did enter: the second segment differs from a run whose clock starts again at 0
    assert not np.array_equal(logs[1].X, logs[0].X)


# ---------------------------------------------------------------- 4. against the policy-rollout kernel
@pytest.mark.parametrize("name,B,N,replan", [("pendulum", 65, 8, 6), ("pendulum_throughput", 3, 8, 3), ("quad3d", 3, 8, 6), ("chainx", 3, 12, 4)])
def test_the_first_segment_is_sample_0_of_the_policy_rollout(name, B, N, replan):
    c = _case(name, B, N)
    s = _solved(c)
    rng = np.random.default_rng(44)
    pol = _policy(s)
    x = pol[0][:, :, 0] + 10.0 * c.sig[0] * rng.standard_normal((B, c.n))
    params = c.base * rng.uniform(0.9, 1.1, c.base.shape)
    sigma = _sigma(c)
    ro = s.RolloutPolicy(x[:, None, :], params[:, None, :], trajectories=True, state_noise=sigma[:, :c.n], control_noise=sigma[:, c.n:], seed=SEED,
                         first_sample=0)
    s.SetPlant(x, params, state_noise=sigma[:, :c.n], control_noise=sigma[:, c.n:], seed=SEED, clock=0)
    _run(s, 1, replan)
    ref, sp, _, _ = _oracle_with_spread(c, x, params, pol, replan, sigma, SEED, 0)
    lg = s.plant_log
    xs, us = TP._scales(ref[3], ref[4])
    for b in range(B):
        assert np.max(np.abs(lg.X[b] - ro.X[b, 0, :, :replan + 1])) <= 1e-9 * xs[b] + 10.0 * sp[1][b, 0], b
        assert np.max(np.abs(lg.U[b] - ro.U[b, 0, :, :replan])) <= 1e-9 * us[b] + 10.0 * sp[2][b, 0], b
    s.RolloutPolicy(x[:, None, :])                                     # (leave the handle without policy noise)
    # MI_F_POLICY_NOISE and MI_F_PLANT_NOISE are independent: clearing the one above left the plant's rows alone
    from drake_ddp_amd import _capi
    got = np.empty((B, c.n + s._md))
    assert s._lib.mi_ilqr_get(s._h, _capi.F_PLANT_NOISE, _capi.ptr(got), got.nbytes) == _capi.OK and np.array_equal(got[:, :c.n + c.m], sigma)
    assert s._lib.mi_ilqr_get(s._h, _capi.F_POLICY_NOISE, _capi.ptr(got), got.nbytes) == _capi.OK and np.all(got == 0.0)


# ---------------------------------------------------------------- 5. failing plants are local
def test_a_failing_plant_is_local():
    """Planar quadruped (a model that can fail), three problems: a mild noise on problem 0, none on problem 2, and on problem 1 a
    control noise that overflows - against the same run without problem 1's noise."""
    B, N, replan, resolves = 3, 8, 3, 2
    c = _case("planar_quad", B, N)
    rng = np.random.default_rng(45)
    got = []
    for huge in (True, False):
        s = _solved(c)
        x = np.array(s.x_bar)[:, :, 0] + 1e-3 * np.random.default_rng(46).standard_normal((B, c.n))
        sx, su = np.zeros((B, c.n)), np.zeros((B, c.m))
        sx[0], su[0] = c.sig[0], c.sig[1]
        if huge:
            su[1] = np.finfo(np.float64).max
        s.SetPlant(x, state_noise=sx, control_noise=su, seed=SEED)
        _run(s, resolves, replan)
        got.append((s, x, s.plant_log, np.array(s.plant_state), np.array(s.mpc_log), _policy(s), np.array(s.status)))
    (s, x, lg, xp, mpc, pol, status), (_, _, lg0, xp0, mpc0, pol0, status0) = got
    K = resolves * replan
    assert np.all(lg0.steps == K) and np.isfinite(lg0.X).all() and lg.steps[0] == lg.steps[2] == K
    k = int(lg.steps[1])
    assert k < K                                                       # the plant stopped ...
    assert np.isfinite(lg.X[1, :, :k + 1]).all() and np.isnan(lg.X[1, :, k + 1:-1]).all() and np.isnan(lg.U[1, :, k:]).all()
    assert np.isnan(lg.stage_cost[1, k:]).all() and np.isfinite(lg.stage_cost[1, :k]).all()
    assert np.isfinite(xp[1]).all() and np.array_equal(xp[1], lg.X[1, :, k]) and np.array_equal(lg.X[1, :, -1], xp[1])     # ... and kept its last state
    if k == 0:
        assert np.array_equal(xp[1], x[1])
    r = k // replan                                                    # the round it stopped in: no MPC log row from there on
    assert np.all(mpc[1, r:] == 0.0) and all(np.any(mpc[1, i] != 0.0) for i in range(r)) and np.all(mpc0[1, :, -1] > 0.0)
    assert np.isfinite(pol[0][1]).all() and np.array_equal(pol[0][1][:, 0], xp[1])       # it was solved on from that state: no NaN reached a solve
    for b in (0, 2):                                                   # the others: bitwise the run without problem 1's noise
        assert np.array_equal(lg.X[b], lg0.X[b]) and np.array_equal(lg.U[b], lg0.U[b]) and np.array_equal(lg.stage_cost[b], lg0.stage_cost[b])
        assert np.array_equal(xp[b], xp0[b]) and np.array_equal(mpc[b], mpc0[b]) and status[b] == status0[b]
        assert all(np.array_equal(p_[b], q_[b]) for p_, q_ in zip(pol, pol0))
    # a later run: the plant stays where it stopped until SetPlant gives it a state again
    _run(s, 1, replan)
    assert np.array_equal(np.array(s.plant_state)[1], xp[1]) and s.plant_log.steps[1] == 0 and np.all(s.mpc_log[1] == 0.0)
    s.SetPlant(xp)
    _run(s, 1, replan)
    assert np.all(s.plant_log.steps == replan)


# ---------------------------------------------------------------- 6. clearing
@pytest.mark.parametrize("name,B,N,replan", [("pendulum", 3, 8, 2), ("pendulum_throughput", 3, 8, 2), ("quad3d", 3, 8, 2)])
def test_clearing_the_plant_is_the_open_loop(name, B, N, replan):
    c = _case(name, B, N)
    a, t = _solved(c), _solved(c)
    a.SetPlant(c.x0 + 0.01, c.base * 1.05, **_plant_kwargs(c))
    a.ClearPlant()
    _run(a, 2, replan); _run(t, 2, replan)
    for f in ("x_bar", "u_bar", "K", "cost", "iterations", "status", "mpc_log"):
        assert np.array_equal(getattr(a, f), getattr(t, f)), f
    from drake_ddp_amd import _capi
    got = np.empty((B, c.n))
    assert a._lib.mi_ilqr_get(a._h, _capi.F_PLANT_STATE, _capi.ptr(got), got.nbytes) == _capi.E_BAD_ARG      # no plant


@pytest.mark.parametrize("name,B,N,replan", [("pendulum", 3, 8, 2), ("acrobot", 65, 6, 4)])
def test_a_solve_after_a_closed_loop_run(name, B, N, replan):
    """... is bitwise the solve of a twin brought to the same x0 and guess (by the pieces of test 2)."""
    from drake_ddp_amd import _capi
    c = _case(name, B, N)
    a, t = _solved(c), _solved(c)
    a.SetPlant(c.x0 + 0.01, c.base * 1.05, **_plant_kwargs(c))
    _run(a, 1, replan)
    xp = np.ascontiguousarray(a.plant_state)
    t.MPCShift(replan)
    assert t._lib.mi_ilqr_set(t._h, _capi.F_X0, _capi.ptr(xp), xp.nbytes) == _capi.OK
    t.solve_resident()
    for s in (a, t):
        s.SetInitialState(c.x0 * 0.5)
        TP._solve(s)
    for f in ("x_bar", "u_bar", "K", "cost", "iterations", "status"):
        assert np.array_equal(getattr(a, f), getattr(t, f)), f


# ---------------------------------------------------------------- 7. the selectors through ctypes
def test_the_selectors_through_the_c_abi():
    from drake_ddp_amd import _capi
    B, N = 3, 8
    c = _case("pendulum", B, N)
    s = _solved(c)
    lib, h, n, m, P = s._lib, s._h, 2, 1, 3
    get = lambda which, a: lib.mi_ilqr_get(h, which, _capi.ptr(a), a.nbytes)            # noqa: E731
    put = lambda which, a, nb=None: lib.mi_ilqr_set(h, which, _capi.ptr(a), a.nbytes if nb is None else nb)   # noqa: E731
    st4, x, prm, nz = np.full(4, -1.0), np.full((B, n), -1.0), np.full((B, P), -1.0), np.full((B, n + m), -1.0)
    # a handle without a plant
    assert get(_capi.F_PLANT_STATE, x) == _capi.E_BAD_ARG and get(_capi.F_PLANT_LOG, np.empty((B, 2, n + m + 1))) == _capi.E_BAD_ARG
    assert get(_capi.F_PLANT_KERNEL_MS, np.empty(1)) == _capi.E_BAD_ARG
    assert get(_capi.F_PLANT_STREAM, st4) == _capi.OK and np.array_equal(st4, [0.0, 0.0, 0.0, 1.0])
    assert get(_capi.F_PLANT_NOISE, nz) == _capi.OK and np.all(nz == 0.0)
    assert get(_capi.F_PLANT_PARAMS, prm) == _capi.OK and np.array_equal(prm, c.base)             # not set: the problems' model rows
    rows = c.base * np.array([[1.1], [0.9], [1.0]])
    s.SetModelParameters(rows)
    assert get(_capi.F_PLANT_PARAMS, prm) == _capi.OK and np.array_equal(prm, rows)
    s.SetModelParameters(None)
    # values and shapes
    xs = np.arange(B * n, dtype=float).reshape(B, n)
    assert put(_capi.F_PLANT_STATE, xs) == _capi.OK
    for bad in (xs[:, :1].copy(), np.zeros((B + 1, n))):
        assert put(_capi.F_PLANT_STATE, bad) == _capi.E_BAD_SHAPE
    for v in (np.nan, np.inf, -np.inf):
        bad = xs.copy(); bad[1, 1] = v
        assert put(_capi.F_PLANT_STATE, bad) == _capi.E_BAD_ARG
    assert lib.mi_ilqr_set(h, _capi.F_PLANT_STATE, None, xs.nbytes) == _capi.E_BAD_ARG
    assert get(_capi.F_PLANT_STATE, x) == _capi.OK and np.array_equal(x, xs)                      # the refused calls changed nothing
    assert get(_capi.F_PLANT_STATE, np.empty((B, n + 1))) == _capi.E_BAD_SHAPE
    prows = c.base * 1.25
    assert put(_capi.F_PLANT_PARAMS, prows) == _capi.OK
    bad = prows.copy(); bad[2, 0] = np.nan
    assert put(_capi.F_PLANT_PARAMS, bad) == _capi.E_BAD_ARG and put(_capi.F_PLANT_PARAMS, prows[:, :2].copy()) == _capi.E_BAD_SHAPE
    assert get(_capi.F_PLANT_PARAMS, prm) == _capi.OK and np.array_equal(prm, prows)
    srows = np.arange(B * (n + m), dtype=float).reshape(B, n + m) * 1e-3
    assert put(_capi.F_PLANT_NOISE, srows) == _capi.OK
    for v in (-1.0, np.nan, np.inf):
        bad = srows.copy(); bad[1, 2] = v
        assert put(_capi.F_PLANT_NOISE, bad) == _capi.E_BAD_ARG
    assert put(_capi.F_PLANT_NOISE, np.zeros((B, n + m + 1))) == _capi.E_BAD_SHAPE
    assert get(_capi.F_PLANT_NOISE, nz) == _capi.OK and np.array_equal(nz, srows)
    top = np.array([2.0 ** 53 - 1, 2.0 ** 32 - 1, 1.0, 0.0])
    assert put(_capi.F_PLANT_STREAM, top) == _capi.OK
    for bad in ([-1.0, 0, 0, 1], [2.0 ** 53, 0, 0, 1], [0.5, 0, 0, 1], [np.nan, 0, 0, 1], [0, -1.0, 0, 1], [0, 2.0 ** 32, 0, 1], [0, 1.5, 0, 1],
                [0, 0, 2.0, 1], [0, 0, np.nan, 1], [0, 0, 0, 0.5], [0, 0, 0, -1.0]):
        assert put(_capi.F_PLANT_STREAM, np.array(bad, dtype=float)) == _capi.E_BAD_ARG, bad
    assert put(_capi.F_PLANT_STREAM, top, 24) == _capi.E_BAD_SHAPE and get(_capi.F_PLANT_STREAM, np.empty(3)) == _capi.E_BAD_SHAPE
    assert get(_capi.F_PLANT_STREAM, st4) == _capi.OK and np.array_equal(st4, top)
    # the read-only selectors cannot be set
    assert put(_capi.F_PLANT_LOG, np.zeros(4)) == _capi.E_BAD_ARG and put(_capi.F_PLANT_KERNEL_MS, np.zeros(1)) == _capi.E_BAD_ARG
    # a run whose clock would pass 2^32 is refused before anything is launched: nothing has moved
    before = [np.array(getattr(s, f)) for f in ("x_bar", "u_bar", "cost")]
    stats = _capi.Stats()
    import ctypes as C
    assert lib.mi_ilqr_mpc_run(h, 1, 2, None, C.byref(stats)) == _capi.E_BAD_ARG
    assert all(np.array_equal(v, getattr(s, f)) for v, f in zip(before, ("x_bar", "u_bar", "cost")))
    assert get(_capi.F_PLANT_STATE, x) == _capi.OK and np.array_equal(x, xs) and get(_capi.F_PLANT_STREAM, st4) == _capi.OK and st4[1] == 2.0 ** 32 - 1
    assert get(_capi.F_PLANT_LOG, np.empty((B, 2, n + m + 1))) == _capi.E_BAD_ARG
    assert lib.mi_ilqr_mpc_run(h, 1, 1, None, C.byref(stats)) == _capi.OK                         # the last step there is
    assert get(_capi.F_PLANT_STREAM, st4) == _capi.OK and st4[1] == 2.0 ** 32
    log = np.empty((B, 1, n + m + 1))
    assert get(_capi.F_PLANT_LOG, log) == _capi.OK and np.array_equal(log[:, 0, :n], xs)
    assert get(_capi.F_PLANT_LOG, np.empty((B, 2, n + m + 1))) == _capi.E_BAD_SHAPE
    ms = np.empty(1)
    assert get(_capi.F_PLANT_KERNEL_MS, ms) == _capi.OK and ms[0] > 0.0 and get(_capi.F_PLANT_KERNEL_MS, np.empty(2)) == _capi.E_BAD_SHAPE
    # the device rows, where there are any
    p_, nb = C.c_void_p(), C.c_size_t()
    assert lib.mi_ilqr_device_ptr(h, _capi.F_PLANT_STATE, C.byref(p_), C.byref(nb)) == _capi.OK and p_.value and nb.value == xs.nbytes
    # everything survives a reset; clearing returns the defaults
    assert lib.mi_ilqr_reset(h) == _capi.OK
    assert get(_capi.F_PLANT_NOISE, nz) == _capi.OK and np.array_equal(nz, srows) and get(_capi.F_PLANT_PARAMS, prm) == _capi.OK and np.array_equal(prm, prows)
    assert get(_capi.F_PLANT_STATE, x) == _capi.OK and np.isfinite(x).all()
    for which in (_capi.F_PLANT_STATE, _capi.F_PLANT_PARAMS, _capi.F_PLANT_NOISE):
        assert lib.mi_ilqr_set(h, which, None, 0) == _capi.OK
    assert get(_capi.F_PLANT_STATE, x) == _capi.E_BAD_ARG and get(_capi.F_PLANT_NOISE, nz) == _capi.OK and np.all(nz == 0.0)
    assert get(_capi.F_PLANT_PARAMS, prm) == _capi.OK and np.array_equal(prm, c.base)
    assert lib.mi_ilqr_device_ptr(h, _capi.F_PLANT_STATE, C.byref(p_), C.byref(nb)) == _capi.E_BAD_ARG


def test_plant_parameters_on_a_parameterless_model():
    from drake_ddp_amd import _capi, plugin
    import models as PM
    sys_ = plugin.build_model(*PM.NOISEPROBE_SPEC)(0.01)
    assert sys_.params.size == 0
    n, m = sys_.n, sys_.m
    p = dict(model_id=sys_.model_id, dt=0.01, N=5, delta=1e-3, beta=0.5, gamma=0.0, Q=np.eye(n), R=np.eye(m), Qf=np.eye(n), x_nom=np.zeros(n))
    s = TP._solver(p, system=sys_, batch=2)
    v = np.zeros((2, 1))
    assert s._lib.mi_ilqr_set(s._h, _capi.F_PLANT_PARAMS, _capi.ptr(v), v.nbytes) == _capi.E_UNSUPPORTED
    assert s._lib.mi_ilqr_set(s._h, _capi.F_PLANT_PARAMS, None, 0) == _capi.E_UNSUPPORTED
    with pytest.raises(ValueError, match="no parameters"):
        s.SetPlant(np.zeros(n), np.zeros(0))
    # the probe passes the disturbances through (x+ = 0 x + u): on a cold handle the plant's states ARE the state normals
    s.SetPlant(np.zeros(n), state_noise=1.0, seed=PN.TEST_SEED, clock=3)
    s.SetInitialState(np.zeros((2, n)))
    _run(s, 1, 3)
    X = s.plant_log.X
    for b in range(2):
        z = PN.state_normals(PN.TEST_SEED, 0, False, b, 0, 3 + np.arange(3), n)          # (3, n)
        assert np.abs(X[b, :, 1:].T - z).max() <= PN.NORMAL_TOL, b
