"""Monte-Carlo rollouts of the solved feedback policy on the device (BatchedIterativeLQR.RolloutPolicy, mi_ilqr_policy_rollout;
csrc/policy_rollout.hpp: one lane per sample) against the NumPy statement of the same thing (tests/policy_rollout_np.py), against
the existing stage entry, and against itself: every kernel family's policy layout, ragged sample counts, per-sample parameters,
control limits, per-problem costs and targets, failing samples, padding controls, and no side effects on the solver.

Tolerance against the oracle, per sample: 1e-9 relative + 10 x the oracle's own spread under a one-ulp np.nextafter perturbation of
x0 in both directions (the rule of tests/test_gpu_control_limits_mid.py: _check_vs_oracle); the perturbations of x0 are small enough
that this spread stays below 1e-6 relative for every sample, which _reference asserts with the oracle alone."""
import functools
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "plugins"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

B = 3
S_VALUES = (1, 65, 130)          # fewer than a wave, one lane into the second wave, a ragged tail
S_MAX = max(S_VALUES)


def _cases():
    from drake_ddp_amd import workloads as W
    z = lambda N: np.zeros((1, N - 1))   # noqa: E731
    # name: (problem, B x0's, initial guess, kernel_mode, std of the x0 perturbations); N of the workloads problems cut to <= 40,
    # further for the models whose NumPy step takes 0.1 - 0.3 ms (the reference is 3 rollouts per sample)
    return {
        "pendulum": lambda: (dict(W.pendulum_problem(), N=40), W.pendulum_batch_x0(B), z(40), "auto", 0.05),
        "pendulum_throughput": lambda: (dict(W.pendulum_problem(), N=40), W.pendulum_batch_x0(B), z(40), "throughput", 0.05),
        "acrobot": lambda: (W.acrobot_problem(40), W.acrobot_batch_x0(B), z(40), "auto", 0.02),
        "cartpole_wall": lambda: (W.cartpole_wall_problem(40), W.cartpole_wall_batch_x0(B), z(40), "auto", 0.01),
        "arm27": lambda: (W.arm27_problem(10), W.arm27_batch_x0(B), W.arm27_u_guess(10), "auto", 1e-3),
        "synth36": lambda: (W.synth36_problem(16), W.synth36_batch_x0(B), W.synth36_u_guess(16), "auto", 1e-2),
        "quad3d": lambda: (W.quad3d_problem(8), W.quad3d_batch_x0(B), W.quad3d_u_guess(8), "auto", 1e-3),
        "planar_quad": lambda: (W.planar_quad_problem(8), W.planar_quad_batch_x0(B), W.planar_quad_u_guess(8), "auto", 1e-3),
    }


CASE_NAMES = ["pendulum", "acrobot", "cartpole_wall", "arm27", "synth36", "quad3d", "planar_quad", "pendulum_throughput"]


def _solver(p, system=None, batch=B, **kw):
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    from drake_ddp_amd.models import ModelSystem
    s = BatchedIterativeLQR(system or ModelSystem(p["model_id"], p["dt"]), p["N"], batch, delta=p["delta"], beta=p["beta"],
                            gamma=p["gamma"], device=0, **kw)
    s.SetTargetState(p["x_nom"]); s.SetRunningCost(p["Q"], p["R"]); s.SetTerminalCost(p["Qf"])
    return s


def _solve(s):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # (max_iters = 3: "not converged" is expected, the policy is what matters)
        return s.Solve()


class _Ctx:
    pass


@functools.lru_cache(maxsize=None)
def _ctx(name):
    """A handle with a policy on it (three iLQR iterations from the problem's own start), the policy on the host, and the samples:
    problem b's own x0 (sample 0) plus seeded perturbations, per-sample parameters scaled by seeded factors in [0.8, 1.2]."""
    from oracle import models_np as M
    c = _Ctx()
    c.p, c.x0b, ug, mode, sigma = _cases()[name]()
    c.s = _solver(c.p, max_iters=3, kernel_mode=mode)
    c.s.SetInitialState(c.x0b); c.s.SetInitialGuess(ug)
    _solve(c.s)
    c.solve_cost = np.array(c.s.cost)
    c.x_bar, c.u_bar, c.K = np.array(c.s.x_bar), np.array(c.s.u_bar), np.array(c.s.K)
    rng = np.random.default_rng(100 + CASE_NAMES.index(name))
    c.x0 = c.x0b[:, None, :] + sigma * rng.standard_normal((B, S_MAX, c.x0b.shape[1]))
    c.x0[:, 0] = c.x0b
    base = np.asarray(M.DEFAULT_PARAMS[c.p["model_id"]], dtype=float)
    c.params = base[None, None, :] * rng.uniform(0.8, 1.2, (B, S_MAX, base.size))
    c.make_model = lambda row=None: M.Model(c.p["model_id"], c.p["dt"], row)
    c.base = np.tile(base, (B, 1))
    return c


def _oracle_with_spread(make_model, x0, params, x_bar, u_bar, K, Q, R, Qf, x_nom, u_min=None, u_max=None):
    """The oracle's cost, x_final, steps, X, U for every sample, and its own spread (cost, X, U per sample) under a one-ulp
    perturbation of x0 in both directions."""
    from policy_rollout_np import rollout
    ref = rollout(make_model, x0, params, x_bar, u_bar, K, Q, R, Qf, x_nom, u_min, u_max)
    sp = [np.zeros(ref[0].shape) for _ in range(3)]
    for d in (np.inf, -np.inf):
        alt = rollout(make_model, np.nextafter(x0, d), params, x_bar, u_bar, K, Q, R, Qf, x_nom, u_min, u_max)
        with np.errstate(invalid="ignore"):
            sp[0] = np.fmax(sp[0], np.abs(alt[0] - ref[0]))
            sp[1] = np.fmax(sp[1], np.nanmax(np.abs(alt[3] - ref[3]), axis=(2, 3)))
            sp[2] = np.fmax(sp[2], np.nanmax(np.abs(alt[4] - ref[4]), axis=(2, 3)) if ref[4].shape[3] > 0 else 0.0)
    return ref, sp


def _assert_spread_small(ref, sp):
    """The comparison must not be swallowed by the spread: below 1e-6 relative for every sample whose rollout is finite."""
    cost, _, _, X, U = ref
    fin = np.isfinite(cost)
    assert fin.any()
    assert np.all(sp[0][fin] <= 1e-6 * np.abs(cost[fin])), float(np.max(sp[0][fin] / np.abs(cost[fin])))
    xs, us = _scales(X, U)
    assert np.all(sp[1][fin] <= 1e-6 * np.broadcast_to(xs[:, None], fin.shape)[fin])
    assert np.all(sp[2][fin] <= 1e-6 * np.broadcast_to(us[:, None], fin.shape)[fin])


def _scales(X, U):
    """What "relative" refers to for the trajectories: the largest |x| and |u| among problem b's samples (one sample's controls may
    all be zero: the nominal sample of a zero guess)."""
    with np.errstate(invalid="ignore"):
        return np.nanmax(np.abs(X), axis=(1, 2, 3)), np.maximum(np.nanmax(np.abs(U), axis=(1, 2, 3)), 1e-300)


def _compare(r, ref, sp, S, report=None):
    """Device result `r` (the first S samples of the reference's) against the oracle: see the module docstring."""
    cost, xf, steps, X, U = (a[:, :S] for a in ref)
    sc, sx, su = (a[:, :S] for a in sp)
    assert r.cost.shape == cost.shape and r.x_final.shape == xf.shape and r.steps.shape == steps.shape and r.steps.dtype == np.int32
    assert r.X.shape == X.shape and r.U.shape == U.shape
    fin = np.isfinite(cost)
    assert np.array_equal(r.steps[fin], steps[fin])
    worst = [0.0, 0.0, 0.0]
    xsc, usc = _scales(ref[3], ref[4])
    for b, s in zip(*np.nonzero(fin)):
        e = abs(r.cost[b, s] - cost[b, s])
        assert e <= 1e-9 * abs(cost[b, s]) + 10.0 * sc[b, s], (b, s, r.cost[b, s], cost[b, s], sc[b, s])
        worst[0] = max(worst[0], e / abs(cost[b, s]))
        xs, us = xsc[b], usc[b]
        ex, eu = np.max(np.abs(r.X[b, s] - X[b, s])), np.max(np.abs(r.U[b, s] - U[b, s]))
        assert ex <= 1e-9 * xs + 10.0 * sx[b, s], (b, s, ex, xs, sx[b, s])
        assert eu <= 1e-9 * us + 10.0 * su[b, s], (b, s, eu, us, su[b, s])
        assert np.max(np.abs(r.x_final[b, s] - xf[b, s])) <= 1e-9 * xs + 10.0 * sx[b, s], (b, s)
        worst[1], worst[2] = max(worst[1], ex / xs), max(worst[2], eu / us)
    for b, s in zip(*np.nonzero(~fin)):                       # the oracle's sample ended early: so did the device's, at the same step
        if r.steps[b, s] == steps[b, s]:                      # (a step ON the feasibility bound may fall either way at round-off level)
            assert r.cost[b, s] == np.inf
            assert np.array_equal(np.isnan(r.X[b, s]), np.isnan(X[b, s])) and np.array_equal(np.isnan(r.U[b, s]), np.isnan(U[b, s]))
    if report is not None:
        print("policy rollout %s S=%d: worst relative device-oracle discrepancy cost %.2e X %.2e U %.2e; oracle spread cost %.2e"
              % (report, S, worst[0], worst[1], worst[2], float(np.max(sc[fin] / np.abs(cost[fin])))))


@functools.lru_cache(maxsize=None)
def _reference(name, per_sample):
    c = _ctx(name)
    p = c.p
    ref, sp = _oracle_with_spread(c.make_model, c.x0, c.params if per_sample else c.base, c.x_bar, c.u_bar, c.K, p["Q"], p["R"], p["Qf"],
                                  p["x_nom"])
    _assert_spread_small(ref, sp)
    return ref, sp


# ---------------------------------------------------------------- 1. against the oracle, every kernel family
@pytest.mark.parametrize("per_sample", [False, True], ids=["own_params", "per_sample_params"])
@pytest.mark.parametrize("S", S_VALUES)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_against_the_oracle(name, S, per_sample):
    c = _ctx(name)
    ref, sp = _reference(name, per_sample)
    r = c.s.RolloutPolicy(c.x0[:, :S], c.params[:, :S] if per_sample else None, trajectories=True)
    _compare(r, ref, sp, S, report="%s %s" % (name, "per-sample params" if per_sample else "own params"))
    lean = c.s.RolloutPolicy(c.x0[:, :S], c.params[:, :S] if per_sample else None)         # without the trajectories: the same numbers
    assert lean.X is None and lean.U is None
    assert np.array_equal(lean.cost, r.cost) and np.array_equal(lean.x_final, r.x_final) and np.array_equal(lean.steps, r.steps)


# ---------------------------------------------------------------- 2. against the existing device path
@pytest.mark.parametrize("name", ["pendulum", "arm27", "quad3d"])
def test_against_stage_rollout(name):
    """One sample per problem: RolloutPolicy(x0') against SetInitialState(x0'); stage_rollout(0.0) on a second handle carrying the
    same state.  Margin: 10 x the discrepancy between stage_rollout(0.0) and the oracle on the same inputs (measured here), with
    a floor of 1e-12 relative."""
    from policy_rollout_np import rollout
    c = _ctx(name)
    p = c.p
    x0 = np.ascontiguousarray(c.x0[:, 1])                      # a perturbed start
    r = c.s.RolloutPolicy(x0[:, None, :], trajectories=True)
    s2 = _solver(p)
    s2.set_state(x_bar=c.x_bar, u_bar=c.u_bar, K=c.K)
    s2.SetInitialState(x0)
    xs, us, L, _ = s2.stage_rollout(0.0)
    o = rollout(c.make_model, x0[:, None, :], c.base, c.x_bar, c.u_bar, c.K, p["Q"], p["R"], p["Qf"], p["x_nom"])
    assert np.isfinite(o[0]).all()
    for b in range(B):
        mL = max(10.0 * abs(L[b] - o[0][b, 0]), 1e-12 * abs(o[0][b, 0]))
        mx = max(10.0 * np.max(np.abs(xs[b] - o[3][b, 0])), 1e-12 * np.max(np.abs(o[3][b, 0])))
        mu = max(10.0 * np.max(np.abs(us[b] - o[4][b, 0])), 1e-12 * np.max(np.abs(o[4][b, 0])))
        print("stage_rollout vs oracle", name, b, abs(L[b] - o[0][b, 0]), "RolloutPolicy vs stage_rollout", abs(r.cost[b, 0] - L[b]))
        assert abs(r.cost[b, 0] - L[b]) <= mL, (b, r.cost[b, 0], L[b], mL)
        assert np.max(np.abs(r.X[b, 0] - xs[b])) <= mx and np.max(np.abs(r.U[b, 0] - us[b])) <= mu, b
        assert r.steps[b, 0] == p["N"] - 1


# ---------------------------------------------------------------- 3. the nominal sample
@pytest.mark.parametrize("name", ["pendulum", "quad3d", "pendulum_throughput"])
def test_the_nominal_sample_reproduces_the_solve(name):
    c = _ctx(name)
    ref, sp = _reference(name, False)
    r = c.s.RolloutPolicy(c.x0[:, :1], trajectories=True)
    for b in range(B):
        assert abs(r.cost[b, 0] - c.solve_cost[b]) <= 1e-9 * abs(c.solve_cost[b]) + 10.0 * sp[0][b, 0], (b, r.cost[b, 0], c.solve_cost[b])
        assert np.max(np.abs(r.X[b, 0] - c.x_bar[b])) <= 1e-9 * np.max(np.abs(c.x_bar[b])) + 10.0 * sp[1][b, 0], b


# ---------------------------------------------------------------- 4. N = 2
def test_one_step():
    """N = 2, S = 1: U is exactly clip(u_bar - K (x0 - x_bar_0)) - gains and offsets are short dyadic numbers, so the sum has one
    value whatever the order and the fusing - and X one call of the oracle's step; costs to 1e-12 relative."""
    from drake_ddp_amd import workloads as W
    from oracle import models_np as M
    p = dict(W.pendulum_problem(), N=2)
    s = _solver(p, control_limits="enforce")
    lo, hi = np.array([[-0.25], [-8.0], [-8.0]]), np.array([[0.25], [8.0], [8.0]])
    s.SetControlLimits(lo, hi)
    x_bar = np.zeros((B, 2, 2)); x_bar[:, :, 0] = [[0.5, -0.25], [1.0, 0.125], [-0.75, 2.0]]
    u_bar = np.array([0.5, -1.25, 2.0]).reshape(B, 1, 1)
    K = np.array([[1.5, 0.25], [-2.0, 0.5], [0.75, -1.0]]).reshape(B, 1, 2, 1)
    x0 = x_bar[:, :, 0] + np.array([[0.5, 0.25], [-0.125, 1.0], [0.375, -0.5]])
    s.set_state(x_bar=x_bar, u_bar=u_bar, K=K)
    r = s.RolloutPolicy(x0[:, None, :], trajectories=True)
    model = M.Model(p["model_id"], p["dt"])
    for b in range(B):
        u = np.clip(u_bar[b, :, 0] - K[b, :, :, 0] @ (x0[b] - x_bar[b, :, 0]), lo[b], hi[b])
        assert np.array_equal(r.U[b, 0, :, 0], u), (b, r.U[b, 0, :, 0], u)
        x1 = model.step(x0[b], u)
        assert np.array_equal(r.X[b, 0, :, 0], x0[b]) and np.max(np.abs(r.X[b, 0, :, 1] - x1)) <= 1e-12 * np.max(np.abs(x1))
        assert np.array_equal(r.x_final[b, 0], r.X[b, 0, :, 1]) and r.steps[b, 0] == 1
        d0, d1 = x0[b] - p["x_nom"], x1 - p["x_nom"]
        L = d0 @ p["Q"] @ d0 + u @ p["R"] @ u + d1 @ p["Qf"] @ d1
        assert abs(r.cost[b, 0] - L) <= 1e-12 * abs(L), (b, r.cost[b, 0], L)
    assert r.U[0, 0, 0, 0] in (-0.25, 0.25)                   # problem 0's law left its box


# ---------------------------------------------------------------- 5. limits
def test_control_limits():
    c = _ctx("pendulum")
    p = c.p
    S = 65
    lo, hi = np.array([[-0.4], [-0.2], [-1.0]]), np.array([[0.3], [0.5], [0.1]])
    rng = np.random.default_rng(5)
    x0 = c.x0b[:, None, :] + 1.5 * rng.standard_normal((B, S, 2))          # far enough out that the feedback saturates
    out = {}
    for mode in ("enforce", "ignore"):
        s = _solver(p, control_limits=mode)
        s.SetControlLimits(lo, hi)
        s.set_state(x_bar=c.x_bar, u_bar=c.u_bar, K=c.K)
        out[mode] = s.RolloutPolicy(x0, trajectories=True)
    r = out["enforce"]
    assert np.all(r.U >= lo[:, None, :, None]) and np.all(r.U <= hi[:, None, :, None])       # exactly
    assert np.any(r.U == lo[:, None, :, None]) and np.any(r.U == hi[:, None, :, None])       # some step rode a bound
    ref, sp = _oracle_with_spread(c.make_model, x0, c.base, c.x_bar, c.u_bar, c.K, p["Q"], p["R"], p["Qf"], p["x_nom"], lo, hi)
    _assert_spread_small(ref, sp)
    _compare(r, ref, sp, S, report="pendulum clamped")
    free = out["ignore"]
    assert np.any(free.U < lo[:, None, :, None]) and np.any(free.U > hi[:, None, :, None])   # "ignore": the reference's no-op
    ref, sp = _oracle_with_spread(c.make_model, x0, c.base, c.x_bar, c.u_bar, c.K, p["Q"], p["R"], p["Qf"], p["x_nom"])
    _compare(free, ref, sp, S)


# ---------------------------------------------------------------- 6. per-problem costs and targets
def test_per_problem_costs_and_targets():
    c = _ctx("pendulum")
    p = c.p
    S = 5
    rng = np.random.default_rng(6)
    A = rng.standard_normal((B, 2, 2))
    Q = np.einsum("bij,bkj->bik", A, A) + p["Q"]
    Qf = 3.0 * Q + p["Qf"]
    x_nom = p["x_nom"][None, :] + 0.3 * rng.standard_normal((B, 2))
    pol = [np.ascontiguousarray(np.broadcast_to(a[:1], a.shape)) for a in (c.x_bar, c.u_bar, c.K)]     # ONE policy, samples and plant
    x0 = np.ascontiguousarray(np.broadcast_to(c.x0[:1, :S], (B, S, 2)))

    def run(order):
        s = _solver(p)
        s.SetRunningCost(Q[order], p["R"]); s.SetTerminalCost(Qf[order]); s.SetTargetState(x_nom[order])
        s.set_state(x_bar=pol[0], u_bar=pol[1], K=pol[2])
        return s.RolloutPolicy(x0)
    r = run([0, 1, 2])
    assert len({float(v) for v in r.cost[:, 0]}) == B                        # the costs do follow the problems' matrices
    sw = run([1, 0, 2])
    assert np.array_equal(sw.cost[0], r.cost[1]) and np.array_equal(sw.cost[1], r.cost[0]) and np.array_equal(sw.cost[2], r.cost[2])
    assert np.array_equal(sw.x_final, r.x_final)
    ref, sp = _oracle_with_spread(c.make_model, x0, c.base, pol[0], pol[1], pol[2], Q, p["R"], Qf, x_nom)
    for b in range(B):
        for s_ in range(S):
            assert abs(r.cost[b, s_] - ref[0][b, s_]) <= 1e-9 * abs(ref[0][b, s_]) + 10.0 * sp[0][b, s_], (b, s_)


# ---------------------------------------------------------------- 7. failing samples do not leak
@pytest.mark.parametrize("name", ["quad3d", "planar_quad"])
def test_failing_samples_do_not_leak(name):
    from oracle import models_np as M
    from policy_rollout_np import rollout
    c = _ctx(name)
    p = c.p
    S = 65
    n = c.x0.shape[2]
    nq, vmax = (M.Q3_NQ, M.DEFAULT_PARAMS[M.QUAD3D][6]) if name == "quad3d" else (M.QUAD_NQ, M.DEFAULT_PARAMS[M.PLANAR_QUAD][8])
    clean = np.ascontiguousarray(c.x0[:, :S])
    bad = clean.copy()
    fast, nan_at = [0, 17, 63, 64], 30
    for s_ in fast:
        bad[:, s_, n - 1 - (s_ % 3)] = 2.0 * vmax                           # a joint rate no step brings back inside the bound
    bad[:, nan_at, 2] = np.nan
    o = rollout(c.make_model, bad, c.base, c.x_bar, c.u_bar, c.K, p["Q"], p["R"], p["Qf"], p["x_nom"])
    failing = sorted(fast + [nan_at])
    assert all(sorted(np.nonzero(~np.isfinite(o[0][b]))[0]) == failing for b in range(B))    # exactly the chosen samples
    assert np.all(o[2][:, failing] == 0)
    r_bad = c.s.RolloutPolicy(bad, trajectories=True)
    r_ok = c.s.RolloutPolicy(clean, trajectories=True)
    assert np.all(r_bad.cost[:, failing] == np.inf) and np.array_equal(r_bad.steps[:, failing], o[2][:, failing])
    assert np.array_equal(r_bad.x_final[:, failing], bad[:, failing], equal_nan=True)         # the last state they held
    assert np.array_equal(r_bad.X[:, failing][..., 0], bad[:, failing], equal_nan=True)
    assert np.isnan(r_bad.X[:, failing][..., 1:]).all() and np.isnan(r_bad.U[:, failing]).all()
    others = [s_ for s_ in range(S) if s_ not in failing]
    assert np.isfinite(r_ok.cost).all() and np.all(r_ok.steps == p["N"] - 1)
    for a in ("cost", "x_final", "steps", "X", "U"):                         # bitwise: lane independence is exact
        assert np.array_equal(getattr(r_bad, a)[:, others], getattr(r_ok, a)[:, others]), a


@pytest.mark.parametrize("name", ["quad3d", "planar_quad"])
def test_a_sample_that_fails_mid_rollout(name):
    """Samples that end at a step t >= 1.  A second handle carries the policy with a torque pulse added to u_bar at step t_b = N - 2 - b,
    large enough to throw a joint rate to about 2 - 3 v_max (1600 / 400 N m: chosen with the oracle); the chosen samples keep the plant's v_max and end there, every other sample's
    plant has v_max = 1e9 and runs to the end (the oracle, on the CPU, confirms both).  steps, the cost, x_final = the state held at
    t, X's steps + 1 and U's steps valid columns and the NaN behind them are the oracle's; the other samples are bitwise what they
    are when the chosen ones survive too."""
    from oracle import models_np as M
    from policy_rollout_np import rollout
    c = _ctx(name)
    p = c.p
    S, N = 65, c.p["N"]
    iv = 6 if name == "quad3d" else 8                                            # v_max among the parameters
    x0 = np.ascontiguousarray(c.x0[:, :S])
    u_bar = c.u_bar.copy()
    t_of = [N - 2 - b for b in range(B)]
    for b in range(B):
        u_bar[b, 0, t_of[b]] += 1600.0 if name == "quad3d" else 400.0
    chosen = [5, 63, 64]
    free = np.ascontiguousarray(np.broadcast_to(c.base[:, None, :], (B, S, c.base.shape[1])))
    free[:, :, iv] = 1e9
    prm = free.copy()
    prm[:, chosen, iv] = c.base[0, iv]
    args = (c.x_bar, u_bar, c.K, p["Q"], p["R"], p["Qf"], p["x_nom"])
    o = rollout(c.make_model, x0, prm, *args)
    others = [s_ for s_ in range(S) if s_ not in chosen]
    for b in range(B):
        assert np.all(o[2][b, chosen] == t_of[b]) and np.all(o[0][b, chosen] == np.inf) and 1 <= t_of[b] < N - 1
        assert np.all(o[2][b, others] == N - 1) and np.isfinite(o[0][b, others]).all()
    s2 = _solver(p)
    s2.set_state(x_bar=c.x_bar, u_bar=u_bar, K=c.K)
    r = s2.RolloutPolicy(x0, prm, trajectories=True)
    r_ok = s2.RolloutPolicy(x0, free, trajectories=True)
    xsc, usc = _scales(o[3], o[4])
    for b in range(B):
        t = t_of[b]
        for s_ in chosen:
            assert r.steps[b, s_] == t and r.cost[b, s_] == np.inf
            assert np.isfinite(r.X[b, s_, :, :t + 1]).all() and np.isnan(r.X[b, s_, :, t + 1:]).all()
            assert np.isfinite(r.U[b, s_, :, :t]).all() and np.isnan(r.U[b, s_, :, t:]).all()
            assert np.array_equal(np.isnan(r.X[b, s_]), np.isnan(o[3][b, s_])) and np.array_equal(np.isnan(r.U[b, s_]), np.isnan(o[4][b, s_]))
            assert np.array_equal(r.x_final[b, s_], r.X[b, s_, :, t])             # the last state it held
            assert np.max(np.abs(r.X[b, s_, :, :t + 1] - o[3][b, s_, :, :t + 1])) <= 1e-9 * xsc[b]
            assert np.max(np.abs(r.U[b, s_, :, :t] - o[4][b, s_, :, :t])) <= 1e-9 * usc[b]
            assert np.max(np.abs(r.x_final[b, s_] - o[1][b, s_])) <= 1e-9 * xsc[b]
            assert r_ok.steps[b, s_] == N - 1 and np.isfinite(r_ok.cost[b, s_])   # (the same lanes, surviving)
    assert np.all(r.steps[:, others] == N - 1) and np.isfinite(r.cost[:, others]).all()
    for a in ("cost", "x_final", "steps", "X", "U"):
        assert np.array_equal(getattr(r, a)[:, others], getattr(r_ok, a)[:, others]), a


def test_params_on_a_model_without_parameters_is_unsupported():
    """The C entry itself (the Python wrapper raises ValueError before it gets there)."""
    from drake_ddp_amd import _capi, plugin
    from drake_ddp_amd import workloads as W
    body = """
    const T w = x[1] + dt * (u[0] - 0.1 * x[1] - 4.0 * mi_sin(x[0]));
    xn[0] = x[0] + dt * w;
    xn[1] = w;
"""
    make = plugin.build_model("pp_noparams", 2, 1, body, [], "small")
    q = W.pendulum_problem()
    s = _solver(dict(q, N=10), system=make(q["dt"]))
    S = 3
    x0, prm, cost = np.zeros((B, S, 2)), np.ones((B, S, 1)), np.empty((B, S))
    rc = s._lib.mi_ilqr_policy_rollout(s._h, S, _capi.ptr(x0), _capi.ptr(prm), _capi.ptr(cost), None, None, None, None)
    assert rc == _capi.E_UNSUPPORTED
    with pytest.raises(ValueError, match="no parameters"):
        s.RolloutPolicy(x0, prm)
    r = s.RolloutPolicy(x0)                                                       # the refusal left a working handle
    assert np.all(r.steps == 9) and np.isfinite(r.cost).all()


# ---------------------------------------------------------------- 8. padding controls, plugin models
@functools.lru_cache(maxsize=None)
def _plugins():
    import models as PM
    from drake_ddp_amd import plugin
    return PM.build_chainx(16, 3, 5), plugin.build_model("vdp", 2, 1, PM.VDP_BODY, PM.VDP_DEFAULTS, "small")


def test_padding_controls():
    """A chainx plugin with n = 37 > 32 and m = 3: four device controls (examples/plugins/models.py: PADDED_SHAPES - LARGE_SHAPES has no
    m % 4 != 0).  U has m rows and everything agrees with the oracle of the unpadded model."""
    import plugin_steps as PS
    from oracle import models_np as M
    nq, m, ne, dt, N, S = 16, 3, 5, 0.02, 12, 65
    n = 2 * nq + ne
    sys_ = _plugins()[0](dt)
    assert sys_.m == m and sys_.m_dev == 4
    p = dict(model_id=sys_.model_id, dt=dt, N=N, delta=1e-3, beta=0.6, gamma=0.0, Q=dt * np.eye(n), R=dt * 0.1 * np.eye(m),
             Qf=5.0 * np.eye(n), x_nom=np.zeros(n))
    rng = np.random.default_rng(8)
    x0b = 0.3 * rng.standard_normal((B, n))
    s = _solver(p, system=sys_, max_iters=3)
    s.SetInitialState(x0b); s.SetInitialGuess(np.zeros((m, N - 1)))
    _solve(s)
    x_bar, u_bar, K = np.array(s.x_bar), np.array(s.u_bar), np.array(s.K)
    assert u_bar.shape == (B, m, N - 1) and K.shape == (B, m, n, N - 1) and np.abs(K).max() > 0.0
    x0 = x0b[:, None, :] + 0.01 * rng.standard_normal((B, S, n)); x0[:, 0] = x0b
    params = sys_.params[None, None, :] * rng.uniform(0.8, 1.2, (B, S, sys_.params.size))
    make = lambda row: M.Model.custom(n, m, PS.chainx_step(nq, m, ne), row, dt)   # noqa: E731
    for prm in (None, params):
        r = s.RolloutPolicy(x0, prm, trajectories=True)
        assert r.U.shape == (B, S, m, N - 1)
        ref, sp = _oracle_with_spread(make, x0, np.tile(sys_.params, (B, 1)) if prm is None else prm, x_bar, u_bar, K, p["Q"], p["R"],
                                      p["Qf"], p["x_nom"])
        _assert_spread_small(ref, sp)
        _compare(r, ref, sp, S, report="chainx (37, 3) plugin")


def test_wave_family_plugin():
    """A family-0 plugin (Van der Pol): plugin.py emits the policy kernels for both families."""
    import plugin_steps as PS
    from oracle import models_np as M
    dt, N, S = 0.02, 30, 65
    sys_ = _plugins()[1](dt)
    p = dict(model_id=sys_.model_id, dt=dt, N=N, delta=1e-3, beta=0.8, gamma=0.0, Q=dt * np.eye(2), R=dt * 0.1 * np.eye(1),
             Qf=10.0 * np.eye(2), x_nom=np.zeros(2))
    rng = np.random.default_rng(9)
    x0b = rng.uniform(-1, 1, (B, 2))
    s = _solver(p, system=sys_, max_iters=3)
    s.SetInitialState(x0b); s.SetInitialGuess(np.zeros((1, N - 1)))
    _solve(s)
    x_bar, u_bar, K = np.array(s.x_bar), np.array(s.u_bar), np.array(s.K)
    x0 = x0b[:, None, :] + 0.05 * rng.standard_normal((B, S, 2))
    make = lambda row: M.Model.custom(2, 1, PS.vdp_step, row, dt)   # noqa: E731
    r = s.RolloutPolicy(x0, trajectories=True)
    ref, sp = _oracle_with_spread(make, x0, np.tile(sys_.params, (B, 1)), x_bar, u_bar, K, p["Q"], p["R"], p["Qf"], p["x_nom"])
    _assert_spread_small(ref, sp)
    _compare(r, ref, sp, S, report="vdp plugin")


# ---------------------------------------------------------------- 9. no side effects
@pytest.mark.parametrize("name", ["pendulum", "pendulum_throughput", "synth36"])
def test_no_side_effects_on_the_solver(name):
    """Solve(); RolloutPolicy(...); Solve() from the same inputs is bitwise Solve(); Solve() on a second handle."""
    c = _ctx(name)
    p, x0b, ug, mode, _ = _cases()[name]()
    got = []
    for with_rollout in (True, False):
        s = _solver(p, max_iters=6, kernel_mode=mode)
        s.SetInitialState(x0b); s.SetInitialGuess(ug)
        _solve(s)
        if with_rollout:
            r = s.RolloutPolicy(c.x0[:, :65], c.params[:, :65], trajectories=True)
            assert np.isfinite(r.cost).any()
        s.SetInitialState(x0b)
        _solve(s)
        got.append([np.array(a) for a in (s.x_bar, s.u_bar, s.K, s.cost, s.iterations)])
    for a, b_ in zip(*got):
        assert np.array_equal(a, b_)


# ---------------------------------------------------------------- the C entry's refusals
def test_c_entry_refuses_bad_arguments():
    from drake_ddp_amd import _capi
    c = _ctx("pendulum")
    lib, h = _capi.load(), c.s._h
    S = 4
    x0 = np.ascontiguousarray(c.x0[:, :S])
    cost = np.empty((B, S))
    call = lambda S_, x, prm, out: lib.mi_ilqr_policy_rollout(h, S_, _capi.ptr(x), _capi.ptr(prm), _capi.ptr(out), None, None, None, None)   # noqa: E731
    assert call(0, x0, None, cost) == _capi.E_BAD_ARG and call(-3, x0, None, cost) == _capi.E_BAD_ARG
    assert call(S, None, None, cost) == _capi.E_BAD_ARG and call(S, x0, None, None) == _capi.E_BAD_ARG
    prm = np.ascontiguousarray(c.params[:, :S]); prm[1, 2, 0] = np.inf
    assert call(S, x0, prm, cost) == _capi.E_BAD_ARG
    assert call(S, x0, None, cost) == _capi.OK                              # every optional output left out: the costs alone
    assert np.array_equal(cost, c.s.RolloutPolicy(x0).cost)
