"""Parameter identification on the device (BatchedIterativeLQR.FitModelParameters; MI_F_FIT_*; csrc/fit.hpp) against the NumPy
statement (tests/fit_np.py) on the cases of tests/fit_cases.py: B = 3 (5 where a batch is mixed), T = 70.

Tolerance against the oracle (the rule of tests/test_gpu_tracking.py): 10 x the oracle's OWN SPREAD - the largest change of the
quantity when theta and the data move by one ulp (all up, all down, and two patterns of random signs per entry), computed here.  The
finite-difference quotient amplifies rounding by about eps / fd_rel, so bitwise agreement is not expected; for a vector or a matrix
the spread is the largest change of any of its entries (a single entry's change can be zero by chance).  Device against device the
results are bitwise equal wherever the rows, the free set and T are the same."""
import functools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fit_cases as FC  # noqa: E402
import fit_np as FN  # noqa: E402

gpu = pytest.mark.gpu
COUNT = [70, 1, 33]          # several waves for every G and a ragged last one; a one-row problem; a count that ends inside a wave
FIELDS = ("cost0", "gradient", "normal_matrix")


@functools.lru_cache(maxsize=None)
def _plugin_case(which):
    """chain3 (family 0: n = 6, m = 2) and the (37, 3) chainx (family 1, four device controls, one of them padding) as cases."""
    sys.path.insert(0, os.path.join(ROOT, "examples", "plugins"))
    import models as PM
    import plugin_steps as PS
    from drake_ddp_amd import plugin
    from oracle import models_np as M
    c = FC.Case()
    c.B, c.T, c.dt = 3, 70, 0.02
    rng = np.random.default_rng(77 if which == "chain3" else 78)
    if which == "chain3":
        c.sys = plugin.build_model("chain3", 6, 2, PM.CHAIN3_BODY, PM.CHAIN3_DEFAULTS, "small")(c.dt)
        c.n, c.m, c.free, step, base = 6, 2, [0, 2], PS.chain3_step, np.array(PM.CHAIN3_DEFAULTS)
    else:
        c.sys = PM.build_chainx(16, 3, 5)(c.dt)
        assert c.sys.m == 3 and c.sys.m_dev == 4
        c.n, c.m, c.free, step, base = 37, 3, [0, 1, 3], PS.chainx_step(16, 3, 5), np.array(PM.CHAINX_DEFAULTS)
    c.truth = np.tile(base, (c.B, 1))
    c.truth[:, c.free] *= 1.0 + 0.1 * rng.uniform(-1, 1, (c.B, len(c.free)))
    c.start = c.truth.copy()
    c.start[:, c.free] *= 1.0 + 0.2 * rng.uniform(-1, 1, (c.B, len(c.free)))
    c.models = [M.Model.custom(c.n, c.m, step, c.truth[b], c.dt) for b in range(c.B)]
    c.x, c.u = 0.5 * rng.standard_normal((c.B, c.T, c.n)), rng.uniform(-1, 1, (c.B, c.T, c.m))
    c.x_next = np.stack([FN.predict(c.models[b], c.truth[b], c.x[b], c.u[b]) for b in range(c.B)])
    return c


def _case(kind, B=3):
    return _plugin_case(kind) if kind in ("chain3", "chainx") else FC.case(kind, B)


def _solver(c, B=None, N=4, **kw):
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    from drake_ddp_amd.models import ModelSystem
    system = c.sys if hasattr(c, "sys") else ModelSystem(c.model_id, c.dt)
    return BatchedIterativeLQR(system, N, c.B if B is None else B, device=0, max_iters=5, **kw)


def _fit(s, c, sel=None, **kw):
    sel = slice(0, s.B) if sel is None else sel
    a = dict(free=c.free, params0=c.start[sel])
    a.update(kw)
    return s.FitModelParameters(c.x[sel], c.u[sel], c.x_next[sel], **a)


def _same(a, b, sel_a=slice(None), sel_b=slice(None)):
    return all(np.array_equal(np.asarray(getattr(a, f))[sel_a], np.asarray(getattr(b, f))[sel_b], equal_nan=True)
               for f in ("params", "cost0", "cost", "damping", "iterations", "accepted", "status", "count", "gradient", "normal_matrix"))


def _ulp_alternates(c, b, seed=0):
    """(theta, x, u, x_next) of problem b moved by one ulp: all up, all down, two patterns of random signs."""
    rng = np.random.default_rng(seed)
    out = []
    for pat in ("up", "down", "r0", "r1"):
        def move(a):
            d = np.inf if pat == "up" else (-np.inf if pat == "down" else np.where(rng.integers(0, 2, a.shape) > 0, np.inf, -np.inf))
            return np.nextafter(a, d)
        th = c.start[b].copy()
        th[c.free] = move(th[c.free])
        out.append((th, move(c.x[b]), move(c.u[b]), move(c.x_next[b])))
    return out


@functools.lru_cache(maxsize=None)
def _normal_reference(kind, free=None):
    """Per problem: the oracle's normal equations at the start over COUNT rows, and their spread."""
    c = _case(kind)
    free = c.free if free is None else list(free)
    out = []
    for b in range(3):
        k = COUNT[b]
        w = np.ones(c.n)
        ref = FN.normal(c.models[b], c.start[b], c.x[b, :k], c.u[b, :k], c.x_next[b, :k], w, free)
        sp = [0.0, 0.0, 0.0]
        for th, x, u, xn in _ulp_alternates(c, b):
            alt = FN.normal(c.models[b], th, x[:k], u[:k], xn[:k], w, free)
            sp = [max(s, float(np.max(np.abs(np.asarray(a) - np.asarray(r))))) for s, a, r in zip(sp, alt, ref)]
        out.append((ref, sp))
    return out


# ---------------------------------------------------------------- 1. one evaluation against the oracle
@gpu
@pytest.mark.parametrize("kind", sorted(FC.KINDS) + ["chain3", "chainx"])
def test_one_evaluation_against_the_oracle(kind):
    c = _case(kind)
    s = _solver(c)
    r = _fit(s, c, count=COUNT, iterations=0)
    P = len(c.free)
    assert r.gradient.shape == (3, P) and r.normal_matrix.shape == (3, P, P) and np.array_equal(r.count, COUNT)
    assert np.array_equal(r.params, c.start) and np.array_equal(r.cost, r.cost0) and not r.iterations.any() and not r.accepted.any()
    assert np.all(r.status == FN.MAX_ITERS) and np.all(r.damping == 1e-3) and r.kernel_ms > 0.0 and r.kernel_ms == s.fit_kernel_ms()
    for b, (ref, sp) in enumerate(_normal_reference(kind)):
        for f, want, spread in zip(FIELDS, ref, sp):
            got = getattr(r, f)[b]
            dist = float(np.max(np.abs(got - want)))
            print(f"{kind}[{b}] {f}: device - oracle {dist:.2e} (relative {dist / max(float(np.max(np.abs(want))), 1e-300):.1e}), "
                  f"the oracle's one-ulp spread {spread:.2e}")
            assert dist <= 10.0 * spread, (kind, b, f, dist, spread)
        assert np.array_equal(r.normal_matrix[b], r.normal_matrix[b].T)


# ---------------------------------------------------------------- 2. recovery
TRIAL_FLOOR = 1e-12


@functools.lru_cache(maxsize=None)
def _trial_reference(kind):
    """Per problem: the oracle's cost after its trials 1, 2, 3 - as far as they are accepted ones with a cost of TRIAL_FLOOR or above -
    and the one-ulp spread of each.  Below that floor a cost is the square of residuals that are themselves round-off (the models that
    are nearly linear in their free parameters are there after one or two trials), and accepts flip on it: nothing to compare."""
    c = FC.case(kind)
    kw = FC.FIT_KW.get(kind, {})
    out = []
    for b in range(c.B):
        ref = FC.oracle_fit(c, b, iterations=3)
        costs = []
        for cost, accepted in ref["trials"]:
            if not accepted or cost < TRIAL_FLOOR:
                break
            costs.append(cost)
        assert costs, (kind, b)                                            # the first trial at least
        sp = np.zeros(len(costs))
        for th, x, u, xn in _ulp_alternates(c, b):
            alt = FN.fit(c.models[b], x, u, xn, th, c.free, iterations=len(costs), **kw)
            assert all(t[1] for t in alt["trials"])
            sp = np.maximum(sp, np.abs(np.array([t[0] for t in alt["trials"]]) - np.array(costs)))
        out.append((costs, sp))
    return out


@gpu
@pytest.mark.parametrize("kind", FC.RECOVERY)
def test_recovery_from_noise_free_data(kind):
    c = FC.case(kind)
    kw = FC.FIT_KW.get(kind, {})
    s = _solver(c)
    r = _fit(s, c, iterations=8, **kw)
    err = FC.rel_error(c, r.params)
    print(f"{kind}: relative parameter error {err}, cost {r.cost0} -> {r.cost}, trials {r.iterations}, accepted {r.accepted}, status {r.status}")
    assert np.all(err <= 1e-10), (kind, err)
    fixed = [k for k in range(c.truth.shape[1]) if k not in c.free]
    assert np.array_equal(r.params[:, fixed], c.start[:, fixed])
    assert np.all(r.cost < r.cost0) and np.all(r.iterations <= 8) and np.all(r.accepted <= r.iterations)
    ref = _trial_reference(kind)
    for k in (1, 2, 3):
        rk = _fit(s, c, iterations=k, **kw)
        for b in range(c.B):
            if k > len(ref[b][0]):
                continue
            want, sp = ref[b][0][k - 1], ref[b][1][k - 1]
            print(f"{kind}[{b}] cost after trial {k}: device {rk.cost[b]:.6e}, oracle {want:.6e}, the oracle's one-ulp spread {sp:.1e}")
            assert rk.accepted[b] == k and abs(rk.cost[b] - want) <= 10.0 * sp, (kind, b, k, rk.cost[b], want, sp)


# ---------------------------------------------------------------- 3. the state hand-over
@gpu
@pytest.mark.parametrize("kind", ("pendulum", "synth36"))
def test_four_iterations_are_two_calls_of_two(kind):
    c = FC.case(kind)
    rng = np.random.default_rng(11)
    xn = c.x_next + 1e-5 * rng.standard_normal(c.x_next.shape)
    s = _solver(c)
    whole = s.FitModelParameters(c.x, c.u, xn, free=c.free, params0=c.start, iterations=4, ftol=0.0)
    a = s.FitModelParameters(c.x, c.u, xn, free=c.free, params0=c.start, iterations=2, ftol=0.0)
    b = s.FitModelParameters(c.x, c.u, xn, free=c.free, params0=a.params, damping=a.damping, iterations=2, ftol=0.0)
    assert np.all(whole.status == FN.MAX_ITERS) and np.all(whole.cost > 0.0) and np.all(whole.accepted >= 2)
    for f in ("params", "cost", "damping", "gradient", "normal_matrix", "status", "count"):
        assert np.array_equal(getattr(whole, f), getattr(b, f)), f
    assert np.array_equal(whole.iterations, a.iterations + b.iterations) and np.array_equal(whole.accepted, a.accepted + b.accepted)
    assert np.array_equal(whole.cost0, a.cost0) and np.array_equal(b.cost0, a.cost)


# ---------------------------------------------------------------- 4. independence
@gpu
def test_a_problem_does_not_depend_on_the_batch_or_the_layout():
    c = FC.case("pendulum", 5)
    ref = _fit(_solver(c), c, iterations=3, count=[70, 1, 33, 70, 64])
    for b, k in ((2, 33), (3, 70)):
        one = _fit(_solver(c, B=1), c, sel=slice(b, b + 1), iterations=3, count=[k])
        assert _same(ref, one, slice(b, b + 1)), b
    for kw in (dict(kernel_mode="throughput"), dict(control_limits="enforce")):
        other = _fit(_solver(c, **kw), c, iterations=3, count=[70, 1, 33, 70, 64])
        assert _same(ref, other), kw


ACROBOT_FREE = ([1], [1, 7, 8], [0, 1, 2, 3, 4, 7, 8], [0, 1, 2, 3, 4, 5, 7, 8])      # G = 2, 4, 8, 16


@gpu
def test_every_group_size_gives_the_same_normal_matrix():
    c = FC.case("acrobot")
    s = _solver(c)
    full = ACROBOT_FREE[-1]
    ref = _normal_reference("acrobot", tuple(full))
    runs = [s.FitModelParameters(c.x, c.u, c.x_next, free=f, params0=c.start, count=COUNT, iterations=0) for f in ACROBOT_FREE]
    for f, r in zip(ACROBOT_FREE, runs):
        idx = [full.index(k) for k in f]
        for b in range(3):
            (_, g, H), sp = ref[b]
            assert abs(r.cost0[b] - runs[-1].cost0[b]) <= 10.0 * sp[0]
            assert np.max(np.abs(r.gradient[b] - runs[-1].gradient[b][idx])) <= 10.0 * sp[1], (f, b)
            assert np.max(np.abs(r.normal_matrix[b] - runs[-1].normal_matrix[b][np.ix_(idx, idx)])) <= 10.0 * sp[2], (f, b)
            assert np.max(np.abs(r.normal_matrix[b] - H[np.ix_(idx, idx)])) <= 10.0 * sp[2], (f, b)


# ---------------------------------------------------------------- 5. freezing and statuses
@gpu
def test_a_mixed_batch_freezes_what_has_finished():
    c = FC.case("pendulum", 5)
    x, u, xn = c.x.copy(), c.u.copy(), c.x_next.copy()
    x[1], u[1], xn[1] = 0.0, 0.0, [1e-3, 0.0]                      # at rest at the bottom without a torque: no parameter is visible
    count, mu = [0, 70, 70, 33, 70], [1e-3, 1e9, 1e-3, 1e-3, 1e-3]
    s = _solver(c)
    r = s.FitModelParameters(x, u, xn, free=c.free, params0=c.start, count=count, damping=mu, iterations=8)
    assert r.status[0] == FN.BAD_DATA and r.cost[0] == np.inf and r.cost0[0] == np.inf and r.iterations[0] == 0
    assert not r.gradient[0].any() and not r.normal_matrix[0].any()
    assert r.status[1] == FN.STALLED and r.iterations[1] == 4 and r.accepted[1] == 0 and r.damping[1] == 1e12 and r.cost[1] == r.cost0[1] > 0.0
    assert np.array_equal(r.params[:2], c.start[:2])               # untouched
    assert np.all(r.status[2:] != FN.BAD_DATA) and np.all(FC.rel_error(c, r.params)[2:] <= 1e-10)
    for b in (2, 3, 4):
        one = _solver(c, B=1).FitModelParameters(x[b:b + 1], u[b:b + 1], xn[b:b + 1], free=c.free, params0=c.start[b:b + 1], count=[count[b]],
                                                 iterations=8)
        assert _same(r, one, slice(b, b + 1)), b
    ref = FN.fit(c.models[1], x[1], u[1], xn[1], c.start[1], c.free, damping=1e9, iterations=8)
    assert (ref["status"], ref["iterations"], ref["damping"]) == (FN.STALLED, 4, 1e12)
    # a first cost that is not finite: ml2 = 0 divides by zero in every prediction
    bad = c.start.copy()
    bad[3, 0] = 0.0
    r = s.FitModelParameters(c.x, c.u, c.x_next, free=[1, 2], params0=bad, iterations=4)
    assert r.status[3] == FN.BAD_DATA and not np.isfinite(r.cost[3]) and np.array_equal(r.params[3], bad[3]) and r.iterations[3] == 0
    assert np.all(r.status[[0, 1, 2, 4]] != FN.BAD_DATA) and np.all(r.cost[[0, 1, 2, 4]] < r.cost0[[0, 1, 2, 4]])


# ---------------------------------------------------------------- 6. bounds
@gpu
def test_a_bound_above_the_truth_holds_the_result():
    c = FC.case("pendulum")
    k = c.free[1]
    lo = np.full(3, -np.inf)
    lo[k] = 1.05 * c.truth[:, k].max()
    s = _solver(c)
    held = _fit(s, c, iterations=12, bounds=(lo, None))
    free = _fit(s, c, iterations=12)
    assert np.all(held.params[:, k] == lo[k]) and np.all(held.cost > free.cost) and np.all(FC.rel_error(c, free.params) <= 1e-10)
    ref = FN.fit(c.models[0], c.x[0], c.u[0], c.x_next[0], c.start[0], c.free, bounds=(lo, np.full(3, np.inf)), iterations=12)
    assert abs(held.cost[0] - ref["cost"]) <= 1e-9 * ref["cost"]


# ---------------------------------------------------------------- 7. apply
def _pendulum_solver(B=3, **kw):
    from drake_ddp_amd import workloads as W
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    from drake_ddp_amd.models import ModelSystem
    p = W.pendulum_problem()
    s = BatchedIterativeLQR(ModelSystem(p["model_id"], p["dt"]), 30, B, delta=p["delta"], beta=p["beta"], gamma=p["gamma"], device=0, max_iters=5, **kw)
    s.SetTargetState(p["x_nom"]); s.SetRunningCost(p["Q"], p["R"]); s.SetTerminalCost(p["Qf"])
    s.SetInitialState(W.pendulum_batch_x0(B))
    return s


def _solve(s):
    s.Reset()
    s.SetInitialGuess(np.zeros((1, s.N - 1)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        s.Solve()
    return [np.array(a) for a in (s.x_bar, s.u_bar, s.cost, s.iterations, s.status)]


def _same_solve(a, b):
    return all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b))


@gpu
def test_apply_is_set_model_parameters_and_nothing_else_touches_a_solve():
    from drake_ddp_amd import _capi
    c = FC.case("pendulum")
    s = _pendulum_solver()
    before = _solve(s)
    p_before = np.array(s.model_params)
    fit = _fit(s, c, iterations=8)
    assert np.array_equal(s.model_params, p_before) and _same_solve(_solve(s), before)           # apply=False
    # a refused command: neither the results nor the parameter rows move
    bad = np.array([8, 1e-12, 1e-6, 1e-8, 1, 0], dtype=np.float64)                             # P = 0
    assert s._lib.mi_ilqr_set(s._h, _capi.F_FIT_RUN, _capi.ptr(bad), bad.nbytes) == _capi.E_BAD_SHAPE
    bad = np.array([8, 1e-12, 1e-6, 1e-8, 1, 2, 1, 1], dtype=np.float64)                       # free not increasing
    assert s._lib.mi_ilqr_set(s._h, _capi.F_FIT_RUN, _capi.ptr(bad), bad.nbytes) == _capi.E_BAD_ARG
    assert np.array_equal(s.model_params, p_before) and _same_solve(_solve(s), before)
    assert np.array_equal(s._fetch(_capi.F_FIT_RESULT, (3, 3 + 7))[:, :3], fit.params)
    applied = _fit(s, c, iterations=8, apply=True)
    assert _same(applied, fit) and np.array_equal(s.model_params, fit.params)
    after = _solve(s)
    other = _pendulum_solver()
    other.SetModelParameters(fit.params)
    assert _same_solve(after, _solve(other)) and not _same_solve(after, before)


# ---------------------------------------------------------------- 8. refusals through the C ABI
@gpu
def test_refusals_through_the_c_abi_leave_a_working_handle():
    from drake_ddp_amd import _capi
    c = FC.case("pendulum")
    s = _solver(c)
    lib, h = s._lib, s._h
    good = _fit(s, c, iterations=3)
    data = np.zeros((3, 70, 5))
    data[:, :, :2], data[:, :, 2:3], data[:, :, 3:] = c.x, c.u, c.x_next
    send = lambda which, a, nbytes=None: lib.mi_ilqr_set(h, which, _capi.ptr(a), a.nbytes if nbytes is None else nbytes)   # noqa: E731
    assert send(_capi.F_FIT_DATA, data, data.nbytes - 8) == _capi.E_BAD_SHAPE
    nan = data.copy()
    nan[1, 69, 4] = np.nan
    assert send(_capi.F_FIT_DATA, nan) == _capi.E_BAD_ARG
    w = np.hstack([np.ones((3, 2)), np.full((3, 1), 70.0)])
    assert send(_capi.F_FIT_WEIGHTS, w, w.nbytes + 8) == _capi.E_BAD_SHAPE
    for bad in (71.0, -1.0, 1.5, np.nan):
        w2 = w.copy()
        w2[2, 2] = bad
        assert send(_capi.F_FIT_WEIGHTS, w2) == _capi.E_BAD_ARG
    w2 = w.copy()
    w2[0, 0] = -1.0
    assert send(_capi.F_FIT_WEIGHTS, w2) == _capi.E_BAD_ARG
    st = np.hstack([c.start, np.full((3, 1), 1e-3)])
    assert send(_capi.F_FIT_START, st, 8) == _capi.E_BAD_SHAPE
    st[1, 3] = 0.0
    assert send(_capi.F_FIT_START, st) == _capi.E_BAD_ARG
    bo = np.array([[0.0, 0.0, 1.0], [1.0, 1.0, 0.0]])
    assert send(_capi.F_FIT_BOUNDS, bo) == _capi.E_BAD_ARG and send(_capi.F_FIT_BOUNDS, bo, 8) == _capi.E_BAD_SHAPE
    run = np.array([3, 1e-12, 1e-6, 1e-8, 0, 3, 0, 1, 2], dtype=np.float64)
    assert send(_capi.F_FIT_RUN, run, run.nbytes - 8) == _capi.E_BAD_SHAPE
    for k, v in ((0, -1.0), (0, 0.5), (1, -1.0), (2, 0.0), (3, np.nan), (4, 2.0), (8, 3.0), (7, 0.0)):
        r2 = run.copy()
        r2[k] = v
        assert send(_capi.F_FIT_RUN, r2) == _capi.E_BAD_ARG, (k, v)
    for which in (_capi.F_FIT_RESULT, _capi.F_FIT_NORMAL, _capi.F_FIT_KERNEL_MS):
        assert send(which, run) == _capi.E_BAD_ARG                             # read-only
    out = np.empty(4)
    assert lib.mi_ilqr_get(h, _capi.F_FIT_RESULT, _capi.ptr(out), out.nbytes) == _capi.E_BAD_SHAPE
    assert lib.mi_ilqr_get(h, _capi.F_FIT_RUN, _capi.ptr(out), out.nbytes) == _capi.E_BAD_ARG
    # none of it moved anything: the command alone runs on what the last good call left, the full call gives the same bits again
    assert send(_capi.F_FIT_RUN, run) == _capi.OK
    assert np.array_equal(s._fetch(_capi.F_FIT_RESULT, (3, 10))[:, :3], good.params)
    assert _same(_fit(s, c, iterations=3), good)
    # before any data or run: refused, then a working call
    s2 = _solver(c)
    assert lib.mi_ilqr_set(s2._h, _capi.F_FIT_RUN, _capi.ptr(run), run.nbytes) == _capi.E_BAD_ARG
    assert lib.mi_ilqr_set(s2._h, _capi.F_FIT_WEIGHTS, _capi.ptr(w), w.nbytes) == _capi.E_BAD_ARG
    assert lib.mi_ilqr_get(s2._h, _capi.F_FIT_KERNEL_MS, _capi.ptr(out), 8) == _capi.E_BAD_ARG
    assert _same(_fit(s2, c, iterations=3), good)


@gpu
def test_a_model_without_parameters_is_refused():
    sys.path.insert(0, os.path.join(ROOT, "examples", "plugins"))
    import models as PM
    from drake_ddp_amd import _capi, plugin
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    system = plugin.build_model(*PM.NOISEPROBE_SPEC)(0.01)
    s = BatchedIterativeLQR(system, 4, 2, device=0, max_iters=2)
    buf = np.zeros(2 * 3 * (2 * 40 + 16))
    for which in (_capi.F_FIT_DATA, _capi.F_FIT_WEIGHTS, _capi.F_FIT_START, _capi.F_FIT_BOUNDS, _capi.F_FIT_RUN):
        assert s._lib.mi_ilqr_set(s._h, which, _capi.ptr(buf), buf.nbytes) == _capi.E_UNSUPPORTED
    for which in (_capi.F_FIT_RESULT, _capi.F_FIT_NORMAL, _capi.F_FIT_KERNEL_MS):
        assert s._lib.mi_ilqr_get(s._h, which, _capi.ptr(buf), 8) == _capi.E_UNSUPPORTED
    with pytest.raises(ValueError, match="FitModelParameters: this model has no parameters"):
        s.FitModelParameters(np.zeros((2, 3, 40)), np.zeros((2, 3, 16)), np.zeros((2, 3, 40)), free=[0])
    x0 = np.ones((2, 40))
    assert s._lib.mi_ilqr_set(s._h, _capi.F_X0, _capi.ptr(x0), x0.nbytes) == _capi.OK           # the handle works on
    assert np.array_equal(s._get(_capi.F_X0, (2, 40)), x0)


@gpu
def test_the_single_problem_class_drops_the_batch_axis():
    from drake_ddp_amd.ilqr import IterativeLinearQuadraticRegulator
    from drake_ddp_amd.models import ModelSystem
    c = FC.case("pendulum")
    s = IterativeLinearQuadraticRegulator(ModelSystem(c.model_id, c.dt), 4, device=0, verbose=False)
    r = s.FitModelParameters(c.x[1], c.u[1], c.x_next[1], free=c.free, params0=c.start[1], iterations=8, count=70)
    assert r.params.shape == (3,) and r.normal_matrix.shape == (3, 3) and np.ndim(r.cost) == 0
    assert np.max(np.abs(r.params - c.truth[1]) / np.abs(c.truth[1])) <= 1e-10
    batch = _fit(_solver(c), c, iterations=8)
    assert np.array_equal(r.params, batch.params[1]) and r.cost == batch.cost[1]
    with pytest.raises(ValueError, match=r"FitModelParameters: x must be \(T, 2\)"):
        s.FitModelParameters(c.x, c.u[1], c.x_next[1], free=c.free)


# ---------------------------------------------------------------- 9. the example
@gpu
def test_the_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "identify_pendulum.py"), "--batch", "8"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    val = {}
    for line in r.stdout.splitlines():
        if line.startswith("RESULT "):
            k, v = line.split()[1:3]
            val[k] = float(v)
    assert val["param_error_after"] < 1e-6 < val["param_error_before"], val
    assert val["realised_cost_after"] < val["realised_cost_before"], val
