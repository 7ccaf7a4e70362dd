"""Per-problem cost matrices (include/mi_ilqr.h: MI_F_COST_MATRICES; SetRunningCost / SetTerminalCost with (B, ..) arguments) on
every kernel family: the wave-per-problem kernels (pendulum, a family-0 plugin; the acrobot with helper wavefronts in the MPC and
stage tests), the lane-per-problem THROUGHPUT kernels (acrobot), the mid-size workgroup kernels (Arm27, a family-1 plugin) and the
n = 33..40 kernels (Synth36 - clustered - and Quad3D), Limited<M> handles included.

Yardsticks: the shared handle itself - a batch with G = 4 interleaved weight sets is, problem by problem and BITWISE, what a shared
handle of the same batch size set to that weight set computes for the problem (one loop builds the constants whichever array the
matrices came from) - and the C oracle, run once per weight set, with the assertions and tolerances of tests/test_gpu_targets.py.

The weight sets are scalings of each workload's own matrices, R x {1, 0.5, 2, 4} and Qf x {1, 2, 0.5, 1}: all symmetric positive
semi-definite, one cost class.  On the CPU the C oracle converged (status 0) on every problem of every set at the sizes used here,
and its iteration and trial counts did not move when x0[:, 0] moved by one ulp.

Sizes: the smallest that still take every path - B = 100 and B = 68 are no multiples of 64 (68: two blocks of the lane kernel, the
second with one live lane per weight set and 60 shadow lanes on problem B - 1; that kernel accepts any B); Synth36 at B = 4 runs
clustered (helper workgroups must serve their problem's row); horizons of 12 .. 50 steps."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "plugins"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

G = 4                                   # distinct weight sets per batch, interleaved: problem b has set b % G
R_FACTORS = (1.0, 0.5, 2.0, 4.0)
QF_FACTORS = (1.0, 2.0, 0.5, 1.0)


def _weights(p):
    """The G weight sets (Q, R, Qf) of a case; set 0 is the workload's own."""
    Q, R, Qf = (np.array(p[k], dtype=np.float64) for k in ("Q", "R", "Qf"))
    return [(Q, R * rf, Qf * qf) for rf, qf in zip(R_FACTORS, QF_FACTORS)]


def _stacked(ws, B):
    """(B, n, n), (B, m, m), (B, n, n): problem b's matrices are set b % G's."""
    return tuple(np.ascontiguousarray(np.stack([ws[b % G][k] for b in range(B)])) for k in range(3))


def _solver(p, B, system=None, limits=None, params=None, **kw):
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    from drake_ddp_amd.models import ModelSystem
    sys_ = system(p["dt"], params) if system is not None else ModelSystem(p["model_id"], p["dt"], params)
    if limits is not None:
        kw = dict(kw, control_limits="enforce")
    s = BatchedIterativeLQR(sys_, p["N"], B, delta=p["delta"], beta=p["beta"], gamma=p["gamma"], device=0, **kw)
    s.SetTargetState(p["x_nom"]); s.SetRunningCost(p["Q"], p["R"]); s.SetTerminalCost(p["Qf"])
    if limits is not None:
        s.SetControlLimits(-limits, limits)
    return s


def _set_weights(s, w):
    s.SetRunningCost(w[0], w[1]); s.SetTerminalCost(w[2])


def _result(s):
    return dict(x=s.x_bar.copy(), u=s.u_bar.copy(), K=s.K.copy(), L=s.cost.copy(), it=s.iterations.copy(), st=s.status.copy(),
                ls=s.ls_trials.copy())


def _solve(s, x0, ug):
    s.SetInitialState(x0)
    s.SetInitialGuess(ug)
    s.Solve()
    return _result(s)


def _assert_rows_equal(a, b, idx, tag):
    for k in a:
        assert np.array_equal(a[k][idx], b[k][idx]), (tag, k)


# ---- the cases: problem, batch, solver options, x0, initial guess
def _pendulum(B=100, N=50, **kw):
    from drake_ddp_amd import workloads as W
    p = dict(W.pendulum_problem(), N=N)
    return p, B, kw, W.pendulum_batch_x0(1024)[:B], np.zeros((1, N - 1))


def _pendulum_lim():
    return _pendulum(limits=np.array([1.0]))


def _acrobot_tp(B=68):
    from drake_ddp_amd import workloads as W
    p = W.acrobot_problem()
    return p, B, {"kernel_mode": "throughput"}, W.acrobot_batch_x0(B), np.zeros((1, p["N"] - 1))


def _acrobot(B=8, N=40):
    from drake_ddp_amd import workloads as W
    p = W.acrobot_problem(N)
    return p, B, {}, W.acrobot_batch_x0(B), np.zeros((1, N - 1))


def _arm27(B=4, N=20, **kw):
    from drake_ddp_amd import workloads as W
    p = W.arm27_problem(N)
    return p, B, kw, W.arm27_batch_x0(64)[:B], W.arm27_u_guess(N)


def _arm27_lim():
    return _arm27(limits=np.array([1.0, 12.0, 4.0, 6.0, 2.0, 2.0, 2.0]) * 2.0)     # (tests/test_gpu_control_limits_mid.py's bounds)


def _synth36(B=4, N=20):
    from drake_ddp_amd import workloads as W
    p = W.synth36_problem(N)
    return p, B, {}, W.synth36_batch_x0(B), W.synth36_u_guess(N)


def _quad3d(B=2, N=12):
    from drake_ddp_amd import workloads as W
    p = W.quad3d_problem(N)
    return p, B, {}, W.quad3d_batch_x0(B), W.quad3d_u_guess(N)


def _plugin_f1():
    import models as PM
    from drake_ddp_amd import plugin
    make = plugin.build_model(*PM.chainx_spec(10, 7, 7))
    sys_ = make(0.02)
    n, m = sys_.n, sys_.m
    p = dict(model_id=None, dt=0.02, N=30, x_nom=np.zeros(n), Q=0.02 * np.eye(n), R=0.02 * 0.1 * np.eye(m), Qf=10.0 * np.eye(n),
             delta=1e-4, beta=0.5, gamma=0.0)
    rng = np.random.default_rng(11)
    return p, 4, {"system": make}, rng.uniform(-0.2, 0.2, (4, n)), np.zeros((m, p["N"] - 1))


def _plugin_f0():
    """A family-0 plugin (wave-per-problem kernels): a damped pendulum with its own parameter layout."""
    from drake_ddp_amd import plugin
    from drake_ddp_amd import workloads as W
    body = """
    const T acc = (p[3] * u[0] - p[1] * x[1] - p[2] * mi_sin(x[0])) / p[0];
    const T w = x[1] + dt * acc;
    xn[0] = x[0] + dt * w;
    xn[1] = w;
"""
    make = plugin.build_model("pp_pendulum4", 2, 1, body, [0.25, 0.1, 4.905, 1.0], "small")
    q = W.pendulum_problem()
    p = dict(model_id=None, dt=q["dt"], N=50, x_nom=q["x_nom"], Q=q["Q"], R=q["R"], Qf=q["Qf"], delta=q["delta"], beta=q["beta"],
             gamma=q["gamma"])
    return p, 8, {"system": make}, W.pendulum_batch_x0(1024)[:8], np.zeros((1, p["N"] - 1))


CASES = {"pendulum": _pendulum, "acrobot_tp": _acrobot_tp, "arm27": _arm27, "synth36": _synth36, "quad3d": _quad3d,
         "plugin_f1": _plugin_f1, "plugin_f0": _plugin_f0, "pendulum_lim": _pendulum_lim, "arm27_lim": _arm27_lim}

_SHARED = {}


def _shared_refs(name):
    """The shared handle's solve of the case for each weight set, computed once per case and left unchanged."""
    if name not in _SHARED:
        p, B, kw, x0, ug = CASES[name]()
        refs = []
        for w in _weights(p)[:min(G, B)]:
            s = _solver(p, B, **kw)
            _set_weights(s, w)
            refs.append(_solve(s, x0, ug))
        _SHARED[name] = refs
    return _SHARED[name]


# ---- 1. bitwise per group, on every family
@pytest.mark.parametrize("name", list(CASES))
def test_per_problem_weights_equal_the_shared_handle_per_group(name):
    """Problem b of the interleaved batch == problem b of a shared handle (same batch size) set to its weight set, bitwise; all
    rows equal to the shared matrices == the shared handle; the weights survive Reset; back to 2-D matrices after Reset the used
    handle gives a fresh shared handle's cold solve."""
    p, B, kw, x0, ug = CASES[name]()
    ws = _weights(p)
    Qs, Rs, Qfs = _stacked(ws, B)
    refs = _shared_refs(name)
    pp = _solver(p, B, **kw)
    pp.SetRunningCost(Qs, Rs); pp.SetTerminalCost(Qfs)
    got = _solve(pp, x0, ug)
    for g, ref in enumerate(refs):
        _assert_rows_equal(got, ref, np.arange(g, B, G), (name, g))
    if name in ("pendulum", "acrobot_tp", "arm27", "synth36", "quad3d"):     # (the cases the C oracle converged on, every problem)
        assert np.all(got["st"] == 0), name
    same = _solver(p, B, **kw)
    same.SetRunningCost(np.tile(ws[0][0], (B, 1, 1)), np.tile(ws[0][1], (B, 1, 1))); same.SetTerminalCost(np.tile(ws[0][2], (B, 1, 1)))
    _assert_rows_equal(_solve(same, x0, ug), refs[0], slice(None), (name, "equal rows"))
    # weights are problem data: Reset, solve cold == the first solve
    pp.Reset()
    for a, b in zip(pp.cost_matrices, (Qs, Rs, Qfs)):
        assert np.array_equal(a, b)
    _assert_rows_equal(_solve(pp, x0, ug), got, slice(None), (name, "reset"))
    # back to shared matrices on the handle that ran per-problem ones
    _set_weights(pp, ws[0])
    pp.Reset()
    _assert_rows_equal(_solve(pp, x0, ug), refs[0], slice(None), (name, "dropped"))


# ---- 2. against the C oracle per group
def _oracle_rows(p, x0, ug, rows):
    """The C oracle, one call per distinct (Q, R, Qf) of `rows` = (Qs, Rs, Qfs)."""
    from oracle import c_oracle, models_np as M
    B = len(x0)
    model = M.Model(p["model_id"], p["dt"])
    out = {k: None for k in ("cost", "iters", "ls", "status", "x_bar", "u_bar", "K")}
    keys = [tuple(a[b].tobytes() for a in rows) for b in range(B)]
    for key in dict.fromkeys(keys):
        idx = np.array([b for b in range(B) if keys[b] == key])
        b0 = idx[0]
        r = c_oracle.solve_batch(model, dict(p, Q=rows[0][b0], R=rows[1][b0], Qf=rows[2][b0]), x0[idx], ug)
        for k in out:
            if out[k] is None:
                out[k] = np.zeros((B,) + r[k].shape[1:], r[k].dtype)
            out[k][idx] = r[k]
    return out


def _assert_matches_the_oracle(name, p, x0, ug, rows, got, flips, u_tol):
    """tests/test_gpu_targets.py::test_per_problem_targets_against_the_c_oracle's assertions: statuses equal; iterations and
    trials equal up to `flips` problems; where they are equal (and the oracle's own counts do not move with one ulp of x0), costs
    to 5e-8 relative and trajectories to 1e-6 of their largest entry, or 10 x what the oracle itself moves with one ulp of x0."""
    B = len(x0)
    r = _oracle_rows(p, x0, ug, rows)
    assert np.array_equal(got["st"], r["status"]) and (got["st"] == 0).mean() >= 0.9
    same = (got["it"] == r["iters"]) & (got["ls"] == r["ls"])
    print(name, "count flips", int((~same).sum()), "iterations", got["it"].tolist()[:8])
    assert int((~same).sum()) <= flips, (name, np.flatnonzero(~same))
    xq = x0.copy()
    xq[:, 0] = np.nextafter(xq[:, 0], np.inf)
    rq = _oracle_rows(p, xq, ug, rows)
    keep = same & (rq["iters"] == r["iters"]) & (rq["ls"] == r["ls"])
    assert keep.sum() >= B - 2 * flips - 2, (name, int(keep.sum()))
    # (on the CPU the oracle's counts did not move with that ulp at any size used here, so a flip is all that may leave the
    #  comparison: the selection below is never empty, even at B = 4)
    assert keep.sum() >= B - max(flips, 1), (name, int(keep.sum()))
    own_L = np.abs(rq["cost"] - r["cost"]) / np.abs(r["cost"])
    e_L = np.abs(got["L"] - r["cost"]) / np.abs(r["cost"])
    print(name, "cost error", e_L[keep].max(), "oracle's own", own_L[keep].max())
    assert np.all(e_L[keep] < np.maximum(5e-8, 10 * own_L[keep])), (name, e_L[keep].max(), own_L[keep].max())
    for k, ko, rtol in (("x", "x_bar", 1e-6), ("u", "u_bar", u_tol)):
        own = np.abs(rq[ko] - r[ko]).reshape(B, -1).max(axis=1)
        e = np.abs(got[k] - r[ko]).reshape(B, -1).max(axis=1)
        tol = rtol * max(1.0, np.abs(r[ko]).max())
        print(name, k, "error", e[keep].max(), "oracle's own", own[keep].max(), "tolerance", tol)
        assert np.all(e[keep] < np.maximum(tol, 10 * own[keep])), (name, k, e[keep].max(), own[keep].max(), tol)


@pytest.mark.parametrize("name,flips,u_tol", [("pendulum", 0, 1e-6), ("synth36", 1, 1e-6)])
def test_per_problem_weights_against_the_c_oracle(name, flips, u_tol):
    """Every problem against the C oracle run with its weight set (budgets: the targets tests' for the same model).  Not
    self-referential: it fails if a kernel picks the wrong row consistently."""
    p, B, kw, x0, ug = CASES[name]()
    rows = _stacked(_weights(p), B)
    s = _solver(p, B, **kw)
    s.SetRunningCost(rows[0], rows[1]); s.SetTerminalCost(rows[2])
    got = _solve(s, x0, ug)
    _assert_matches_the_oracle(name, p, x0, ug, rows, got, flips, u_tol)
    if name == "pendulum":                      # what makes the bitwise test sharp: the sets differ in what they converge to
        assert len({float(got["L"][g]) for g in range(G)}) == G


# ---- 3. MPC
def _mpc(s, x0, ug, R, replan, step=None):
    s.SetInitialState(x0); s.SetInitialGuess(ug)
    s.Solve()
    s.MPCRun(R, replan, target_step=step)
    return dict(log=s.mpc_log.copy(), x=s.x_bar.copy(), u=s.u_bar.copy(), st=s.status.copy())


@pytest.mark.parametrize("name,R,replan", [("acrobot", 3, 2), ("synth36", 2, 2)])
def test_mpc_with_per_problem_weights_equals_the_shared_handle_per_group(name, R, replan):
    """MPCRun in one launch (acrobot B = 8: wave-per-problem kernels with helper wavefronts; Synth36 B = 4: clustered workgroups):
    problem b's log, final trajectory and status == the shared handle's for its weight set, bitwise."""
    p, B, kw, x0, ug = _acrobot() if name == "acrobot" else _synth36()
    ws = _weights(p)
    rows = _stacked(ws, B)
    s = _solver(p, B, **kw)
    s.SetRunningCost(rows[0], rows[1]); s.SetTerminalCost(rows[2])
    got = _mpc(s, x0, ug, R, replan)
    for g in range(G):
        r = _solver(p, B, **kw)
        _set_weights(r, ws[g])
        ref = _mpc(r, x0, ug, R, replan)
        idx = np.arange(g, B, G)
        for k in ("log", "x", "u", "st"):
            assert np.array_equal(got[k][idx], ref[k][idx]), (name, g, k)


def test_mpc_with_per_problem_weights_targets_and_steps():
    """Per-problem weights together with per-problem targets and a per-problem target_step (acrobot, B = 8): problem b == the shared
    handle set to b's weights, b's target and b's step."""
    p, B, kw, x0, ug = _acrobot()
    ws = _weights(p)
    rows = _stacked(ws, B)
    tg = [p["x_nom"] + np.array([d, 0.0, 0.0, 0.0]) for d in (0.0, -0.2, 0.2, 0.1)]
    st = [np.array([a, 0.0, 0.0, 0.0]) for a in (0.0, 0.01, -0.01, 0.02)]
    # weights cycle with period 4, targets and steps with period 4 shifted by b // 4: B = 8 sees eight of the sixteen pairs
    tsel = [(b + b // G) % G for b in range(B)]
    s = _solver(p, B, **kw)
    s.SetTargetState(np.stack([tg[t] for t in tsel]))
    s.SetRunningCost(rows[0], rows[1]); s.SetTerminalCost(rows[2])
    got = _mpc(s, x0, ug, 3, 2, np.stack([st[t] for t in tsel]))
    for b in range(B):
        r = _solver(p, B, **kw)
        _set_weights(r, ws[b % G])
        r.SetTargetState(tg[tsel[b]])
        ref = _mpc(r, x0, ug, 3, 2, st[tsel[b]])
        for k in ("log", "x", "u", "st"):
            assert np.array_equal(got[k][b], ref[k][b]), (b, k)


def test_mpc_with_per_problem_weights_and_model_parameters():
    """Per-problem weights together with SetModelParameters((B, n_params)) on the pendulum: problem b == the handle created with
    b's plant and set to b's weights."""
    from oracle import models_np as M
    p, B, kw, x0, ug = _pendulum(8)
    ws = _weights(p)
    rows = _stacked(ws, B)
    d = np.array(M.DEFAULT_PARAMS[p["model_id"]], dtype=np.float64)
    pg = [d * np.array(v) for v in ((1, 1, 1), (.8, 1, .8), (1.2, 1.5, 1.2), (1.1, .5, .9))]
    psel = [(b + b // G) % G for b in range(B)]
    s = _solver(p, B, **kw)
    s.SetModelParameters(np.stack([pg[i] for i in psel]))
    s.SetRunningCost(rows[0], rows[1]); s.SetTerminalCost(rows[2])
    got = _mpc(s, x0, ug, 2, 2)
    for b in range(B):
        r = _solver(p, B, params=pg[psel[b]], **kw)
        _set_weights(r, ws[b % G])
        ref = _mpc(r, x0, ug, 2, 2)
        for k in ("log", "x", "u", "st"):
            assert np.array_equal(got[k][b], ref[k][b]), (b, k)


# ---- 4. stage entry
def test_stage_backward_with_per_problem_weights_against_the_numpy_oracle():
    """stage_backward on a handle with per-problem weights against OracleILQR.backward, problem by problem, from the device's own
    x_bar, u_bar, fx and fu: 1e-9 relative, the stage goldens' tolerance (tests/test_gpu_parity.py::test_stage_level)."""
    from oracle import models_np as M
    from oracle.ilqr_np import OracleILQR
    from common import rel_err
    p, B, kw, x0, ug = _acrobot()
    ws = _weights(p)
    rows = _stacked(ws, B)
    rng = np.random.default_rng(5)
    u0 = rng.uniform(-0.5, 0.5, (B, 1, p["N"] - 1))
    s = _solver(p, B, kernel_mode="latency")
    s.SetRunningCost(rows[0], rows[1]); s.SetTerminalCost(rows[2])
    s.SetInitialState(x0); s.SetInitialGuess(u0)
    xt, ut, _, _ = s.stage_rollout(1.0)
    xt, ut = xt.copy(), ut.copy()
    s.set_state(x_bar=xt, u_bar=ut)
    s.stage_linearize()
    fx, fu = s.fx.copy(), s.fu.copy()
    s.stage_backward()
    K, kap, dV = s.K.copy(), s.kappa.copy(), s.dV_coeff.copy()
    for b in range(B):
        o = OracleILQR(M.Model(p["model_id"], p["dt"]), p["N"], p["delta"], p["beta"], p["gamma"], jacobian="fd", fd_step=1e-5)
        o.set_problem(x0[b], p["x_nom"], rows[0][b], rows[1][b], rows[2][b], u0[b])
        o.x_bar, o.u_bar = xt[b].copy(), ut[b].copy()
        o.fx, o.fu = fx[b].copy(), fu[b].copy()
        o.backward()
        print(b, "K", rel_err(K[b], o.K), "kappa", rel_err(kap[b], o.kappa), "dV", rel_err(dV[b], o.dV))
        assert rel_err(K[b], o.K) < 1e-9 and rel_err(kap[b], o.kappa) < 1e-9 and rel_err(dV[b], o.dV) < 1e-9, b
    # (the sets' gains do differ: the comparison is not vacuous)
    assert all(not np.array_equal(K[g], K[0]) for g in range(1, G))


# ---- 5. mixed cost class
@pytest.mark.parametrize("name,flips", [("pendulum", 0), ("arm27", 1)])
def test_one_asymmetric_row_puts_the_handle_on_the_general_form(name, flips):
    """One row's Q is not symmetric - by a quarter of Q's largest entry, far above the 8 eps averaging threshold - and all others
    are: the handle runs the general form for all rows, and every problem matches the C oracle run with its own matrices (the
    targets tests' budgets for the model; not bitwise against the shared handle, whose symmetric sets run the fast forms).  A
    non-finite entry is refused and leaves the previous weights in place."""
    from drake_ddp_amd import _capi
    p, B, kw, x0, ug = _pendulum(8) if name == "pendulum" else _arm27()
    rows = [a.copy() for a in _stacked(_weights(p), B)]
    i, j = (0, 1) if name == "pendulum" else (7, 8)
    rows[0][0, i, j] += 0.25 * np.abs(rows[0][0]).max()      # (problem 0: with this row the C oracle converges on every problem)
    assert not np.array_equal(rows[0][0], rows[0][0].T)
    s = _solver(p, B, **kw)
    s.SetRunningCost(rows[0], rows[1]); s.SetTerminalCost(rows[2])
    got = _solve(s, x0, ug)
    _assert_matches_the_oracle(name, p, x0, ug, rows, got, flips, 1e-6)
    # that comparison does tell the general form from the fast ones: a form that used symmetry would solve problem 0 with the
    # symmetrised Q or with one of its triangles mirrored, and the oracle's own solutions for those lie thousands of tolerances
    # away from the one for Q as given (pendulum 0.10 against 1.9e-5 in u, Arm27 12 against 1.6e-5)
    from oracle import c_oracle, models_np as M
    Qa = rows[0][0]
    tol = 1e-6 * max(1.0, np.abs(got["u"]).max())
    for Qs in (0.5 * (Qa + Qa.T), np.triu(Qa) + np.triu(Qa, 1).T, np.tril(Qa) + np.tril(Qa, -1).T):
        o = c_oracle.solve_batch(M.Model(p["model_id"], p["dt"]), dict(p, Q=Qs, R=rows[1][0], Qf=rows[2][0]), x0[:1], ug)
        assert np.abs(o["u_bar"][0] - got["u"][0]).max() > 1000 * tol
    # refusals: Python and the C entry; the handle keeps its rows
    n, m = rows[0].shape[1], rows[1].shape[1]
    flat = np.empty((B, 2 * n * n + m * m))
    assert s._lib.mi_ilqr_get(s._h, _capi.F_COST_MATRICES, _capi.ptr(flat), flat.nbytes) == _capi.OK
    for v in (np.nan, np.inf):
        bad = flat.copy(); bad[B - 1, n * n] = v
        assert s._lib.mi_ilqr_set(s._h, _capi.F_COST_MATRICES, _capi.ptr(bad), bad.nbytes) == _capi.E_BAD_ARG
    now = np.empty_like(flat)
    assert s._lib.mi_ilqr_get(s._h, _capi.F_COST_MATRICES, _capi.ptr(now), now.nbytes) == _capi.OK and np.array_equal(now, flat)
    Rbad = rows[1].copy(); Rbad[0, 0, 0] = np.nan
    s.SetRunningCost(rows[0], Rbad)
    with pytest.raises(ValueError):
        s.Solve()
    s.SetRunningCost(rows[0], rows[1])
    s.Reset()
    _assert_rows_equal(_solve(s, x0, ug), got, slice(None), (name, "after refusals"))


# ---- 6. forced switches
_SWITCH_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[2]); sys.path.insert(0, sys.argv[2] + "/tests")
import test_gpu_cost_matrices as T
p, B, kw, x0, ug = T._synth36()
rows = T._stacked(T._weights(p), B)
s = T._solver(p, B, **kw)
s.SetRunningCost(rows[0], rows[1]); s.SetTerminalCost(rows[2])
r = T._solve(s, x0, ug)
np.savez(sys.argv[1], L=r["L"], it=r["it"], u=r["u"], st=r["st"])
"""


def test_kernel_switches_agree_with_the_default_run(tmp_path):
    """Synth36, B = 4, per-problem weights: MI_ILQR_CLUSTER=2, MI_ILQR_SPEC=2 and MI_ILQR_NO_HELPER=1 give the default run's solve -
    iterations equal, costs to 1e-12 relative (tests/test_gpu_control_limits_mid.py's switch test).  One child process at a time,
    each under its own time limit; a child that fails ends the test."""
    runs = {}
    for tag, env_ in (("default", {}), ("cluster2", {"MI_ILQR_CLUSTER": "2"}), ("spec2", {"MI_ILQR_SPEC": "2"}),
                      ("nohelper", {"MI_ILQR_NO_HELPER": "1"})):
        f = str(tmp_path / (tag + ".npz"))
        env = dict(os.environ, **env_)
        r = subprocess.run([sys.executable, "-c", _SWITCH_SCRIPT, f, ROOT], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, (tag, r.returncode, r.stderr[-2000:])
        runs[tag] = np.load(f)
    ref = runs["default"]
    assert np.all(ref["st"] == 0)
    for tag, v in runs.items():
        assert np.array_equal(v["it"], ref["it"]), tag
        assert np.max(np.abs(v["L"] - ref["L"]) / np.abs(ref["L"])) <= 1e-12, tag


# ---- 7. interface
def test_read_back_shapes_and_mixed_forms():
    from drake_ddp_amd import _capi
    p, B, kw, x0, ug = _acrobot()
    ws = _weights(p)
    Qs, Rs, Qfs = _stacked(ws, B)
    n, m = Qs.shape[1], Rs.shape[1]
    s = _solver(p, B, **kw)
    lib, h = s._lib, s._h
    flat = np.empty((B, 2 * n * n + m * m))
    shared = np.concatenate([ws[0][0].ravel(), ws[0][1].ravel(), ws[0][2].ravel()])
    ptr, nb = C.c_void_p(), C.c_size_t()
    # shared mode: broadcast copies, no device rows
    for a, w in zip(s.cost_matrices, ws[0]):
        assert a.shape == (B,) + w.shape and np.array_equal(a, np.tile(w, (B, 1, 1)))
    ref = _solve(s, x0, ug)
    assert lib.mi_ilqr_get(h, _capi.F_COST_MATRICES, _capi.ptr(flat), flat.nbytes) == _capi.OK and np.array_equal(flat, np.tile(shared, (B, 1)))
    assert lib.mi_ilqr_device_ptr(h, _capi.F_COST_MATRICES, C.byref(ptr), C.byref(nb)) == _capi.E_BAD_ARG
    # wrong shapes
    for bad in (np.zeros((B - 1, n, n)), np.zeros((B, n, n + 1)), np.zeros((n,))):
        with pytest.raises(AssertionError):
            s.SetRunningCost(bad, ws[0][1])
        with pytest.raises(AssertionError):
            s.SetTerminalCost(bad)
    with pytest.raises(AssertionError):
        s.SetRunningCost(ws[0][0], np.zeros((B, m + 1, m + 1)))
    short = np.zeros((B - 1, 2 * n * n + m * m))
    assert lib.mi_ilqr_set(h, _capi.F_COST_MATRICES, _capi.ptr(short), short.nbytes) == _capi.E_BAD_SHAPE
    assert lib.mi_ilqr_set(h, _capi.F_COST_MATRICES, _capi.ptr(flat), flat.nbytes - 8) == _capi.E_BAD_SHAPE
    assert lib.mi_ilqr_set(h, _capi.F_COST_MATRICES, None, flat.nbytes) == _capi.E_BAD_ARG
    assert lib.mi_ilqr_get(h, _capi.F_COST_MATRICES, _capi.ptr(short), short.nbytes) == _capi.E_BAD_SHAPE
    # (B, n, n) Q with 2-D R and Qf: the shared ones are repeated
    Q2 = np.stack([ws[0][0] * f for f in np.linspace(1.0, 2.0, B)])
    s.SetRunningCost(Q2, ws[0][1])
    s.Reset()
    mixed = _solve(s, x0, ug)
    got = s.cost_matrices
    assert np.array_equal(got[0], Q2) and np.array_equal(got[1], np.tile(ws[0][1], (B, 1, 1))) and np.array_equal(got[2], np.tile(ws[0][2], (B, 1, 1)))
    assert lib.mi_ilqr_get(h, _capi.F_COST_MATRICES, _capi.ptr(flat), flat.nbytes) == _capi.OK
    assert np.array_equal(flat[:, :n * n], Q2.reshape(B, -1)) and np.array_equal(flat[:, n * n:], np.tile(shared[n * n:], (B, 1)))
    assert lib.mi_ilqr_device_ptr(h, _capi.F_COST_MATRICES, C.byref(ptr), C.byref(nb)) == _capi.OK and nb.value == flat.nbytes and ptr.value
    _assert_rows_equal(mixed, ref, [0], "problem 0 has the shared Q")
    assert not np.array_equal(mixed["L"][1:], ref["L"][1:])
    # mi_ilqr_set(NULL, 0): back to whatever mi_ilqr_set_cost last set
    assert lib.mi_ilqr_set(h, _capi.F_COST_MATRICES, None, 0) == _capi.OK
    assert lib.mi_ilqr_get(h, _capi.F_COST_MATRICES, _capi.ptr(flat), flat.nbytes) == _capi.OK and np.array_equal(flat, np.tile(shared, (B, 1)))
    assert lib.mi_ilqr_device_ptr(h, _capi.F_COST_MATRICES, C.byref(ptr), C.byref(nb)) == _capi.E_BAD_ARG
    # all three 2-D again: the shared handle
    s.SetRunningCost(ws[0][0], ws[0][1])
    s.Reset()
    _assert_rows_equal(_solve(s, x0, ug), ref, slice(None), "2-D again")
