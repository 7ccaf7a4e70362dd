"""Per-problem model parameters (include/mi_ilqr.h: MI_F_MODEL_PARAMS) on every kernel family: the wave-per-problem kernels
(pendulum at C2's shape, acrobot MPC, a family-0 plugin), the lane-per-problem THROUGHPUT kernels (acrobot, B = 8192), the mid-size
workgroup kernels (Arm27, a family-1 plugin) and the n = 33..40 kernels (Synth36 - clustered - and Quad3D), Limited<M> handles
included.

Yardsticks: the shared handle itself - a batch with 4 interleaved plants is, problem by problem and BITWISE, what a handle of the
same batch size created with that plant computes for the problem (the kernels take the same values, from a row instead of the
kernel arguments) - and the C oracle, run once per parameter group (oracle.models_np.Model(model_id, dt, params)), with the
tolerances of tests/test_gpu_targets.py.

The parameter groups are scale vectors on the models' default parameters.  Pendulum, acrobot and Synth36: the issue's.  Arm27 and
Quad3D: a few percent on masses, inertias and the hand's offset; on the CPU the C oracle converged on every problem of every group
and its iteration and trial counts did not move when x0[:, 0] moved by one ulp."""
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

G = 4                                   # distinct plants per batch, interleaved: problem b has plant b % G


def _scales(n_params, *groups):
    """Scale vectors from {index: factor} dicts (ones elsewhere)."""
    out = []
    for g in groups:
        v = np.ones(n_params)
        for i, f in g.items():
            v[i] = f
        out.append(v)
    return out


def _system(p, params=None, system=None):
    """The case's system with `params` (None: its defaults)."""
    from drake_ddp_amd.models import ModelSystem
    if system is not None:                                   # a plugin's factory
        return system(p["dt"], params)
    return ModelSystem(p["model_id"], p["dt"], params)


def _solver(p, B, params=None, system=None, **kw):
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    s = BatchedIterativeLQR(_system(p, params, system), p["N"], B, delta=p["delta"], beta=p["beta"], gamma=p["gamma"], device=0, **kw)
    s.SetTargetState(p["x_nom"]); s.SetRunningCost(p["Q"], p["R"]); s.SetTerminalCost(p["Qf"])
    return s


def _result(s):
    return dict(x=s.x_bar.copy(), u=s.u_bar.copy(), K=s.K.copy(), L=s.cost.copy(), it=s.iterations.copy(), st=s.status.copy(),
                ls=s.ls_trials.copy())


def _solve(s, x0, ug):
    s.SetInitialState(x0)
    s.SetInitialGuess(ug)
    s.Solve()
    return _result(s)


def _rows(groups, B):
    return np.ascontiguousarray(np.stack([groups[b % G] for b in range(B)]))


def _assert_rows_equal(a, b, idx, tag):
    for k in a:
        assert np.array_equal(a[k][idx], b[k][idx]), (tag, k)


# ---- the cases: problem, batch, solver options, x0, initial guess, G parameter vectors (group 0: the defaults)
def _defaults(p):
    from oracle import models_np as M
    return np.array(M.DEFAULT_PARAMS[p["model_id"]], dtype=np.float64)


def _pendulum(B=1024):
    from drake_ddp_amd import workloads as W
    p = W.pendulum_problem()
    sc = [np.array(v) for v in ((1, 1, 1), (.8, 1, .8), (1.2, 1.5, 1.2), (1.1, .5, .9))]
    return p, B, {}, W.pendulum_batch_x0(1024)[:B], np.zeros((1, p["N"] - 1)), [_defaults(p) * s for s in sc]


ACROBOT_SCALES = [np.ones(10), np.array((1.1, .9, 1, 1, 1, 1.1, .9, 1, 1, 1)), np.array((.9, 1.1, 1, 1, 1, .9, 1.1, 2, 2, 1)),
                  np.array((1, 1, 1, 1, 1, 1, 1, .5, .5, 1))]


def _acrobot_tp():
    from drake_ddp_amd import workloads as W
    p = W.acrobot_problem()
    return (p, 8192, {"kernel_mode": "throughput"}, W.acrobot_batch_x0(8192), np.zeros((1, p["N"] - 1)),
            [_defaults(p) * s for s in ACROBOT_SCALES])


def _acrobot(N=40, B=64):
    from drake_ddp_amd import workloads as W
    p = W.acrobot_problem(N)
    return p, B, {}, W.acrobot_batch_x0(B), np.zeros((1, N - 1)), [_defaults(p) * s for s in ACROBOT_SCALES]


def _arm27(B=64):
    from drake_ddp_amd import workloads as W
    p = W.arm27_problem()
    # [g, k, sigma, dn, mu, b_joint, m_ball, r_ball, r_ee, m_elbow, m_hand, I_shoulder, I_elbow, I_wrist, ee_off]
    sc = _scales(15, {}, {6: 1.05, 9: 0.95}, {10: 1.05, 11: 1.03, 14: 1.02}, {6: 0.96, 9: 1.04, 10: 0.97, 12: 1.05})
    return p, B, {}, W.arm27_batch_x0(64)[:B], W.arm27_u_guess(p["N"]), [_defaults(p) * s for s in sc]


def _synth36(B=64):
    from drake_ddp_amd import workloads as W
    p = W.synth36_problem()
    sc = [np.array(v) for v in ((1, 1, 1, 1), (.8, 1, 1, 1), (1.2, 1.2, 1, 1), (1, .8, 1.2, .9))]
    return p, B, {}, W.synth36_batch_x0(B), W.synth36_u_guess(p["N"]), [_defaults(p) * s for s in sc]


def _quad3d():
    from drake_ddp_amd import workloads as W
    p = W.quad3d_problem()
    # [g, k, sigma, dn, mu, b_joint, v_max, m_trunk, Ixx, Iyy, Izz, I_abad, I_hip, I_knee]
    sc = _scales(14, {}, {7: 1.05}, {7: 0.95, 8: 1.05, 9: 1.03}, {7: 1.02, 12: 1.04, 13: 0.96})
    return p, 16, {}, W.quad3d_batch_x0(16), W.quad3d_u_guess(p["N"]), [_defaults(p) * s for s in sc]


def _plugin_f1():
    import models as PM
    from drake_ddp_amd import plugin
    make = plugin.build_model(*PM.chainx_spec(10, 7, 7))
    sys_ = make(0.02)
    n, m = sys_.n, sys_.m
    p = dict(model_id=None, dt=0.02, N=30, x_nom=np.zeros(n), Q=0.02 * np.eye(n), R=0.02 * 0.1 * np.eye(m), Qf=10.0 * np.eye(n),
             delta=1e-4, beta=0.5, gamma=0.0)
    rng = np.random.default_rng(11)
    d = np.array(sys_.params, dtype=np.float64)
    pg = [d] + [d * rng.uniform(0.8, 1.2, d.size) for _ in range(G - 1)]
    return p, 16, {"system": make}, rng.uniform(-0.2, 0.2, (16, n)), np.zeros((m, p["N"] - 1)), pg


def _plugin_f0():
    """A family-0 plugin (wave-per-problem kernels): a damped pendulum with its own parameter layout [inertia, damping, gravity
    torque, input gain]."""
    from drake_ddp_amd import plugin
    body = """
    const T acc = (p[3] * u[0] - p[1] * x[1] - p[2] * mi_sin(x[0])) / p[0];
    const T w = x[1] + dt * acc;
    xn[0] = x[0] + dt * w;
    xn[1] = w;
"""
    make = plugin.build_model("pp_pendulum4", 2, 1, body, [0.25, 0.1, 4.905, 1.0], "small")
    from drake_ddp_amd import workloads as W
    q = W.pendulum_problem()
    p = dict(model_id=None, dt=q["dt"], N=q["N"], x_nom=q["x_nom"], Q=q["Q"], R=q["R"], Qf=q["Qf"], delta=q["delta"], beta=q["beta"],
             gamma=q["gamma"])
    d = np.array([0.25, 0.1, 4.905, 1.0])
    pg = [d, d * np.array([.8, 1, .8, 1]), d * np.array([1.2, 1.5, 1.2, .9]), d * np.array([1.1, .5, .9, 1.1])]
    return p, 64, {"system": make}, W.pendulum_batch_x0(1024)[:64], np.zeros((1, p["N"] - 1)), pg


CASES = {"pendulum": _pendulum, "acrobot_tp": _acrobot_tp, "arm27": _arm27, "synth36": _synth36, "quad3d": _quad3d,
         "plugin_f1": _plugin_f1, "plugin_f0": _plugin_f0}


@pytest.mark.parametrize("name", list(CASES))
def test_per_problem_parameters_equal_the_shared_handle_per_group(name):
    """Problem b of a batch with interleaved plants == problem b of a handle CREATED with its plant (same batch size), bitwise;
    all rows equal to the defaults == the plain handle; back in shared mode the handle is a never-per-problem one again; rows
    survive Reset."""
    p, B, kw, x0, ug, pg = CASES[name]()
    rows = _rows(pg, B)
    pp = _solver(p, B, **kw)
    assert np.array_equal(pp.model_params, np.tile(pg[0], (B, 1)))          # shared mode: the descriptor's row repeated
    pp.SetModelParameters(rows)
    assert np.array_equal(pp.model_params, rows)
    got = _solve(pp, x0, ug)
    ref0 = None
    for g in range(G):
        ref = _solve(_solver(p, B, params=pg[g], **kw), x0, ug)
        _assert_rows_equal(got, ref, np.arange(g, B, G), (name, g))
        if g == 0:
            ref0 = ref
            same = _solver(p, B, **kw)
            same.SetModelParameters(pg[0])                                   # (n_params,): broadcast to rows
            _assert_rows_equal(_solve(same, x0, ug), ref, slice(None), (name, "equal rows"))
    if not name.startswith("plugin"):                                        # (the built-in cases: the oracle converged on every problem)
        assert np.all(got["st"] == 0), name
    # rows are problem data: Reset, solve cold == the first solve
    pp.Reset()
    assert np.array_equal(pp.model_params, rows)
    _assert_rows_equal(_solve(pp, x0, ug), got, slice(None), (name, "reset"))
    # back to the system's own parameters on the handle that ran per-problem ones: bitwise the plain handle's cold solve
    pp.SetModelParameters(None)
    pp.Reset()
    assert np.array_equal(pp.model_params, np.tile(pg[0], (B, 1)))
    _assert_rows_equal(_solve(pp, x0, ug), ref0, slice(None), (name, "dropped"))


def test_wrong_rows_show_in_the_pendulums_iteration_counts():
    """What makes the bitwise test sharp: the pendulum groups differ in their iteration counts, so a kernel that reads another
    problem's row cannot pass it."""
    p, B, kw, x0, ug, pg = _pendulum()
    s = _solver(p, B, **kw)
    s.SetModelParameters(_rows(pg, B))
    it = _solve(s, x0, ug)["it"]
    assert len({int(it[g::G].max()) for g in range(G)}) >= 3


def _oracle_groups(p, x0, ug, pg, B):
    from oracle import c_oracle, models_np as M
    out = {k: None for k in ("cost", "iters", "ls", "status", "x_bar", "u_bar", "K")}
    for g in range(G):
        idx = np.arange(g, B, G)
        r = c_oracle.solve_batch(M.Model(p["model_id"], p["dt"], pg[g]), p, x0[idx], ug)
        for k in out:
            if out[k] is None:
                out[k] = np.zeros((B,) + r[k].shape[1:], r[k].dtype)
            out[k][idx] = r[k]
    return out


@pytest.mark.parametrize("name,flips,u_tol", [("pendulum", 0, 1e-6), ("acrobot_tp", 0, 1e-4), ("arm27", 1, 1e-6), ("synth36", 1, 1e-6),
                                             ("quad3d", 1, 1e-6)])
def test_per_problem_parameters_against_the_c_oracle(name, flips, u_tol):
    """Every problem against the C oracle run for its parameter group - the assertions and tolerances of
    tests/test_gpu_targets.py::test_per_problem_targets_against_the_c_oracle: statuses equal; iterations and trials equal up to
    `flips` problems on the workgroup families; where they are equal (and the oracle's own counts do not move with one ulp of
    x0), costs to 5e-8 relative and trajectories to 1e-6 (acrobot controls 1e-4) of their largest entry, or 10 x what the oracle
    itself moves when x0 moves by one ulp."""
    p, B, kw, x0, ug, pg = CASES[name]()
    s = _solver(p, B, **kw)
    s.SetModelParameters(_rows(pg, B))
    got = _solve(s, x0, ug)
    r = _oracle_groups(p, x0, ug, pg, B)
    assert np.array_equal(got["st"], r["status"]) and (got["st"] == 0).mean() >= 0.9
    same = (got["it"] == r["iters"]) & (got["ls"] == r["ls"])
    print(name, "count flips", int((~same).sum()), "iterations per group", [int(got["it"][g::G].max()) for g in range(G)])
    assert int((~same).sum()) <= flips, (name, np.flatnonzero(~same))
    xq = x0.copy()
    xq[:, 0] = np.nextafter(xq[:, 0], np.inf)
    rq = _oracle_groups(p, xq, ug, pg, B)
    keep = same & (rq["iters"] == r["iters"]) & (rq["ls"] == r["ls"])
    assert keep.sum() >= B - 2 * flips - 2, (name, int(keep.sum()))
    own_L = np.abs(rq["cost"] - r["cost"]) / np.abs(r["cost"])
    e_L = np.abs(got["L"] - r["cost"]) / np.abs(r["cost"])
    print(name, "cost error", e_L[keep].max(), "oracle's own", own_L[keep].max())
    assert np.all(e_L[keep] < np.maximum(5e-8, 10 * own_L[keep])), (name, e_L[keep].max(), own_L[keep].max())
    for k, ko, rtol in (("x", "x_bar", 1e-6), ("u", "u_bar", u_tol)):
        own = np.abs(rq[ko] - r[ko]).reshape(B, -1).max(axis=1)
        e = np.abs(got[k] - r[ko]).reshape(B, -1).max(axis=1)
        tol = rtol * max(1.0, np.abs(r[ko]).max())          # (relative to the batch's largest entry, like tests/common.py: rel_err)
        print(name, k, "error", e[keep].max(), "oracle's own", own[keep].max(), "tolerance", tol)
        assert np.all(e[keep] < np.maximum(tol, 10 * own[keep])), (name, k, e[keep].max(), own[keep].max(), tol)


def test_permuting_problems_and_rows_permutes_the_results():
    """Synth36 at B = 16: clusters of helper workgroups engage (each helper takes the row of the problem it serves)."""
    p, B, kw, x0, ug, pg = _synth36(16)
    rows = _rows(pg, B)
    s = _solver(p, B, **kw)
    s.SetModelParameters(rows)
    a = _solve(s, x0, ug)
    perm = np.random.default_rng(3).permutation(B)
    s = _solver(p, B, **kw)
    s.SetModelParameters(rows[perm])
    b = _solve(s, x0[perm], ug)
    for k in a:
        assert np.array_equal(b[k], a[k][perm]), k


def _mpc(s, x0, ug, R, replan):
    s.SetInitialState(x0); s.SetInitialGuess(ug)
    s.Solve()
    s.MPCRun(R, replan)
    return dict(log=s.mpc_log.copy(), x=s.x_bar.copy(), u=s.u_bar.copy(), st=s.status.copy())


@pytest.mark.parametrize("name", ["acrobot", "synth36"])
def test_mpc_single_launch_equals_shift_and_solve_launches(name):
    """MPCRun(R, r) in one launch, per-problem parameters == the loop written out with the C entries (mpc_shift, solve), same
    rows, bitwise; and problem b's log == the log of a handle created with its plant.  Acrobot N = 40 (wave-per-problem kernels),
    Synth36 (workgroup-per-problem, clustered)."""
    from drake_ddp_amd import _capi
    p, B, kw, x0, ug, pg = _acrobot(40, 64) if name == "acrobot" else _synth36(64)
    rows = _rows(pg, B)
    R, replan = 5, 4
    s = _solver(p, B, **kw)
    s.SetModelParameters(rows)
    a = _mpc(s, x0, ug, R, replan)
    assert np.array_equal(s.model_params, rows)
    s = _solver(p, B, **kw)
    s.SetModelParameters(rows)
    s.SetInitialState(x0); s.SetInitialGuess(ug)
    s.Solve()
    lib, h = s._lib, s._h
    costs = []
    for _ in range(R):
        _capi.check(lib.mi_ilqr_mpc_shift(h, replan), "mi_ilqr_mpc_shift")
        _capi.check(lib.mi_ilqr_solve(h, None), "mi_ilqr_solve")
        costs.append(s.cost.copy())
    assert np.array_equal(a["log"][:, :, -2], np.stack(costs, axis=1))
    assert np.array_equal(a["x"], s.x_bar) and np.array_equal(a["u"], s.u_bar)
    for g in range(G):
        ref = _mpc(_solver(p, B, params=pg[g], **kw), x0, ug, R, replan)
        idx = np.arange(g, B, G)
        for k in ("log", "x", "u", "st"):
            assert np.array_equal(a[k][idx], ref[k][idx]), (name, g, k)


def test_mpc_host_loop_form_with_per_problem_parameters():
    """Acrobot N = 520, beyond the in-kernel shift: mpc_run loops on the host; problem b == the handle created with its plant."""
    p, B, kw, x0, ug, pg = _acrobot(520, 16)
    s = _solver(p, B, **kw)
    s.SetModelParameters(_rows(pg, B))
    a = _mpc(s, x0, ug, 3, 4)
    for g in range(G):
        ref = _mpc(_solver(p, B, params=pg[g], **kw), x0, ug, 3, 4)
        idx = np.arange(g, B, G)
        for k in ("log", "x", "u", "st"):
            assert np.array_equal(a[k][idx], ref[k][idx]), (g, k)


def _stages(s, x0, u0):
    s.SetInitialState(x0); s.SetInitialGuess(u0)
    xt, ut, Lt, ex = s.stage_rollout(1.0)
    out = dict(xt=xt.copy(), ut=ut.copy(), Lt=np.array(Lt, copy=True), ex=np.array(ex, copy=True))
    s.set_state(x_bar=xt, u_bar=ut)
    s.stage_linearize()
    out.update(fx=s.fx.copy(), fu=s.fu.copy())
    s.stage_backward()
    out.update(K=s.K.copy(), kap=s.kappa.copy())
    Lf, ef, tf = s.stage_forward(np.inf)
    out.update(Lf=np.array(Lf, copy=True), ef=np.array(ef, copy=True), tf=np.array(tf, copy=True), xf=s.x_bar.copy(), uf=s.u_bar.copy())
    return out


@pytest.mark.parametrize("name", ["acrobot", "arm27"])
def test_stage_entries_with_per_problem_parameters(name):
    """rollout, linearize, stage_backward and forward with per-problem rows == the shared handle's, row by row, bitwise."""
    p, B, kw, x0, ug, pg = _acrobot(40, 8) if name == "acrobot" else _arm27(8)
    kw = dict(kw, kernel_mode="latency")
    rng = np.random.default_rng(5)
    m = p["R"].shape[0]
    u0 = np.broadcast_to(ug, (B, m, p["N"] - 1)) + rng.uniform(-0.05, 0.05, (B, m, p["N"] - 1))
    s = _solver(p, B, **kw)
    s.SetModelParameters(_rows(pg, B))
    got = _stages(s, x0, u0)
    base = None
    for g in range(G):
        ref = _stages(_solver(p, B, params=pg[g], **kw), x0, u0)
        _assert_rows_equal(got, ref, np.arange(g, B, G), (name, g))
        base = base or ref
    # (the groups' rollouts do differ from the default plant's: the comparison above is not vacuous)
    assert all(not np.array_equal(got["xt"][g], base["xt"][g]) for g in range(1, G))


@pytest.mark.parametrize("name", ["pendulum", "arm27"])
def test_limited_handles_with_per_problem_parameters(name):
    """Limited<M> kernels (per-problem bounds too): per-problem parameters == the limited handle created with the plant, bitwise."""
    p, B, kw, x0, ug, pg = CASES[name]()
    if name == "pendulum":
        B, x0 = 256, x0[:256]
        lo = -np.linspace(1.0, 3.0, B)[:, None]
    else:
        B, x0 = 16, x0[:16]
        lo = -np.tile(np.array([1.0, 12.0, 4.0, 6.0, 2.0, 2.0, 2.0]) * 2.0, (B, 1))
    lim = dict(kw, control_limits="enforce")

    def run(params, rows=None):
        s = _solver(p, B, params=params, **lim)
        s.SetControlLimits(lo, -lo)
        if rows is not None:
            s.SetModelParameters(rows)
        return _solve(s, x0, ug)
    got = run(None, _rows(pg, B))
    for g in range(G):
        _assert_rows_equal(got, run(pg[g]), np.arange(g, B, G), (name, g))


def test_limited_lane_kernels_with_per_problem_parameters():
    """The Limited<M> lane-per-problem kernels (acrobot, throughput mode, B = 1024)."""
    p, _, kw, x0, ug, pg = _acrobot_tp()
    B, x0 = 1024, x0[:1024]
    lim = dict(kw, control_limits="enforce")

    def run(params, rows=None):
        s = _solver(p, B, params=params, **lim)
        s.SetControlLimits(-8.0, 8.0)
        if rows is not None:
            s.SetModelParameters(rows)
        return _solve(s, x0, ug)
    got = run(None, _rows(pg, B))
    for g in range(G):
        _assert_rows_equal(got, run(pg[g]), np.arange(g, B, G), g)


@pytest.mark.parametrize("name", ["pendulum", "acrobot_tp_small", "synth36"])
def test_per_problem_parameters_together_with_per_problem_targets(name):
    """Both on one handle: problem b == the handle created with b's plant and set to b's target."""
    if name == "pendulum":
        p, B, kw, x0, ug, pg = _pendulum(256)
        tg = [p["x_nom"] + np.array([d, 0.0]) for d in (0.0, -0.4, 0.4, 0.8)]
    elif name == "synth36":
        from drake_ddp_amd import workloads as W
        p, B, kw, x0, ug, pg = _synth36(16)
        tg = []
        for v in W.SYNTH_TARGET_VEL * np.array([1.0, 0.5, 1.5, 0.0]):
            t = p["x_nom"].copy(); t[0] = v * p["N"] * p["dt"]; t[18] = v
            tg.append(t)
    else:
        p, _, kw, x0, ug, pg = _acrobot_tp()
        B, x0 = 1024, x0[:1024]
        tg = [p["x_nom"] + np.array([d, 0.0, 0.0, 0.0]) for d in (0.0, -0.2, 0.2, 0.1)]
    # targets cycle with period 4, plants with period 4 shifted by b // 4: every (plant, target) pair occurs
    prow = np.stack([pg[(b + b // G) % G] for b in range(B)])
    s = _solver(p, B, **kw)
    s.SetTargetState(_rows(tg, B))
    s.SetModelParameters(prow)
    got = _solve(s, x0, ug)
    for gp in range(G):
        for gt in range(G):
            idx = np.array([b for b in range(B) if (b + b // G) % G == gp and b % G == gt])
            r = _solver(p, B, params=pg[gp], **kw)
            r.SetTargetState(tg[gt])
            _assert_rows_equal(got, _solve(r, x0, ug), idx, (name, gp, gt))


def test_refusals_leave_the_handle_usable():
    from drake_ddp_amd import _capi
    p, B, kw, x0, ug, pg = _acrobot(40, 8)
    s = _solver(p, B, **kw)
    lib, h = s._lib, s._h
    ref = _solve(s, x0, ug)
    s.Reset()
    good = _rows(pg, B)
    short = np.zeros((B - 1, 10))
    assert lib.mi_ilqr_set(h, _capi.F_MODEL_PARAMS, _capi.ptr(short), short.nbytes) == _capi.E_BAD_SHAPE
    assert lib.mi_ilqr_set(h, _capi.F_MODEL_PARAMS, _capi.ptr(good), good.nbytes - 8) == _capi.E_BAD_SHAPE
    assert lib.mi_ilqr_set(h, _capi.F_MODEL_PARAMS, None, good.nbytes) == _capi.E_BAD_ARG
    out = np.empty((B, 9))
    assert lib.mi_ilqr_get(h, _capi.F_MODEL_PARAMS, _capi.ptr(out), out.nbytes) == _capi.E_BAD_SHAPE
    for v in (np.nan, np.inf, -np.inf):
        bad = good.copy(); bad[3, 1] = v
        assert lib.mi_ilqr_set(h, _capi.F_MODEL_PARAMS, _capi.ptr(bad), bad.nbytes) == _capi.E_BAD_ARG
    ptr, nb = C.c_void_p(), C.c_size_t()
    assert lib.mi_ilqr_device_ptr(h, _capi.F_MODEL_PARAMS, C.byref(ptr), C.byref(nb)) == _capi.E_BAD_ARG   # shared mode: no rows
    assert np.array_equal(s.model_params, np.tile(pg[0], (B, 1)))
    _assert_rows_equal(_solve(s, x0, ug), ref, slice(None), "still the shared handle")
    # per-problem mode: a refused call keeps the rows
    s.SetModelParameters(good)
    assert lib.mi_ilqr_device_ptr(h, _capi.F_MODEL_PARAMS, C.byref(ptr), C.byref(nb)) == _capi.OK and nb.value == good.nbytes and ptr.value
    s.Reset()
    per = _solve(s, x0, ug)
    bad = good.copy(); bad[0, 0] = np.nan
    assert lib.mi_ilqr_set(h, _capi.F_MODEL_PARAMS, _capi.ptr(bad), bad.nbytes) == _capi.E_BAD_ARG
    assert lib.mi_ilqr_set(h, _capi.F_MODEL_PARAMS, _capi.ptr(short), short.nbytes) == _capi.E_BAD_SHAPE
    with pytest.raises(ValueError):
        s.SetModelParameters(bad)
    with pytest.raises(ValueError):
        s.SetModelParameters(short)
    assert np.array_equal(s.model_params, good)
    s.Reset()
    _assert_rows_equal(_solve(s, x0, ug), per, slice(None), "rows kept after refusals")
    assert not np.array_equal(per["L"], ref["L"])


def test_a_model_without_parameters_is_unsupported():
    from drake_ddp_amd import _capi, plugin
    body = """
    const T w = x[1] + dt * (u[0] - 0.1 * x[1] - 4.0 * mi_sin(x[0]));
    xn[0] = x[0] + dt * w;
    xn[1] = w;
"""
    make = plugin.build_model("pp_noparams", 2, 1, body, [], "small")
    from drake_ddp_amd import workloads as W
    q = W.pendulum_problem()
    p = dict(dt=q["dt"], N=40, x_nom=q["x_nom"], Q=q["Q"], R=q["R"], Qf=q["Qf"], delta=q["delta"], beta=q["beta"], gamma=q["gamma"])
    B = 4
    s = _solver(p, B, system=make)
    one = np.zeros((B, 1))
    assert s._lib.mi_ilqr_set(s._h, _capi.F_MODEL_PARAMS, _capi.ptr(one), 0) == _capi.E_UNSUPPORTED
    assert s._lib.mi_ilqr_set(s._h, _capi.F_MODEL_PARAMS, None, 0) == _capi.E_UNSUPPORTED
    assert s._lib.mi_ilqr_get(s._h, _capi.F_MODEL_PARAMS, _capi.ptr(one), 0) == _capi.E_UNSUPPORTED
    with pytest.raises(ValueError):
        s.SetModelParameters(np.zeros((B, 0)))
    r = _solve(s, W.pendulum_batch_x0(1024)[:B], np.zeros((1, p["N"] - 1)))
    assert np.all(np.isfinite(r["L"])) and np.all(r["it"] > 0)              # the refusals left a working handle


_SWITCH_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[2]); sys.path.insert(0, sys.argv[2] + "/tests")
import test_gpu_model_params as T
out = {}
for tag, case in (("s", T._synth36(16)), ("a", T._arm27(16)), ("p", T._acrobot(40, 64))):
    p, B, kw, x0, ug, pg = case
    s = T._solver(p, B, **kw)
    s.SetModelParameters(T._rows(pg, B))
    r = T._solve(s, x0, ug)
    s.MPCRun(3, 4)
    out.update({tag + "_L": r["L"], tag + "_it": r["it"], tag + "_u": r["u"], tag + "_st": r["st"], tag + "_log": s.mpc_log, tag + "_mst": s.status})
np.savez(sys.argv[1], **out)
"""


def test_kernel_switches_agree_with_the_default_run(tmp_path):
    """Synth36 and Arm27 at B = 16 and the acrobot at B = 64 (helper wavefronts), per-problem parameters: MI_ILQR_CLUSTER=2,
    MI_ILQR_SPEC=0, MI_ILQR_SPEC=2 and MI_ILQR_NO_HELPER=1 give the default run's solve and MPC log (the bounds of
    tests/test_gpu_targets.py: counts equal, costs to 1e-12, controls to 1e-9).  One child process at a time."""
    runs = {}
    for tag, env_ in (("default", {}), ("cluster2", {"MI_ILQR_CLUSTER": "2"}), ("spec0", {"MI_ILQR_SPEC": "0"}),
                      ("spec2", {"MI_ILQR_SPEC": "2"}), ("nohelper", {"MI_ILQR_NO_HELPER": "1"})):
        f = str(tmp_path / (tag + ".npz"))
        env = dict(os.environ, **env_)
        r = subprocess.run([sys.executable, "-c", _SWITCH_SCRIPT, f, ROOT], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, (tag, r.returncode, r.stderr[-2000:])
        runs[tag] = np.load(f)
    ref = runs["default"]
    for c in "sap":
        assert np.all(ref[c + "_st"] == 0) and np.all(ref[c + "_mst"] == 0), c
        for tag, v in runs.items():
            assert np.array_equal(v[c + "_it"], ref[c + "_it"]), (c, tag)
            assert np.max(np.abs(v[c + "_L"] - ref[c + "_L"]) / np.abs(ref[c + "_L"])) <= 1e-12, (c, tag)
            assert np.max(np.abs(v[c + "_u"] - ref[c + "_u"])) <= 1e-9 * max(1.0, np.abs(ref[c + "_u"]).max()), (c, tag)
            assert np.array_equal(v[c + "_log"][:, :, -1], ref[c + "_log"][:, :, -1]), (c, tag)
            lg, lr = v[c + "_log"][:, :, -2], ref[c + "_log"][:, :, -2]
            assert np.max(np.abs(lg - lr) / np.abs(lr)) <= 1e-12, (c, tag)


def test_the_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "mpc_randomized_pendulum.py")], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "plants" in r.stdout and "seed  0:" in r.stdout
