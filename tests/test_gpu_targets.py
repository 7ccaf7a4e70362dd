"""Per-problem targets (include/mi_ilqr.h: MI_F_X_NOM / MI_F_TARGET_STEP) on every kernel family: the wave-per-problem kernels
(pendulum at C2's shape, acrobot MPC), the lane-per-problem THROUGHPUT kernels (acrobot, B = 8192), the mid-size workgroup kernels
(Arm27, a family-1 plugin) and the n = 33..40 kernels (Synth36, Quad3D), Limited<M> handles included.

Yardsticks: the C oracle, run once per target group (it takes one x_nom per call), with the suite's tolerances; and the shared
target itself - a batch with 4 interleaved targets is, problem by problem and BITWISE, what the shared handle of the same batch size
computes for that problem's target (the kernels build the same constants by the same loop, whichever array x_nom comes from)."""
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

G = 4                                   # distinct targets per batch, interleaved: problem b has target b % G


def _solver(p, B, system=None, **kw):
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    from drake_ddp_amd.models import ModelSystem
    sys_ = system or ModelSystem(p["model_id"], p["dt"])
    s = BatchedIterativeLQR(sys_, p["N"], B, delta=p["delta"], beta=p["beta"], gamma=p["gamma"], device=0, **kw)
    s.SetTargetState(p["x_nom"]); s.SetRunningCost(p["Q"], p["R"]); s.SetTerminalCost(p["Qf"])
    return s


def _result(s):
    return dict(x=s.x_bar.copy(), u=s.u_bar.copy(), K=s.K.copy(), L=s.cost.copy(), it=s.iterations.copy(), st=s.status.copy(),
                ls=s.ls_trials.copy())


def _solve(s, x0, ug, target):
    s.SetTargetState(target)
    s.SetInitialState(x0)
    s.SetInitialGuess(ug)
    s.Solve()
    return _result(s)


def _rows(targets, B):
    return np.ascontiguousarray(np.stack([targets[b % G] for b in range(B)]))


def _assert_rows_equal(a, b, idx, tag):
    for k in a:
        assert np.array_equal(a[k][idx], b[k][idx]), (tag, k)


# ---- the cases: problem, batch, solver options, x0, initial guess, G targets
def _pendulum():
    from drake_ddp_amd import workloads as W
    p = W.pendulum_problem()
    tg = [p["x_nom"] + np.array([d, 0.0]) for d in (0.0, -0.4, 0.4, 0.8)]
    return p, 1024, {}, W.pendulum_batch_x0(1024), np.zeros((1, p["N"] - 1)), tg


def _acrobot_tp():
    from drake_ddp_amd import workloads as W
    p = W.acrobot_problem()
    tg = [p["x_nom"] + np.array([d, 0.0, 0.0, 0.0]) for d in (0.0, -0.2, 0.2, 0.1)]
    return p, 8192, {"kernel_mode": "throughput"}, W.acrobot_batch_x0(8192), np.zeros((1, p["N"] - 1)), tg


def _arm27():
    from drake_ddp_amd import workloads as W
    p = W.arm27_problem()
    tg = []
    for dx, dy in ((0.0, 0.0), (0.05, 0.0), (0.0, -0.05), (-0.03, 0.05)):
        t = p["x_nom"].copy(); t[11] += dx; t[12] += dy
        tg.append(t)
    return p, 64, {}, W.arm27_batch_x0(64), W.arm27_u_guess(p["N"]), tg


def _synth36(B=64):
    from drake_ddp_amd import workloads as W
    p = W.synth36_problem()
    tg = []
    for v in W.SYNTH_TARGET_VEL * np.array([1.0, 0.5, 1.5, 0.0]):
        t = p["x_nom"].copy(); t[0] = v * p["N"] * p["dt"]; t[18] = v
        tg.append(t)
    return p, B, {}, W.synth36_batch_x0(B), W.synth36_u_guess(p["N"]), tg


def _quad3d():
    from drake_ddp_amd import workloads as W
    p = W.quad3d_problem()
    tg = [W.quad3d_problem(target_vel=v)["x_nom"] for v in (W.QUAD3D_TARGET_VEL, 0.0, 0.5 * W.QUAD3D_TARGET_VEL, 1.5 * W.QUAD3D_TARGET_VEL)]
    return p, 16, {}, W.quad3d_batch_x0(16), W.quad3d_u_guess(p["N"]), tg


def _plugin():
    import models as PM
    from drake_ddp_amd import plugin
    sys_ = plugin.build_model(*PM.chainx_spec(10, 7, 7))(0.02)
    n, m = sys_.n, sys_.m
    p = dict(model_id=None, dt=0.02, N=30, x_nom=np.zeros(n), Q=0.02 * np.eye(n), R=0.02 * 0.1 * np.eye(m), Qf=10.0 * np.eye(n),
             delta=1e-4, beta=0.5, gamma=0.0)
    rng = np.random.default_rng(11)
    tg = [np.zeros(n)] + [np.concatenate([rng.uniform(-0.3, 0.3, 10), np.zeros(n - 10)]) for _ in range(G - 1)]
    return p, 16, {"system": sys_}, rng.uniform(-0.2, 0.2, (16, n)), np.zeros((m, p["N"] - 1)), tg


CASES = {"pendulum": _pendulum, "acrobot_tp": _acrobot_tp, "arm27": _arm27, "synth36": _synth36, "quad3d": _quad3d,
         "plugin_f1": _plugin}


@pytest.mark.parametrize("name", list(CASES))
def test_per_problem_targets_equal_the_shared_handle_per_group(name):
    """Problem b of a batch with interleaved targets == problem b of the shared handle set to its target (same batch size),
    bitwise; all rows equal to the shared target == the shared handle; after set_cost(x_nom) the handle is a never-per-problem
    one again; targets survive Reset."""
    p, B, kw, x0, ug, tg = CASES[name]()
    pp = _solver(p, B, **kw)
    got = _solve(pp, x0, ug, _rows(tg, B))
    assert np.array_equal(pp.x_nom, _rows(tg, B))
    for g in range(G):
        sh = _solver(p, B, **kw)
        ref = _solve(sh, x0, ug, tg[g])
        _assert_rows_equal(got, ref, np.arange(g, B, G), (name, g))
        if g == 0:
            same = _solver(p, B, **kw)
            _assert_rows_equal(_solve(same, x0, ug, _rows([tg[0]] * G, B)), ref, slice(None), (name, "equal rows"))
    # back to the shared target on the handle that ran per-problem targets: bitwise the never-per-problem handle's cold solve
    pp.Reset()
    ref0 = _solve(_solver(p, B, **kw), x0, ug, tg[0])
    _assert_rows_equal(_solve(pp, x0, ug, tg[0]), ref0, slice(None), (name, "dropped"))
    # targets are problem data: set, Reset, solve cold == a fresh per-problem handle's solve
    pp.SetTargetStateResident(_rows(tg, B))
    pp.Reset()
    _assert_rows_equal(_solve(pp, x0, ug, _rows(tg, B)), got, slice(None), (name, "reset"))


def _oracle_groups(p, x0, ug, tg, B):
    from oracle import c_oracle, models_np as M
    model = M.Model(p["model_id"], p["dt"])
    out = {k: None for k in ("cost", "iters", "ls", "status", "x_bar", "u_bar", "K")}
    for g in range(G):
        idx = np.arange(g, B, G)
        r = c_oracle.solve_batch(model, dict(p, x_nom=tg[g]), x0[idx], ug)
        for k in out:
            if out[k] is None:
                out[k] = np.zeros((B,) + r[k].shape[1:], r[k].dtype)
            out[k][idx] = r[k]
    return out


@pytest.mark.parametrize("name,flips,u_tol", [("pendulum", 0, 1e-6), ("acrobot_tp", 0, 1e-4), ("arm27", 1, 1e-6), ("synth36", 1, 1e-6),
                                             ("quad3d", 1, 1e-6)])
def test_per_problem_targets_against_the_c_oracle(name, flips, u_tol):
    """Every problem against the C oracle run for its target group: statuses equal; iterations and trials equal (up to `flips`
    problems on the workgroup families, whose central differences round differently - tests/test_gpu_arm27.py).  Where they are
    equal: costs to 5e-8 relative and trajectories to 1e-6 of their largest entry (test_c2_full_batch_properties), or - targets away from the
    scripts' own make some optima flat - to 10 x what the oracle itself moves when x0 moves by one ulp (tests/test_gpu_arm27.py).
    The acrobot's controls: 1e-4 of their largest entry - its optimum is flat, x moves at FD-noise level and u = u_bar - K dx
    with K checked to 100 x x's tolerance (test_throughput_mode_matches_latency_mode_and_oracle)."""
    p, B, kw, x0, ug, tg = CASES[name]()
    s = _solver(p, B, **kw)
    got = _solve(s, x0, ug, _rows(tg, B))
    r = _oracle_groups(p, x0, ug, tg, B)
    assert np.array_equal(got["st"], r["status"]) and (got["st"] == 0).mean() >= 0.9
    same = (got["it"] == r["iters"]) & (got["ls"] == r["ls"])
    assert int((~same).sum()) <= flips, (name, np.flatnonzero(~same))
    xq = x0.copy()
    xq[:, 0] = np.nextafter(xq[:, 0], np.inf)
    rq = _oracle_groups(p, xq, ug, tg, B)
    keep = same & (rq["iters"] == r["iters"]) & (rq["ls"] == r["ls"])
    assert keep.sum() >= B - 2 * flips - 2, (name, int(keep.sum()))
    own_L = np.abs(rq["cost"] - r["cost"]) / np.abs(r["cost"])
    e_L = np.abs(got["L"] - r["cost"]) / np.abs(r["cost"])
    assert np.all(e_L[keep] < np.maximum(5e-8, 10 * own_L[keep])), (name, e_L[keep].max(), own_L[keep].max())
    for k, ko, rtol in (("x", "x_bar", 1e-6), ("u", "u_bar", u_tol)):
        own = np.abs(rq[ko] - r[ko]).reshape(B, -1).max(axis=1)
        e = np.abs(got[k] - r[ko]).reshape(B, -1).max(axis=1)
        tol = rtol * max(1.0, np.abs(r[ko]).max())          # (relative to the batch's largest entry, like tests/common.py: rel_err)
        assert np.all(e[keep] < np.maximum(tol, 10 * own[keep])), (name, k, e[keep].max(), own[keep].max(), tol)


def test_permuting_problems_and_targets_permutes_the_results():
    """Synth36 at B = 16: clusters of helper workgroups engage (each helper loads the row of the problem it serves)."""
    p, B, kw, x0, ug, tg = _synth36(16)
    rows = _rows(tg, B)
    a = _solve(_solver(p, B, **kw), x0, ug, rows)
    perm = np.random.default_rng(3).permutation(B)
    s = _solver(p, B, **kw)
    b = _solve(s, x0[perm], ug, rows[perm])
    for k in a:
        assert np.array_equal(b[k], a[k][perm]), k


def _mpc(s, x0, ug, target, R, replan, step):
    s.SetTargetState(target); s.SetInitialState(x0); s.SetInitialGuess(ug)
    s.Solve()
    s.MPCRun(R, replan, target_step=step)
    return dict(log=s.mpc_log.copy(), x=s.x_bar.copy(), u=s.u_bar.copy(), st=s.status.copy(), x_nom=np.array(s.x_nom, copy=True))


def _repeated(x_nom, step, R):
    out = np.array(x_nom, dtype=np.float64, copy=True)
    for _ in range(R):
        out = out + step
    return out


@pytest.mark.parametrize("name,N", [("acrobot", 40), ("acrobot_hostloop", 520), ("synth36", 40)])
def test_mpc_per_problem_steps_equal_the_shared_step_per_group(name, N):
    """MPCRun with (B, n) steps: problem b's log and final state == the shared-step run's for its group, bitwise, in the
    single-launch form (acrobot N = 40, Synth36) and the host-loop form (acrobot N = 520, beyond the in-kernel shift); MI_F_X_NOM
    afterwards is x_nom_b + step_b added R times."""
    from drake_ddp_amd import workloads as W
    if name.startswith("acrobot"):
        p = W.acrobot_problem(N)
        B, x0, ug = 64, W.acrobot_batch_x0(64), np.zeros((1, N - 1))
        tg = [p["x_nom"] + np.array([d, 0.0, 0.0, 0.0]) for d in (0.0, -0.2, 0.2, 0.1)]
        st = [np.array([a, 0.0, 0.0, 0.0]) for a in (0.0, 0.01, -0.01, 0.02)]
    else:
        p, B, _, x0, ug, tg = _synth36(64)
        st = []
        for v in W.SYNTH_TARGET_VEL * np.array([1.0, 0.5, 1.5, 0.25]):   # (all moving: the shared runs then keep the same kernel path)
            d = np.zeros(36); d[0] = v * p["dt"] * 4
            st.append(d)
    R, replan = 6, 4
    got = _mpc(_solver(p, B), x0, ug, _rows(tg, B), R, replan, _rows(st, B))
    assert np.array_equal(got["x_nom"], _repeated(_rows(tg, B), _rows(st, B), R))
    for g in range(G):
        ref = _mpc(_solver(p, B), x0, ug, tg[g], R, replan, st[g])
        idx = np.arange(g, B, G)
        for k in ("log", "x", "u", "st"):
            assert np.array_equal(got[k][idx], ref[k][idx]), (name, g, k)


def test_mpc_single_launch_equals_shift_and_solve_launches():
    """The single-launch loop with per-problem steps == the loop written out with the C entries (mpc_shift, set MI_F_X_NOM, solve),
    bitwise, and MI_F_X_NOM agrees."""
    from drake_ddp_amd import _capi
    from drake_ddp_amd import workloads as W
    p = W.acrobot_problem()
    B, R, replan = 64, 5, 4
    x0, ug = W.acrobot_batch_x0(B), np.zeros((1, p["N"] - 1))
    tg = _rows([p["x_nom"] + np.array([d, 0.0, 0.0, 0.0]) for d in (0.0, -0.2, 0.2, 0.1)], B)
    st = _rows([np.array([a, 0.0, 0.0, 0.0]) for a in (0.0, 0.01, -0.01, 0.02)], B)
    a = _mpc(_solver(p, B), x0, ug, tg, R, replan, st)
    s = _solver(p, B)
    s.SetTargetState(tg); s.SetInitialState(x0); s.SetInitialGuess(ug)
    s.Solve()
    lib, h = s._lib, s._h
    xn = tg.copy()
    costs = []
    for _ in range(R):
        _capi.check(lib.mi_ilqr_mpc_shift(h, replan), "mi_ilqr_mpc_shift")
        xn = xn + st
        _capi.check(lib.mi_ilqr_set(h, _capi.F_X_NOM, _capi.ptr(xn), xn.nbytes), "mi_ilqr_set")
        _capi.check(lib.mi_ilqr_solve(h, None), "mi_ilqr_solve")
        costs.append(s.cost.copy())
    assert np.array_equal(a["log"][:, :, -2], np.stack(costs, axis=1))
    assert np.array_equal(a["x"], s.x_bar) and np.array_equal(a["u"], s.u_bar)
    assert np.array_equal(a["x_nom"], xn)


@pytest.mark.parametrize("name", ["pendulum", "arm27"])
def test_limited_handles_with_per_problem_targets(name):
    """Limited<M> kernels (per-problem bounds too): per-problem targets == the limited shared handle per group, bitwise."""
    p, B, kw, x0, ug, tg = CASES[name]()
    if name == "pendulum":
        B, x0 = 256, x0[:256]
        lo = -np.linspace(1.0, 3.0, B)[:, None]
    else:
        B, x0 = 16, x0[:16]
        lo = -np.tile(np.array([1.0, 12.0, 4.0, 6.0, 2.0, 2.0, 2.0]) * 2.0, (B, 1))
    lim = dict(kw, control_limits="enforce")

    def run(target):
        s = _solver(p, B, **lim)
        s.SetControlLimits(lo, -lo)
        return _solve(s, x0, ug, target)
    got = run(_rows(tg, B))
    for g in range(G):
        _assert_rows_equal(got, run(tg[g]), np.arange(g, B, G), (name, g))


def test_stage_entries_with_per_problem_targets():
    """rollout and backward stage entries with per-problem targets against OracleILQR's stages, one problem per target."""
    from oracle import models_np as M
    from oracle.ilqr_np import OracleILQR
    from drake_ddp_amd import workloads as W
    p = W.acrobot_problem()
    B = 8
    x0 = W.acrobot_batch_x0(B)
    tg = _rows([p["x_nom"] + np.array([d, 0.0, 0.0, 0.0]) for d in (0.0, -0.2, 0.2, 0.1)], B)
    rng = np.random.default_rng(5)
    u0 = rng.uniform(-0.5, 0.5, (B, 1, p["N"] - 1))
    s = _solver(p, B, kernel_mode="latency")
    s.SetTargetState(tg); s.SetInitialState(x0); s.SetInitialGuess(u0)
    xt, ut, Lt, _ = s.stage_rollout(1.0)
    s.set_state(x_bar=xt, u_bar=ut)
    s.stage_linearize()
    s.stage_backward()
    K, kap = s.K, s.kappa
    for b in range(B):
        o = OracleILQR(M.Model(p["model_id"], p["dt"]), p["N"], p["delta"], p["beta"], p["gamma"], jacobian="fd", fd_step=1e-5)
        o.set_problem(x0[b], tg[b], p["Q"], p["R"], p["Qf"], u0[b])
        xo, uo, Lo, _ = o.rollout(1.0)
        assert abs(Lt[b] - Lo) <= 1e-12 * abs(Lo) and np.max(np.abs(xt[b] - xo)) <= 1e-12, b
        o.x_bar, o.u_bar = xo, uo
        o.linearize(xo, uo)
        o.backward()
        sc = max(1.0, np.abs(o.K).max())
        assert np.max(np.abs(K[b] - o.K)) <= 1e-6 * sc, b
        assert np.max(np.abs(kap[b] - o.kappa)) <= 1e-6 * max(1.0, np.abs(o.kappa).max()), b


def test_refusals_leave_the_handle_usable():
    from drake_ddp_amd import _capi
    from drake_ddp_amd import workloads as W
    p = W.acrobot_problem()
    B = 8
    s = _solver(p, B)
    x0 = W.acrobot_batch_x0(B)
    s.SetInitialState(x0); s.SetInitialGuess(np.zeros((1, p["N"] - 1)))
    lib, h = s._lib, s._h
    good = np.tile(p["x_nom"], (B, 1))
    short = np.zeros((B - 1, 4))
    assert lib.mi_ilqr_set(h, _capi.F_X_NOM, _capi.ptr(short), short.nbytes) == _capi.E_BAD_SHAPE
    assert lib.mi_ilqr_set(h, _capi.F_TARGET_STEP, _capi.ptr(short), short.nbytes) == _capi.E_BAD_SHAPE
    out = np.empty((B, 3))
    assert lib.mi_ilqr_get(h, _capi.F_X_NOM, _capi.ptr(out), out.nbytes) == _capi.E_BAD_SHAPE
    bad = good.copy(); bad[3, 1] = np.nan
    assert lib.mi_ilqr_set(h, _capi.F_X_NOM, _capi.ptr(bad), bad.nbytes) == _capi.E_BAD_ARG
    ptr, nb = C.c_void_p(), C.c_size_t()
    assert lib.mi_ilqr_device_ptr(h, _capi.F_X_NOM, C.byref(ptr), C.byref(nb)) == _capi.E_BAD_ARG   # shared mode: no (B, n) copy
    x, u, _, L = s.Solve()                                                  # still the shared handle
    ref = _result(s)
    s.SetTargetState(good)
    s.Reset()
    s.Solve()
    _assert_rows_equal(_result(s), ref, slice(None), "equal rows after refusals")
    assert lib.mi_ilqr_device_ptr(h, _capi.F_X_NOM, C.byref(ptr), C.byref(nb)) == _capi.OK and nb.value == good.nbytes
    step = np.zeros(4)
    assert lib.mi_ilqr_mpc_run(h, 2, 4, _capi.ptr(step), None) == _capi.E_BAD_ARG
    assert lib.mi_ilqr_set(h, _capi.F_TARGET_STEP, _capi.ptr(bad), bad.nbytes) == _capi.E_BAD_ARG
    steps = np.zeros((B, 4))
    assert lib.mi_ilqr_get(h, _capi.F_TARGET_STEP, _capi.ptr(steps), steps.nbytes) == _capi.OK and not steps.any()
    s.MPCRun(2, 4, target_step=np.full((B, 4), 0.01))
    assert np.array_equal(s.x_nom, _repeated(good, np.full((B, 4), 0.01), 2))


_SWITCH_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[2]); sys.path.insert(0, sys.argv[2] + "/tests")
import test_gpu_targets as T
p, B, kw, x0, ug, tg = T._synth36(16)
s = T._solver(p, B, **kw)
r = T._solve(s, x0, ug, T._rows(tg, B))
step = np.zeros((B, 36)); step[:, 0] = np.linspace(0.0, 0.004, B)
s.MPCRun(4, 4, target_step=step)
np.savez(sys.argv[1], L=r["L"], it=r["it"], u=r["u"], st=r["st"], log=s.mpc_log, mst=s.status)
"""


def test_kernel_switches_agree_with_the_default_run(tmp_path):
    """Synth36, B = 16, per-problem targets and steps: MI_ILQR_CLUSTER=2, MI_ILQR_SPEC=2, MI_ILQR_EARLY=0 and MI_ILQR_LS_GROUPS=0
    give the default run's solve and MPC log.  One child process at a time."""
    runs = {}
    for tag, env_ in (("default", {}), ("cluster2", {"MI_ILQR_CLUSTER": "2"}), ("spec2", {"MI_ILQR_SPEC": "2"}),
                      ("early0", {"MI_ILQR_EARLY": "0"}), ("groups0", {"MI_ILQR_LS_GROUPS": "0"})):
        f = str(tmp_path / (tag + ".npz"))
        env = dict(os.environ, **env_)
        r = subprocess.run([sys.executable, "-c", _SWITCH_SCRIPT, f, ROOT], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, (tag, r.returncode, r.stderr[-2000:])
        runs[tag] = np.load(f)
    ref = runs["default"]
    assert np.all(ref["st"] == 0) and np.all(ref["mst"] == 0)
    for tag, v in runs.items():
        assert np.array_equal(v["it"], ref["it"]), tag
        assert np.max(np.abs(v["L"] - ref["L"]) / np.abs(ref["L"])) <= 1e-12, tag
        assert np.max(np.abs(v["u"] - ref["u"])) <= 1e-9 * max(1.0, np.abs(ref["u"]).max()), tag
        assert np.array_equal(v["log"][:, :, -1], ref["log"][:, :, -1]), tag
        assert np.max(np.abs(v["log"][:, :, -2] - ref["log"][:, :, -2]) / np.abs(ref["log"][:, :, -2])) <= 1e-12, tag


def test_the_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "mpc_many_legs_speeds.py")], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "target speeds" in r.stdout and "seed  0:" in r.stdout
