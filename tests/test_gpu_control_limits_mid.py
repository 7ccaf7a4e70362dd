"""Control limits on the MID-SIZE workgroup-per-problem family (n <= 32, m <= 16; ilqr_large.hpp: mid_backward_limited, the clamped
large_rollout / mid_rollout4) against the NumPy statement of the same semantics for any m (tests/limited_ilqr_mid_np.py): the arm +
ball (Arm27, Arm27C) with joint-torque limits, solve and device MPC; chainx plugins built with control_limits=True at (12, 4) with
u >= 0, (32, 16), (7, 3), (16, 1), per-problem bounds and autodiff Jacobians; the backward stage entry; equivalences (infinite
bounds, cleared limits, the kernel switches in child processes); refusals of the n > 32 kernels."""
import concurrent.futures
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "plugins"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

FLIP_BUDGET = 1                   # problems per batch whose decisions may differ from the oracle's at round-off level
ARM_TAU = np.array([1.0, 12.0, 4.0, 6.0, 2.0, 2.0, 2.0])   # |tau| <= ARM_TAU (N m): the base yaw's push torque binds


def _solver(p, B, **kw):
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    from drake_ddp_amd.models import ModelSystem
    sys_ = kw.pop("system", None) or ModelSystem(p["model_id"], p["dt"])
    s = BatchedIterativeLQR(sys_, p["N"], B, delta=p["delta"], beta=p["beta"], gamma=p["gamma"], device=0, **kw)
    s.SetTargetState(p["x_nom"]); s.SetRunningCost(p["Q"], p["R"]); s.SetTerminalCost(p["Qf"])
    return s


def _oracle(p, lo, hi, model, jac="fd"):
    from limited_ilqr_mid_np import LimitedMidOracleILQR
    return LimitedMidOracleILQR(model, p["N"], p["delta"], p["beta"], p["gamma"], jacobian="ad" if jac == "autodiff" else "fd",
                                fd_step=1e-5, u_min=lo, u_max=hi)


def _check_vs_oracle(s, p, x0, ug, lo, hi, model, idx, jac="fd"):
    """costs 1e-9 relative + 10 x the oracle's own one-ulp spread; iterations, trials and the final clamped set equal up to
    FLIP_BUDGET problems; gains and kappa where the spread is below 1e-10 relative; bounds hold bitwise."""
    from limited_ilqr_mid_np import LinesearchFailed
    L, it, ls, u, st, K, kap = s.cost, s.iterations, s.ls_trials, s.u_bar, s.status, s.K, s.kappa
    lo_b = lambda b: lo[b] if np.ndim(lo) == 2 else lo   # noqa: E731
    hi_b = lambda b: hi[b] if np.ndim(hi) == 2 else hi   # noqa: E731
    for b in range(u.shape[0]):
        assert np.all(u[b] >= np.asarray(lo_b(b))[:, None]) and np.all(u[b] <= np.asarray(hi_b(b))[:, None]), b
    flips = 0
    for b in idx:
        ugb = ug if ug.ndim == 2 else ug[b]
        o = _oracle(p, lo_b(b), hi_b(b), model, jac)
        o.set_problem(x0[b], p["x_nom"], p["Q"], p["R"], p["Qf"], ugb)
        try:
            xo, uo, Lo, hist = o.solve()
        except LinesearchFailed:
            flips += st[b] != 2
            continue
        spread = 0.0
        for d in (np.inf, -np.inf):
            o2 = _oracle(p, lo_b(b), hi_b(b), model, jac)
            o2.set_problem(np.nextafter(x0[b], d), p["x_nom"], p["Q"], p["R"], p["Qf"], ugb)
            try:
                spread = max(spread, abs(o2.solve()[2] - Lo))
            except LinesearchFailed:
                spread = np.inf
        clamped_dev = np.all(K[b] == 0.0, axis=1)
        same = (st[b] == 0 and len(hist) == it[b] and sum(h[2] for h in hist) == ls[b] and np.array_equal(clamped_dev, o.clamped))
        flips += not same
        if same:
            assert abs(L[b] - Lo) <= 1e-9 * abs(Lo) + 10.0 * spread, (b, L[b], Lo, spread)
            if spread <= 1e-10 * abs(Lo):
                sc = max(1.0, np.abs(o.K).max())
                assert np.max(np.abs(K[b] - o.K)) <= 1e-6 * sc, b
                assert np.max(np.abs(kap[b] - o.kappa)) <= 1e-6 * max(1.0, np.abs(o.kappa).max()), b
                assert np.max(np.abs(u[b] - uo)) <= 1e-6 * max(1.0, np.abs(uo).max()), b
    assert flips <= FLIP_BUDGET, flips


def _arm(model_id):
    from drake_ddp_amd import workloads as W
    from oracle import models_np as M
    if model_id == "arm27":
        p, ug = W.arm27_problem(), W.arm27_u_guess(50)
    else:
        p, ug = W.arm27c_problem(), W.arm27c_u_guess(50)
    return p, ug, M.Model(p["model_id"], p["dt"])


@pytest.mark.parametrize("arm", ["arm27", "arm27c"])
def test_arm_torque_limits_match_the_oracle(arm):
    from drake_ddp_amd import workloads as W
    p, ug, model = _arm(arm)
    B = 2
    x0 = W.arm27_batch_x0(B)
    s = _solver(p, B, control_limits="enforce")
    s.SetControlLimits(-ARM_TAU, ARM_TAU)
    s.SetInitialState(x0); s.SetInitialGuess(ug)
    s.Solve()
    assert (np.all(s.K == 0.0, axis=2)).any()            # some input rode its bound
    _check_vs_oracle(s, p, x0, ug, -ARM_TAU, ARM_TAU, model, range(B))


def test_arm_mpc_matches_the_host_loop_of_the_oracle():
    from drake_ddp_amd import workloads as W
    p, ug, model = _arm("arm27")
    B, R, r = 2, 2, 2
    x0 = W.arm27_batch_x0(B, seed=9)
    s = _solver(p, B, control_limits="enforce")
    s.SetControlLimits(-ARM_TAU, ARM_TAU)
    s.SetInitialState(x0); s.SetInitialGuess(ug)
    s.Solve()
    s.MPCRun(R, r)
    log = s.mpc_log
    assert np.all(s.u_bar >= -ARM_TAU[:, None]) and np.all(s.u_bar <= ARM_TAU[:, None])
    for b in range(B):
        o = _oracle(p, -ARM_TAU, ARM_TAU, model)
        o.set_problem(x0[b], p["x_nom"], p["Q"], p["R"], p["Qf"], ug)
        o.solve()
        for k in range(R):
            xs, us = W.mpc_shift(o.x_bar, o.u_bar, r)
            o.x0, o.u_bar = xs, us
            _, _, Lo, hist = o.solve()
            assert abs(log[b, k, p["x_nom"].size] - Lo) <= 1e-7 * abs(Lo), (b, k, log[b, k, p["x_nom"].size], Lo)
            assert int(log[b, k, -1]) == len(hist), (b, k)


# ---- chainx plugins built with control limits -------------------------------------------------------------------------------
CHAINX_LIM = {"n12_m4": (6, 4, 0), "n32_m16": (16, 16, 0), "n7_m3": (3, 3, 1), "n16_m1": (8, 1, 0)}
_built = {}


def _chainx(key):
    if not _built:
        import models as PM
        from drake_ddp_amd import plugin
        specs = {k: PM.chainx_spec(*sh) for k, sh in CHAINX_LIM.items()}
        with concurrent.futures.ThreadPoolExecutor(len(specs)) as ex:
            sos = dict(zip(specs, ex.map(lambda sp: plugin.compile_model(*sp, control_limits=True), specs.values())))
        for k, so in sos.items():
            _built[k] = plugin.load_model(so)
    return _built[key]


def _chainx_problem(key, N=30, seed=0):
    import plugin_steps as PS
    from oracle import models_np as M
    nq, m, ne = CHAINX_LIM[key]
    n = 2 * nq + ne
    make = _chainx(key)
    sys_ = make(0.02)
    model = M.Model.custom(n, m, PS.chainx_step(nq, m, ne), sys_.params, 0.02)
    p = dict(model_id=None, dt=0.02, N=N, x_nom=np.zeros(n), Q=np.eye(n), R=0.1 * np.eye(m), Qf=10.0 * np.eye(n),
             delta=1e-6, beta=0.9, gamma=0.0)
    rng = np.random.default_rng(seed + n)
    x0 = 0.6 * rng.standard_normal((3, n))
    return p, sys_, model, x0, np.zeros((m, N - 1))


@pytest.mark.parametrize("key,kind,jac", [("n12_m4", "nonneg", "fd"), ("n12_m4", "per_problem", "autodiff"),
                                          ("n32_m16", "sym", "fd"), ("n7_m3", "sym", "autodiff"), ("n16_m1", "sym", "fd")])
def test_chainx_limits_match_the_oracle(key, kind, jac):
    p, sys_, model, x0, ug = _chainx_problem(key)
    B, m = x0.shape[0], ug.shape[0]
    s = _solver(p, B, system=sys_, control_limits="enforce", jacobian_mode=jac)
    # the unlimited solve's controls set the scale of bounds that bind
    s0 = _solver(p, B, system=sys_, jacobian_mode=jac)
    s0.SetInitialState(x0); s0.SetInitialGuess(ug)
    s0.Solve()
    umax = np.abs(s0.u_bar).max(axis=2)                  # (B, m)
    if kind == "nonneg":
        lo, hi = np.zeros(m), np.full(m, np.inf)
    elif kind == "per_problem":
        lo, hi = -0.4 * umax, 0.6 * umax
    else:
        lo, hi = -0.5 * umax.min(axis=0), 0.5 * umax.min(axis=0)
    s.SetControlLimits(lo, hi)
    s.SetInitialState(x0); s.SetInitialGuess(ug)
    s.Solve()
    assert np.all(s.K == 0.0, axis=2).any()
    _check_vs_oracle(s, p, x0, ug, lo, hi, model, range(B), jac)


def test_stage_backward_matches_the_oracle():
    p, sys_, model, x0, ug = _chainx_problem("n12_m4")
    B, m = x0.shape[0], ug.shape[0]
    s = _solver(p, B, system=sys_, control_limits="enforce")
    s.SetControlLimits(np.zeros(m), np.full(m, np.inf))
    s.SetInitialState(x0); s.SetInitialGuess(ug)
    s.Solve()                                            # the device's own trajectory
    xb, ub, fx, fu = s.x_bar, s.u_bar, s.fx, s.fu
    lo = np.zeros(m)
    hi = 0.5 * np.abs(ub).max() * np.ones(m)
    s.SetControlLimits(lo, hi)
    s.set_state(x_bar=xb, u_bar=ub, fx=fx, fu=fu)
    s.stage_backward()
    K, kap, dV = s.K, s.kappa, s.dV_coeff
    nclamped = 0
    for b in range(B):
        o = _oracle(p, lo, hi, model)
        o.set_problem(x0[b], p["x_nom"], p["Q"], p["R"], p["Qf"], ub[b])
        o.x_bar, o.fx, o.fu = xb[b], fx[b], fu[b]
        assert o.backward()
        nclamped += o.clamped.sum()
        assert np.array_equal(np.all(K[b] == 0.0, axis=1), o.clamped)
        for dev, ref in ((kap[b], o.kappa), (K[b], o.K), (dV[b], o.dV)):
            assert np.max(np.abs(dev - ref)) <= 1e-10 * max(1.0, np.abs(ref).max())
    assert nclamped > 0


def test_infinite_bounds_agree_with_the_unlimited_solve():
    from drake_ddp_amd import workloads as W
    p, ug, model = _arm("arm27")
    B = 4
    x0 = W.arm27_batch_x0(B, seed=11)
    res = []
    for enforce in (False, True):
        s = _solver(p, B, control_limits="enforce" if enforce else "ignore")
        if enforce:
            s.SetControlLimits(np.full(7, -np.inf), np.full(7, np.inf))
        s.SetInitialState(x0); s.SetInitialGuess(ug)
        s.Solve()
        res.append((s.cost.copy(), s.iterations.copy()))
    assert np.array_equal(res[0][1], res[1][1])
    assert np.max(np.abs(res[0][0] - res[1][0]) / np.abs(res[0][0])) <= 1e-9


def test_cleared_limits_are_bitwise_a_never_limited_handle():
    from drake_ddp_amd import workloads as W
    p, ug, model = _arm("arm27c")
    B = 4
    x0 = W.arm27_batch_x0(B, seed=12)
    res = []
    for enforce in (False, True):
        s = _solver(p, B, control_limits="enforce" if enforce else "ignore")
        if enforce:
            s.SetControlLimits(-ARM_TAU, ARM_TAU)
            s.SetControlLimits(None, None)
        s.SetInitialState(x0); s.SetInitialGuess(ug)
        x, u, _, L = s.Solve()
        res.append((x.copy(), u.copy(), L.copy(), s.K.copy(), s.iterations.copy()))
    for a, b in zip(*res):
        assert np.array_equal(a, b)


_SWITCH_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[2])
from drake_ddp_amd import workloads as W
from drake_ddp_amd.ilqr import BatchedIterativeLQR
from drake_ddp_amd.models import ModelSystem
p, ug = W.arm27_problem(), W.arm27_u_guess(50); B = 4
tau = np.array([1.0, 12.0, 4.0, 6.0, 2.0, 2.0, 2.0])
s = BatchedIterativeLQR(ModelSystem(p["model_id"], p["dt"]), p["N"], B, delta=p["delta"], beta=p["beta"], gamma=p["gamma"],
                        control_limits="enforce")
s.SetTargetState(p["x_nom"]); s.SetRunningCost(p["Q"], p["R"]); s.SetTerminalCost(p["Qf"])
s.SetControlLimits(-tau, tau)
s.SetInitialState(W.arm27_batch_x0(B, seed=13)); s.SetInitialGuess(ug)
x, u, _, L = s.Solve()
np.savez(sys.argv[1], u=u, L=L, it=s.iterations, st=s.status)
"""


def test_kernel_switches_agree_with_the_default_run(tmp_path):
    """MI_ILQR_CLUSTER=2 (limited handles run one workgroup per problem: forced off), MI_ILQR_SPEC=0 and =2 (the four-candidate
    line search clamps every candidate) give the default run's result.  One child process at a time."""
    runs = {}
    for tag, env_ in (("default", {}), ("cluster2", {"MI_ILQR_CLUSTER": "2"}), ("spec0", {"MI_ILQR_SPEC": "0"}),
                      ("spec2", {"MI_ILQR_SPEC": "2"})):
        f = str(tmp_path / (tag + ".npz"))
        env = dict(os.environ, **env_)
        r = subprocess.run([sys.executable, "-c", _SWITCH_SCRIPT, f, ROOT], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, (tag, r.returncode, r.stderr[-2000:])
        runs[tag] = np.load(f)
    ref = runs["default"]
    assert np.all(ref["st"] == 0)
    for tag, v in runs.items():
        assert np.array_equal(v["it"], ref["it"]), tag
        assert np.max(np.abs(v["L"] - ref["L"]) / np.abs(ref["L"])) <= 1e-12, tag
        assert np.max(np.abs(v["u"] - ref["u"])) <= 1e-9 * max(1.0, np.abs(ref["u"]).max()), tag


def test_the_n_above_32_kernels_still_refuse():
    import models as PM
    from drake_ddp_amd import plugin
    from drake_ddp_amd import workloads as W
    for prob in (W.synth36_problem(), W.planar_quad_problem(), W.quad3d_problem()):
        with pytest.raises(ValueError, match="m <= 2"):
            _solver(prob, 2, control_limits="enforce")
    # an n > 32 plugin, and a mid-size plugin built without limits
    nq, m, ne = PM.LARGE_SHAPES[0]
    for spec in (PM.chainx_spec(nq, m, ne), PM.chainx_spec(5, 3, 0)):
        sys_ = plugin.build_model(*spec)(0.02)
        n = sys_.n
        prob = dict(model_id=None, dt=0.02, N=10, x_nom=np.zeros(n), Q=np.eye(n), R=np.eye(sys_.m), Qf=np.eye(n),
                    delta=1e-3, beta=0.9, gamma=0.0)
        with pytest.raises(ValueError, match="m <= 2"):
            _solver(prob, 2, system=sys_, control_limits="enforce")
    with pytest.raises(ValueError):
        plugin.source("x", 36, 4, "", [], "large", control_limits=True)
