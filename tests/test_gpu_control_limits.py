"""Control-limited iLQR on the device (mi_ilqr_set_control_limits; Limited<M> kernels) against the NumPy statement of
the same semantics (tests/limited_ilqr_np.py): pendulum batches, acrobot MPC, cart-pole + wall at a long horizon, the
chain3 plugin (m = 2, per-problem bounds), the THROUGHPUT kernels, the backward stage entry, equivalences and refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "plugins"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

# problems whose decisions may differ from the oracle's at round-off level: a line-search acceptance, or a step's clamped set
# (at the ends of an arc on the bound the box QP's unconstrained minimiser sits on the bound itself, and K's row there
# switches between Quu^-1 Qux and 0 on the last bit) - such a problem's trajectory is not compared to round-off
FLIP_BUDGET = 3
N_ORACLE = 16                     # problems of each batch re-solved by the NumPy oracle


def _solver(p, B, **kw):
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    from drake_ddp_amd.models import ModelSystem
    sys_ = kw.pop("system", None) or ModelSystem(p["model_id"], p["dt"])
    s = BatchedIterativeLQR(sys_, p["N"], B, delta=p["delta"], beta=p["beta"], gamma=kw.pop("gamma", p["gamma"]),
                            device=0, **kw)
    s.SetTargetState(p["x_nom"]); s.SetRunningCost(p["Q"], p["R"]); s.SetTerminalCost(p["Qf"])
    return s


def _oracle(p, lo, hi, jac="fd", gamma=None, model=None):
    from oracle import models_np as M
    from limited_ilqr_np import LimitedOracleILQR
    model = model or M.Model(p["model_id"], p["dt"])
    return LimitedOracleILQR(model, p["N"], p["delta"], p["beta"], p["gamma"] if gamma is None else gamma,
                             jacobian="ad" if jac == "autodiff" else "fd", fd_step=1e-5, u_min=lo, u_max=hi)


def _check_vs_oracle(s, p, x0, ug, lo, hi, jac="fd", gamma=None, model=None, idx=None):
    """costs 1e-9 relative (or within the problem's own round-off spread), iterations, trials and the final clamped set
    equal up to FLIP_BUDGET problems."""
    from limited_ilqr_np import LinesearchFailed
    L, it, ls, u, st, K = s.cost, s.iterations, s.ls_trials, s.u_bar, s.status, s.K
    flips = 0
    idx = list(range(N_ORACLE) if idx is None else idx)
    idx += [b for b in np.flatnonzero(st != 0) if b not in idx]      # every problem that did not converge
    for b in idx:
        o = _oracle(p, lo[b] if np.ndim(lo) == 2 else lo, hi[b] if np.ndim(hi) == 2 else hi, jac, gamma, model)
        o.set_problem(x0[b], p["x_nom"], p["Q"], p["R"], p["Qf"], ug if ug.ndim == 2 else ug[b])
        try:
            xo, uo, Lo, hist = o.solve()
        except LinesearchFailed:                                   # the reference's RuntimeError (ilqr.py:337)
            flips += st[b] != 2
            continue
        # the problem's own sensitivity to round-off: the oracle again from x0 moved by one ulp either way.  A long arc on
        # the bound can make a solve that stops at delta = 1e-2 land 1e-5 apart from such a neighbour (same iterations, same
        # trials); the device must then be as close to the oracle as the oracle is to itself
        spread = 0.0
        for d in (np.inf, -np.inf):
            o2 = _oracle(p, lo[b] if np.ndim(lo) == 2 else lo, hi[b] if np.ndim(hi) == 2 else hi, jac, gamma, model)
            o2.set_problem(np.nextafter(x0[b], d), p["x_nom"], p["Q"], p["R"], p["Qf"], ug if ug.ndim == 2 else ug[b])
            try:
                spread = max(spread, abs(o2.solve()[2] - Lo))
            except LinesearchFailed:
                spread = np.inf
        clamped_dev = np.all(K[b] == 0.0, axis=1)                   # (m, N-1): rows of K that are exact zeros
        same = (st[b] == 0 and len(hist) == it[b] and sum(h[2] for h in hist) == ls[b] and
                np.array_equal(clamped_dev, o.clamped))
        flips += not same
        if same:
            assert abs(L[b] - Lo) <= 1e-9 * abs(Lo) + 10.0 * spread, (b, L[b], Lo, spread)
            if spread <= 1e-10 * abs(Lo):
                assert np.max(np.abs(u[b] - uo)) <= 1e-6 * max(1.0, np.abs(uo).max()), b
    assert flips <= FLIP_BUDGET, flips


def _pendulum_bound(B):
    from drake_ddp_amd import workloads as W
    p = W.pendulum_problem()
    x0 = W.pendulum_batch_x0(1024)[:B]
    s = _solver(p, B)
    s.SetInitialState(x0); s.SetInitialGuess(np.zeros((1, p["N"] - 1)))
    _, u, _, _ = s.Solve()
    return p, x0, 0.5 * float(np.abs(u).max())


@pytest.mark.parametrize("jac,gamma", [("fd", 0.0), ("autodiff", 0.0), ("fd", 0.5)])
def test_pendulum_batch_matches_the_oracle(jac, gamma):
    B = 128
    p, x0, ub = _pendulum_bound(B)
    s = _solver(p, B, jacobian_mode=jac, gamma=gamma, control_limits="enforce")
    s.SetControlLimits(-ub, ub)
    ug = np.zeros((1, p["N"] - 1))
    s.SetInitialState(x0); s.SetInitialGuess(ug)
    _, u, _, L = s.Solve()
    assert np.all(u >= -ub) and np.all(u <= ub)                  # exactly inside, no tolerance
    active = (np.abs(u) == ub).any(axis=(1, 2))
    assert active.sum() >= B // 8, active.sum()                  # converged solutions with steps on the bound
    assert (s.status == 0).sum() >= B - 4
    _check_vs_oracle(s, p, x0, ug, [-ub], [ub], jac, gamma)


def test_acrobot_mpc_matches_the_host_loop_of_the_oracle():
    from drake_ddp_amd import workloads as W
    p = W.acrobot_problem()
    B, R, r = 8, 3, 2
    x0 = W.acrobot_batch_x0(B)
    ug = np.zeros((1, p["N"] - 1))
    s = _solver(p, B, control_limits="enforce")
    s.SetControlLimits(-2.0, 2.0)
    s.SetInitialState(x0); s.SetInitialGuess(ug)
    s.Solve()
    s.MPCRun(R, r)
    log = s.mpc_log
    u = s.u_bar
    assert np.all(np.abs(u) <= 2.0)
    for b in range(B):
        o = _oracle(p, [-2.0], [2.0])
        o.set_problem(x0[b], p["x_nom"], p["Q"], p["R"], p["Qf"], ug)
        o.solve()
        for k in range(R):
            xs, us = W.mpc_shift(o.x_bar, o.u_bar, r)
            o.x0, o.u_bar = xs, us
            _, _, Lo, hist = o.solve()
            assert abs(log[b, k, p["x_nom"].size] - Lo) <= 1e-9 * abs(Lo), (b, k)
            assert int(log[b, k, -1]) == len(hist), (b, k)


def test_cartpole_wall_long_horizon():
    from drake_ddp_amd import workloads as W
    p = W.cartpole_wall_problem(N=200)
    B = 8
    x0 = W.cartpole_wall_batch_x0(B)
    ug = np.zeros((1, p["N"] - 1))
    s = _solver(p, B, control_limits="enforce")
    s.SetControlLimits(-8.0, 8.0)
    s.SetInitialState(x0); s.SetInitialGuess(ug)
    _, u, _, _ = s.Solve()
    assert np.all(np.abs(u) <= 8.0) and (np.abs(u) == 8.0).any()
    _check_vs_oracle(s, p, x0, ug, [-8.0], [8.0], idx=range(4))


def test_chain3_per_problem_bounds():
    import models as PM
    import plugin_steps as PS
    from oracle import models_np as M
    n, m, dt, N, B = 6, 2, 0.02, 60, 16
    sys_ = PM.build_all()["chain3"](dt)
    p = dict(N=N, dt=dt, delta=1e-3, beta=0.7, gamma=0.0, x_nom=np.array([np.pi, np.pi, np.pi, 0, 0, 0.0]),
             Q=dt * np.diag([1, 1, 1, .1, .1, .1]), R=dt * 0.05 * np.eye(2), Qf=20.0 * np.eye(6))
    rng = np.random.default_rng(5)
    x0 = p["x_nom"] + rng.uniform(-0.6, 0.6, (B, n))
    ug = np.zeros((m, N - 1))
    s0 = _solver(p, B, system=sys_)
    s0.SetInitialState(x0); s0.SetInitialGuess(ug)
    _, u0, _, _ = s0.Solve()
    amax = np.abs(u0).max(axis=2)                                # (B, m)
    scale = np.where(np.arange(B)[:, None] % 3 == np.array([[0, 1]]), 2.0, 0.5)   # one or both components active
    hi = amax * scale
    lo = -hi
    s = _solver(p, B, system=sys_, control_limits="enforce")
    s.SetControlLimits(lo, hi)
    s.SetInitialState(x0); s.SetInitialGuess(ug)
    _, u, _, L = s.Solve()
    assert np.all(u >= lo[:, :, None]) and np.all(u <= hi[:, :, None])
    assert (u == hi[:, :, None]).any() or (u == lo[:, :, None]).any()
    for b in range(0, B, 4):                                     # B separate single-bound solves
        s1 = _solver(p, 1, system=sys_, control_limits="enforce")
        s1.SetControlLimits(lo[b], hi[b])
        s1.SetInitialState(x0[b:b + 1]); s1.SetInitialGuess(ug)
        _, u1, _, L1 = s1.Solve()
        assert np.array_equal(u1[0], u[b]) and L1[0] == L[b], b
    model = M.Model.custom(n, m, PS.chain3_step, sys_.params, dt)
    _check_vs_oracle(s, p, x0, ug, lo, hi, model=model, idx=range(8))


def test_throughput_kernels_match_latency():
    from drake_ddp_amd import workloads as W
    p = W.pendulum_problem()
    B = 8192
    x0 = np.tile(W.pendulum_batch_x0(1024), (8, 1))
    ug = np.zeros((1, p["N"] - 1))
    out = {}
    for mode in ("latency", "throughput"):
        s = _solver(p, B, kernel_mode=mode, control_limits="enforce")
        s.SetControlLimits(-1.5, 1.5)
        s.SetInitialState(x0); s.SetInitialGuess(ug)
        _, u, _, L = s.Solve()
        out[mode] = (u.copy(), L.copy(), s.iterations.copy())
    (ul, Ll, il), (ut, Lt, it) = out["latency"], out["throughput"]
    assert np.all(np.abs(ut) <= 1.5)
    # the two families associate the same sums differently; with a torque bound active on long arcs a solve that stops at
    # delta = 1e-2 is sensitive to that (see _check_vs_oracle), so: most problems take the same iterations and agree to
    # round-off, and every problem converges to the same solution within what delta allows
    same = il == it
    assert same.mean() >= 0.95, (~same).sum()
    rel = np.abs(Lt - Ll) / np.abs(Ll)
    assert np.median(rel[same]) <= 1e-12
    assert rel.max() <= 1e-3


def test_stage_backward_matches_the_oracle():
    from drake_ddp_amd import workloads as W
    p = W.pendulum_problem()
    B = 4
    x0 = W.pendulum_batch_x0(1024)[:B]
    s = _solver(p, B)
    s.SetInitialState(x0); s.SetInitialGuess(np.zeros((1, p["N"] - 1)))
    s.Solve()
    xb, ub, fx, fu = s.x_bar, s.u_bar, s.fx, s.fu
    lim = 0.3 * np.abs(ub).max()
    sl = _solver(p, B, control_limits="enforce")
    sl.SetControlLimits(-lim, lim)
    sl.SetInitialState(x0)
    sl.set_state(x_bar=xb, u_bar=ub, fx=fx, fu=fu)
    sl.stage_backward()
    K, kap, dV = sl.K, sl.kappa, sl.dV_coeff
    for b in range(B):
        o = _oracle(p, [-lim], [lim])
        o.set_problem(x0[b], p["x_nom"], p["Q"], p["R"], p["Qf"], ub[b])
        o.x_bar, o.fx, o.fu = xb[b], fx[b], fu[b]
        o.backward()
        assert o.clamped.any()
        for dev, ref in ((kap[b], o.kappa), (K[b], o.K), (dV[b], o.dV)):
            assert np.max(np.abs(dev - ref)) <= 1e-9 * max(1.0, np.abs(ref).max())
        assert np.all(K[b][:, :, o.clamped[0]] == 0.0)


_SEQ_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[2])
from drake_ddp_amd import workloads as W
from drake_ddp_amd.ilqr import BatchedIterativeLQR
from drake_ddp_amd.models import ModelSystem
p = W.pendulum_problem(); B = 64
s = BatchedIterativeLQR(ModelSystem(p["model_id"], p["dt"]), p["N"], B, delta=p["delta"], beta=p["beta"], gamma=p["gamma"])
s.SetTargetState(p["x_nom"]); s.SetRunningCost(p["Q"], p["R"]); s.SetTerminalCost(p["Qf"])
s.SetInitialState(W.pendulum_batch_x0(1024)[:B]); s.SetInitialGuess(np.zeros((1, p["N"] - 1)))
x, u, _, L = s.Solve()
np.savez(sys.argv[1], u=u, L=L, it=s.iterations)
"""


def test_infinite_bounds_match_the_sequential_unlimited_solve(tmp_path):
    from drake_ddp_amd import workloads as W
    f = str(tmp_path / "seq.npz")
    env = dict(os.environ, MI_ILQR_SEQ_BACKWARD="1", MI_ILQR_SEQ_ROLLOUT="1")
    r = subprocess.run([sys.executable, "-c", _SEQ_SCRIPT, f, ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    ref = np.load(f)
    p = W.pendulum_problem()
    B = 64
    s = _solver(p, B, control_limits="enforce")
    s.SetControlLimits(-np.inf, np.inf)
    s.SetInitialState(W.pendulum_batch_x0(1024)[:B]); s.SetInitialGuess(np.zeros((1, p["N"] - 1)))
    _, u, _, L = s.Solve()
    same = s.iterations == ref["it"]
    assert (~same).sum() <= FLIP_BUDGET
    assert np.max(np.abs(L[same] - ref["L"][same]) / np.abs(ref["L"][same])) <= 1e-9
    assert np.max(np.abs(u[same] - ref["u"][same])) <= 1e-6 * max(1.0, np.abs(ref["u"]).max())


def test_cleared_limits_are_bitwise_a_never_limited_handle():
    from drake_ddp_amd import workloads as W
    p = W.pendulum_problem()
    B = 32
    x0 = W.pendulum_batch_x0(1024)[:B]
    res = []
    for enforce in (False, True):
        s = _solver(p, B, control_limits="enforce" if enforce else "ignore")
        if enforce:
            s.SetControlLimits(-0.5, 0.5)
            s.SetControlLimits(None, None)
        s.SetInitialState(x0); s.SetInitialGuess(np.zeros((1, p["N"] - 1)))
        x, u, _, L = s.Solve()
        res.append((x.copy(), u.copy(), L.copy(), s.K.copy(), s.iterations.copy()))
    for a, b in zip(*res):
        assert np.array_equal(a, b)


def test_ignore_keeps_the_stub_and_refusals():
    from drake_ddp_amd import workloads as W
    p = W.pendulum_problem()
    B = 4
    x0 = W.pendulum_batch_x0(1024)[:B]
    s = _solver(p, B, control_limits="enforce")
    with pytest.raises(ValueError):
        s.SetControlLimits(1.0, -1.0)
    with pytest.raises(ValueError):
        s.SetControlLimits(np.nan, 1.0)
    q = W.synth36_problem()
    with pytest.raises(ValueError, match="m <= 2"):
        _solver(q, 2, control_limits="enforce")
