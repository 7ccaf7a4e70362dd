"""The key-point methods (ilqr.py:380-621) at their edges on every kernel family (configurations: tests/keypoint_edges.py).

  * wave-per-problem (pendulum, acrobot, cart-pole) and workgroup-per-problem kernels (arm + ball: mid-size; the 36-state
    chain: n = 33..40) through the stage entry mi_ilqr_linearize, from crafted trajectories and fx / fu preset to a sentinel
    that differs by problem, row and element: the list and count exact, rows the reference leaves stale hold the sentinel bit
    for bit, every other row is the NumPy oracle's to 1e-10;
  * lane-per-problem kernels (no stage entries) through Solve: one iteration against OracleILQR stepped once from the same
    state (fx / fu / K / kappa, every row), and whole solves against the C oracle (statuses, iterations, trials, the key-point
    count of every iteration and the last list, exact), plus one AUTO handle that lands on these kernels (acrobot, N = 750).
"""
import warnings

import numpy as np
import pytest

from common import make_oracle, rel_err
from keypoint_edges import (benign_sentinels, crafted_x_bar, edge_configs, expected_list, fu_sentinel, fx_sentinel,
                            iterations_before_roundoff, short_configs)
from test_gpu_parity import make_solver

pytestmark = pytest.mark.gpu


def _problem(family, N):
    from drake_ddp_amd import workloads as W
    return {"pendulum": lambda: dict(W.pendulum_problem(), N=N),
            "acrobot": lambda: W.acrobot_problem(N),
            "cartpole": lambda: W.cartpole_problem(N),
            "cartpole_wall": lambda: W.cartpole_wall_problem(N),
            "arm27": lambda: W.arm27_problem(N),
            "synth36": lambda: W.synth36_problem(N)}[family]()


def _x0(family, B):
    from drake_ddp_amd import workloads as W
    return {"pendulum": lambda: W.pendulum_batch_x0(B), "acrobot": lambda: W.acrobot_batch_x0(B),
            "cartpole": lambda: W.cartpole_wall_batch_x0(B),
            "cartpole_wall": lambda: W.cartpole_wall_batch_x0(B), "arm27": lambda: W.arm27_batch_x0(B),
            "synth36": lambda: W.synth36_batch_x0(B)}[family]()


def _cases(N):
    return edge_configs(N) if N >= 6 else short_configs()


def _check_rows(dev, ref, sentinel, label):
    """Per problem and row t: the oracle's row still the sentinel -> the device's is, bit for bit; otherwise within 1e-10 of
    the oracle relative to the largest entry the oracle computed."""
    B = dev.shape[0]
    for b in range(B):
        stale = np.array([np.array_equal(ref[b][..., t], sentinel[b][..., t]) for t in range(ref.shape[-1])])
        assert np.array_equal(dev[b][..., stale], sentinel[b][..., stale]), (label, b, np.nonzero(stale)[0])
        if (~stale).any():
            assert rel_err(dev[b][..., ~stale], ref[b][..., ~stale]) < 1e-10, (label, b, rel_err(dev[b][..., ~stale], ref[b][..., ~stale]))


STAGE = [("pendulum", N) for N in (40, 2, 3, 4, 5)] + [("acrobot", N) for N in (40, 2, 3, 4, 5)] + \
        [("cartpole", 40), ("arm27", 30), ("synth36", 30)]


@pytest.mark.parametrize("family,N", STAGE)
def test_stage_linearize_at_the_keypoint_edges(family, N):
    prob = _problem(family, N)
    n, m = prob["Q"].shape[0], prob["R"].shape[0]
    B = 3
    rng = np.random.default_rng(N * 7 + len(family))
    x0 = _x0(family, B)
    xb = crafted_x_bar(x0, N, rng)
    ub = 0.2 * rng.standard_normal((B, m, N - 1))
    fx0, fu0 = fx_sentinel(B, n, N), fu_sentinel(B, n, m, N)
    for label, cfg in _cases(N).items():
        s = make_solver(prob, B=B, keypoint=cfg, jac="ad")
        s.SetInitialState(x0)
        s.set_state(x_bar=xb, u_bar=ub, fx=fx0, fu=fu0)
        s.stage_linearize()
        fx, fu, nk, kl, pct = s.fx, s.fu, s.keypoint_count, s.keypoint_list, s.percentage_derivs
        rfx, rfu = np.empty_like(fx0), np.empty_like(fu0)
        for b in range(B):
            o = make_oracle(prob, keypoint=cfg, jacobian="ad")
            o.fx, o.fu = fx0[b].copy(), fu0[b].copy()
            kp = o.linearize(xb[b], ub[b])
            want = expected_list(cfg, N)
            assert want is None or kp == want, (label, b)
            assert nk[b] == len(kp) and np.array_equal(kl[b][:len(kp)], kp), (family, N, label, b, kl[b][:nk[b]], kp)
            assert pct[b] == o.percentage_derivs, (label, b)
            rfx[b], rfu[b] = o.fx, o.fu
        _check_rows(fx, rfx, fx0, (family, N, label, "fx"))
        _check_rows(fu, rfu, fu0, (family, N, label, "fu"))


def _solve_quiet(s):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # (max_iters reached: the point of these solves)
        return s.Solve()


def _one_iteration(family, N, cfg, label, B=4, **kw):
    """Solve with max_iters = 1 on a handle whose fx / fu are preset (benign_sentinels) against OracleILQR stepped once from
    the same state: the rollout of u_guess, linearize, backward.  Every row of fx, fu, K and kappa."""
    prob = _problem(family, N)
    n, m = prob["Q"].shape[0], prob["R"].shape[0]
    rng = np.random.default_rng(N + 3)
    x0 = _x0(family, B)
    ug = 0.1 * rng.standard_normal((B, m, N - 1))
    fx0, fu0 = benign_sentinels(B, n, m, N)
    s = make_solver(prob, B=B, keypoint=cfg, jac="ad", max_iters=1, hist_cap=4, **kw)
    s.SetInitialState(x0)
    s.SetInitialGuess(ug)
    s.set_state(fx=fx0, fu=fu0)
    _solve_quiet(s)
    assert (s.iterations == 1).all(), (label, s.iterations)
    fx, fu, K, kappa, nk, kl = s.fx, s.fu, s.K, s.kappa, s.keypoint_count, s.keypoint_list
    rfx, rfu = np.empty_like(fx0), np.empty_like(fu0)
    for b in range(B):
        o = make_oracle(prob, keypoint=cfg, jacobian="ad")
        o.set_problem(x0[b], prob["x_nom"], prob["Q"], prob["R"], prob["Qf"], ug[b])
        o.fx, o.fu = fx0[b].copy(), fu0[b].copy()
        o.forward(np.inf)
        o.backward()
        kp = list(o.keypoints)
        assert nk[b] == len(kp) and np.array_equal(kl[b][:len(kp)], kp), (family, N, label, b, kl[b][:nk[b]], kp)
        rfx[b], rfu[b] = o.fx, o.fu
        assert rel_err(K[b], o.K) < 1e-8 and rel_err(kappa[b], o.kappa) < 1e-8, (family, N, label, b, rel_err(K[b], o.K), rel_err(kappa[b], o.kappa))
    _check_rows(fx, rfx, fx0, (family, N, label, "fx"))
    _check_rows(fu, rfu, fu0, (family, N, label, "fu"))
    return s


LANE = [("pendulum", N) for N in (40, 2, 3, 4, 5)] + [("acrobot", N) for N in (40, 2, 3, 4, 5)] + \
       [("cartpole", 40), ("cartpole_wall", 40)]


@pytest.mark.parametrize("family,N", LANE)
def test_lane_kernels_one_iteration_at_the_keypoint_edges(family, N):
    """Fails before the duplicate walk was fixed: with minN = 1 and a threshold of -inf, or maxN = 1, the list starts
    [0, 0, ...] and the fused evaluate-and-interpolate pass stopped after t = 0."""
    for label, cfg in _cases(N).items():
        _one_iteration(family, N, cfg, label, kernel_mode="throughput")


def test_auto_handle_on_the_lane_kernels_long_horizon():
    """acrobot.py's horizon N = 750: AUTO serves it with the lane-per-problem kernels (no stage entries there), with the
    duplicate key-point t = 0 of adaptiveJerk (minN = 1, threshold -inf, and maxN = 1)."""
    from drake_ddp_amd import _capi
    from drake_ddp_amd._capi import MiIlqrError
    for label, cfg in (("aj_min1_neginf", edge_configs(750)["aj_min1_neginf"]), ("aj_max1", edge_configs(750)["aj_max1"])):
        s = _one_iteration("acrobot", 750, cfg, label, B=3)
        with pytest.raises(MiIlqrError) as e:                  # (the lane-per-problem kernels: no stage entries)
            s.stage_linearize()
        assert e.value.code == _capi.E_UNSUPPORTED


@pytest.mark.parametrize("family,N", [("pendulum", 60), ("acrobot", 40), ("cartpole", 40), ("cartpole_wall", 40), ("pendulum", 4)])
def test_lane_kernels_whole_solves_at_the_keypoint_edges_vs_c_oracle(family, N):
    """Whole solves from cold (central differences on both sides) against the C oracle: status, iterations, trials, the
    key-point count of every iteration and the last list exact for every problem.  Costs to 1e-6, as
    test_randomized_keypoint_configs_vs_c_oracle holds them (cart-pole + wall: 1.3e-7 after four iterations with every
    decision the same - its contact amplifies round-off about tenfold per iteration).  A problem's solve stops before its
    first iteration decided at round-off (keypoint_edges.iterations_before_roundoff, measured on the C oracle): the handle
    runs once per distinct cap."""
    from oracle import c_oracle, models_np as M
    prob = _problem(family, N)
    m = prob["R"].shape[0]
    model = M.Model(prob["model_id"], prob["dt"])
    B = 6
    x0 = _x0(family, B)
    ug = np.zeros((1, m, N - 1))
    for label, cfg in _cases(N).items():
        full = c_oracle.solve_batch(model, prob, x0, ug, keypoint=cfg, hist_cap=64, max_iters=64)
        caps = np.array([max(1, iterations_before_roundoff(full["hist"][b, :min(int(full["iters"][b]), 64), 0])) for b in range(B)])
        for cap in np.unique(caps):
            sel = np.nonzero(caps == cap)[0]
            r = c_oracle.solve_batch(model, prob, x0[sel], ug, keypoint=cfg, hist_cap=64, max_iters=int(cap))
            s = make_solver(prob, B=len(sel), keypoint=cfg, jac="fd", kernel_mode="throughput", max_iters=int(cap), hist_cap=64)
            s.SetInitialState(x0[sel]); s.SetInitialGuess(ug[0])
            _, _, _, L = _solve_quiet(s)
            h, nk, kl = s.history, s.keypoint_count, s.keypoint_list
            for j in range(len(sel)):
                it = int(r["iters"][j])
                what = (family, N, label, int(sel[j]), int(cap))
                assert s.status[j] == r["status"][j] and s.iterations[j] == it and s.ls_trials[j] == r["ls"][j], \
                    (what, s.status[j], r["status"][j], s.iterations[j], it, s.ls_trials[j], r["ls"][j])
                assert np.array_equal(np.round(h[j, :it, 3] * (N - 1) / 100.0), r["hist"][j, :it, 3]), what
                assert np.array_equal(h[j, :it, 1:3], r["hist"][j, :it, 1:3]), what
                assert nk[j] == r["kp_count"][j] and np.array_equal(kl[j][:nk[j]], r["kp_list"][j][:nk[j]]), what
                if r["status"][j] != 2:
                    assert abs(L[j] - r["cost"][j]) <= 1e-6 * abs(r["cost"][j]), (what, L[j], r["cost"][j])
