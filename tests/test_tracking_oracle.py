"""tests/tracking_ilqr_np.py (the NumPy statement of reference trajectories) against oracle/ilqr_np.py and against itself: a one-row
reference is OracleILQR bitwise; past its end the reference holds its last row; an MPC loop whose clock moves the window equals a loop
whose reference rows are shifted by hand."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N, T = 12, 10


def _problem():
    from drake_ddp_amd import workloads as W
    p = dict(W.acrobot_problem(N))
    return p, W.acrobot_batch_x0(1)[0], np.zeros((1, N - 1))


def _oracle(cls, p):
    from oracle import models_np as M
    return cls(M.Model(p["model_id"], p["dt"]), p["N"], delta=p["delta"], beta=p["beta"], gamma=p["gamma"], jacobian="fd", fd_step=1e-5)


def _ramp(p, d):
    """(T, n): from x_nom to x_nom + d over the first T / 2 rows, then held."""
    s = np.minimum(np.arange(T) / (T // 2), 1.0)
    return p["x_nom"][None, :] + s[:, None] * d[None, :]


def _state(o):
    return [np.array(a) for a in (o.x_bar, o.u_bar, o.K, o.kappa, o.dV)]


def test_a_one_row_reference_is_the_constant_target_bitwise():
    from oracle.ilqr_np import OracleILQR
    from tracking_ilqr_np import TrackingOracleILQR
    p, x0, ug = _problem()
    target = p["x_nom"] + np.array([0.3, -0.2, 0.0, 0.1])
    a = _oracle(OracleILQR, p)
    a.set_problem(x0, target, p["Q"], p["R"], p["Qf"], ug)
    _, _, La, ha = a.solve()
    b = _oracle(TrackingOracleILQR, p)
    b.set_problem(x0, p["x_nom"], p["Q"], p["R"], p["Qf"], ug)       # (x_nom is ignored while a reference is held)
    b.set_reference(target[None, :], clock=0)
    _, _, Lb, hb = b.solve()
    assert La == Lb and ha == hb
    for u, v in zip(_state(a), _state(b)):
        assert np.array_equal(u, v)
    # ... and without a reference the subclass is its parent
    c = _oracle(TrackingOracleILQR, p)
    c.set_problem(x0, target, p["Q"], p["R"], p["Qf"], ug)
    _, _, Lc, hc = c.solve()
    assert La == Lc and ha == hc


def test_the_reference_holds_its_last_row_past_its_end():
    from tracking_ilqr_np import TrackingOracleILQR
    p, x0, ug = _problem()
    ref = _ramp(p, np.array([0.4, -0.3, 0.2, 0.0]))
    o = _oracle(TrackingOracleILQR, p)
    o.set_reference(ref, clock=3)
    assert np.array_equal(o.r(0), ref[3]) and np.array_equal(o.r(6), ref[9])
    assert np.array_equal(o.r(7), ref[9]) and np.array_equal(o.r(N - 1), ref[9])          # clock + t runs off the end inside the horizon
    # the same solve on a reference that spells the held rows out
    long = np.vstack([ref, np.repeat(ref[-1:], N, axis=0)])
    res = []
    for r_ in (ref, long):
        o = _oracle(TrackingOracleILQR, p)
        o.set_problem(x0, p["x_nom"], p["Q"], p["R"], p["Qf"], ug)
        o.set_reference(r_, clock=3)
        _, _, L, h = o.solve()
        res.append((L, h, _state(o)))
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1]
    for u, v in zip(res[0][2], res[1][2]):
        assert np.array_equal(u, v)
    # and it is not the constant-target problem
    o = _oracle(TrackingOracleILQR, p)
    o.set_problem(x0, p["x_nom"], p["Q"], p["R"], p["Qf"], ug)
    assert o.solve()[2] != res[0][0]


def test_an_mpc_loop_with_a_moving_window_equals_one_shifted_by_hand():
    from drake_ddp_amd import workloads as W
    from tracking_ilqr_np import TrackingOracleILQR
    p, x0, ug = _problem()
    ref = _ramp(p, np.array([0.4, -0.3, 0.2, 0.0]))
    R, r = 3, 2
    a = _oracle(TrackingOracleILQR, p)
    b = _oracle(TrackingOracleILQR, p)
    for o in (a, b):
        o.set_problem(x0, p["x_nom"], p["Q"], p["R"], p["Qf"], ug)
        o.set_reference(ref, clock=0)
        o.solve()
    for k in range(1, R + 1):
        for o in (a, b):
            o.x0, o.u_bar = W.mpc_shift(o.x_bar, o.u_bar, r)
        a.clock = k * r                                                           # the clock moves the window ...
        b.set_reference(np.vstack([ref[min(k * r, T - 1):], ref[-1:]]), clock=0)      # ... or the rows are cut off by hand
        _, _, La, ha = a.solve()
        _, _, Lb, hb = b.solve()
        assert La == Lb and ha == hb, k
        for u, v in zip(_state(a), _state(b)):
            assert np.array_equal(u, v)
