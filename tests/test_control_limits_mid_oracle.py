"""CPU checks of the control-limit oracle for any m (tests/limited_ilqr_mid_np.py), the statement of the mid-size workgroup
kernels' box QP: brute force over every face of the box for m <= 6, KKT at m = 16, agreement with the m <= 2 box_qp,
infinite bounds against OracleILQR on a chainx shape, and the refusal of an indefinite Quu."""
import itertools
import os
import sys

import numpy as np
import pytest

from tests import limited_ilqr_np as L2
from tests.limited_ilqr_mid_np import LimitedMidOracleILQR, box_qp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_pd(rng, m):
    A = rng.standard_normal((m, m))
    return A @ A.T + 0.2 * np.eye(m)


def _random_box(rng, m, kind):
    lo, hi = rng.uniform(-2.0, 0.0, m), rng.uniform(0.0, 2.0, m)
    if kind == "one_sided":                      # u >= u_min only (a thrust), and one input without limits
        hi[:] = np.inf
        lo[-1] = -np.inf
    elif kind == "inf":
        lo[0], hi[-1] = -np.inf, np.inf
    elif kind == "offset":                       # a box that does not contain 0
        lo, hi = lo + 2.5, hi + 2.5
    return lo, hi


def _brute(H, g, lo, hi):
    """The minimiser over all 3^m faces: each component free, on lo or on hi; the best feasible face minimiser."""
    m = len(g)
    best, arg = np.inf, None
    for face in itertools.product((0, 1, 2), repeat=m):
        x = np.zeros(m)
        ok = True
        for a, f in enumerate(face):
            if f == 1:
                ok = ok and np.isfinite(lo[a])
                x[a] = lo[a]
            elif f == 2:
                ok = ok and np.isfinite(hi[a])
                x[a] = hi[a]
        if not ok:
            continue
        free = np.array([f == 0 for f in face])
        if free.any():
            x[free] = np.linalg.solve(H[np.ix_(free, free)], -(g[free] + H[np.ix_(free, ~free)] @ x[~free]))
        if np.any(x < lo - 1e-12) or np.any(x > hi + 1e-12):
            continue
        v = 0.5 * x @ H @ x + g @ x
        if v < best:
            best, arg = v, x
    return best, arg


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("kind", ["finite", "one_sided", "inf", "offset"])
def test_box_qp_matches_every_face(m, kind):
    rng = np.random.default_rng(1000 * m + len(kind))
    for _ in range(12 if m >= 5 else 30):
        H = _random_pd(rng, m)
        g = 3.0 * rng.standard_normal(m)
        lo, hi = _random_box(rng, m, kind)
        d, cl, pd = box_qp(H, g, lo, hi)
        assert pd
        assert np.all(d >= lo - 1e-12) and np.all(d <= hi + 1e-12)
        best, arg = _brute(H, g, lo, hi)
        assert np.max(np.abs(d - arg)) <= 1e-9 * max(1.0, np.abs(arg).max()), (d, arg)
        assert 0.5 * d @ H @ d + g @ d <= best + 1e-12 * max(1.0, abs(best))


def test_box_qp_kkt_at_m16():
    rng = np.random.default_rng(16)
    for kind in ("finite", "one_sided", "offset"):
        for _ in range(20):
            H = _random_pd(rng, 16)
            g = 5.0 * rng.standard_normal(16)
            lo, hi = _random_box(rng, 16, kind)
            d, cl, pd = box_qp(H, g, lo, hi)
            assert pd
            cl = np.array(cl)
            grad = H @ d + g
            scale = np.abs(g).max() + np.abs(H).max() * max(1.0, np.abs(d).max())
            assert np.all(np.abs(grad[~cl]) <= 1e-12 * scale), (kind, grad[~cl])          # stationary on the free set
            assert np.all(d[~cl] >= lo[~cl]) and np.all(d[~cl] <= hi[~cl])
            on_lo = cl & (d == lo)
            on_hi = cl & (d == hi)
            assert np.all((on_lo | on_hi)[cl])                                            # clamped = exactly on a bound
            assert np.all(grad[on_lo & ~on_hi] >= 0.0) and np.all(grad[on_hi & ~on_lo] <= 0.0)   # multipliers' signs


@pytest.mark.parametrize("m", [1, 2])
def test_box_qp_equals_the_m2_construction(m):
    rng = np.random.default_rng(7 + m)
    for kind in ("finite", "inf", "offset", "one_sided"):
        for _ in range(60):
            H = _random_pd(rng, m)
            g = 3.0 * rng.standard_normal(m)
            lo, hi = _random_box(rng, m, kind)
            d, cl, pd = box_qp(H, g, lo, hi)
            d2, cl2, pd2 = L2.box_qp(H, g, lo, hi)
            assert pd and pd2
            assert np.max(np.abs(d - d2)) <= 1e-12 * max(1.0, np.abs(d2).max()), (d, d2)
            assert list(cl) == list(cl2)


def test_indefinite_quu_is_not_pd():
    H = np.diag([1.0, 2.0, -0.5, 3.0])
    assert not box_qp(H, np.ones(4), -np.ones(4), np.ones(4))[2]
    assert not box_qp(np.full((3, 3), np.nan), np.ones(3), -np.ones(3), np.ones(3))[2]


def _chainx_model(nq, m, ne, dt=0.02):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import plugin_steps as PS
    from oracle import models_np as M
    return M.Model.custom(2 * nq + ne, m, PS.chainx_step(nq, m, ne), np.array([4.0, 0.5, 6.0, 2.0]), dt)


def test_infinite_bounds_reproduce_the_oracle_on_chainx():
    from oracle.ilqr_np import OracleILQR
    nq, m, ne = 6, 4, 0                          # (n, m) = (12, 4)
    n, N = 2 * nq + ne, 30
    model = _chainx_model(nq, m, ne)
    rng = np.random.default_rng(3)
    x0 = 0.3 * rng.standard_normal(n)
    args = (x0, np.zeros(n), np.eye(n), 0.1 * np.eye(m), 10.0 * np.eye(n), np.zeros((m, N - 1)))
    o = OracleILQR(model, N, 1e-2, 0.95, 0.0, jacobian="ad")
    o.set_problem(*args)
    xo, uo, Lo, ho = o.solve()
    lim = LimitedMidOracleILQR(model, N, 1e-2, 0.95, 0.0, jacobian="ad", u_min=np.full(m, -np.inf), u_max=np.full(m, np.inf))
    lim.set_problem(*args)
    xl, ul, Ll, hl = lim.solve()
    assert len(hl) == len(ho) and [h[2] for h in hl] == [h[2] for h in ho]
    assert abs(Ll - Lo) <= 1e-12 * abs(Lo)
    assert np.max(np.abs(ul - uo)) <= 1e-12 * max(1.0, np.abs(uo).max())
    assert not lim.clamped.any()


def test_bounds_bind_and_hold_on_chainx():
    nq, m, ne = 6, 4, 0
    n, N = 2 * nq + ne, 30
    model = _chainx_model(nq, m, ne)
    rng = np.random.default_rng(4)
    lim = LimitedMidOracleILQR(model, N, 1e-2, 0.95, 0.0, jacobian="ad", u_min=np.zeros(m), u_max=np.full(m, np.inf))
    lim.set_problem(0.5 * rng.standard_normal(n), np.zeros(n), np.eye(n), 0.1 * np.eye(m), 10.0 * np.eye(n), np.zeros((m, N - 1)))
    x, u, L, hist = lim.solve()
    assert np.all(u >= 0.0)
    assert lim.clamped.any() and not lim.not_pd
    assert np.all(lim.K[:, :, :][np.broadcast_to(lim.clamped[:, None, :], lim.K.shape)] == 0.0)
