"""CPU checks of control-limited iLQR: the box-QP oracle against brute force, the limited oracle with infinite bounds
against OracleILQR, and the C ABI's declaration of mi_ilqr_set_control_limits (include/mi_ilqr.h, ABI 10)."""
import os
import re

import numpy as np
import pytest

from tests.common import load_golden, make_oracle
from tests.limited_ilqr_np import LimitedOracleILQR, box_qp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_pd(rng, m):
    A = rng.standard_normal((m, m))
    return A @ A.T + 0.2 * np.eye(m)


def _random_box(rng, m, kind):
    lo, hi = rng.uniform(-2.0, 0.0, m), rng.uniform(0.0, 2.0, m)
    if kind == "inf":
        lo[0], hi[-1] = -np.inf, np.inf
    elif kind == "equal":
        hi[0] = lo[0]
    elif kind == "offset":                       # a box that does not contain 0 (u_bar outside the limits)
        lo, hi = lo + 2.5, hi + 2.5
    return lo, hi


def _brute(Quu, Qu, lo, hi, n=801):
    """Dense grid over the (finite-clipped) box: the smallest objective found."""
    axes = [np.linspace(max(l, -6.0), min(h, 6.0), n if h > l else 1) for l, h in zip(lo, hi)]
    grid = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, len(lo))
    f = 0.5 * np.einsum("ki,ij,kj->k", grid, Quu, grid) + grid @ Qu
    return float(f.min())


@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("kind", ["finite", "inf", "equal", "offset"])
def test_box_qp_matches_brute_force_and_kkt(m, kind):
    rng = np.random.default_rng(100 * m + len(kind))
    for _ in range(40):
        Quu = _random_pd(rng, m)
        Qu = 3.0 * rng.standard_normal(m)
        lo, hi = _random_box(rng, m, kind)
        d, cl, pd = box_qp(Quu, Qu, lo, hi)
        assert pd
        assert np.all(d >= lo) and np.all(d <= hi)
        obj = 0.5 * d @ Quu @ d + Qu @ d
        assert obj <= _brute(Quu, Qu, lo, hi, 2001 if m == 1 else 401) + 1e-9
        # KKT: the gradient vanishes on free components, points out of the box on clamped ones
        g = Quu @ d + Qu
        for a in range(m):
            if not cl[a]:
                assert abs(g[a]) < 1e-9 * max(1.0, np.abs(Qu).max()), (a, g, cl)
            elif hi[a] > lo[a]:
                if d[a] == lo[a]:
                    assert g[a] >= -1e-9
                else:
                    assert d[a] == hi[a] and g[a] <= 1e-9


def test_box_qp_refuses_indefinite():
    d, cl, pd = box_qp(np.array([[1.0, 2.0], [2.0, 1.0]]), np.array([1.0, 0.0]), np.array([-1.0, -1.0]), np.array([1.0, 1.0]))
    assert not pd
    assert not box_qp(np.array([[-1.0]]), np.array([1.0]), np.array([-1.0]), np.array([1.0]))[2]


def test_infinite_bounds_reproduce_the_oracle():
    g, prob = load_golden("pendulum_c1")
    args = (prob["x0"] if "x0" in prob else g["x0"], prob["x_nom"], prob["Q"], prob["R"], prob["Qf"], g["u_guess"])
    o = make_oracle(prob, jacobian="ad")
    o.set_problem(*args)
    xo, uo, Lo, ho = o.solve()
    from oracle import models_np as M
    lim = LimitedOracleILQR(M.Model(prob["model_id"], prob["dt"]), prob["N"], delta=prob["delta"], beta=prob["beta"],
                            gamma=prob["gamma"], jacobian="ad", u_min=[-np.inf], u_max=[np.inf])
    lim.set_problem(*args)
    xl, ul, Ll, hl = lim.solve()
    assert len(hl) == len(ho)
    assert [h[2] for h in hl] == [h[2] for h in ho]
    assert abs(Ll - Lo) <= 1e-12 * abs(Lo)
    assert np.max(np.abs(xl - xo)) <= 1e-12 * max(1.0, np.max(np.abs(xo)))
    assert np.max(np.abs(ul - uo)) <= 1e-12 * max(1.0, np.max(np.abs(uo)))


def test_limited_oracle_stays_in_the_box():
    g, prob = load_golden("pendulum_c1")
    from oracle import models_np as M
    lim = LimitedOracleILQR(M.Model(prob["model_id"], prob["dt"]), prob["N"], delta=prob["delta"], beta=prob["beta"],
                            gamma=prob["gamma"], jacobian="ad", u_min=[-1.0], u_max=[1.0])
    lim.set_problem(g["x0"], prob["x_nom"], prob["Q"], prob["R"], prob["Qf"], 5.0 * np.ones_like(g["u_guess"]))
    x, u, L, hist = lim.solve()
    assert np.all(u >= -1.0) and np.all(u <= 1.0)
    assert lim.clamped.any()
    assert np.all(lim.K[:, :, lim.clamped[0]] == 0.0)


def test_header_declares_set_control_limits():
    hdr = open(os.path.join(ROOT, "include", "mi_ilqr.h")).read()
    assert re.search(r"int\s+mi_ilqr_set_control_limits\s*\(\s*mi_ilqr_t\s*\*\s*h\s*,\s*const double\s*\*\s*u_min\s*,\s*"
                     r"const double\s*\*\s*u_max\s*,\s*int32_t\s+per_problem\s*\)\s*;", hdr)
    assert re.search(r"#define MI_ILQR_ABI_VERSION 10\b", hdr)
    from drake_ddp_amd import _capi
    assert _capi.ABI_VERSION == 10
    assert "mi_ilqr_set_control_limits" in _capi.EXPORTS
