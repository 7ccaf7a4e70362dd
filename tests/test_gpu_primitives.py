"""The scalar primitives of the device models (csrc/dual.hpp, csrc/fastmath.hpp) against mpmath, through probe plugins and the
existing stage entries (tests/primitive_probes.py: probes, inputs, bounds and their reasons; truth: tests/golden/prim_<name>.npz).

  wave   n = 6, m = 1, family 0, kernel_mode = "latency"       wave-per-problem kernels        stage entries
  lane   the same plugins, kernel_mode = "throughput"          lane-per-problem kernels        Solve, max_iters = 1 (no stage entries)
  mid    n = 12, m = 4, family 1                               mid-size workgroup kernels      stage entries
  large  n = 36, m = 4, family 1                               n = 33..40 matrix-core kernels  stage entries

Values (double overloads) and "ad" diagonals (Dual1 rules) at >= 2^16 points per primitive within the project's own bounds, fx off
the diagonal and fu exactly zero, bit for bit the same on every family; "fd" diagonals within the central-difference bound.
Non-finite inputs go through the stage entries only (the lane kernels see 1.0 in their place).  The plugins cannot reach
SoftplusPool::in_vgprs (the built-in cart-pole + wall passes it down its rollout loop): same polynomial, same constants.
The measured maxima are printed (pytest -s) and recorded in DESIGN.md.
"""
import concurrent.futures
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import primitive_probes as P  # noqa: E402

pytestmark = pytest.mark.gpu

N = 4                                     # the shortest horizon every family accepts; only the first step is read
FAMILIES = {"wave": (("probe_small_a", "probe_small_b"), dict(kernel_mode="latency"), 8192),
            "lane": (("probe_small_a", "probe_small_b"), dict(kernel_mode="throughput"), 8192),
            "mid": (("probe_mid",), {}, 8192),
            "large": (("probe_large",), {}, 4096)}


@pytest.fixture(scope="module")
def probes():
    from drake_ddp_amd import plugin
    specs = P.specs()
    with concurrent.futures.ThreadPoolExecutor(min(6, len(specs))) as ex:
        sos = list(ex.map(lambda sp: plugin.compile_model(*sp), specs))
    return {sp[0]: plugin.load_model(so) for sp, so in zip(specs, sos)}


def _benign(prim, x):
    """Inputs whose result or derivative is not finite -> 1.0 (linearization: 0 x NaN off the diagonal; the lane kernels' Solve)."""
    bad = ~np.isfinite(x) | ((x == 0.0) if prim == "rcp" else False)
    return np.where(bad, 1.0, x)


def _solver(make, n, m, B, jac, fd_step, **kw):
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    s = BatchedIterativeLQR(make(1.0), N, B, delta=1e-3, beta=0.5, jacobian_mode=jac, fd_step=fd_step, **kw)
    s.SetTargetState(np.zeros(n)); s.SetRunningCost(np.zeros((n, n)), np.eye(m)); s.SetTerminalCost(np.zeros((n, n)))
    return s


def _run(make, name, pools, family, jac, B, fd_step=P.FD_H, values=True):
    """One probe over its pools -> ({prim: values}, {prim: derivative diagonal}); asserts fx off the diagonal and fu zero."""
    from drake_ddp_amd import _capi
    n, m, _, slots = P.PROBES[name]
    kw = FAMILIES[family][1]
    pools = {p: x for p, x in pools.items() if p in slots}
    x0, where = P.pack(slots, pools, B)
    x0_lin, _ = P.pack(slots, {p: _benign(p, x) for p, x in pools.items()}, B)
    L = x0.shape[0]
    val, der = np.empty((L, B, n)), np.empty((L, B, n))
    eye = np.eye(n, dtype=bool)
    s = _solver(make, n, m, B, jac, fd_step, **(dict(kw, max_iters=1, hist_cap=4) if family == "lane" else kw))
    for l in range(L):
        if family == "lane":
            s.SetInitialState(x0_lin[l]); s.SetInitialGuess(np.full((m, N - 1), 0.1))
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)        # (max_iters reached)
                s.Solve()
            val[l] = s.x_bar[:, :, 1]
            if l == 0:                                                 # the lane-per-problem kernels served it: they alone have no stage entries
                with pytest.raises(_capi.MiIlqrError) as e:
                    s.stage_linearize()
                assert e.value.code == _capi.E_UNSUPPORTED
        else:
            s.SetInitialState(x0[l]); s.SetInitialGuess(np.zeros((m, N - 1)))
            s.set_state(K=np.zeros((B, m, n, N - 1)), kappa=np.zeros((B, m, N - 1)))
            if values:
                val[l] = s.stage_rollout(1.0)[0][:, :, 1]
            s.SetInitialState(x0_lin[l])
            s.set_state(x_bar=np.repeat(x0_lin[l][:, :, None], N, axis=2), u_bar=np.zeros((B, m, N - 1)))
            s.stage_linearize()
        fx, fu = s.fx[:, :, :, 0], s.fu[:, :, :, 0]
        der[l] = fx[:, eye]
        assert np.all(fx[:, ~eye] == 0.0), (name, family, jac, "fx off the diagonal")
        assert np.all(fu == 0.0), (name, family, jac, "fu")
    return P.unpack(val, where, pools), P.unpack(der, where, pools)


@pytest.fixture(scope="module")
def evaluated(probes):
    """{family: ({prim: values}, {prim: "ad" diagonals})} at every input of every primitive."""
    pools = {p: P.inputs(p) for p in P.PRIMS}
    out = {}
    for family, (names, _, B) in FAMILIES.items():
        val, der = {}, {}
        for name in names:
            v, d = _run(probes[name], name, pools, family, "ad", B)
            for p in v:
                # a primitive in both small probes: the same bits from either
                assert p not in val or (_same(val[p], v[p]) and _same(der[p], d[p])), (family, name, p)
                val[p], der[p] = v[p], d[p]
        out[family] = (val, der)
    return out


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _truth(prim, deriv):
    """(indices, hi, lo) of the points with truth."""
    g = P.load(prim)
    m = np.nonzero(P.measured(prim))[0]
    if not deriv:
        return m, g["hi"][m], g["lo"][m]
    if prim == "sin":
        c = P.load("cos")
        return m, c["hi"][m], c["lo"][m]
    if prim == "cos":
        s_ = P.load("sin")
        return m, -s_["hi"][m], -s_["lo"][m]
    if prim == "exp":
        return m, g["hi"][m], g["lo"][m]
    return P.deriv_index(prim), g["d_hi"], g["d_lo"]


def _errors(prim, dev, hi, lo, bound):
    """Per point: error in ulp, whether it is within the primitive's bound, and - for the points judged by an absolute rule (sin /
    cos below 1e-6: 1e-15; the softplus below 2^-1022: 2^-1022), which the ulp figure leaves out - the absolute error (else NaN)."""
    err = P.ulp_error(dev, hi, lo)
    ok = err <= bound
    absolute = np.abs(dev - hi - lo.astype(np.float64) * np.spacing(np.abs(hi)))
    rule = np.zeros(hi.size, bool)
    if prim in ("sin", "cos"):
        rule = np.abs(hi) < P.TRIG_SMALL
        ok = np.where(rule, absolute <= P.TRIG_ABS, ok)
    if prim == "softplus":
        rule = np.abs(hi) < P.TINY
        ok = np.where(rule, absolute <= P.TINY, ok)
    return np.where(rule, 0.0, err), ok, np.where(rule, absolute, np.nan)


def _check(prim, family, dev, deriv):
    idx, hi, lo = _truth(prim, deriv)
    bound = (P.DERIV_ULP if deriv else P.VALUE_ULP)[prim]
    x = P.inputs(prim)
    if family == "lane":                                  # finite inputs only
        keep = np.isfinite(x[idx])
        idx, hi, lo = idx[keep], hi[keep], lo[keep]
    err, ok, absolute = _errors(prim, dev[idx], hi, lo, bound)
    what = "d/dx " + prim if deriv else prim
    bad = []
    for label, kind, sl in P.segments(prim)[0]:
        inside = (idx >= sl.start) & (idx < sl.stop)
        if kind == "ulp" and inside.any():
            ruled = inside & ~np.isnan(absolute)
            print("\nULP %-14s %-5s %-34s max %.3f ulp  (bound %.1f, %d points)%s" % (
                what, family, label, err[inside & ~ruled].max() if (inside & ~ruled).any() else 0.0, bound, (inside & ~ruled).sum(),
                "; %d points under the absolute rule: max %.3e" % (ruled.sum(), absolute[ruled].max()) if ruled.any() else ""))
            if not ok[inside].all():
                w = np.nonzero(inside & ~ok)[0]
                bad.append((label, int(w.size), float(x[idx[w[0]]]), float(err[w].max())))
        elif kind == "bounded" and not deriv and family != "lane":
            d = dev[sl]
            assert np.isfinite(d).all() and np.abs(d).max() <= 1.0 + 4.0 * np.spacing(1.0), (what, family, label, np.abs(d).max())
        elif kind == "nan" and not deriv and family != "lane":
            assert np.isnan(dev[sl]).all(), (what, family, label, dev[sl])
    assert not bad, (what, family, bad)


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("prim", P.PRIMS)
def test_values_against_mpmath(evaluated, prim, family):
    _check(prim, family, evaluated[family][0][prim], deriv=False)


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("prim", P.PRIMS)
def test_dual1_derivatives_against_mpmath(evaluated, prim, family):
    _check(prim, family, evaluated[family][1][prim], deriv=True)


@pytest.mark.parametrize("prim", P.PRIMS)
def test_every_family_gives_the_same_bits(evaluated, prim):
    """One source, four kernel families: a difference would mean a family compiles the primitives differently."""
    x = P.inputs(prim)
    finite = np.isfinite(x) & ~((x == 0.0) if prim == "rcp" else False)
    ref_v, ref_d = evaluated["wave"][0][prim], evaluated["wave"][1][prim]
    for family in ("mid", "large", "lane"):
        v, d = evaluated[family][0][prim], evaluated[family][1][prim]
        sel = finite if family == "lane" else np.ones(x.size, bool)
        assert _same(v[sel], ref_v[sel]), (prim, family, "values", int((v[sel] != ref_v[sel]).sum()))
        assert _same(d[finite], ref_d[finite]), (prim, family, "derivatives", int((d[finite] != ref_d[finite]).sum()))


_NP = {"sin": np.sin, "cos": np.cos, "rcp": lambda x: 1.0 / x, "exp": np.exp, "log1p": np.log1p, "sqrt": np.sqrt,
       "softplus": lambda x: np.logaddexp(0.0, x)}


@pytest.mark.parametrize("family", ["wave", "mid", "large"])
def test_central_differences_within_their_bound(probes, family):
    """fx's diagonal with jacobian_mode = "fd", h = 2^-17 and x on a 2^-30 grid (x +- h exact, 1 / 2h exact):
    |fd - f'| <= h^2 / 6 max |f'''| + (value bound in ulp) ulp(f) / h, max |f'''| per primitive in primitive_probes.FD_RANGE."""
    h = P.FD_H
    pools = {p: P.fd_inputs(p) for p in P.PRIMS}
    names, _, _ = FAMILIES[family]
    seen = set()
    for name in names:
        _, der = _run(probes[name], name, pools, family, "fd", P.FD_POINTS, values=False)
        for prim, d in der.items():
            g = P.load(prim)
            hi, lo = g["fd_hi"], g["fd_lo"].astype(np.float64)
            x = pools[prim]
            fmag = np.abs(_NP[prim](x)) + 1.01 * h * np.abs(hi)                 # (the size of f on [x - h, x + h]: for ulp(f) only)
            val_err = P.VALUE_ULP[prim] * np.spacing(fmag)
            if prim in ("sin", "cos"):
                val_err = np.where(fmag < P.TRIG_SMALL, np.maximum(val_err, P.TRIG_ABS), val_err)
            bound = h * h / 6.0 * P.FD_RANGE[prim][2] + val_err / h
            err = np.abs(d - hi - lo * np.spacing(np.abs(hi)))
            print("\nFD  %-10s %-5s max error %.3e, smallest bound %.3e, largest error / bound %.3f" % (prim, family, err.max(), bound.min(), (err / bound).max()))
            assert np.all(err <= bound), (prim, family, float((err / bound).max()))
            seen.add(prim)
    assert seen == set(P.PRIMS)
