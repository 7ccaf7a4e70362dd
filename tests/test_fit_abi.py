"""Parameter identification without a device: the MI_F_FIT_* selectors and the MI_FIT_* statuses as the header states them, the
bindings, the layering of the new units, the argument checks (drake_ddp_amd.argcheck.check_fit_args) and the result class.  CPU only."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HEADER = os.path.join(ROOT, "include", "mi_ilqr.h")
CSRC = os.path.join(ROOT, "drake_ddp_amd", "csrc")

NAMES = ("DATA", "WEIGHTS", "START", "BOUNDS", "RUN", "RESULT", "NORMAL", "KERNEL_MS")


def _header():
    with open(HEADER) as f:
        return f.read()


def test_the_header_states_the_selectors_and_the_rules():
    from drake_ddp_amd import _capi
    src = _header()
    last = int(re.search(r"\bMI_F_SEEDS_KERNEL_MS\s*=\s*(\d+)", src).group(1))
    for i, name in enumerate(NAMES):                               # values 45 .. 52, counted on from the selector before them
        k = int(re.search(r"\bMI_F_FIT_%s\s*=\s*MI_F_SEEDS_KERNEL_MS \+ (\d+)," % name, src).group(1))
        assert last + k == 45 + i == getattr(_capi, "F_FIT_" + name), name
    assert re.search(r"enum \{ MI_FIT_CONVERGED = 0, MI_FIT_MAX_ITERS = 1, MI_FIT_STALLED = 2, MI_FIT_BAD_DATA = 3 \};", src)
    assert (_capi.FIT_CONVERGED, _capi.FIT_MAX_ITERS, _capi.FIT_STALLED, _capi.FIT_BAD_DATA) == (0, 1, 2, 3)
    assert re.search(r"#define MI_FIT_MAX_FREE 8\b", src) and _capi.FIT_MAX_FREE == 8
    assert (_capi.FIT_RUN_DOUBLES, _capi.FIT_RESULT_EXTRA) == (6, 7)
    assert re.search(r"#define MI_ILQR_ABI_VERSION 10\b", src) and _capi.ABI_VERSION == 10
    declared = re.findall(r"^(?:int|void|const char\s*\*|size_t|double)\s*(mi_ilqr_\w+)\(", src, re.M)
    assert len(declared) == len(set(declared)) == 48 == len(_capi.EXPORTS)            # no new entry point
    flat = " ".join(re.sub(r"\n\s*\*", " ", src).split())
    for phrase in ("---- Parameter identification (ABI 10; selectors MI_F_FIT_* of mi_ilqr_set / mi_ilqr_get, no new entry point)",
                   "A model without parameters answers MI_ILQR_E_UNSUPPORTED", "A refused call changes nothing",
                   "mi_ilqr_set(MI_F_FIT_DATA, rows, B*T*(2n+m)*8)", "row j of problem b = x_j | u_j | x_next_j", "Rows need not be consecutive in time",
                   "mi_ilqr_set(MI_F_FIT_WEIGHTS, rows, B*(n+1)*8)", "count an integer in [0, T]", "mi_ilqr_set(MI_F_FIT_START, rows, B*(n_params+1)*8)",
                   "row b = theta0 | mu0", "mi_ilqr_set(MI_F_FIT_BOUNDS, rows, 2*n_params*8)", "mi_ilqr_set(MI_F_FIT_RUN, v, (6+P)*8)",
                   "v = iterations | ftol | fd_rel | fd_floor | apply | P | free[0] .. free[P-1]", "P in [1, MI_FIT_MAX_FREE]",
                   "free strictly increasing indices below n_params", "h_k = fd_rel max(|theta_k|, fd_floor) at the point being evaluated",
                   "(H + mu D) delta = g by Cholesky, D_ii = H_ii where H_ii > 0, else 1", "theta' = clip(theta + delta) on the free entries",
                   "a pivot that is not positive or not finite is a rejected trial", "mu <- max(mu / 10, 1e-12)", "mu <- min(10 mu, 1e12)",
                   "`iterations` counts trials", "an accepted trial with c - c' <= ftol c, or c' == 0", "a rejected trial with mu already at 1e12",
                   "A finished problem is frozen while the rest of the batch goes on", "the models' feasibility bounds are not consulted",
                   "G = P + 1 rounded up to a power of two slots per transition", "an order that is a function of T and P alone",
                   "I + 1 launches of each on the handle's stream", "exactly what mi_ilqr_set(MI_F_MODEL_PARAMS, theta) would leave",
                   "apply = 0 reads and writes nothing a solve uses", "mi_ilqr_get(MI_F_FIT_RESULT, dst, B*(n_params+7)*8)",
                   "row b = theta | cost0 | cost | mu | iterations | accepted | status | count", "mi_ilqr_get(MI_F_FIT_NORMAL, dst, B*(P+P*P)*8)",
                   "inv(H) cost / (count n - P)"):
        assert phrase in flat, phrase


def test_the_bindings_and_the_units():
    from drake_ddp_amd import argcheck, build, ilqr, plugin, results
    from drake_ddp_amd.ilqr import BatchedIterativeLQR, IterativeLinearQuadraticRegulator
    assert callable(BatchedIterativeLQR.FitModelParameters) and callable(BatchedIterativeLQR.fit_kernel_ms)
    assert IterativeLinearQuadraticRegulator.FitModelParameters is not BatchedIterativeLQR.FitModelParameters
    assert ilqr.ParamFit is results.ParamFit and ilqr.check_fit_args is argcheck.check_fit_args
    assert results.ParamFit.__slots__ == ("params", "cost0", "cost", "damping", "iterations", "accepted", "status", "count", "gradient",
                                         "normal_matrix", "kernel_ms")

    def includes(name):
        with open(os.path.join(CSRC, name)) as f:
            return re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M)
    assert sorted(includes("fit.hpp")) == ["fastmath.hpp", "host.hpp", "models.hpp", "wave_ops.hpp"]
    assert includes("k_fit.hip") == ["fit.hpp"] and includes("h_fit.hip") == ["host_internal.hpp"]
    host_units = {os.path.basename(s) for s in build.host_sources()}
    assert "h_fit.hip" in host_units and "k_fit.hip" not in host_units
    for name in os.listdir(CSRC):
        if name.endswith(".hpp") or name in host_units:
            assert "fit.hpp" not in includes(name), name
    with open(os.path.join(CSRC, "fit.hpp")) as f:
        text = f.read()
    assert "fit_normal_kernel(" in text and "fit_update_kernel(mi_host::FitUpdateArgs" not in text    # the model-free kernel: the unit's
    with open(os.path.join(CSRC, "k_fit.hip")) as f:
        unit = f.read()
    assert "fit_update_kernel(mi_host::FitUpdateArgs" in unit
    for model in ("Pendulum", "Acrobot", "CartPole", "CartPoleWall", "Synth36", "PlanarQuad", "Quad3D", "Arm27", "Arm27C"):
        assert "launch_fit_normal<mi::%s>" % model in unit, model
    with open(os.path.join(CSRC, "host.hpp")) as f:
        host = f.read()
    assert "struct FitArgs" in host and "struct FitUpdateArgs" in host and "kModeFitNormal" in host
    assert "if (mode == kModeFitNormal) return launch_fit_normal<M>" in host
    with open(os.path.join(CSRC, "kernel_args.hpp")) as f:
        assert "fit" not in f.read().lower()                                   # (KArgs is what it was)
    for family in ("small", "large"):
        assert '#include "fit.hpp"' in plugin.source("t", 2, 1, "xn[0] = x[0]; xn[1] = x[1] + dt * u[0];", [], family)


def test_param_fit_from_rows():
    from drake_ddp_amd.results import ParamFit
    B, npar, P = 2, 3, 2
    res = np.arange(B * (npar + 7), dtype=float).reshape(B, npar + 7)
    nor = np.arange(B * (P + P * P), dtype=float).reshape(B, P + P * P)
    f = ParamFit.from_rows(res, nor, npar, P, 0.25)
    assert np.array_equal(f.params, res[:, :3]) and np.array_equal(f.cost0, res[:, 3]) and np.array_equal(f.cost, res[:, 4])
    assert np.array_equal(f.damping, res[:, 5]) and f.iterations.dtype == np.int64 and np.array_equal(f.iterations, [6, 16])
    assert np.array_equal(f.accepted, [7, 17]) and np.array_equal(f.status, [8, 18]) and np.array_equal(f.count, [9, 19])
    assert np.array_equal(f.gradient, nor[:, :2]) and f.normal_matrix.shape == (B, P, P) and np.array_equal(f.normal_matrix[1], [[8, 9], [10, 11]])
    one = f._without_batch_axis()
    assert one.params.shape == (3,) and one.normal_matrix.shape == (P, P) and one.kernel_ms == 0.25 and int(one.status) == 8


# ---------------------------------------------------------------- check_fit_args
B, T, n, m, NP = 3, 5, 2, 1, 3


def _args(**kw):
    rng = np.random.default_rng(0)
    a = dict(x=rng.standard_normal((B, T, n)), u=rng.standard_normal((B, T, m)), x_next=rng.standard_normal((B, T, n)), free=[0, 2],
             params0=np.array([0.25, 0.1, 4.9]))
    a.update(kw)
    return a


def _chk(**kw):
    from drake_ddp_amd.argcheck import check_fit_args
    a = _args(**kw)
    npar = a.pop("n_params", NP)
    return check_fit_args(a.pop("x"), a.pop("u"), a.pop("x_next"), B, n, m, npar, **a)


def test_check_fit_args_accepts():
    a = _args()
    data, w, start, bounds, run = _chk()
    assert data.shape == (B, T, 2 * n + m) and data.flags["C_CONTIGUOUS"] and data.dtype == np.float64
    assert np.array_equal(data[:, :, :n], a["x"]) and np.array_equal(data[:, :, n:n + m], a["u"]) and np.array_equal(data[:, :, n + m:], a["x_next"])
    assert np.array_equal(w, np.hstack([np.ones((B, n)), np.full((B, 1), T)])) and bounds is None
    assert np.array_equal(start, np.tile([0.25, 0.1, 4.9, 1e-3], (B, 1)))
    assert np.array_equal(run, [20, 1e-12, 1e-6, 1e-8, 0, 2, 0, 2])
    # a padding control, counts that cut rows (NaN past a count is no data), per-problem weights, rows and dampings, half-open bounds
    x = a["x"].copy()
    x[1, 3:] = np.nan
    p0 = np.arange(B * NP, dtype=float).reshape(B, NP) + 1.0
    data, w, start, bounds, run = _chk(x=x, count=[5, 3, 0], weights=np.full((B, n), 2.0), params0=p0, damping=[1.0, 2.0, 3.0], m_dev=4,
                                       bounds=(None, [1.0, np.inf, 2.0]), iterations=0, ftol=0, fd_rel=1e-5, fd_floor=1e-9, apply=True,
                                       free=(np.int64(1),))
    assert data.shape == (B, T, 2 * n + 4) and not data[1, 3:].any() and not data[2].any() and not data[:, :, n + m:n + 4].any()
    assert np.array_equal(data[0, :, n + 4:], a["x_next"][0]) and np.array_equal(w[:, n], [5, 3, 0]) and np.all(w[:, :n] == 2.0)
    assert np.array_equal(start[:, :NP], p0) and np.array_equal(start[:, NP], [1.0, 2.0, 3.0])
    assert np.array_equal(bounds, [[-np.inf] * 3, [1.0, np.inf, 2.0]])
    assert np.array_equal(run, [0, 0.0, 1e-5, 1e-9, 1, 1, 1])
    assert _chk(free=list(range(8)), n_params=9, params0=np.ones(9))[4].size == 14           # eight free parameters: the most


REFUSED = [
    (dict(n_params=0, params0=None), "FitModelParameters: this model has no parameters"),
    (dict(x=np.zeros((T, n))), f"FitModelParameters: x must be ({B}, T, {n}) with T >= 1; got (5, 2)"),
    (dict(x=np.zeros((B, 0, n))), f"FitModelParameters: x must be ({B}, T, {n}) with T >= 1; got (3, 0, 2)"),
    (dict(u=np.zeros((B, T, m + 1))), f"FitModelParameters: u must be ({B}, {T}, {m}) with T >= 1; got (3, 5, 2)"),
    (dict(x_next=np.zeros((B, T + 1, n))), f"FitModelParameters: x_next must be ({B}, {T}, {n}) with T >= 1; got (3, 6, 2)"),
    (dict(x="abc"), "FitModelParameters: x is not an array of numbers"),
    (dict(free=3), "FitModelParameters: free must be a list of parameter indices; got 3"),
    (dict(free=[]), "FitModelParameters: free must hold between 1 and 8 parameter indices; got 0"),
    (dict(free=list(range(9)), n_params=12, params0=np.ones(12)), "FitModelParameters: free must hold between 1 and 8 parameter indices; got 9"),
    (dict(free=[0, 3]), "FitModelParameters: free[1] must be an integer in [0, 2]; got 3"),
    (dict(free=[-1]), "FitModelParameters: free[0] must be an integer in [0, 2]; got -1"),
    (dict(free=[0.5]), "FitModelParameters: free[0] must be an integer in [0, 2]; got 0.5"),
    (dict(free=[2, 0]), "FitModelParameters: free must be strictly increasing; got [2, 0]"),
    (dict(free=[1, 1]), "FitModelParameters: free must be strictly increasing; got [1, 1]"),
    (dict(count=[5, 5, 6]), f"FitModelParameters: count must be ({B},) integers in [0, {T}]; got [5, 5, 6]"),
    (dict(count=[5, 5]), f"FitModelParameters: count must be ({B},) integers in [0, {T}]; got [5, 5]"),
    (dict(count=[1, -1, 1]), f"FitModelParameters: count must be ({B},) integers in [0, {T}]; got [1, -1, 1]"),
    (dict(count=[1, 1.5, 1]), f"FitModelParameters: count must be ({B},) integers in [0, {T}]; got [1, 1.5, 1]"),
    (dict(x=np.full((B, T, n), np.nan)), "FitModelParameters: NaN or infinity in x"),
    (dict(u=np.full((B, T, m), np.inf)), "FitModelParameters: NaN or infinity in u"),
    (dict(x_next=np.full((B, T, n), np.nan), count=[0, 0, 1]), "FitModelParameters: NaN or infinity in x_next"),
    (dict(weights=[1.0, -1.0]), "FitModelParameters: negative entry in weights"),
    (dict(weights=[1.0, np.nan]), "FitModelParameters: NaN or infinity in weights"),
    (dict(weights=np.ones(3)), f"FitModelParameters: weights must be ({n},) or ({B}, {n}); got (3,)"),
    (dict(params0=None), "FitModelParameters: params0 is required"),
    (dict(params0=np.ones(2)), f"FitModelParameters: params0 must be ({B}, {NP}) or ({NP},); got (2,)"),
    (dict(params0=[1.0, np.inf, 1.0]), "FitModelParameters: NaN or infinity in params0"),
    (dict(damping=0.0), "FitModelParameters: damping must be a scalar or (3,), finite and > 0; got 0.0"),
    (dict(damping=[1.0, 1.0]), "FitModelParameters: damping must be a scalar or (3,), finite and > 0; got [1.0, 1.0]"),
    (dict(damping=np.nan), "FitModelParameters: damping must be a scalar or (3,), finite and > 0; got nan"),
    (dict(bounds=[0.0]), "FitModelParameters: bounds must be a pair (lo, hi)"),
    (dict(bounds=(np.zeros(2), None)), f"FitModelParameters: bounds lo must be ({NP},); got (2,)"),
    (dict(bounds=(None, [1.0, np.nan, 1.0])), "FitModelParameters: NaN in bounds hi"),
    (dict(bounds=(np.ones(3), np.zeros(3))), "FitModelParameters: bounds has lo > hi"),
    (dict(iterations=-1), "FitModelParameters: iterations must be an integer in [0, 2^20]; got -1"),
    (dict(iterations=True), "FitModelParameters: iterations must be an integer in [0, 2^20]; got True"),
    (dict(ftol=-1e-3), "FitModelParameters: ftol must be a finite number >= 0; got -0.001"),
    (dict(fd_rel=0.0), "FitModelParameters: fd_rel must be a finite number > 0; got 0.0"),
    (dict(fd_floor=np.nan), "FitModelParameters: fd_floor must be a finite number > 0; got nan"),
    (dict(apply=1), "FitModelParameters: apply must be True or False; got 1"),
]


@pytest.mark.parametrize("kw,message", REFUSED, ids=[str(i) for i in range(len(REFUSED))])
def test_check_fit_args_refuses(kw, message):
    with pytest.raises(ValueError) as e:
        _chk(**kw)
    assert str(e.value).startswith(message), str(e.value)


def test_a_nan_past_the_count_is_no_data_but_one_inside_is():
    x = _args()["x"].copy()
    x[0, 4, 1] = np.nan
    _chk(x=x, count=[4, 5, 5])
    with pytest.raises(ValueError, match="NaN or infinity in x"):
        _chk(x=x, count=[5, 5, 5])
