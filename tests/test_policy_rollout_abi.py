"""mi_ilqr_policy_rollout in the C ABI and the Python classes: include/mi_ilqr.h declares it, the library exports it, the ctypes
binding lists it in EXPORTS and has its prototype, the ABI version stays 10, and RolloutPolicy decides shapes and non-finite parameters on the host.  CPU only."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi_ilqr.h")


def _header():
    with open(HEADER) as f:
        return f.read()


def test_the_symbol_is_declared_and_exported():
    from drake_ddp_amd import _capi
    src = _header()
    m = re.search(r"^int mi_ilqr_policy_rollout\(([^;]*)\);", src, re.M)
    assert m, "include/mi_ilqr.h does not declare mi_ilqr_policy_rollout"
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["mi_ilqr_t* h", "int32_t S", "const double* x0", "const double* params", "double* cost", "double* x_final",
                    "int32_t* steps", "double* X", "double* U"]
    assert _capi.EXPORTS.count("mi_ilqr_policy_rollout") == 1 and not hasattr(_capi, "POLICY_EXPORTS")
    lib = _capi.load()
    assert hasattr(lib, "mi_ilqr_policy_rollout")
    assert len(lib.mi_ilqr_policy_rollout.argtypes) == 9
    # a NULL handle is refused before anything touches a device
    assert lib.mi_ilqr_policy_rollout(None, 1, None, None, None, None, None, None, None) == _capi.E_BAD_ARG


def test_the_abi_version_stays_10():
    from drake_ddp_amd import _capi
    assert re.search(r"#define MI_ILQR_ABI_VERSION 10\b", _header())
    assert _capi.ABI_VERSION == 10 and _capi.load().mi_ilqr_abi_version() == 10
    assert _capi.F_POLICY_KERNEL_MS == int(re.search(r"\bMI_F_POLICY_KERNEL_MS\s*=\s*(\d+)", _header()).group(1))


def test_the_header_documents_the_conventions():
    src = " ".join(re.sub(r"\n\s*\*", " ", _header()).split())
    for phrase in ("one GPU lane per sample", "+inf for a sample that ended early", "steps completed, N-1 for a full rollout",
                   "the last state the sample held", "The handle is only READ", "params for a model with n_params == 0 MI_ILQR_E_UNSUPPORTED",
                   "a NaN or an infinity in params MI_ILQR_E_BAD_ARG", "S < 1, NULL x0 or cost MI_ILQR_E_BAD_ARG"):
        assert phrase in src, phrase


def test_rollout_policy_checks_its_arguments_without_a_device():
    from drake_ddp_amd import ilqr
    for cls in (ilqr.BatchedIterativeLQR, ilqr.IterativeLinearQuadraticRegulator):
        assert callable(getattr(cls, "RolloutPolicy"))
    chk = ilqr.check_rollout_args
    B, S, n, P = 3, 5, 2, 3
    x0 = np.arange(B * S * n, dtype=np.float64).reshape(B, S, n)
    x, p = chk(x0, None, B, n, P)
    assert p is None and x.shape == (B, S, n) and x.flags["C_CONTIGUOUS"] and np.array_equal(x, x0)
    x, p = chk(x0[0], np.ones((S, P)), B, n, P)                        # (S, n) and (S, n_params): broadcast over the problems
    assert x.shape == (B, S, n) and x.flags["C_CONTIGUOUS"] and np.array_equal(x[2], x0[0])
    assert p.shape == (B, S, P) and p.flags["C_CONTIGUOUS"]
    x, p = chk(x0[:, ::-1], np.ones((B, S, P)), B, n, P)               # a view with negative strides arrives contiguous
    assert x.flags["C_CONTIGUOUS"] and np.array_equal(x, x0[:, ::-1])
    nan0 = x0.copy(); nan0[1, 2, 0] = np.nan                           # a non-finite x0 is data, not an error
    assert np.isnan(chk(nan0, None, B, n, P)[0][1, 2, 0])
    for bad in (np.zeros(n), np.zeros((B, S, n, 1)), 1.0):             # wrong rank
        with pytest.raises(ValueError):
            chk(bad, None, B, n, P)
    for bad in (np.zeros((B, S, n + 1)), np.zeros((S, n + 1)), np.zeros((B + 1, S, n)), np.zeros((B, 0, n))):   # wrong n, B, S
        with pytest.raises(ValueError):
            chk(bad, None, B, n, P)
    for bad in (np.ones((B, S, P + 1)), np.ones((B, S + 1, P)), np.ones(P), np.ones((B, P))):
        with pytest.raises(ValueError):
            chk(x0, bad, B, n, P)
    for v in (np.nan, np.inf, -np.inf):                                # NaN / infinity in params
        prm = np.ones((B, S, P)); prm[2, 4, 1] = v
        with pytest.raises(ValueError, match="NaN or infinity"):
            chk(x0, prm, B, n, P)
    with pytest.raises(ValueError, match="no parameters"):             # params on a parameterless plugin
        chk(x0, np.zeros((B, S, 0)), B, n, 0)
    assert chk(x0, None, B, n, 0)[1] is None


def test_rollout_policy_raises_before_it_touches_the_handle():
    """The methods themselves, on objects that have no handle at all (no device, no library call can have happened)."""
    from drake_ddp_amd import ilqr

    class _System:
        params = np.array([0.25, 0.1, 4.905])

    for cls, B in ((ilqr.BatchedIterativeLQR, 3), (ilqr.IterativeLinearQuadraticRegulator, 1)):
        s = object.__new__(cls)
        s.B, s.n, s.m, s.N, s.system = B, 2, 1, 10, _System()                  # what the argument checks read; no _h, no _lib
        for x0, prm in ((np.zeros(2), None), (np.zeros((4, 3)), None), (np.zeros((4, 2)), np.full((4, 3), np.nan)),
                        (np.zeros((4, 2)), np.ones((4, 2)))):
            with pytest.raises(ValueError):
                s.RolloutPolicy(x0, prm)
        _System.params = np.array([0.25, 0.1, 4.905])
    single = object.__new__(ilqr.IterativeLinearQuadraticRegulator)
    single.B, single.n, single.m, single.N, single.system = 1, 2, 1, 10, _System()
    with pytest.raises(ValueError, match=r"x0 must be \(S, 2\)"):              # the drop-in class takes (S, n) only
        single.RolloutPolicy(np.zeros((1, 4, 2)))
    _System.params = np.zeros(0)                                                 # a parameterless model
    with pytest.raises(ValueError, match="no parameters"):
        single.RolloutPolicy(np.zeros((4, 2)), np.zeros((4, 0)))
