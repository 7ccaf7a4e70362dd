"""Per-problem model parameters in the C ABI and the Python class (include/mi_ilqr.h: MI_F_MODEL_PARAMS): the header declares
the selector with its (B,n_params) shape and documents the mode rules, the ctypes binding exposes it, the ABI version stays 10
with no new entry point, and BatchedIterativeLQR.SetModelParameters decides shapes and non-finite values on the host.  CPU only."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi_ilqr.h")

# the entry points of ABI 10: the 47 the per-problem targets left (this selector adds none) and mi_ilqr_policy_rollout
ABI10_ENTRY_POINTS = 48


def _header():
    with open(HEADER) as f:
        return f.read()


def _enum_value(src, name):
    m = re.search(r"\b%s\s*=\s*(\d+)\s*," % name, src)
    assert m, name
    return int(m.group(1))


def test_header_declares_the_selector_with_its_shape():
    src = _header()
    v = _enum_value(src, "MI_F_MODEL_PARAMS")
    others = [int(x) for k, x in re.findall(r"\b(MI_F_[A-Z0-9_]+)\s*=\s*(\d+)", src) if k != "MI_F_MODEL_PARAMS"]
    assert len(others) >= 16 and v not in others and v < 100
    line = next(ln for ln in src.splitlines() if re.search(r"\bMI_F_MODEL_PARAMS\s*=", ln))
    assert "(B,n_params)" in line, line


def test_header_documents_the_mode_rules():
    src = " ".join(re.sub(r"\n\s*\*", " ", _header()).split())     # comment text with the line breaks and leading '*' dropped
    assert "PER-PROBLEM PARAMETERS" in src
    assert "mi_ilqr_set(MI_F_MODEL_PARAMS, NULL, 0)" in src and "never left them" in src
    assert "the descriptor's row repeated" in src
    assert "survive mi_ilqr_reset" in src
    assert "wrong `bytes` MI_ILQR_E_BAD_SHAPE" in src and "a NaN or an infinity MI_ILQR_E_BAD_ARG" in src
    assert "(n_params == 0) MI_ILQR_E_UNSUPPORTED" in src and "a refused call changes nothing" in src


def test_capi_exposes_the_selector_and_the_abi_stays_10():
    from drake_ddp_amd import _capi
    src = _header()
    assert _capi.F_MODEL_PARAMS == _enum_value(src, "MI_F_MODEL_PARAMS")
    assert _capi.ABI_VERSION == 10
    assert re.search(r"#define MI_ILQR_ABI_VERSION 10\b", src)
    # no new entry point: the selector rides on the existing field accessors
    declared = re.findall(r"^(?:int|void|const char\s*\*|size_t|double)\s*(mi_ilqr_\w+)\(", src, re.M)
    assert len(declared) == len(set(declared)) == ABI10_ENTRY_POINTS
    assert set(declared) == set(_capi.EXPORTS)
    assert not any("param" in e for e in _capi.EXPORTS if e != "mi_ilqr_model_info")


def test_the_library_exports_no_new_symbol():
    """The built library's dynamic symbol table: exactly the header's entry points (whatever else the change added is hidden)."""
    from drake_ddp_amd import _capi
    lib = _capi.load()
    for fn in _capi.EXPORTS:
        assert hasattr(lib, fn), fn
    for fn in ("mi_ilqr_set_model_params", "mi_ilqr_get_model_params", "set_model_params"):
        assert not hasattr(lib, fn), fn


def test_set_model_parameters_checks_its_argument_without_a_device():
    from drake_ddp_amd import ilqr
    assert callable(getattr(ilqr.BatchedIterativeLQR, "SetModelParameters"))
    assert isinstance(ilqr.BatchedIterativeLQR.model_params, property)
    chk = ilqr.check_model_params
    B, P = 6, 3
    assert chk(None, B, P) is None
    rows = np.arange(B * P, dtype=np.float64).reshape(B, P) + 1.0
    out = chk(rows, B, P)
    assert out.shape == (B, P) and out.dtype == np.float64 and out.flags["C_CONTIGUOUS"] and np.array_equal(out, rows)
    out = chk(rows[:, ::-1], B, P)                         # a view with negative strides arrives contiguous
    assert out.flags["C_CONTIGUOUS"] and np.array_equal(out, rows[:, ::-1])
    one = chk([0.25, 0.1, 4.905], B, P)                    # (n_params,): broadcast to rows
    assert one.shape == (B, P) and one.flags["C_CONTIGUOUS"] and np.array_equal(one, np.tile([0.25, 0.1, 4.905], (B, 1)))
    for bad in (np.zeros((B - 1, P)), np.zeros((B, P + 1)), np.zeros((1, P)), np.zeros(P + 1), np.zeros((B, P, 1)), 1.0):
        with pytest.raises(ValueError):
            chk(bad, B, P)
    for v in (np.nan, np.inf, -np.inf):
        r = rows.copy(); r[4, 1] = v
        with pytest.raises(ValueError):
            chk(r, B, P)
        with pytest.raises(ValueError):
            chk([1.0, v, 2.0], B, P)
    with pytest.raises(ValueError):
        chk(np.zeros((B, 0)), B, 0)                        # a model without parameters
    # B == n_params: (n_params,) is still one row for everybody, (B, n_params) still rows
    sq = chk(np.array([1.0, 2.0, 3.0]), 3, 3)
    assert np.array_equal(sq, np.tile([1.0, 2.0, 3.0], (3, 1)))
