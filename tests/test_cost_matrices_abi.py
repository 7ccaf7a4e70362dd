"""Per-problem cost matrices in the C ABI (include/mi_ilqr.h: MI_F_COST_MATRICES): the header declares the selector with its
(B,2*n*n+m*m) shape and documents the mode rules, the ctypes binding exposes it, and the ABI version stays 10 (a new selector of the
existing mi_ilqr_set / mi_ilqr_get / mi_ilqr_device_ptr, no new symbol).  CPU only."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi_ilqr.h")
NAME = "MI_F_COST_MATRICES"


def _header():
    with open(HEADER) as f:
        return f.read()


def _enum_value(src, name):
    m = re.search(r"\b%s\s*=\s*(\d+)\s*," % name, src)
    assert m, name
    return int(m.group(1))


def test_header_declares_the_selector_with_its_shape():
    src = _header()
    v = _enum_value(src, NAME)
    # a double field: below the int32 selectors (100 ..), distinct from every other double selector
    others = [int(x) for k, x in re.findall(r"\b(MI_F_[A-Z_]+)\s*=\s*(\d+)", src) if k != NAME]
    assert v not in others and v < 100
    line = next(ln for ln in src.splitlines() if re.search(r"\b%s\s*=" % NAME, ln))
    assert "(B,2*n*n+m*m)" in line and "Q_b | R_b | Qf_b" in line, line
    # letters and underscores only, and none of the words the other selectors' ABI tests match on
    assert re.fullmatch(r"[A-Z_]+", NAME) and not any(w in NAME.lower() for w in ("target", "x_nom", "param"))


def test_header_documents_the_mode_rules():
    src = " ".join(re.sub(r"\n\s*\*", " ", _header()).split())     # comment text with the line breaks and leading '*' dropped
    assert "PER-PROBLEM COST MATRICES" in src
    blk = src[src.index("PER-PROBLEM COST MATRICES"):]
    blk = blk[:blk.index("*/")]
    # into per-problem mode and the two ways back
    assert "mi_ilqr_set(MI_F_COST_MATRICES, rows, B*(2*n*n+m*m)*8)" in blk
    assert "mi_ilqr_set(MI_F_COST_MATRICES, NULL, 0) returns it to SHARED mode" in blk and "whatever mi_ilqr_set_cost last set" in blk
    assert "mi_ilqr_set_cost with any of Q, R, Qf non-NULL returns it to shared mode" in blk
    assert "bitwise a handle that never left it" in blk
    # the class is per handle; rows survive reset; refusals
    assert "most general kernel form any of its rows needs" in blk
    assert "survive mi_ilqr_reset" in blk
    assert "wrong `bytes` MI_ILQR_E_BAD_SHAPE" in blk and "a NaN or an infinity MI_ILQR_E_BAD_ARG" in blk
    assert "a refused call changes nothing" in blk


def test_capi_exposes_the_selector_and_the_abi_stays_10():
    from drake_ddp_amd import _capi
    src = _header()
    assert _capi.F_COST_MATRICES == _enum_value(src, NAME)
    assert _capi.ABI_VERSION == 10
    assert re.search(r"#define MI_ILQR_ABI_VERSION 10\b", src)
    # no new entry point: the selector rides on the existing field accessors
    for fn in ("mi_ilqr_set", "mi_ilqr_get", "mi_ilqr_device_ptr"):
        assert fn in _capi.EXPORTS
    assert not any("cost_matri" in e or "cost_rows" in e for e in _capi.EXPORTS)
    assert sum("cost" in e for e in _capi.EXPORTS) == 1 and "mi_ilqr_set_cost" in _capi.EXPORTS


def test_the_python_setters_take_both_forms():
    """SetRunningCost / SetTerminalCost document the (B, ..) forms; cost_matrices is the read-back."""
    from drake_ddp_amd.ilqr import BatchedIterativeLQR as S
    assert "(B, n, n)" in S.SetRunningCost.__doc__ and "(B, n, n)" in S.SetTerminalCost.__doc__
    assert isinstance(S.cost_matrices, property)
