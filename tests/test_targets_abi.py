"""Per-problem targets in the C ABI (include/mi_ilqr.h: MI_F_X_NOM, MI_F_TARGET_STEP): the header declares both selectors with
their (B, n) shapes and documents the mode rules, the ctypes binding exposes them, and the ABI version stays 10 (new selectors of
the existing mi_ilqr_set / mi_ilqr_get / mi_ilqr_device_ptr, no new symbol).  CPU only."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi_ilqr.h")


def _header():
    with open(HEADER) as f:
        return f.read()


def _enum_value(src, name):
    m = re.search(r"\b%s\s*=\s*(\d+)\s*," % name, src)
    assert m, name
    return int(m.group(1))


def test_header_declares_the_target_selectors_with_their_shapes():
    src = _header()
    x_nom, step = _enum_value(src, "MI_F_X_NOM"), _enum_value(src, "MI_F_TARGET_STEP")
    assert x_nom != step
    # double fields: below the int32 selectors (100 ..), distinct from every other double selector
    others = [int(v) for k, v in re.findall(r"\b(MI_F_[A-Z_]+)\s*=\s*(\d+)", src) if k not in ("MI_F_X_NOM", "MI_F_TARGET_STEP")]
    assert x_nom not in others and step not in others and max(x_nom, step) < 100
    for name in ("MI_F_X_NOM", "MI_F_TARGET_STEP"):
        line = next(ln for ln in src.splitlines() if re.search(r"\b%s\s*=" % name, ln))
        assert "(B,n)" in line, line


def test_header_documents_the_mode_rules():
    src = " ".join(re.sub(r"\n\s*\*", " ", _header()).split())     # comment text with the line breaks and leading '*' dropped
    assert "PER-PROBLEM TARGETS" in src
    # mpc_run: target_step must be NULL in per-problem mode, each row moves, repeated addition afterwards
    assert "target_step must be NULL" in src and "MI_ILQR_E_BAD_ARG" in src
    assert "num_resolves times" in src and "repeated addition" in src
    # back to shared mode, survival across reset, refusals
    assert "returns the handle to shared mode" in src and "never-per-problem" in src
    assert "survive mi_ilqr_reset" in src
    assert "Wrong `bytes` is MI_ILQR_E_BAD_SHAPE" in src and "a NaN MI_ILQR_E_BAD_ARG" in src


def test_capi_exposes_the_selectors_and_the_abi_stays_10():
    from drake_ddp_amd import _capi
    src = _header()
    assert _capi.F_X_NOM == _enum_value(src, "MI_F_X_NOM")
    assert _capi.F_TARGET_STEP == _enum_value(src, "MI_F_TARGET_STEP")
    assert _capi.ABI_VERSION == 10
    assert re.search(r"#define MI_ILQR_ABI_VERSION 10\b", src)
    # no new entry point: the selectors ride on the existing field accessors
    for fn in ("mi_ilqr_set", "mi_ilqr_get", "mi_ilqr_device_ptr"):
        assert fn in _capi.EXPORTS
    assert not any("target" in e or "x_nom" in e for e in _capi.EXPORTS)
