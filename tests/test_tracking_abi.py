"""Reference trajectories in the C ABI and the Python classes (include/mi_ilqr.h: MI_F_X_REF / MI_F_REF_CLOCK): two selectors with
values of their own, mirrored by the ctypes binding; no new entry point, ABI 10; the header documents the rules; and
SetTargetTrajectory's argument checking decides shapes, T = 0, non-finite values and the clock on the host.  CPU only."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi_ilqr.h")
ABI10_ENTRY_POINTS = 48


def _header():
    with open(HEADER) as f:
        return f.read()


def test_the_two_selectors_have_values_no_other_selector_uses():
    src = _header()
    pairs = re.findall(r"\b(MI_F_[A-Z0-9_]+)\s*=\s*(\d+)", src)
    values = dict((k, int(v)) for k, v in pairs)
    assert len(values) == len(pairs)                                   # every selector declared once
    assert values["MI_F_X_REF"] == 27 and values["MI_F_REF_CLOCK"] == 28
    assert len(set(values.values())) == len(values)                    # ... with a value of its own
    line = next(ln for ln in src.splitlines() if re.search(r"\bMI_F_X_REF\s*=", ln))
    assert "(B,T,n)" in line, line
    line = next(ln for ln in src.splitlines() if re.search(r"\bMI_F_REF_CLOCK\s*=", ln))
    assert "(1,)" in line, line


def test_capi_mirrors_them_and_the_abi_stays_10_with_48_entry_points():
    from drake_ddp_amd import _capi
    src = _header()
    assert (_capi.F_X_REF, _capi.F_REF_CLOCK) == (27, 28)
    assert _capi.ABI_VERSION == 10 and re.search(r"#define MI_ILQR_ABI_VERSION 10\b", src)
    declared = re.findall(r"^(?:int|void|const char\s*\*|size_t|double)\s*(mi_ilqr_\w+)\(", src, re.M)
    assert len(declared) == len(set(declared)) == ABI10_ENTRY_POINTS
    assert set(declared) == set(_capi.EXPORTS)


def test_header_documents_the_rules():
    src = " ".join(re.sub(r"\n\s*\*", " ", _header()).split())
    assert "Reference trajectories" in src and "min(c + t, T-1)" in src
    assert "holds its last row" in src
    assert "mi_ilqr_set(MI_F_X_REF, rows, B*T*n*8)" in src and "MI_ILQR_E_BAD_SHAPE" in src
    assert "bitwise one that never held a reference" in src
    assert "c + k replan_steps" in src and "target_step must be NULL" in src
    assert "wave- and lane-per-problem families return MI_ILQR_E_UNSUPPORTED" in src
    assert "refuses MI_F_PLANT_STATE and mi_ilqr_policy_rollout" in src


def test_set_target_trajectory_checks_its_argument_without_a_device():
    from drake_ddp_amd.ilqr import check_target_trajectory
    B, n, T = 3, 5, 4
    rows, c = check_target_trajectory(np.ones((T, n)), 2, B, n)
    assert rows.shape == (B, T, n) and rows.flags["C_CONTIGUOUS"] and rows.dtype == np.float64 and c == 2
    rows, c = check_target_trajectory(np.arange(B * T * n).reshape(B, T, n), 0, B, n)
    assert rows.shape == (B, T, n) and rows[2, 3, 4] == B * T * n - 1
    assert check_target_trajectory(None, 0, B, n) == (None, 0)
    assert check_target_trajectory(np.ones((1, n)), 0, B, n)[0].shape == (B, 1, n)
    nan = np.ones((T, n)); nan[1, 2] = np.nan
    inf = np.ones((B, T, n)); inf[0, 0, 0] = np.inf
    for bad in (np.ones(n), np.ones((T, n + 1)), np.ones((B + 1, T, n)), np.ones((B, T, n, 1)), np.ones((0, n)), np.ones((B, 0, n)),
                nan, inf, "reference", [[1.0, 2.0], [3.0]]):
        with pytest.raises(ValueError, match="SetTargetTrajectory"):
            check_target_trajectory(bad, 0, B, n)
    for clock in (-1, 1.5, 2 ** 30, "soon", None, np.nan):
        with pytest.raises(ValueError, match="clock"):
            check_target_trajectory(np.ones((T, n)), clock, B, n)
