"""The on-device Monte-Carlo's interface without a device: the four selectors in the header and the bindings, the rules the header
states, the unchanged entry-point list and ABI version, the header layering of the new kernel header, and the host-side argument
checks (drake_ddp_amd.ilqr.check_mc_args).  CPU only."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HEADER = os.path.join(ROOT, "include", "mi_ilqr.h")
CSRC = os.path.join(ROOT, "drake_ddp_amd", "csrc")


def _header():
    with open(HEADER) as f:
        return f.read()


def test_the_four_selectors_and_nothing_else_changed():
    from drake_ddp_amd import _capi
    src = _header()
    want = {"MI_F_POLICY_MC_DIST": 29, "MI_F_POLICY_MC_RUN": 30, "MI_F_POLICY_MC_STATS": 31, "MI_F_POLICY_MC_SAMPLES": 32}
    sel = {k: int(v) for k, v in re.findall(r"\b(MI_(?:F|I|I64)_\w+)\s*=\s*(\d+)", src)}
    for name, value in want.items():
        assert sel[name] == value, name
        assert [k for k, v in sel.items() if v == value] == [name]                   # no other selector's value
    assert len(set(sel.values())) == len(sel)
    assert (_capi.F_POLICY_MC_DIST, _capi.F_POLICY_MC_RUN, _capi.F_POLICY_MC_STATS, _capi.F_POLICY_MC_SAMPLES) == (29, 30, 31, 32)
    assert (_capi.MC_DIST_NORMAL, _capi.MC_DIST_UNIFORM, _capi.MC_FIELDS) == (0, 1, 10)
    assert sel["MI_I_POLICY_MC_PASSES"] == 105 == _capi.I_POLICY_MC_PASSES                # the diagnostic beside them: passes of the last run
    assert re.search(r"MI_F_POLICY_MC_DIST\s*=\s*29,\s*/\*\s*\(B,3n\+2n_params\)", src)
    assert re.search(r"MI_F_POLICY_MC_STATS\s*=\s*31,\s*/\*\s*\(B,10\) read-only", src)
    assert re.search(r"MI_F_POLICY_MC_SAMPLES\s*=\s*32,\s*/\*\s*\(B,S,n\+n_params\+2\) read-only", src)
    assert re.search(r"#define MI_ILQR_ABI_VERSION 10\b", src) and _capi.ABI_VERSION == 10
    declared = re.findall(r"^(?:int|void|const char\s*\*|size_t|double)\s*(mi_ilqr_\w+)\(", src, re.M)
    assert len(declared) == len(set(declared)) == 48 and set(declared) == set(_capi.EXPORTS)


def test_the_header_states_the_rules():
    flat = " ".join(re.sub(r"\n\s*\*", " ", _header()).split())
    for phrase in ("Monte-Carlo on the device", "Philox block 512 + i / 4 (parameters: 768 + j / 4)", "d = (w + 1/2) 2^-31 - 1",
                   "counter = (g, 0, common ? 0 : b, block)", "blocks 0 .. 9 and 256 .. 259 only",
                   "A sample is COUNTED iff it ran all N-1 steps and its cost is finite",
                   "S | counted | success | mean | M2 | min | max | argmin | argmax | steps_total", "ties go to the lower g",
                   "counted = 0: mean = M2 = NaN, min = +inf, max = -inf, argmin = argmax = -1",
                   "groups of 64 by s / 64", "lane distance 1, 2, 4, 8, 16, 32", "mean = meanA + delta (nB / n)",
                   "M2 = (M2A + M2B) + (delta delta) ((nA nB) / n)", "A always the operand from the lower lane",
                   "count-0 operand returning the other operand's bits", "folded left to right in group order",
                   "MI_ILQR_MC_PASS_GROUPS=k", "does not depend on the window, bit for bit",
                   "a negative spread or goal: MI_ILQR_E_BAD_ARG", "A refused call changes nothing",
                   "first_sample + S > 2^32", "sample_params = 1 on a model without parameters",
                   "A refused run leaves the rows and the last results in place", "before any run MI_ILQR_E_BAD_ARG",
                   "The fold kernels are NOT included", "a solve after the run is bitwise the solve without it"):
        assert phrase in flat, phrase


def test_the_kernel_header_keeps_the_layering():
    """policy_mc.hpp may include the family header policy_rollout.hpp; no family header and nothing of the host includes it; the two
    units and the plugin template do."""
    def includes(path):
        with open(path) as f:
            return re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M)
    assert "policy_rollout.hpp" in includes(os.path.join(CSRC, "policy_mc.hpp")) and "wave_ops.hpp" in includes(os.path.join(CSRC, "policy_mc.hpp"))
    from drake_ddp_amd import build
    host_units = {os.path.basename(s) for s in build.host_sources()}
    assert {"mi_ilqr.hip", "h_policy.hip"} <= host_units
    for name in os.listdir(CSRC):
        if name.endswith(".hpp") or name in host_units:
            assert "policy_mc.hpp" not in includes(os.path.join(CSRC, name)), name
    assert includes(os.path.join(CSRC, "k_policy_mc.hip")) == ["policy_mc.hpp"] == includes(os.path.join(CSRC, "k_policy_mc_noise.hip"))
    from drake_ddp_amd import plugin
    text = plugin.source("t", 2, 1, "xn[0] = x[0]; xn[1] = x[1] + dt * u[0];", [], "small")
    assert '#include "policy_mc.hpp"' in text
    with open(os.path.join(CSRC, "host.hpp")) as f:
        host = f.read()
    assert "kModePolicyMC" in host and "struct PolicyMcArgs" in host and "MI_ILQR_MC_PASS_GROUPS" in host


# ---------------------------------------------------------------- check_mc_args
def test_check_mc_args_accepts():
    from drake_ddp_amd.ilqr import check_mc_args as chk
    B, n, npar = 3, 2, 3
    rows, run = chk(130, [1.0, 2.0], [0.5, 0.0], B, n, npar)
    assert rows.shape == (B, 3 * n + 2 * npar) and rows.dtype == np.float64 and rows.flags["C_CONTIGUOUS"]
    assert np.array_equal(rows[1], [1.0, 2.0, 0.5, 0.0, np.inf, np.inf, 0, 0, 0, 0, 0, 0])
    assert run.dtype == np.float64 and run.tolist() == [130.0, 0.0, 1.0, 0.0, 0.0]
    per = np.arange(B * n, dtype=float).reshape(B, n)
    rows, run = chk(1, per, per, B, n, npar, x0_dist="uniform", params_mean=[1.0, 2.0, 3.0], params_spread=np.full((B, npar), 0.25),
                    params_dist="normal", goal=[0.1, np.inf], samples=True, first_sample=2 ** 32 - 1)
    assert np.array_equal(rows[2], [4.0, 5.0, 4.0, 5.0, 0.1, np.inf, 1.0, 2.0, 3.0, 0.25, 0.25, 0.25])
    assert run.tolist() == [1.0, 1.0, 0.0, 1.0, 1.0]
    rows, run = chk(np.int64(7), [0.0, 0.0], [0.0, 0.0], B, n, npar, params_mean=[1.0, 2.0, 3.0])           # a mean alone: spread zero
    assert run[3] == 1.0 and np.all(rows[:, 3 * n + npar:] == 0.0)
    assert chk(2 ** 32, [0.0, 0.0], [1.0, 1.0], B, n, 0)[1][0] == 2.0 ** 32                                  # the largest S


def test_check_mc_args_refuses():
    from drake_ddp_amd.ilqr import check_mc_args as chk
    B, n, npar = 3, 2, 3
    ok = ([1.0, 2.0], [0.5, 0.5])
    for bad in (np.zeros(3), np.zeros((B, 3)), np.zeros((B + 1, n)), np.zeros((1, n)), 1.0, "x"):          # shapes
        with pytest.raises(ValueError):
            chk(4, bad, ok[1], B, n, npar)
        with pytest.raises(ValueError):
            chk(4, ok[0], bad, B, n, npar)
        with pytest.raises(ValueError):
            chk(4, *ok, B, n, npar, goal=bad)
        if np.shape(bad) not in ((npar,), (B, npar)):                                                       # (those ARE parameter rows)
            with pytest.raises(ValueError):
                chk(4, *ok, B, n, npar, params_mean=bad)
    for bad in (np.nan, np.inf, -np.inf):                                                                   # NaN / infinity
        with pytest.raises(ValueError, match="NaN"):
            chk(4, [bad, 0.0], ok[1], B, n, npar)
        with pytest.raises(ValueError, match="NaN|negative"):
            chk(4, ok[0], [bad, 0.0], B, n, npar)
        with pytest.raises(ValueError, match="NaN"):
            chk(4, *ok, B, n, npar, params_mean=[1.0, bad, 1.0])
    with pytest.raises(ValueError, match="NaN"):
        chk(4, *ok, B, n, npar, goal=[np.nan, 1.0])
    chk(4, *ok, B, n, npar, goal=[np.inf, 1.0])                                                             # (+inf is a goal)
    with pytest.raises(ValueError, match="negative"):
        chk(4, ok[0], [0.5, -1e-300], B, n, npar)
    with pytest.raises(ValueError, match="negative"):
        chk(4, *ok, B, n, npar, goal=[-0.5, 1.0])
    with pytest.raises(ValueError, match="negative"):
        chk(4, *ok, B, n, npar, params_mean=[1.0, 1.0, 1.0], params_spread=[0.1, -0.1, 0.1])
    for bad in (0, -1, 1.5, 4.0, True, None, "4"):                                                          # S
        with pytest.raises(ValueError, match="S must be"):
            chk(bad, *ok, B, n, npar)
    with pytest.raises(ValueError, match="2\\^32"):
        chk(2 ** 32 + 1, *ok, B, n, npar)
    with pytest.raises(ValueError, match="first_sample \\+ S"):
        chk(4, *ok, B, n, npar, first_sample=2 ** 32 - 3)
    chk(3, *ok, B, n, npar, first_sample=2 ** 32 - 3)
    with pytest.raises(ValueError, match="first_sample"):
        chk(4, *ok, B, n, npar, first_sample=-1)
    with pytest.raises(ValueError, match="no parameters"):
        chk(4, *ok, B, n, 0, params_mean=[])
    with pytest.raises(ValueError, match="params_spread needs params_mean"):
        chk(4, *ok, B, n, npar, params_spread=[0.1, 0.1, 0.1])
    for name in ("x0_dist", "params_dist"):
        with pytest.raises(ValueError, match=name):
            chk(4, *ok, B, n, npar, **{name: "gaussian"})


def test_the_library_refuses_a_null_handle():
    from drake_ddp_amd import _capi
    lib = _capi.load()
    v = np.zeros(10)
    for which in (_capi.F_POLICY_MC_DIST, _capi.F_POLICY_MC_RUN, _capi.F_POLICY_MC_STATS, _capi.F_POLICY_MC_SAMPLES):
        assert lib.mi_ilqr_set(None, which, _capi.ptr(v), 40) == _capi.E_BAD_ARG
        assert lib.mi_ilqr_get(None, which, _capi.ptr(v), 40) == _capi.E_BAD_ARG
