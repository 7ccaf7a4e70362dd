"""The interface of the envelopes and the safety box without a device: the five selectors in the header and the bindings, the rules the
header states, the unchanged entry-point list and ABI version, and the layering of the new kernel header.  CPU only."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HEADER = os.path.join(ROOT, "include", "mi_ilqr.h")
CSRC = os.path.join(ROOT, "drake_ddp_amd", "csrc")


def _header():
    with open(HEADER) as f:
        return f.read()


def test_the_five_selectors_and_no_new_entry_point():
    from drake_ddp_amd import _capi
    src = _header()
    want = {"MI_F_POLICY_MC_BOX": 33, "MI_F_POLICY_MC_OBSERVE": 34, "MI_F_POLICY_MC_ENVELOPE": 35, "MI_F_POLICY_MC_ENVELOPE_U": 36,
            "MI_F_POLICY_MC_SAFETY": 37}
    sel = {k: int(v) for k, v in re.findall(r"\b(MI_(?:F|I|I64)_\w+)\s*=\s*(\d+)", src)}
    for name, value in want.items():
        assert sel[name] == value, name
        assert [k for k, v in sel.items() if v == value] == [name]
    assert len(set(sel.values())) == len(sel)
    assert (_capi.F_POLICY_MC_BOX, _capi.F_POLICY_MC_OBSERVE, _capi.F_POLICY_MC_ENVELOPE, _capi.F_POLICY_MC_ENVELOPE_U,
            _capi.F_POLICY_MC_SAFETY) == (33, 34, 35, 36, 37)
    assert (_capi.MC_OBSERVE_X, _capi.MC_OBSERVE_U, _capi.MC_ENV_FIELDS) == (1, 2, 8)
    assert re.search(r"MI_F_POLICY_MC_BOX\s*=\s*33,\s*/\*\s*\(B,2n\)", src)
    assert re.search(r"MI_F_POLICY_MC_ENVELOPE\s*=\s*35,\s*/\*\s*\(B,N,n,8\) read-only", src)
    assert re.search(r"MI_F_POLICY_MC_ENVELOPE_U\s*=\s*36,\s*/\*\s*\(B,N-1,m,8\) read-only", src)
    assert re.search(r"MI_F_POLICY_MC_SAFETY\s*=\s*37,\s*/\*\s*\(B,3\+N\) read-only", src)
    assert re.search(r"#define MI_ILQR_ABI_VERSION 10\b", src) and _capi.ABI_VERSION == 10
    declared = re.findall(r"^(?:int|void|const char\s*\*|size_t|double)\s*(mi_ilqr_\w+)\(", src, re.M)
    assert len(declared) == len(set(declared)) == 48 and set(declared) == set(_capi.EXPORTS)


def test_the_header_states_the_rules():
    flat = " ".join(re.sub(r"\n\s*\*", " ", _header()).split())
    for phrase in ("Envelopes and a safety box", "count | K | s1 | s2 | min | max | argmin | argmax", "LEFT FOLD in global sample order",
                   "a non-finite v is skipped", "the first finite v sets K = v", "d = v - K, s1 += d, s2 += d d",
                   "a rounded product, then a rounded sum: no FMA", "a tie keeps the lower sample number",
                   "count = 0, K = s1 = s2 = 0, min = +inf, max = -inf, argmin = argmax = -1",
                   "mean = K + s1 / count, M2 = max(0, s2 - s1 s1 / count)", "do not depend on the window",
                   "a NaN is never outside, a value on a bound is inside", "the first t at which the sample is outside, t = 0 included",
                   "safe = ran and never outside", "|x_{N-1}[i] - x_nom_b[i]| <= goal[b,i]", "The box only observes",
                   "ran | safe | safe_success | exits[0 .. N-1]", "A NaN or lo > hi: MI_ILQR_E_BAD_ARG", "(NULL, 0) clears the box",
                   "While the handle holds a box, runs observe it", "Any other value: MI_ILQR_E_BAD_ARG",
                   "When the last run did not produce them: MI_ILQR_E_BAD_ARG", "(read-only)", "A run that observes nothing is the run it was",
                   "refused with MI_ILQR_E_UNSUPPORTED and the last results stay in place"):
        assert phrase in flat, phrase


def test_the_kernel_header_keeps_the_layering():
    """policy_env.hpp knows no model: it includes host.hpp alone; no other header and nothing of the host includes it; its unit does."""
    def includes(path):
        with open(path) as f:
            return re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M)
    assert includes(os.path.join(CSRC, "policy_env.hpp")) == ["host.hpp"]
    from drake_ddp_amd import build
    host_units = {os.path.basename(s) for s in build.host_sources()}
    assert {"mi_ilqr.hip", "h_policy.hip"} <= host_units
    for name in os.listdir(CSRC):
        if name.endswith(".hpp") or name in host_units:
            assert "policy_env.hpp" not in includes(os.path.join(CSRC, name)), name
    assert includes(os.path.join(CSRC, "k_policy_env.hip")) == ["policy_env.hpp"]
    with open(os.path.join(CSRC, "host.hpp")) as f:
        host = f.read()
    assert "launch_policy_env" in host and "launch_policy_box" in host
    with open(os.path.join(CSRC, "policy_env.hpp")) as f:
        assert not re.search(r"^\s*template\s*<", f.read(), re.M)                                          # no model templates: plugin units do not grow


def test_the_library_refuses_a_null_handle():
    from drake_ddp_amd import _capi
    lib = _capi.load()
    v = np.zeros(10)
    for which in (_capi.F_POLICY_MC_BOX, _capi.F_POLICY_MC_OBSERVE, _capi.F_POLICY_MC_ENVELOPE, _capi.F_POLICY_MC_ENVELOPE_U,
                  _capi.F_POLICY_MC_SAFETY):
        assert lib.mi_ilqr_set(None, which, _capi.ptr(v), 8) == _capi.E_BAD_ARG
        assert lib.mi_ilqr_get(None, which, _capi.ptr(v), 8) == _capi.E_BAD_ARG
