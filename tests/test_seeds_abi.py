"""The multi-start interface without a device: the seven selectors in the header and the bindings, the rules the header states, the
unchanged entry-point list and ABI version, the layering of the new kernel header, and the host-side argument checks
(drake_ddp_amd.ilqr.check_seed_args).  CPU only."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HEADER = os.path.join(ROOT, "include", "mi_ilqr.h")
CSRC = os.path.join(ROOT, "drake_ddp_amd", "csrc")

WANT = {"MI_F_SEEDS_SIGMA": 38, "MI_F_SEEDS_RUN": 39, "MI_F_SEEDS_BEST": 40, "MI_F_SEEDS_X_BAR": 41, "MI_F_SEEDS_U_BAR": 42,
        "MI_F_SEEDS_COST": 43, "MI_F_SEEDS_KERNEL_MS": 44}


def _header():
    with open(HEADER) as f:
        return f.read()


def test_the_seven_selectors_and_nothing_else_changed():
    from drake_ddp_amd import _capi
    src = _header()
    sel = {k: int(v) for k, v in re.findall(r"\b(MI_(?:F|I|I64)_\w+)\s*=\s*(\d+)", src)}
    for name, value in WANT.items():
        assert sel[name] == value == getattr(_capi, name[3:]), name
        assert [k for k, v in sel.items() if v == value] == [name]                   # no other selector's value
    assert len(set(sel.values())) == len(sel)
    assert sel["MI_F_POLICY_MC_SAFETY"] == 37 and max(v for k, v in sel.items() if k.startswith("MI_F_")) == 44   # appended behind it
    assert (_capi.SEEDS_PERTURB, _capi.SEEDS_SELECT, _capi.SEEDS_RESEED, _capi.SEEDS_GATHER) == (0, 1, 2, 3)
    assert re.search(r"MI_F_SEEDS_RUN\s*=\s*39,\s*/\*\s*\(6,\) write-only COMMAND: K \| op \| seed \| round \| hold \| reserved = 0", src)
    assert re.search(r"MI_F_SEEDS_BEST\s*=\s*40,\s*/\*\s*\(G,3\) read-only", src)
    assert re.search(r"#define MI_ILQR_ABI_VERSION 10\b", src) and _capi.ABI_VERSION == 10
    declared = re.findall(r"^(?:int|void|const char\s*\*|size_t|double)\s*(mi_ilqr_\w+)\(", src, re.M)
    assert len(declared) == len(set(declared)) == 48 and set(declared) == set(_capi.EXPORTS)


def test_the_header_states_the_rules():
    flat = " ".join(re.sub(r"\n\s*\*", " ", _header()).split())
    for phrase in ("---- Multi-start (ABI 10", "G = B / K SEED GROUPS of K consecutive problems", "group g holds problems g K .. g K + K - 1",
                   "member 0, the ELITE slot, gets base unchanged", "the pending guess, else u_bar, else zeros",
                   "counter = (round, t div hold, b, 768 + j / 4), Box-Muller normal j mod 4 of the block",
                   "not on K, not on the launch, not on the layout", "hold >= 1 keeps the disturbance constant over `hold` steps",
                   "a rounded product, the sum a rounded sum (no FMA)", "The result is not clamped", "cold, the guess pending",
                   "MI_STATUS_FLAG_INDEFINITE masked off is MI_STATUS_CONVERGED or MI_STATUS_MAX_ITERS and its cost is finite",
                   "ties go to the lowest index", "no eligible member: -1 | +inf | 0", "the winner's slot gets its own u_bar unperturbed",
                   "non-finite entries read as 0", "a group without a winner: NaN rows, +inf",
                   "a solve after them is bitwise the solve without them", "zero on padding controls",
                   "K not dividing B, an unknown op, hold < 1", "MI_ILQR_E_UNSUPPORTED", "A refused command changes nothing",
                   "before any: MI_ILQR_E_BAD_ARG", "nothing of size B m (N-1) crosses the bus"):
        assert phrase in flat, phrase


def test_the_kernel_header_keeps_the_layering():
    """seeds.hpp knows no model: it includes host.hpp, philox.hpp and wave_ops.hpp alone; no other header and nothing of the host
    includes it; its unit does.  The host reaches the launcher through host.hpp; h_seeds.hip is a host unit."""
    def includes(path):
        with open(path) as f:
            return re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M)
    assert includes(os.path.join(CSRC, "seeds.hpp")) == ["host.hpp", "philox.hpp", "wave_ops.hpp"]
    from drake_ddp_amd import build
    host_units = {os.path.basename(s) for s in build.host_sources()}
    assert {"mi_ilqr.hip", "h_policy.hip", "h_seeds.hip"} <= host_units and "k_seeds.hip" not in host_units
    for name in os.listdir(CSRC):
        if name.endswith(".hpp") or name in host_units:
            assert "seeds.hpp" not in includes(os.path.join(CSRC, name)), name
    assert includes(os.path.join(CSRC, "k_seeds.hip")) == ["seeds.hpp"]
    assert includes(os.path.join(CSRC, "h_seeds.hip")) == ["host_internal.hpp"]
    with open(os.path.join(CSRC, "host.hpp")) as f:
        host = f.read()
    assert "struct SeedsArgs" in host and "launch_seeds" in host
    with open(os.path.join(CSRC, "kernel_args.hpp")) as f:
        assert "seeds" not in f.read().lower()                               # (KArgs is what it was)


# ---------------------------------------------------------------- check_seed_args
def test_check_seed_args_accepts():
    from drake_ddp_amd.ilqr import check_seed_args as chk
    B, m = 12, 3
    K, rows, seed, rnd, hold = chk(4, B, m, 0.5)
    assert (K, seed, rnd, hold) == (4, 0, 0, 1) and rows.shape == (B, m) and rows.dtype == np.float64 and rows.flags["C_CONTIGUOUS"]
    assert np.all(rows == 0.5)
    K, rows, seed, rnd, hold = chk(np.int64(3), B, m, [0.1, 0.0, 0.3], seed=2 ** 53 - 1, round=2 ** 32 - 1, hold=7, m_dev=4)
    assert (K, seed, rnd, hold) == (3, 2 ** 53 - 1, 2 ** 32 - 1, 7) and rows.shape == (B, 4)
    assert np.array_equal(rows[5], [0.1, 0.0, 0.3, 0.0])                   # the padding control: zero
    per = np.arange(B * m, dtype=float).reshape(B, m)
    assert np.array_equal(chk(12, B, m, per)[1], per) and chk(1, B, m, per)[0] == 1
    assert chk(6.0, B, m)[:2] == (6, None)                                   # SelectBest / GatherBest: no sigma


def test_check_seed_args_refuses():
    from drake_ddp_amd.ilqr import check_seed_args as chk
    B, m = 12, 3
    for bad in (0, -1, 1.5, True, None, "4", np.nan, 2 ** 31):
        with pytest.raises(ValueError, match="K must be"):
            chk(bad, B, m, 0.1)
    for bad in (5, 7, 8, 24):
        with pytest.raises(ValueError, match="K must divide"):
            chk(bad, B, m, 0.1)
    for bad in (0, -3, 0.5, False, None, 2 ** 31):
        with pytest.raises(ValueError, match="hold must be"):
            chk(4, B, m, 0.1, hold=bad)
    for bad in (-1, 2 ** 53, 1.5, "0"):
        with pytest.raises(ValueError, match="seed must be"):
            chk(4, B, m, 0.1, seed=bad)
    for bad in (-1, 2 ** 32, 0.25):
        with pytest.raises(ValueError, match="round must be"):
            chk(4, B, m, 0.1, round=bad)
    for bad in (np.zeros(2), np.zeros((B, 2)), np.zeros((B + 1, m)), np.zeros((1, m)), "x"):
        with pytest.raises(ValueError, match="sigma_u"):
            chk(4, B, m, bad)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="NaN|negative"):
            chk(4, B, m, [0.1, bad, 0.1])
    with pytest.raises(ValueError, match="negative"):
        chk(4, B, m, [0.1, -1e-300, 0.1])
    with pytest.raises(ValueError, match="GatherBest: K must divide"):
        chk(5, B, m, what="GatherBest")


def test_the_library_refuses_a_null_handle():
    from drake_ddp_amd import _capi
    lib = _capi.load()
    v = np.zeros(6)
    for name in WANT:
        which = getattr(_capi, name[3:])
        assert lib.mi_ilqr_set(None, which, _capi.ptr(v), 48) == _capi.E_BAD_ARG
        assert lib.mi_ilqr_get(None, which, _capi.ptr(v), 48) == _capi.E_BAD_ARG
