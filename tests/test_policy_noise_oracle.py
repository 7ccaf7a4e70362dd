"""The noisy policy rollouts without a device: the NumPy statement of the generator (tests/policy_noise_np.py) against Random123's
known-answer vectors, against mpmath and against the moments of a normal stream; the noisy restatement of the rollout against the
noise-free one; the two selectors in the header and the bindings; the host-side argument checks.  CPU only."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
HEADER = os.path.join(ROOT, "include", "mi_ilqr.h")

import policy_noise_np as PN  # noqa: E402


def _header():
    with open(HEADER) as f:
        return f.read()


# ---------------------------------------------------------------- Philox4x32-10
KAT = [  # Random123's kat_vectors for philox4x32 with 10 rounds: counter, key, output
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


@pytest.mark.parametrize("ctr,key,out", KAT, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(ctr, key, out):
    assert [int(w) for w in PN.philox4x32_10(ctr, key)] == out


def test_philox_is_vectorised_consistently():
    ctr = np.array([k[0] for k in KAT], dtype=np.uint64)
    key = np.array([k[1] for k in KAT], dtype=np.uint64)
    assert np.array_equal(PN.philox4x32_10(ctr, key), np.array([k[2] for k in KAT], dtype=np.uint64))


def test_the_device_header_states_the_same_cipher():
    """csrc/philox.hpp compiled for the host (the header is plain C++ there): the three vectors, and random blocks against NumPy."""
    import shutil
    import subprocess
    import tempfile
    from drake_ddp_amd import build
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or build.HIPCC      # (a .cpp file: host C++ for hipcc too)
    rng = np.random.default_rng(11)
    blocks = rng.integers(0, 2 ** 32, (64, 6), dtype=np.uint64)
    blocks[:3] = [k[0] + k[1] for k in KAT]
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "kat.cpp")
        with open(src, "w") as f:
            f.write('#include <cstdio>\n#include "%s"\nint main() {\n  unsigned c0, c1, c2, c3, k0, k1;\n'
                    '  while (std::scanf("%%u %%u %%u %%u %%u %%u", &c0, &c1, &c2, &c3, &k0, &k1) == 6) {\n'
                    '    uint32_t c[4] = {c0, c1, c2, c3};\n    mi::philox4x32_10(k0, k1, c);\n'
                    '    std::printf("%%u %%u %%u %%u\\n", c[0], c[1], c[2], c[3]);\n  }\n  return 0;\n}\n'
                    % os.path.join(ROOT, "drake_ddp_amd", "csrc", "philox.hpp"))
        exe = os.path.join(d, "kat")
        subprocess.run([cxx, "-std=c++17", "-O1", src, "-o", exe], check=True)
        text = "\n".join(" ".join(str(int(v)) for v in row) for row in blocks) + "\n"
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    got = np.array([[int(v) for v in line.split()] for line in out.splitlines()], dtype=np.uint64)
    assert np.array_equal(got, PN.philox4x32_10(blocks[:, :4], blocks[:, 4:]))
    assert [int(v) for v in got[2]] == KAT[2][2]


# ---------------------------------------------------------------- Box-Muller
def test_box_muller_against_mpmath():
    """|z - z_mp| <= 4e-14 absolute (policy_noise_np.NORMAL_TOL: its derivation) over a few thousand word pairs, the extreme
    words included."""
    import mpmath
    mpmath.mp.dps = 50
    rng = np.random.default_rng(12)
    edge = [0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1, 2 ** 30, 3 * 2 ** 30]       # (the last two: 2 pi u_b next to pi/2, 3 pi/2)
    pairs = [(a, b) for a in edge for b in edge] + [tuple(int(v) for v in p) for p in rng.integers(0, 2 ** 32, (3000, 2), dtype=np.uint64)]
    wa, wb = np.array(pairs, dtype=np.uint64).T
    z0, z1 = PN.box_muller(wa, wb)
    worst = 0.0
    for i, (a, b) in enumerate(pairs):
        ua, ub = (mpmath.mpf(a) + 0.5) / 2 ** 32, (mpmath.mpf(b) + 0.5) / 2 ** 32
        r = mpmath.sqrt(-2 * mpmath.log(ua))
        e0, e1 = abs(mpmath.mpf(float(z0[i])) - r * mpmath.cos(2 * mpmath.pi * ub)), abs(mpmath.mpf(float(z1[i])) - r * mpmath.sin(2 * mpmath.pi * ub))
        worst = max(worst, float(e0), float(e1))
        assert e0 <= PN.NORMAL_TOL and e1 <= PN.NORMAL_TOL, (a, b, float(e0), float(e1))
    print("Box-Muller vs mpmath: worst absolute error %.2e over %d pairs" % (worst, len(pairs)))
    top = np.sqrt(66 * np.log(2)) + PN.NORMAL_TOL                              # sqrt(-2 ln 2^-33), to rounding
    assert np.abs(z0).max() <= top and np.abs(z1).max() <= top
    z_top, _ = PN.box_muller(0, 2 ** 32 - 1)                                   # the largest |z| the generator can give
    assert 6.76 < abs(float(z_top)) <= top


# ---------------------------------------------------------------- the counter layout
def test_the_counter_layout():
    seed, first, b, s, t = PN.TEST_SEED, 7, 2, 5, 3
    key = [seed & 0xffffffff, seed >> 32]
    assert key[1] != 0
    zx = PN.state_normals(seed, first, False, b, s, t, 7)
    zu = PN.control_normals(seed, first, False, b, s, t, 6)
    for i in range(7):
        w = PN.philox4x32_10([first + s, t, b, i // 4], key)
        z = PN.box_muller(w[0], w[1]) + PN.box_muller(w[2], w[3])
        assert zx[i] == z[i % 4]
    for k in range(6):
        w = PN.philox4x32_10([first + s, t, b, 256 + k // 4], key)
        z = PN.box_muller(w[0], w[1]) + PN.box_muller(w[2], w[3])
        assert zu[k] == z[k % 4]
    # common: problem 0's stream for everybody; first_sample shifts the sample index; n does not change a component
    assert np.array_equal(PN.state_normals(seed, first, True, b, s, t, 7), PN.state_normals(seed, first, False, 0, s, t, 7))
    assert np.array_equal(PN.state_normals(seed, 0, False, b, first + s, t, 7), zx)
    assert np.array_equal(PN.state_normals(seed, first, False, b, s, t, 40)[:7], zx)
    ss, tt = np.arange(4)[:, None], np.arange(3)[None, :]
    grid = PN.state_normals(seed, first, False, b, ss, tt, 7)
    assert grid.shape == (4, 3, 7) and np.array_equal(grid[2, 1], PN.state_normals(seed, first, False, b, 2, 1, 7))


def test_moments_of_the_stream_the_gpu_test_uses():
    """4096 samples x 4 steps x 40 components of problem 0 under TEST_SEED, state and control stream: the reference alone stays
    inside the bounds the device is held to (tests/test_gpu_policy_noise.py)."""
    ss, tt = np.arange(4096)[:, None], np.arange(4)[None, :]
    PN.assert_moments(PN.state_normals(PN.TEST_SEED, 0, False, 0, ss, tt, 40))
    PN.assert_moments(PN.control_normals(PN.TEST_SEED, 0, False, 0, ss, tt, 16))


# ---------------------------------------------------------------- the noisy restatement
def test_zero_sigma_is_the_noise_free_rollout():
    from oracle import models_np as M
    from policy_rollout_np import rollout_sample
    from drake_ddp_amd import workloads as W
    p = W.pendulum_problem()
    N = 12
    rng = np.random.default_rng(13)
    x_bar, u_bar, K = rng.standard_normal((2, N)), rng.standard_normal((1, N - 1)), 0.3 * rng.standard_normal((1, 2, N - 1))
    model = M.Model(p["model_id"], p["dt"])
    zx, zu = rng.standard_normal((N - 1, 2)), rng.standard_normal((N - 1, 1))
    for lim in ((None, None), (np.array([-0.2]), np.array([0.3]))):
        x0 = x_bar[:, 0] + 0.1
        a = rollout_sample(model, x0, x_bar, u_bar, K, p["Q"], p["R"], p["Qf"], p["x_nom"], *lim)
        b = PN.rollout_sample_noisy(model, x0, x_bar, u_bar, K, p["Q"], p["R"], p["Qf"], p["x_nom"], np.zeros(2), np.zeros(1), zx, zu, *lim)
        assert a[0] == b[0] and a[2] == b[2] == N - 1
        assert all(np.array_equal(u, v) for u, v in zip((a[1], a[3], a[4]), (b[1], b[3], b[4])))
        c = PN.rollout_sample_noisy(model, x0, x_bar, u_bar, K, p["Q"], p["R"], p["Qf"], p["x_nom"], np.array([0.0, 1e-3]), np.array([1e-2]),
                                    zx, zu, *lim)
        assert c[0] != a[0] and np.array_equal(c[4][:, 0], a[4][:, 0])           # the first COMMANDED control saw no noise yet
        if lim[0] is not None:
            assert np.all(c[4] >= lim[0][:, None]) and np.all(c[4] <= lim[1][:, None])
        # one step by hand: the disturbance on u after the clamp, the one on x after the step
        u0 = c[4][:, 0]
        x1 = model.step_unchecked(x0, u0 + 1e-2 * zu[0]) + np.array([0.0, 1e-3]) * zx[0]
        assert np.array_equal(c[3][:, 1], x1)


# ---------------------------------------------------------------- header and bindings
def test_the_header_declares_both_selectors():
    from drake_ddp_amd import _capi
    src = _header()
    m = re.search(r"\bMI_F_POLICY_NOISE\s*=\s*(\d+),\s*/\*\s*\(B,n\+m\)", src)
    assert m and int(m.group(1)) == 19 == _capi.F_POLICY_NOISE
    m = re.search(r"\bMI_F_POLICY_STREAM\s*=\s*(\d+),\s*/\*\s*\(3,\)", src)
    assert m and int(m.group(1)) == 20 == _capi.F_POLICY_STREAM
    assert re.search(r"#define MI_ILQR_ABI_VERSION 10\b", src) and _capi.ABI_VERSION == 10
    declared = re.findall(r"^(?:int|void|const char\s*\*|size_t|double)\s*(mi_ilqr_\w+)\(", src, re.M)
    assert len(declared) == len(set(declared)) == 48 and set(declared) == set(_capi.EXPORTS)
    flat = " ".join(re.sub(r"\n\s*\*", " ", src).split())
    for phrase in ("counter = (first_sample + s, t, common ? 0 : b, j)", "key = (seed mod 2^32, seed div 2^32)",
                   "j = 256 + k / 4 for control component k", "0xD2511F53, 0xCD9E8D57", "0x9E3779B9, 0xBB67AE85",
                   "U holds the commanded controls, X the noisy states", "is not clamped again",
                   "a non-zero sigma on a padding control", "first_sample + S > 2^32: MI_ILQR_E_BAD_ARG", "mi_ilqr_set(MI_F_POLICY_NOISE, NULL, 0) clears it"):
        assert phrase in flat, phrase


def test_the_library_refuses_a_null_handle():
    from drake_ddp_amd import _capi
    lib = _capi.load()
    v = np.zeros(3)
    assert lib.mi_ilqr_abi_version() == 10
    for which in (_capi.F_POLICY_NOISE, _capi.F_POLICY_STREAM):
        assert lib.mi_ilqr_set(None, which, _capi.ptr(v), 24) == _capi.E_BAD_ARG
        assert lib.mi_ilqr_get(None, which, _capi.ptr(v), 24) == _capi.E_BAD_ARG


# ---------------------------------------------------------------- argument checks
def test_check_noise_args():
    from drake_ddp_amd.ilqr import check_noise_args as chk
    B, n, m = 3, 4, 2
    rows, stream = chk(None, None, 0, 0, False, B, n, m)
    assert rows is None and np.array_equal(stream, [0.0, 0.0, 0.0]) and stream.dtype == np.float64
    rows, stream = chk(0.5, None, 7, 9, True, B, n, m)
    assert rows.shape == (B, n + m) and rows.flags["C_CONTIGUOUS"] and rows.dtype == np.float64
    assert np.all(rows[:, :n] == 0.5) and np.all(rows[:, n:] == 0.0) and np.array_equal(stream, [7.0, 9.0, 1.0])
    rows, _ = chk([0.0, 1.0, 2.0, 3.0], np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]), 0, 0, False, B, n, m, m_dev=4)
    assert rows.shape == (B, n + 4) and np.array_equal(rows[1], [0.0, 1.0, 2.0, 3.0, 3.0, 4.0, 0.0, 0.0])      # padded with zeros
    rows, _ = chk(None, 2.0, 0, 0, False, B, n, m, m_dev=4)
    assert np.array_equal(rows[0], [0, 0, 0, 0, 2.0, 2.0, 0, 0])
    rows, stream = chk(np.zeros((B, n)), None, 2 ** 53 - 1, 2 ** 32 - 1, False, B, n, m, S=1)                   # the largest of each
    assert stream[0] == 2.0 ** 53 - 1 and stream[1] == 2.0 ** 32 - 1
    assert chk(1.0, None, np.int64(5), 3.0, 0, B, n, m)[1].tolist() == [5.0, 3.0, 0.0]                          # integer-valued numbers
    for bad in (np.zeros(n + 1), np.zeros((B, n + 1)), np.zeros((B + 1, n)), np.zeros((1, n)), np.zeros((B, n, 1)), "x"):
        with pytest.raises(ValueError, match="state_noise"):
            chk(bad, None, 0, 0, False, B, n, m)
    for bad in (np.zeros(m + 1), np.zeros((B, 4)), np.zeros((B + 1, m))):                                       # (user width, not the device's)
        with pytest.raises(ValueError, match="control_noise"):
            chk(None, bad, 0, 0, False, B, n, m, m_dev=4)
    for v in (-1e-300, -1.0, np.nan, np.inf, -np.inf):
        for args in ((v, None), (None, v), (np.array([0.0, 0.0, v, 0.0]), None), (1.0, np.array([[0.0, 0.0], [0.0, v], [0.0, 0.0]]))):
            with pytest.raises(ValueError, match="negative|NaN or infinity"):
                chk(args[0], args[1], 0, 0, False, B, n, m)
    for seed in (-1, 2 ** 53, 1.5, np.nan, np.inf, "7", None, True):
        with pytest.raises(ValueError, match="seed"):
            chk(1.0, None, seed, 0, False, B, n, m)
    for first in (-1, 2 ** 32, 0.5, np.nan, "0", None):
        with pytest.raises(ValueError, match="first_sample"):
            chk(1.0, None, 0, first, False, B, n, m)
    with pytest.raises(ValueError, match="first_sample"):
        chk(1.0, None, 0, 2 ** 32 - 4, False, B, n, m, S=5)
    assert chk(1.0, None, 0, 2 ** 32 - 4, False, B, n, m, S=4)[0] is not None


def test_the_methods_raise_before_they_touch_a_handle():
    """On objects that have no handle at all (no device, no library call can have happened)."""
    import inspect
    from drake_ddp_amd import ilqr

    class _System:
        params = np.array([0.25, 0.1, 4.905])

    for cls, B in ((ilqr.BatchedIterativeLQR, 3), (ilqr.IterativeLinearQuadraticRegulator, 1)):
        sig = inspect.signature(cls.RolloutPolicy)
        assert list(sig.parameters)[:4] == ["self", "x0", "params", "trajectories"]                 # the positional calls keep working
        for kw, default in (("state_noise", None), ("control_noise", None), ("seed", 0), ("first_sample", 0), ("common_noise", False)):
            assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[kw].default == default
        s = object.__new__(cls)
        s.B, s.n, s.m, s.N, s.system, s._md = B, 2, 1, 10, _System(), 1                             # no _h, no _lib
        x0 = np.zeros((4, 2))
        for kw in (dict(state_noise=-1.0), dict(state_noise=np.zeros(3)), dict(control_noise=np.nan), dict(control_noise=np.zeros((B, 2))),
                   dict(state_noise=1.0, seed=-1), dict(state_noise=1.0, seed=2 ** 53), dict(state_noise=1.0, first_sample=2 ** 32),
                   dict(state_noise=1.0, first_sample=2 ** 32 - 3), dict(control_noise=1.0, seed=0.5)):
            with pytest.raises(ValueError):
                s.RolloutPolicy(x0, None, False, **kw)
        with pytest.raises(ValueError):                                                             # the x0 check still comes first
            s.RolloutPolicy(np.zeros(2), state_noise=1.0)
