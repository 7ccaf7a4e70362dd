"""Sampling-based MPC without a device: the sampling form of MI_F_SEEDS_RUN as the header states it (and the two older forms'
comments as they were), the bindings, the layering of the new kernel header, the argument checks
(drake_ddp_amd.ilqr.check_mppi_args) and the NumPy statement (tests/mppi_np.py) against closed forms.  CPU only."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HEADER = os.path.join(ROOT, "include", "mi_ilqr.h")
CSRC = os.path.join(ROOT, "drake_ddp_amd", "csrc")

import mppi_np as MP  # noqa: E402
import policy_noise_np as PN  # noqa: E402
import seeds_np as SN  # noqa: E402


def _header():
    with open(HEADER) as f:
        return f.read()


def test_the_header_states_the_sampling_form():
    src = _header()
    flat = " ".join(re.sub(r"\n\s*\*", " ", src).split())
    for phrase in ("---- Sampling-based MPC (ABI 10; the SAMPLING FORM of MI_F_SEEDS_RUN, 10 doubles, no new selector, no new entry point)",
                   "mi_ilqr_set(MI_F_SEEDS_RUN, v, 80)",
                   "v = S | op | seed | first_sample | hold | reserved = 0 | iterations | shift | temperature | reserved = 0",
                   "op must be RESEED (2), as in the long form", "first_sample + iterations S <= 2^32", "shift in [0, N - 2]",
                   "temperature >= 0 and no NaN", "88 bytes and more stay MI_ILQR_E_BAD_SHAPE", "A refused command changes nothing",
                   "the pending guess, else u_bar, else zeros", "counter = (g, t div hold, b, 1024 + k / 4), Box-Muller normal k mod 4 of the block",
                   "g = first_sample + i S + s the GLOBAL SAMPLE NUMBER", "z does not depend on S, on B, on the launch or on the layout",
                   "SAMPLE 0 IS THE ELITE SLOT", "a rounded product, the sum a rounded sum (no FMA)", "on the APPLIED control v",
                   "ties to the lowest s", "temperature = 0 is the indicator of the argmin", "skipped, not multiplied by zero",
                   "SEQUENTIALLY IN s = 0, 1, .. S - 1, an order that is a function of S alone", "A problem without a finite sample keeps u",
                   "no finite sample: -1 | +inf | 0", "u_guess[t] = u[min(t + shift, N-2)]",
                   "mi_ilqr_get(MI_F_SEEDS_BEST, dst, I*B*3*8)", "mi_ilqr_get(MI_F_SEEDS_COST, dst, (I+1)*B*2*8)",
                   "mi_ilqr_get(MI_F_SEEDS_U_BAR, dst, B*m*(N-1)*8)", "one call of I iterations is bitwise I calls of one iteration",
                   "nothing of size S (N-1) is ever stored"):
        assert phrase in flat, phrase
    # the selector's comment: the two older forms as they were, the sampling form behind the long form's words
    assert re.search(r"MI_F_SEEDS_RUN\s*=\s*39,\s*/\*\s*\(6,\) write-only COMMAND: K \| op \| seed \| round \| hold \| reserved = 0", src)
    assert re.search(r"MI_F_SEEDS_RUN\s*=\s*39,\s*/\*\s*\(6,\) write-only COMMAND: K \| op \| seed \| round \| hold \| reserved = 0.*\(8,\): the long form"
                     r".*\(10,\): the sampling form", src)
    assert re.search(r"MI_F_SEEDS_BEST\s*=\s*40,\s*/\*\s*\(G,3\) read-only.*\(R\+1,G,3\) after a long-form run", src)
    assert re.search(r"#define MI_ILQR_ABI_VERSION 10\b", src)
    sel = {k: int(v) for k, v in re.findall(r"\b(MI_F_\w+)\s*=\s*(\d+)", src)}
    assert max(sel.values()) == 44
    declared = re.findall(r"^(?:int|void|const char\s*\*|size_t|double)\s*(mi_ilqr_\w+)\(", src, re.M)
    assert len(declared) == len(set(declared)) == 48


def test_the_bindings_and_the_kernel_units():
    from drake_ddp_amd import _capi, build, plugin
    from drake_ddp_amd.ilqr import BatchedIterativeLQR, IterativeLinearQuadraticRegulator, MPPIResult
    assert (_capi.SEEDS_RUN_DOUBLES, _capi.SEEDS_MPC_RUN_DOUBLES, _capi.SEEDS_MPPI_RUN_DOUBLES, _capi.SEEDS_RESEED) == (6, 8, 10, 2)
    assert _capi.ABI_VERSION == 10 and len(_capi.EXPORTS) == 48
    assert callable(BatchedIterativeLQR.MPPIRun) and IterativeLinearQuadraticRegulator.MPPIRun is BatchedIterativeLQR.MPPIRun
    assert MPPIResult.__slots__ == ("u", "best_sample", "best_cost", "finite", "ess", "nominal_cost", "kernel_ms")

    def includes(name):
        with open(os.path.join(CSRC, name)) as f:
            return re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M)
    # mppi.hpp includes what policy_rollout.hpp includes, plus wave_ops.hpp - and not seeds.hpp
    assert sorted(includes("mppi.hpp")) == sorted(includes("policy_rollout.hpp") + ["wave_ops.hpp"])
    assert includes("k_mppi.hip") == ["mppi.hpp"] and includes("h_mppi.hip") == ["host_internal.hpp"]
    host_units = {os.path.basename(s) for s in build.host_sources()}
    assert "h_mppi.hip" in host_units and "k_mppi.hip" not in host_units
    for name in os.listdir(CSRC):
        if name.endswith(".hpp") or name in host_units:
            assert "mppi.hpp" not in includes(name), name
    # the kernels without a model live in the unit, not in the header a plugin unit includes
    with open(os.path.join(CSRC, "mppi.hpp")) as f:
        assert "mppi_update_kernel(mi_host::MppiUpdateArgs" not in f.read()
    with open(os.path.join(CSRC, "host.hpp")) as f:
        host = f.read()
    assert "struct MppiArgs" in host and "struct MppiUpdateArgs" in host and "kModeSampledRollout" in host
    with open(os.path.join(CSRC, "kernel_args.hpp")) as f:
        assert "mppi" not in f.read().lower()                                  # (KArgs is what it was)
    for family in ("small", "large"):
        assert '#include "mppi.hpp"' in plugin.source("t", 2, 1, "xn[0] = x[0]; xn[1] = x[1] + dt * u[0];", [], family)


# ---------------------------------------------------------------- check_mppi_args
def test_check_mppi_args_accepts():
    from drake_ddp_amd.ilqr import check_mppi_args as chk
    B, m, N = 6, 3, 12
    S, I, rows, T, seed, first, hold, shift = chk(70, 3, B, m, N, 0.5, 1.0)
    assert (S, I, T, seed, first, hold, shift) == (70, 3, 1.0, 0, 0, 1, 0) and isinstance(T, float)
    assert rows.shape == (B, m) and rows.dtype == np.float64 and rows.flags["C_CONTIGUOUS"] and np.all(rows == 0.5)
    S, I, rows, T, seed, first, hold, shift = chk(np.int64(1), 2.0, B, m, N, [0.1, 0.0, 0.3], 0, seed=2 ** 53 - 1, first_sample=2 ** 32 - 2,
                                                  hold=7, shift=N - 2, m_dev=4)
    assert (S, I, T, seed, first, hold, shift) == (1, 2, 0.0, 2 ** 53 - 1, 2 ** 32 - 2, 7, N - 2)
    assert rows.shape == (B, 4) and np.array_equal(rows[5], [0.1, 0.0, 0.3, 0.0])              # the padding control: zero
    per = np.arange(B * m, dtype=float).reshape(B, m)
    assert np.array_equal(chk(2 ** 31 - 64, 1, B, m, N, per, np.inf)[2], per)                  # the largest S: whole waves fit 32 bits
    assert chk(2 ** 16, 2 ** 16, B, m, N, 0.0, 1e-300)[:2] == (2 ** 16, 2 ** 16)                # first_sample + I S = 2^32: the last that fits


def test_check_mppi_args_refuses():
    from drake_ddp_amd.ilqr import check_mppi_args as chk
    B, m, N = 6, 3, 12
    for bad in (0, -1, 1.5, True, None, "4", np.nan, 2 ** 31, 2 ** 31 - 63):
        with pytest.raises(ValueError, match="MPPIRun: S must be"):
            chk(bad, 3, B, m, N, 0.1, 1.0)
    for bad in (0, -1, 1.5, True, None, "4", np.nan, 2 ** 31):
        with pytest.raises(ValueError, match="MPPIRun: iterations must be"):
            chk(8, bad, B, m, N, 0.1, 1.0)
    for bad in (0, -3, 0.5, False, None, 2 ** 31):
        with pytest.raises(ValueError, match="MPPIRun: hold must be"):
            chk(8, 3, B, m, N, 0.1, 1.0, hold=bad)
    for bad in (-1, 2 ** 53, 1.5, "0"):
        with pytest.raises(ValueError, match="MPPIRun: seed must be"):
            chk(8, 3, B, m, N, 0.1, 1.0, seed=bad)
    for bad in (-1, 2 ** 32, 0.25, None):
        with pytest.raises(ValueError, match="MPPIRun: first_sample must be"):
            chk(8, 3, B, m, N, 0.1, 1.0, first_sample=bad)
    with pytest.raises(ValueError, match="first_sample \\+ iterations S"):
        chk(2 ** 16, 2 ** 16, B, m, N, 0.1, 1.0, first_sample=1)
    for bad in (-1, N - 1, N, 1.5, True, None):
        with pytest.raises(ValueError, match="MPPIRun: shift must be"):
            chk(8, 3, B, m, N, 0.1, 1.0, shift=bad)
    for bad in (-1e-300, -1, np.nan, None, "1", True, -np.inf):
        with pytest.raises(ValueError, match="MPPIRun: temperature must be"):
            chk(8, 3, B, m, N, 0.1, bad)
    with pytest.raises(ValueError, match="MPPIRun: sigma_u is required"):
        chk(8, 3, B, m, N, None, 1.0)
    for bad in (np.zeros(2), np.zeros((B, 2)), np.zeros((B + 1, m)), "x"):
        with pytest.raises(ValueError, match="MPPIRun: sigma_u"):
            chk(8, 3, B, m, N, bad, 1.0)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="NaN"):
            chk(8, 3, B, m, N, [0.1, bad, 0.1], 1.0)
    with pytest.raises(ValueError, match="negative"):
        chk(8, 3, B, m, N, [0.1, -1e-300, 0.1], 1.0)


def test_the_method_checks_its_arguments_first():
    import types
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    s = types.SimpleNamespace(B=6, m=3, n=4, N=12, _md=3)                    # (no handle: a call that got past the checks would fail on it)
    with pytest.raises(ValueError, match="MPPIRun: S must be"):
        BatchedIterativeLQR.MPPIRun(s, 0, 3, 0.1, 1.0)
    with pytest.raises(ValueError, match="MPPIRun: temperature must be"):
        BatchedIterativeLQR.MPPIRun(s, 8, 3, 0.1, -1.0)
    with pytest.raises(AttributeError):
        BatchedIterativeLQR.MPPIRun(s, 8, 3, 0.1, 1.0)


# ---------------------------------------------------------------- the NumPy statement
def test_the_normals_are_the_new_blocks_of_the_same_generator():
    """Block 1024 + k / 4 at counter (g, t div hold, b, .): the seeds' stream (block 768 + j / 4, counter (round, t div hold, b, .))
    moved by 256 blocks - checked against the Philox restatement directly - and a function of (seed, g, t div hold, b, k) alone."""
    seed, b, m, steps = PN.TEST_SEED, 3, 7, 11
    g = np.array([0, 5, 2 ** 32 - 1])
    z = MP.normals(seed, g, b, steps, m, hold=5)
    assert z.shape == (3, m, steps)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    for gi, gv in enumerate(g):
        for t in (0, 4, 5, 10):
            for k in range(m):
                w = PN.philox4x32_10(np.array([gv, t // 5, b, 1024 + k // 4], dtype=np.uint64), key)
                pair = PN.box_muller(w[2], w[3]) if k & 2 else PN.box_muller(w[0], w[1])
                assert z[gi, k, t] == pair[k & 1], (gv, t, k)
    assert np.array_equal(z[:, :, 0], z[:, :, 4]) and np.array_equal(z[:, :, 5], z[:, :, 9]) and not np.array_equal(z[:, :, 4], z[:, :, 5])
    assert np.array_equal(MP.normals(seed, [5], b, steps, m, 5)[0], z[1])                      # not on the other samples of the call
    assert np.array_equal(MP.normals(seed, g, b, steps, 3, 5), z[:, :3])                       # ... nor on m
    assert not np.array_equal(MP.normals(seed, g, b + 1, steps, m, 5), z)
    assert not np.array_equal(SN.normals(seed, 5, b, steps, m, 5), z[1])                       # the seeds' blocks are others


class _Integrator:
    """x+ = x + dt u, n = m: the oracle's model interface."""
    model_id, params = -1, np.zeros(0)

    def __init__(self, dt=0.1):
        self.dt = dt

    def step_unchecked(self, x, u):
        return x + self.dt * u


def _problem(B=3, m=2, N=6, seed=0):
    rng = np.random.default_rng(seed)
    return dict(models=[_Integrator() for _ in range(B)], x0=rng.standard_normal((B, m)), u=rng.uniform(-1.0, 1.0, (B, m, N - 1)),
                sigma=np.full((B, m), 0.5), Q=np.eye(m), R=0.1 * np.eye(m), Qf=5.0 * np.eye(m), x_nom=np.zeros(m))


def test_one_sample_leaves_the_plan_alone():
    p = _problem()
    r = MP.run(S=1, iterations=2, temperature=1.0, seed=3, **p)
    assert np.array_equal(r["u"], p["u"]) and np.all(r["ess"] == 1.0) and np.all(r["best_sample"] == 0) and np.all(r["finite"] == 1)
    assert np.array_equal(r["nominal_cost"][0], r["nominal_cost"][2]) and np.array_equal(r["best_cost"], r["nominal_cost"][:2])
    for b in range(3):                                                                         # the cost is the closed form's
        x, L = p["x0"][b].copy(), 0.0
        for t in range(5):
            L += x @ x + 0.1 * p["u"][b, :, t] @ p["u"][b, :, t]
            x = x + 0.1 * p["u"][b, :, t]
        assert abs(r["nominal_cost"][0, b] - (L + 5.0 * x @ x)) <= 1e-12 * abs(L)


def test_equal_costs_give_the_plain_mean():
    """Zero cost matrices: every sample costs 0, every weight is 1 / S, ESS = S, and the update is the sequential mean of the applied
    controls, the elite's included."""
    p = _problem()
    p.update(Q=np.zeros((2, 2)), R=np.zeros((2, 2)), Qf=np.zeros((2, 2)))
    S = 8                                                                                       # (a power of two: 1 / S is exact)
    r = MP.run(S=S, iterations=1, temperature=0.7, seed=11, hold=2, **p)
    assert np.all(r["ess"] == S) and np.all(r["best_sample"] == 0) and np.all(r["best_cost"] == 0.0) and np.all(r["finite"] == S)
    for b in range(3):
        v = MP.applied(p["u"][b], p["sigma"][b], MP.normals(11, np.arange(S), b, 5, 2, 2))
        assert np.array_equal(v[0], p["u"][b])
        assert np.allclose(r["u"][b], v.mean(axis=0), rtol=0.0, atol=4e-16 * np.abs(v).max())
        acc = v[0] / S
        for s in range(1, S):
            acc = acc + v[s] / S
        assert np.array_equal(r["u"][b], acc)                                                   # the documented order, bit for bit


def test_temperature_zero_takes_the_best_sample():
    p = _problem(seed=1)
    lo, hi = np.full((3, 2), -0.8), np.full((3, 2), 0.9)
    r = MP.run(S=20, iterations=3, temperature=0.0, seed=5, shift=2, u_min=lo, u_max=hi, **p)
    assert np.all(r["ess"] == 1.0)
    assert np.array_equal(r["nominal_cost"][1:], r["best_cost"])                               # the cost never rises
    assert np.all(np.diff(r["nominal_cost"], axis=0) <= 0.0) and np.any(np.diff(r["nominal_cost"], axis=0) < 0.0)
    u = p["u"].copy()
    for i in range(3):
        for b in range(3):
            v = MP.applied(u[b], p["sigma"][b], MP.normals(5, i * 20 + np.arange(20), b, 5, 2), lo[b], hi[b])
            u[b] = v[r["best_sample"][i, b]]
    assert np.array_equal(r["u"], u) and np.all(r["u"] >= -0.8) and np.all(r["u"] <= 0.9)
    assert np.array_equal(r["u_guess"][:, :, :3], r["u"][:, :, 2:]) and np.array_equal(r["u_guess"][:, :, 3:], np.repeat(r["u"][:, :, -1:], 2, axis=2))


def test_dead_samples_are_skipped_and_splitting_is_exact():
    p = _problem(seed=2)
    p["sigma"] = np.array([[0.5, 0.5], [1e200, 1e200], [0.5, 0.0]])
    p["x0"][2, 0] = np.nan
    r = MP.run(S=9, iterations=2, temperature=2.0, seed=9, **p)
    assert r["finite"][:, 1].tolist() == [1, 1] and np.array_equal(r["u"][1], p["u"][1]) and np.all(r["ess"][:, 1] == 1.0)
    assert r["best_sample"][:, 2].tolist() == [-1, -1] and np.all(r["best_cost"][:, 2] == np.inf) and r["finite"][:, 2].tolist() == [0, 0]
    assert np.isnan(r["ess"][:, 2]).all() and np.array_equal(r["u"][2], p["u"][2]) and np.all(r["nominal_cost"][:, 2] == np.inf)
    assert np.all(r["finite"][:, 0] == 9) and np.all((r["ess"][:, 0] > 1.0) & (r["ess"][:, 0] <= 9.0))
    one = MP.run(S=9, iterations=1, temperature=2.0, seed=9, **p)
    two = MP.run(S=9, iterations=1, temperature=2.0, seed=9, first_sample=9, **dict(p, u=one["u"]))
    assert np.array_equal(two["u"], r["u"]) and np.array_equal(two["best_cost"][0], r["best_cost"][1])
