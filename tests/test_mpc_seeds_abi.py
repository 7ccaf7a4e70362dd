"""Multi-start in the receding-horizon loop without a device: the long form of MI_F_SEEDS_RUN as the header states it, the bindings,
the argument checks of BatchedIterativeLQR.MPCRunMultiStart (they raise before anything reaches the library), mpc_winner_log, and the
NumPy statement of the join (tests/mpc_seeds_np.py) against seeds_np.reseed applied to the shifted plans.  CPU only."""
import os
import re
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HEADER = os.path.join(ROOT, "include", "mi_ilqr.h")
CSRC = os.path.join(ROOT, "drake_ddp_amd", "csrc")

import mpc_seeds_np as MS  # noqa: E402
import seeds_np as SN  # noqa: E402


def test_the_header_states_the_long_form():
    with open(HEADER) as f:
        src = f.read()
    flat = " ".join(re.sub(r"\n\s*\*", " ", src).split())
    for phrase in ("---- Multi-start in the receding-horizon loop (ABI 10; the LONG FORM of MI_F_SEEDS_RUN, no new selector, no new entry point)",
                   "mi_ilqr_set(MI_F_SEEDS_RUN, v, 64)", "v = K | op | seed | round | hold | reserved = 0 | num_resolves | replan_steps",
                   "op must be RESEED (2)", "num_resolves >= 1", "1 <= replan_steps < N - 1", "The 48-byte form is what it was",
                   "every other `bytes`: MI_ILQR_E_BAD_SHAPE", "The handle must hold a solve", "A refused command changes nothing",
                   "x0[gK+k] <- x_bar[gK+w][:, r]", "u_guess[gK+k][j,t] <- u_bar[gK+w][j, min(t + r, N-2)]",
                   "z(seed, round + i, gK+k, t div hold, j) for k != w", "applied in that order",
                   "get the shifted value bit for bit", "a rounded product, the sum a rounded sum (no FMA)",
                   "each member's own shifted plan with non-finite entries read as 0, member 0 unperturbed, each member's own x_bar[:, r]",
                   "its `dead` flag of the MPC log is cleared", "The long form carries no shared target_step",
                   "mi_ilqr_get(MI_F_SEEDS_BEST, dst, (R+1)*G*3*8)", "the join kernels' own events, summed over the run",
                   "leaves the reference's clock where it was", "mi_ilqr_mpc_run itself, in both forms, is untouched",
                   "for K = 1 every member continues its own plan and the loop is bitwise mi_ilqr_mpc_shift + mi_ilqr_solve"):
        assert phrase in flat, phrase
    assert re.search(r"MI_F_SEEDS_RUN\s*=\s*39,\s*/\*\s*\(6,\) write-only COMMAND: K \| op \| seed \| round \| hold \| reserved = 0.*\(8,\): the long form", src)
    assert re.search(r"MI_F_SEEDS_BEST\s*=\s*40,\s*/\*\s*\(G,3\) read-only.*\(R\+1,G,3\) after a long-form run", src)


def test_the_bindings_and_the_kernel_unit():
    from drake_ddp_amd import _capi
    from drake_ddp_amd.ilqr import BatchedIterativeLQR, IterativeLinearQuadraticRegulator
    assert (_capi.SEEDS_RUN_DOUBLES, _capi.SEEDS_MPC_RUN_DOUBLES, _capi.SEEDS_RESEED) == (6, 8, 2)
    assert callable(BatchedIterativeLQR.MPCRunMultiStart) and callable(BatchedIterativeLQR.mpc_winner_log)
    assert IterativeLinearQuadraticRegulator.MPCRunMultiStart is BatchedIterativeLQR.MPCRunMultiStart      # (nothing of its own)
    with open(os.path.join(CSRC, "seeds.hpp")) as f:
        src = f.read()
    assert "seeds_mpc_join_kernel(SeedsJoinArgs a)" in src and src.count("__global__") == 2
    assert src.count("seeds_select(") == 3                                   # one definition, the two kernels call it
    with open(os.path.join(CSRC, "host.hpp")) as f:
        host = f.read()
    assert "struct SeedsJoinArgs" in host and "launch_seeds_mpc_join" in host


def _fake(B=12, m=3, n=4, N=10, md=None):
    return types.SimpleNamespace(B=B, m=m, n=n, N=N, _md=m if md is None else md)


def test_the_method_checks_its_arguments_first():
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    run = BatchedIterativeLQR.MPCRunMultiStart
    s = _fake()                                                              # (no handle: a call that got past the checks would fail on it)
    for bad in (0, -1, 1.5, True, None, 2 ** 31):
        with pytest.raises(ValueError, match="MPCRunMultiStart: K must be"):
            run(s, bad, 2, 1, 0.1)
    with pytest.raises(ValueError, match="MPCRunMultiStart: K must divide"):
        run(s, 5, 2, 1, 0.1)
    with pytest.raises(ValueError, match="MPCRunMultiStart: sigma_u is required"):
        run(s, 4, 2, 1, None)
    with pytest.raises(ValueError, match="MPCRunMultiStart: negative"):
        run(s, 4, 2, 1, -0.1)
    for bad in (0, -2, 1.0, True, None, 2 ** 31):
        with pytest.raises(ValueError, match="MPCRunMultiStart: num_resolves must be"):
            run(s, 4, bad, 1, 0.1)
    for bad in (0, 9, 10, 2.0, False, None):                                 # 1 <= replan_steps < N - 1 = 9
        with pytest.raises(ValueError, match="MPCRunMultiStart: replan_steps must be"):
            run(s, 4, 2, bad, 0.1)
    with pytest.raises(ValueError, match="MPCRunMultiStart: hold must be"):
        run(s, 4, 2, 1, 0.1, hold=0)
    with pytest.raises(ValueError, match="MPCRunMultiStart: seed must be"):
        run(s, 4, 2, 1, 0.1, seed=-1)
    with pytest.raises(ValueError, match="MPCRunMultiStart: round must be"):
        run(s, 4, 2, 1, 0.1, round=2 ** 32)
    with pytest.raises(ValueError, match="round \\+ num_resolves"):
        run(s, 4, 3, 1, 0.1, round=2 ** 32 - 2)
    with pytest.raises(AttributeError):                                      # valid arguments: the first thing after the checks is the handle
        run(s, 4, 3, 8, 0.1, round=2 ** 32 - 3)


def test_mpc_winner_log():
    from drake_ddp_amd.ilqr import BatchedIterativeLQR, SeedSelection
    G, K, R, n = 3, 2, 2, 2
    log = np.arange(G * K * R * (n + 2), dtype=float).reshape(G * K, R, n + 2)
    s = types.SimpleNamespace(mpc_log=log, _mpc_resolves=R, n=n)
    sel = [SeedSelection(K, np.array(w), np.zeros(G), np.ones(G, dtype=np.int64)) for w in ([0, 0, 0], [1, -1, 0], [0, 1, -1])]
    out = BatchedIterativeLQR.mpc_winner_log(s, sel)
    assert out.shape == (G, R, n + 2)
    assert np.array_equal(out[0, 0], log[1, 0]) and np.isnan(out[1, 0]).all() and np.array_equal(out[2, 0], log[4, 0])
    assert np.array_equal(out[0, 1], log[0, 1]) and np.array_equal(out[1, 1], log[3, 1]) and np.isnan(out[2, 1]).all()
    with pytest.raises(ValueError, match="mpc_winner_log"):
        BatchedIterativeLQR.mpc_winner_log(s, sel[:2])


@pytest.mark.parametrize("replan,hold", [(1, 1), (2, 3), (8, 2)])           # N = 10: replan_steps = N - 2 = 8 is the largest
def test_the_join_is_reseed_after_shift(replan, hold):
    """Random data, G = 3 groups of K = 4: group 0's winner is member 2, group 1 has no winner and non-finite controls, group 2 a tie."""
    rng = np.random.default_rng(10 * replan + hold)
    B, K, n, m, N = 12, 4, 3, 5, 10
    x, u = rng.standard_normal((B, n, N)), rng.uniform(-1.0, 1.0, (B, m, N - 1))
    u[4, 0, 3], u[5, 1, 8], u[6, 4, 0] = np.nan, np.inf, -np.inf
    cost = np.array([3.0, 2.0, 1.0, 4.0,   1.0, np.nan, np.inf, 2.0,   5.0, 5.0, 6.0, 7.0])
    status = np.array([0, 1, 16, 0,   2, 0, 0, 3,   1, 0, 0, 0])
    sigma = rng.choice([0.0, 0.25, 0.5], size=(B, m))
    x0, ug, best = MS.join(x, u, cost, status, K, replan, sigma, 77, 5, hold)
    assert best[:, 0].tolist() == [2, -1, 0] and best[:, 2].tolist() == [4, 0, 4]
    want, wb = SN.reseed(MS.shift(u, replan), cost, status, K, sigma, 77, 5, hold)
    assert np.array_equal(ug, want) and np.array_equal(best, wb) and np.isfinite(ug).all()
    pick = np.array([2, 2, 2, 2,   4, 5, 6, 7,   8, 8, 8, 8])
    assert np.array_equal(x0, x[pick, :, replan])
    sh = MS.shift(u, replan)
    assert np.array_equal(ug[2], sh[2]) and np.array_equal(ug[8], sh[8])     # the winners' slots: their own shifted plans, bit for bit
    assert np.array_equal(ug[4], np.where(np.isfinite(sh[4]), sh[4], 0.0))   # the fallback's member 0
    assert np.array_equal(sh[:, :, -1], u[:, :, -1]) and np.array_equal(sh[:, :, 0], u[:, :, replan])
    if replan == N - 2:
        assert np.array_equal(sh, np.repeat(u[:, :, -1:], N - 1, axis=2))    # everything past the horizon: the last column held


def test_k_one_is_the_shift():
    rng = np.random.default_rng(3)
    B, n, m, N = 6, 2, 3, 9
    x, u = rng.standard_normal((B, n, N)), rng.standard_normal((B, m, N - 1))
    cost, status = rng.uniform(1.0, 2.0, B), np.zeros(B, dtype=int)
    x0, ug, best = MS.join(x, u, cost, status, 1, 2, 0.5, 1, 0, 1)
    assert np.array_equal(ug, MS.shift(u, 2)) and np.array_equal(x0, x[:, :, 2]) and np.array_equal(best[:, 0], np.zeros(B))
    status[3] = 2                                                            # a failed member is its own group without a winner
    u[3, 1, 4] = np.nan
    x0, ug, best = MS.join(x, u, cost, status, 1, 2, 0.5, 1, 0, 1)
    sh = MS.shift(u, 2)
    assert best[3].tolist() == [-1.0, np.inf, 0.0] and np.array_equal(ug[3], np.where(np.isfinite(sh[3]), sh[3], 0.0))
    assert np.array_equal(np.delete(ug, 3, axis=0), np.delete(sh, 3, axis=0))
