"""The Dual2 overloads of operator/ (its three forms), mi_exp, mi_log1p, mi_sqrt and mi_softplus at work: an n = 2, m = 1 plugin -
the shape whose eps = 1 trial runs as Newton's method on the whole trajectory with Dual2 step Jacobians (ilqr_small.hpp) - that
uses every one of them: a pendulum with a soft end-stop, a drag v / (2 + q^2) and small terms through the other primitives.
B = 256 problems solved (a) by default, (b) with the sequential passes forced in a child process, (c) by the NumPy oracle driven by
the Python twin of the step (tests/plugin_steps.py: endstop2_step): the same iterations and line-search trials everywhere, flip
budget 0 (tests/test_dual2_model_oracle.py shows the oracle keeps its own counts when x0 moves by one ulp), tolerances of
test_time_parallel_passes_match_the_sequential_ones and of the plugin tests.

Whether the Newton rollout converged or fell back to the sequential one is not reported by a regular build (only by one with
-DMI_PROF_NEWTON); what the handle does expose is the line search's cycle count (mi_ilqr_get_cycles).  A fallback pays the Newton
sweeps AND the sequential rollout, so a batch whose time-parallel trials fell back spends more cycles in its line searches than
the same batch on the sequential passes alone: the default run must spend fewer.  (A wrong Dual2 derivative rule leaves the
fixed point - defined by the values - where it is, but the sweeps then stop converging within their budget and fall back.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

FLIP_BUDGET = 0

ENDSTOP2_BODY = """    const double g_l = p[0], c = p[1], k = p[2], sig = p[3], qmax = p[4];
    const T q = x[0], v = x[1];
    const T w = q * q;
    T a = u[0] - g_l * mi_sin(q) - c * (v / (2.0 + w)) - (k * sig) * mi_softplus((q - qmax) / sig);
    a = a - 0.05 * (v / mi_sqrt(1.0 + v * v)) + 0.1 * mi_exp(-w) - 0.05 * mi_log1p(w) + 0.02 * (1.0 / (3.0 + w)) * mi_cos(q);
    const T vn = v + dt * a;
    xn[1] = vn; xn[0] = q + dt * vn;"""
ENDSTOP2_DEFAULTS = [4.0, 0.5, 60.0, 0.05, 1.0]
CASE = dict(dt=0.02, N=120, B=256, x_nom=np.array([0.8, 0.0]), Q=np.eye(2), R=0.1 * np.eye(1), Qf=20.0 * np.eye(2), delta=1e-3, beta=0.7)


def problems():
    """x0 on both sides of the end-stop at q = 1 (the target sits just inside it), one shared guess."""
    rng = np.random.default_rng(2)
    x0 = np.stack([rng.uniform(-1.5, 1.6, CASE["B"]), rng.uniform(-2.0, 2.0, CASE["B"])], axis=1)
    return x0, rng.uniform(-0.1, 0.1, (1, CASE["N"] - 1))


_SCRIPT = """
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_gpu_dual2_overloads as T
np.savez(sys.argv[1], **T.solve())
"""


def solve():
    from drake_ddp_amd import plugin
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    c = CASE
    sys_ = plugin.build_model("endstop2", 2, 1, ENDSTOP2_BODY, ENDSTOP2_DEFAULTS, "small")(c["dt"])
    x0, ug = problems()
    s = BatchedIterativeLQR(sys_, c["N"], c["B"], delta=c["delta"], beta=c["beta"], jacobian_mode="ad", kernel_mode="latency")
    s.SetTargetState(c["x_nom"]); s.SetRunningCost(c["dt"] * c["Q"], c["dt"] * c["R"]); s.SetTerminalCost(c["Qf"])
    s.SetInitialState(x0); s.SetInitialGuess(ug)
    x, u, _, L = s.Solve()
    return dict(x=x, u=u, L=L, K=s.K, it=s.iterations, ls=s.ls_trials, st=s.status, cyc=s.stage_cycles)


def test_n2_model_on_every_dual2_overload_solves_like_the_sequential_passes_and_the_oracle(tmp_path):
    import plugin_steps as PS
    from oracle import models_np as M
    from oracle.ilqr_np import OracleILQR
    c = CASE
    par = solve()
    assert (par["st"] == 0).all()
    f = str(tmp_path / "seq.npz")
    r = subprocess.run([sys.executable, "-c", _SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests")), f], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, MI_ILQR_SEQ_ROLLOUT="1", MI_ILQR_SEQ_BACKWARD="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    seq = np.load(f)
    # (a) against (b): test_time_parallel_passes_match_the_sequential_ones' tolerances
    assert np.array_equal(par["it"], seq["it"]) and np.array_equal(par["ls"], seq["ls"]) and (seq["st"] == 0).all()
    rel_L = np.abs(par["L"] - seq["L"]) / np.abs(seq["L"])
    assert np.max(rel_L) < 5e-8 and np.median(rel_L) < 1e-10, (np.max(rel_L), np.median(rel_L))
    assert np.max(np.abs(par["x"] - seq["x"])) < 1e-6 and np.max(np.abs(par["u"] - seq["u"])) < 1e-6
    assert np.max(np.abs(par["K"] - seq["K"])) < 1e-5 * np.max(np.abs(seq["K"]))
    # the time-parallel trials ran and did not fall back (module docstring)
    ls_par, ls_seq = int(par["cyc"][:, 0].sum()), int(seq["cyc"][:, 0].sum())
    print("\nline-search cycles over the batch: time-parallel %d, sequential %d (%.2f)" % (ls_par, ls_seq, ls_par / ls_seq))
    assert ls_par < ls_seq, (ls_par, ls_seq)
    # (a) against (c): the plugin tests' tolerances, every problem, no flips
    x0, ug = problems()
    model = M.Model.custom(2, 1, PS.endstop2_step, np.array(ENDSTOP2_DEFAULTS), c["dt"])
    flips = 0
    for b in range(c["B"]):
        o = OracleILQR(model, c["N"], c["delta"], c["beta"], 0.0, jacobian="ad")
        o.set_problem(x0[b], c["x_nom"], c["dt"] * c["Q"], c["dt"] * c["R"], c["Qf"], ug)
        xo, uo, Lo, hist = o.solve()
        same = len(hist) == par["it"][b] and int(sum(h[2] for h in hist)) == par["ls"][b]
        flips += not same
        if same:
            assert abs(par["L"][b] - Lo) < 1e-9 * abs(Lo) and np.max(np.abs(par["x"][b] - xo)) < 1e-6 * max(1.0, np.abs(xo).max()), b
    assert flips <= FLIP_BUDGET, flips
