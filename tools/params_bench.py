"""Per-problem model parameters set to identical rows beside the shared parameters: C2's shape (pendulum, B = 1024, N = 200, cold
solves), C5's (Synth36, B = 64, N = 40: a cold solve, then MPCRun(20, 4)) and the throughput shape (acrobot, N = 40, B = 262 144,
lane-per-problem kernels, cold solves).

    python tools/params_bench.py [--reps R] [--rounds K] [--configs c2,c5,tp]

One process, two handles per config - one in shared mode, one with every row equal to the shared parameters - run alternately
`rounds` times (at least twice): both compute the same bits (tests/test_gpu_model_params.py), so the ratio is the cost of taking
the parameters per problem.  A run reports iterations per second of kernel time (the batch's iterations / kernel ms), median over
`reps` solves after one warm-up.  The spread between the rounds of ONE mode is the yardstick for the ratio.  Prints one JSON line;
ratio = per-problem / shared (1.0 = no cost)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LABELS = {"c2": "pendulum B=1024 N=200", "c5": "synth36 B=64 N=40 MPCRun(20, 4)", "tp": "acrobot throughput B=262144 N=40"}


def make(config, per_problem):
    from drake_ddp_amd import workloads as W
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    from drake_ddp_amd.models import ModelSystem
    kw = {}
    if config == "c5":
        p = W.synth36_problem(); B = 64
        x0, ug = W.synth36_batch_x0(B), W.synth36_u_guess(p["N"])
    elif config == "tp":
        p = W.acrobot_problem(40); B = 262144
        x0, ug = W.acrobot_batch_x0(B), np.zeros((1, p["N"] - 1))
        kw = dict(kernel_mode="throughput", pinned_results=False)
    else:
        p = W.pendulum_problem(); B = 1024
        x0, ug = W.pendulum_batch_x0(B), np.zeros((1, p["N"] - 1))
    sys_ = ModelSystem(p["model_id"], p["dt"])
    s = BatchedIterativeLQR(sys_, p["N"], B, delta=p["delta"], beta=p["beta"], gamma=p["gamma"], hist_cap=2, **kw)
    s.SetTargetState(p["x_nom"]); s.SetRunningCost(p["Q"], p["R"]); s.SetTerminalCost(p["Qf"])
    if per_problem:
        s.SetModelParameters(sys_.params)          # (n_params,): every row the shared parameters
    s.SetInitialState(x0); s.SetInitialGuess(ug); s._push_problem()
    return s, x0, ug


def measure(config, handle, reps):
    s, x0, ug = handle
    rates = []
    for r in range(reps + 1):
        if config == "c5":
            s.SetInitialState(x0); s.SetInitialGuess(ug); s.Reset()
            s.Solve()
            st = s.MPCRun(20, 4)
        else:
            s.rearm(cold=True)
            st = s.solve_resident()
        if r > 0:                                   # (the first run warms the kernels up)
            rates.append(st.total_iters / (st.kernel_ms * 1e-3))
    return dict(it_per_s=float(np.median(rates)), iters=int(st.total_iters), kernel_ms=float(st.kernel_ms))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2, help="alternations shared / per-problem per config (at least 2)")
    ap.add_argument("--configs", default="c2,c5,tp")
    a = ap.parse_args()
    out = dict()
    for config in a.configs.split(","):
        handles = {False: make(config, False), True: make(config, True)}
        runs = {False: [], True: []}
        for _ in range(max(2, a.rounds)):
            for mode in (False, True):
                runs[mode].append(measure(config, handles[mode], a.reps if config != "tp" else min(a.reps, 3)))
        assert all(x["iters"] == runs[False][0]["iters"] for x in runs[False] + runs[True]), (config, runs)   # same bits: same iterations
        s_rate = float(np.median([x["it_per_s"] for x in runs[False]]))
        p_rate = float(np.median([x["it_per_s"] for x in runs[True]]))
        out[config] = dict(config=LABELS[config], shared_it_per_s=s_rate, per_problem_it_per_s=p_rate, ratio=p_rate / s_rate,
                           spread_shared=[x["it_per_s"] for x in runs[False]], spread_per_problem=[x["it_per_s"] for x in runs[True]])
        del handles
    print(json.dumps(out))
