"""Per-problem cost matrices set to identical rows beside the shared matrices, on C2's shape (pendulum, B = 1024, N = 200: cold
solves), C5's (Synth36, B = 64, N = 40: a cold solve, then MPCRun(20, 4)) and the lane-per-problem kernels (acrobot,
kernel_mode="throughput", B = 8192, N = 40: cold solves - their per-problem instantiation holds the matrices in registers).

    python tools/costs_bench.py [--reps R]

Child processes on the same device, one per (config, mode), alternated shared / per-problem `rounds` times: both modes compute
the same bits (tests/test_gpu_cost_matrices.py), so the ratio is the cost of reading Q, R, Qf per problem.  Each child
reports iterations per second of kernel time (sum over the batch of the iterations / kernel ms), median over `reps` runs.
Prints one JSON line; ratio = per-problem / shared (1.0 = no cost)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from drake_ddp_amd import workloads as W
from drake_ddp_amd.ilqr import BatchedIterativeLQR
from drake_ddp_amd.models import ModelSystem
per_problem, reps, config = sys.argv[2] == "1", int(sys.argv[3]), sys.argv[4]
kw = {}
if config == "c5":
    p = W.synth36_problem(); B = 64
    x0, ug = W.synth36_batch_x0(B), W.synth36_u_guess(p["N"])
elif config == "lane":
    p = W.acrobot_problem(); B = 8192; kw = dict(kernel_mode="throughput")
    x0, ug = W.acrobot_batch_x0(B), np.zeros((1, p["N"] - 1))
else:
    p = W.pendulum_problem(); B = 1024
    x0, ug = W.pendulum_batch_x0(B), np.zeros((1, p["N"] - 1))
s = BatchedIterativeLQR(ModelSystem(p["model_id"], p["dt"]), p["N"], B, delta=p["delta"], beta=p["beta"], gamma=p["gamma"], hist_cap=2, **kw)
rep = (lambda a: np.tile(np.asarray(a, dtype=np.float64), (B, 1, 1))) if per_problem else (lambda a: a)
s.SetTargetState(p["x_nom"])
s.SetRunningCost(rep(p["Q"]), rep(p["R"])); s.SetTerminalCost(rep(p["Qf"]))
s.SetInitialState(x0); s.SetInitialGuess(ug); s._push_problem()
step = np.zeros(p["x_nom"].shape); step[0] = W.SYNTH_TARGET_VEL * p["dt"] * 4
rates = []
for r in range(reps + 1):
    if config == "c5":
        s.SetTargetState(p["x_nom"])
        s.SetInitialState(x0); s.SetInitialGuess(ug); s.Reset()
        s.Solve()
        st = s.MPCRun(20, 4, target_step=step)
    else:
        s.rearm(cold=True)
        st = s.solve_resident()
    if r > 0:                                   # (the first run warms the kernels up)
        rates.append(st.total_iters / (st.kernel_ms * 1e-3))
print(json.dumps(dict(it_per_s=float(np.median(rates)), iters=int(st.total_iters), kernel_ms=float(st.kernel_ms))))
"""


def run(per_problem, reps, config):
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, "1" if per_problem else "0", str(reps), config],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"child ({config}, {'per-problem' if per_problem else 'shared'}) failed with {r.returncode}:\n{r.stderr[-3000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2, help="alternations shared / per-problem per config")
    a = ap.parse_args()
    out = dict()
    for config, label in (("c2", "pendulum B=1024 N=200"), ("c5", "synth36 B=64 N=40 MPCRun(20, 4)"),
                          ("lane", "acrobot throughput B=8192 N=40")):
        shared, pp = [], []
        for _ in range(a.rounds):
            shared.append(run(False, a.reps, config))
            pp.append(run(True, a.reps, config))
        assert all(x["iters"] == shared[0]["iters"] for x in shared + pp), (config, shared, pp)   # same bits: same iterations
        s_rate = float(np.median([x["it_per_s"] for x in shared]))
        p_rate = float(np.median([x["it_per_s"] for x in pp]))
        out[config] = dict(config=label, shared_it_per_s=s_rate, per_problem_it_per_s=p_rate, ratio=p_rate / s_rate,
                           spread_shared=[x["it_per_s"] for x in shared], spread_per_problem=[x["it_per_s"] for x in pp])
    print(json.dumps(out))
