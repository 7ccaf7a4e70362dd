"""What a reference trajectory costs, on C5's shape (Synth36, B = 64, N = 40: a cold solve, then MPCRun(20, 4)) and C6's (Arm27, B = 64,
N = 50: cold solves).

    python tools/tracking_bench.py [--reps R] [--rounds K] [--other-lib PATH]

Child processes on the same device, one per (config, mode), the modes alternated `rounds` times:
  shared     the constant target x_nom, no reference;
  reference  a reference of T = N rows that all equal x_nom - the same optimisation problem, the same bits (a reference whose rows
             are equal is the constant target: tests/test_gpu_tracking.py), so the ratio is the cost of reading r_t per step and of
             the per-step 2 r_t^T Q rows;
  other      (with --other-lib) the `shared` run on ANOTHER build of the library, e.g. the parent commit's: what the feature costs a
             handle that does not use it.
Each child reports iterations per second of kernel time (sum over the batch of the iterations / kernel ms), median over `reps` runs.
Prints one JSON line; ratios are mode / shared (1.0 = no cost), with every mode's own runs beside them (the run-to-run spread)."""
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
tracked, reps, config = sys.argv[2] == "1", int(sys.argv[3]), sys.argv[4]
B = 64
if config == "c5":
    p = W.synth36_problem()
    x0, ug = W.synth36_batch_x0(B), W.synth36_u_guess(p["N"])
else:
    p = W.arm27_problem()
    x0, ug = W.arm27_batch_x0(B), W.arm27_u_guess(p["N"])
s = BatchedIterativeLQR(ModelSystem(p["model_id"], p["dt"]), p["N"], B, delta=p["delta"], beta=p["beta"], gamma=p["gamma"], hist_cap=2)
s.SetTargetState(p["x_nom"]); s.SetRunningCost(p["Q"], p["R"]); s.SetTerminalCost(p["Qf"])
ref = np.tile(p["x_nom"], (p["N"], 1))
rates = []
for r in range(reps + 1):
    s.SetInitialState(x0); s.SetInitialGuess(ug); s.Reset()
    if tracked:
        s.SetTargetTrajectory(ref, clock=0)
    s.Solve()
    st = s.MPCRun(20, 4) if config == "c5" else s.stats
    if r > 0:                                   # (the first run warms the kernels up)
        rates.append(st.total_iters / (st.kernel_ms * 1e-3))
print(json.dumps(dict(it_per_s=float(np.median(rates)), iters=int(st.total_iters), kernel_ms=float(st.kernel_ms))))
"""


def run(mode, reps, config, other_lib):
    env = dict(os.environ)
    if mode == "other":
        env["MI_ILQR_LIB"] = other_lib
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, "1" if mode == "reference" else "0", str(reps), config],
                       capture_output=True, text=True, timeout=600, env=env)
    if r.returncode != 0:
        raise SystemExit(f"child ({config}, {mode}) failed with {r.returncode}:\n{r.stderr[-3000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2, help="alternations of the modes per config")
    ap.add_argument("--other-lib", default=None, help="another build of libmi_ilqr.so to run the shared mode on")
    a = ap.parse_args()
    modes = ["shared", "reference"] + (["other"] if a.other_lib else [])
    out = dict()
    for config, label in (("c5", "synth36 B=64 N=40 Solve + MPCRun(20, 4)"), ("c6", "arm27 B=64 N=50 Solve")):
        runs = {m: [] for m in modes}
        for _ in range(a.rounds):
            for m in modes:
                runs[m].append(run(m, a.reps, config, a.other_lib))
        first = runs["shared"][0]["iters"]
        assert all(x["iters"] == first for m in modes for x in runs[m]), (config, runs)   # same bits: same iterations
        rate = {m: float(np.median([x["it_per_s"] for x in runs[m]])) for m in modes}
        out[config] = dict(config=label, it_per_s=rate, ratio={m: rate[m] / rate["shared"] for m in modes if m != "shared"},
                           runs={m: [x["it_per_s"] for x in runs[m]] for m in modes})
    print(json.dumps(out))
