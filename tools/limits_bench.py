"""Control-limited pendulum at C2's shape (B = 1024, N = 200) beside the unlimited solve with sequential passes.

    python tools/limits_bench.py [--reps R] [--bound U]

Two child processes on the same device: the limited handle (Limited<Pendulum> kernels: sequential clamped rollout,
box-QP backward pass) and the unlimited one with MI_ILQR_SEQ_BACKWARD=1 MI_ILQR_SEQ_ROLLOUT=1 (the same pass shapes
without the limits).  Each runs `reps` cold solves from resident inputs and reports iterations per second of kernel
time (sum over the batch of the iterations / kernel ms).  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from drake_ddp_amd import workloads as W
from drake_ddp_amd.ilqr import BatchedIterativeLQR
from drake_ddp_amd.models import ModelSystem
limited, reps, bound = sys.argv[2] == "1", int(sys.argv[3]), float(sys.argv[4])
p = W.pendulum_problem(); B = 1024
s = BatchedIterativeLQR(ModelSystem(p["model_id"], p["dt"]), p["N"], B, delta=p["delta"], beta=p["beta"], gamma=p["gamma"],
                        hist_cap=2, control_limits="enforce" if limited else "ignore")
s.SetTargetState(p["x_nom"]); s.SetRunningCost(p["Q"], p["R"]); s.SetTerminalCost(p["Qf"])
if limited:
    s.SetControlLimits(-bound, bound)
s.SetInitialState(W.pendulum_batch_x0(B)); s.SetInitialGuess(np.zeros((1, p["N"] - 1))); s._push_problem()
rates = []
for r in range(reps + 1):
    s.rearm(cold=True)
    st = s.solve_resident()
    if r > 0:                                   # (the first solve warms the kernel up)
        rates.append(st.total_iters / (st.kernel_ms * 1e-3))
print(json.dumps(dict(it_per_s=float(np.median(rates)), iters=int(st.total_iters), kernel_ms=float(st.kernel_ms),
                      active=int((np.abs(s.u_bar) == bound).sum()) if limited else 0)))
"""


def run(limited, reps, bound):
    env = dict(os.environ)
    if not limited:
        env.update(MI_ILQR_SEQ_BACKWARD="1", MI_ILQR_SEQ_ROLLOUT="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, "1" if limited else "0", str(reps), str(bound)],
                       capture_output=True, text=True, timeout=600, env=env)
    if r.returncode != 0:
        raise SystemExit(f"child ({'limited' if limited else 'sequential'}) failed with {r.returncode}:\n{r.stderr[-3000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--bound", type=float, default=1.0, help="torque bound |u| <= U of the limited run")
    a = ap.parse_args()
    lim = run(True, a.reps, a.bound)
    seq = run(False, a.reps, a.bound)
    print(json.dumps(dict(config="pendulum B=1024 N=200", bound=a.bound, limited=lim, unlimited_sequential=seq,
                          ratio=lim["it_per_s"] / seq["it_per_s"])))
