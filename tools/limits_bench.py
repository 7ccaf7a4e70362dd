"""Control-limited pendulum at C2's shape (B = 1024, N = 200) beside the unlimited solve with sequential passes; or (--model arm27)
the arm + ball at C6's shape (B = 64, N = 50) with joint-torque limits beside the unlimited solve.

    python tools/limits_bench.py [--reps R] [--bound U] [--model pendulum|arm27]

Two child processes on the same device: the limited handle (Limited<Pendulum> kernels: sequential clamped rollout,
box-QP backward pass) and the unlimited one with MI_ILQR_SEQ_BACKWARD=1 MI_ILQR_SEQ_ROLLOUT=1 (the same pass shapes
without the limits).  Each runs `reps` cold solves from resident inputs and reports iterations per second of kernel
time (sum over the batch of the iterations / kernel ms) and iterations per solve.  For the arm the unlimited run is the default one
(the mid-size family's limited kernels keep the four-candidate line search and turn clusters off); --bound scales the torque
limits |tau| <= U x (1, 12, 4, 6, 2, 2, 2) N m.  Prints one JSON line."""
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
limited, reps, bound, model = sys.argv[2] == "1", int(sys.argv[3]), float(sys.argv[4]), sys.argv[5]
if model == "arm27":
    p = W.arm27_problem(); B = 64
    lim = bound * np.array([1.0, 12.0, 4.0, 6.0, 2.0, 2.0, 2.0])
    x0, ug = W.arm27_batch_x0(B), W.arm27_u_guess(p["N"])
else:
    p = W.pendulum_problem(); B = 1024
    lim = bound
    x0, ug = W.pendulum_batch_x0(B), np.zeros((1, p["N"] - 1))
s = BatchedIterativeLQR(ModelSystem(p["model_id"], p["dt"]), p["N"], B, delta=p["delta"], beta=p["beta"], gamma=p["gamma"],
                        hist_cap=2, control_limits="enforce" if limited else "ignore")
s.SetTargetState(p["x_nom"]); s.SetRunningCost(p["Q"], p["R"]); s.SetTerminalCost(p["Qf"])
if limited:
    s.SetControlLimits(-lim, lim)
s.SetInitialState(x0); s.SetInitialGuess(ug); s._push_problem()
rates = []
for r in range(reps + 1):
    s.rearm(cold=True)
    st = s.solve_resident()
    if r > 0:                                   # (the first solve warms the kernel up)
        rates.append(st.total_iters / (st.kernel_ms * 1e-3))
lim_b = np.broadcast_to(np.reshape(lim, (-1, 1)), s.u_bar.shape[1:])
print(json.dumps(dict(it_per_s=float(np.median(rates)), iters=int(st.total_iters), iters_per_solve=st.total_iters / B,
                      kernel_ms=float(st.kernel_ms), active=int((np.abs(s.u_bar) == lim_b).sum()) if limited else 0)))
"""


def run(limited, reps, bound, model="pendulum"):
    env = dict(os.environ)
    if not limited and model == "pendulum":
        env.update(MI_ILQR_SEQ_BACKWARD="1", MI_ILQR_SEQ_ROLLOUT="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, "1" if limited else "0", str(reps), str(bound), model],
                       capture_output=True, text=True, timeout=600, env=env)
    if r.returncode != 0:
        raise SystemExit(f"child ({'limited' if limited else 'sequential'}) failed with {r.returncode}:\n{r.stderr[-3000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--bound", type=float, default=1.0, help="torque bound |u| <= U of the limited run")
    ap.add_argument("--model", choices=("pendulum", "arm27"), default="pendulum")
    a = ap.parse_args()
    lim = run(True, a.reps, a.bound, a.model)
    ref = run(False, a.reps, a.bound, a.model)
    if a.model == "arm27":
        print(json.dumps(dict(config="arm27 B=64 N=50", bound=a.bound, limited=lim, unlimited=ref,
                              ratio=lim["it_per_s"] / ref["it_per_s"],
                              iters_ratio=lim["iters_per_solve"] / ref["iters_per_solve"])))
    else:
        print(json.dumps(dict(config="pendulum B=1024 N=200", bound=a.bound, limited=lim, unlimited_sequential=ref,
                              ratio=lim["it_per_s"] / ref["it_per_s"])))
