#!/usr/bin/env python
"""Tuning cost weights on the pendulum swing-up: a grid over the scale of the terminal weight Qf and the effort weight R, every
grid point its own problem of ONE batch on one handle.  With the reference that is one solver object per weight set
(SetRunningCost / SetTerminalCost are per object); here SetRunningCost((B, n, n), (B, m, m)) and SetTerminalCost((B, n, n)) give
problem b its own matrices (include/mi_ilqr.h: "Per-problem cost matrices").  The candidates are compared by a score that does not
depend on their own weights: distance from the upright state at the end of the plan plus the effort spent."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from drake_ddp_amd import workloads as W  # noqa: E402
from drake_ddp_amd.ilqr import BatchedIterativeLQR  # noqa: E402
from drake_ddp_amd.models import ModelSystem  # noqa: E402

p = W.pendulum_problem()
num_steps, dt = p["N"], p["dt"]
qf_scales = np.logspace(-1, 1, 16)                         # Qf x 0.1 .. 10
r_scales = np.logspace(-1, 1, 16)                          # R x 0.1 .. 10
grid = np.array([(a, b) for a in qf_scales for b in r_scales])
B = len(grid)

ilqr = BatchedIterativeLQR(ModelSystem(p["model_id"], dt), num_steps, B, beta=p["beta"], delta=p["delta"], gamma=p["gamma"])
ilqr.SetTargetState(p["x_nom"])
ilqr.SetRunningCost(p["Q"], grid[:, 1, None, None] * p["R"])     # Q shared, R per problem: any mix of the two forms
ilqr.SetTerminalCost(grid[:, 0, None, None] * p["Qf"])
ilqr.SetInitialState(np.tile(W.pendulum_batch_x0(1)[0], (B, 1)))
ilqr.SetInitialGuess(np.zeros((1, num_steps - 1)))

st = time.time()
x, u, _, cost = ilqr.Solve()
elapsed = time.time() - st
end_error = np.linalg.norm(x[:, :, -1] - p["x_nom"], axis=1)
effort = dt * np.sum(u[:, 0, :] ** 2, axis=1)
score = end_error + 0.01 * effort
ok = ilqr.status == 0
best = int(np.argmin(np.where(ok, score, np.inf)))
for b in np.argsort(np.where(ok, score, np.inf))[:5]:
    print(f"Qf x{grid[b, 0]:6.2f}  R x{grid[b, 1]:6.2f}: {ilqr.iterations[b]:3d} iterations, end error {end_error[b]:.4f}, "
          f"effort {effort[b]:7.2f}, score {score[b]:.4f}")
print(f"{B} weight sets in one solve of {elapsed * 1e3:.1f} ms; {int(ok.sum())} converged; best set: Qf x{grid[best, 0]:.2f}, "
      f"R x{grid[best, 1]:.2f} (score {score[best]:.4f})")
