#!/usr/bin/env python
"""Measure the mismatch, then remove it: B pendulums whose true inertia, damping and gravity torque differ from the controller's model
run in closed loop (SetPlant + MPCRun, examples/mpc_closed_loop_pendulum.py); the transitions the plants really made are sliced out
of plant_log, FitModelParameters fits every problem's own parameter row to its own transitions on the device and - apply=True -
makes the fitted rows the solver's per-problem model; the same closed loop runs again.  Printed: the parameter error and the cost the
plants realised (stage costs plus the terminal term at the last state), before and after the fit.  The closed loop runs for two
horizons (400 steps): the horizon recedes, so a cost taken while the plants still swing up (measured at 120 and at 240 steps) says
where each plant happens to be at that step, not how well it was controlled, and is no lower with the right model."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from drake_ddp_amd import workloads as W  # noqa: E402
from drake_ddp_amd.ilqr import BatchedIterativeLQR  # noqa: E402
from drake_ddp_amd.models import ModelSystem  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--resolves", type=int, default=100)      # x 4 steps = two horizons: every swing-up is over when the cost is taken
B = ap.parse_args().batch
num_resolves, replan_steps = ap.parse_args().resolves, 4
p = W.pendulum_problem()
num_steps, dt = p["N"], p["dt"]
system = ModelSystem(p["model_id"], dt)                    # the controller's model: [ml2, b, mgl]

rng = np.random.default_rng(0)
true_rows = system.params * rng.uniform([0.7, 0.5, 0.7], [1.3, 1.5, 1.3], (B, 3))
x_start = np.tile(W.pendulum_batch_x0(1)[0], (B, 1))

ilqr = BatchedIterativeLQR(system, num_steps, B, beta=p["beta"], delta=p["delta"], gamma=p["gamma"])
ilqr.SetTargetState(p["x_nom"])
ilqr.SetRunningCost(p["Q"], p["R"])
ilqr.SetTerminalCost(p["Qf"])


def closed_loop():
    """Plan on the solver's model rows, run the true plants under the plan's feedback, re-plan every replan_steps steps."""
    ilqr.Reset()
    ilqr.SetInitialState(x_start)
    ilqr.SetInitialGuess(np.zeros((1, num_steps - 1)))
    ilqr.Solve()
    ilqr.SetPlant(x_start, true_rows)
    ilqr.MPCRun(num_resolves, replan_steps)
    log = ilqr.plant_log                                   # X (B, n, K+1), U (B, m, K), stage_cost (B, K), steps (B,)
    err = log.X[:, :, -1] - p["x_nom"]
    err[:, 0] = (err[:, 0] + np.pi) % (2.0 * np.pi) - np.pi
    realised = np.nansum(log.stage_cost, axis=1) + np.einsum("bi,ij,bj->b", err, p["Qf"], err)
    ilqr.ClearPlant()
    return log, realised


def param_error():
    return float(np.max(np.abs(ilqr.model_params - true_rows) / np.abs(true_rows)))


err_before = param_error()
log, cost_before = closed_loop()
# row j of problem b: the state before step j, the control the plant got, the state after it
x = np.ascontiguousarray(np.moveaxis(log.X[:, :, :-1], 1, 2))
x_next = np.ascontiguousarray(np.moveaxis(log.X[:, :, 1:], 1, 2))
u = np.ascontiguousarray(np.moveaxis(log.U, 1, 2))
fit = ilqr.FitModelParameters(x, u, x_next, free=[0, 1, 2], count=log.steps, iterations=20, apply=True)
err_after = param_error()
_, cost_after = closed_loop()

for b in range(0, B, max(B // 4, 1)):
    print(f"plant {b:3d}: true {np.round(true_rows[b], 4).tolist()}, fitted {np.round(fit.params[b], 4).tolist()} from {int(fit.count[b])} "
          f"transitions in {int(fit.iterations[b])} trials (status {int(fit.status[b])}), prediction error {fit.cost0[b]:.2e} -> {fit.cost[b]:.2e}; "
          f"realised cost {cost_before[b]:.3f} -> {cost_after[b]:.3f}")
print(f"{B} plants identified in {fit.kernel_ms:.3f} ms of kernels; worst relative parameter error {err_before:.2e} -> {err_after:.2e}; "
      f"mean realised cost {cost_before.mean():.4f} -> {cost_after.mean():.4f}")
print(f"RESULT param_error_before {err_before:.6e}")
print(f"RESULT param_error_after {err_after:.6e}")
print(f"RESULT realised_cost_before {cost_before.mean():.6e}")
print(f"RESULT realised_cost_after {cost_after.mean():.6e}")
