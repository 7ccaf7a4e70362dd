#!/usr/bin/env python
"""Closed-loop receding-horizon control of the pendulum: B controllers share ONE model, and each of them meets a true plant whose
inertia, damping and gravity torque are drawn around that model, with actuation noise on top.  SetPlant gives every problem its
plant (include/mi_ilqr.h: "Closed-loop MPC"); MPCRun then advances the plants between the re-solves on the device - under the
feedback policy of the previous solve - and starts every re-solve from where its plant really is.  Printed: the share of the plants
brought to the upright position, and the cost they realised against the cost the first open-loop plan predicted."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from drake_ddp_amd import workloads as W  # noqa: E402
from drake_ddp_amd.ilqr import BatchedIterativeLQR  # noqa: E402
from drake_ddp_amd.models import ModelSystem  # noqa: E402

B, num_resolves, replan_steps = 256, 60, 4
p = W.pendulum_problem()
num_steps, dt = p["N"], p["dt"]
system = ModelSystem(p["model_id"], dt)                    # the controller's model: [ml2, b, mgl]

rng = np.random.default_rng(0)
scale = rng.uniform([0.8, 0.5, 0.8], [1.2, 1.5, 1.2], (B, 3))
scale[0] = 1.0                                             # plant 0 is the model itself
plants = system.params * scale
x_start = np.tile(W.pendulum_batch_x0(1)[0], (B, 1))

ilqr = BatchedIterativeLQR(system, num_steps, B, beta=p["beta"], delta=p["delta"], gamma=p["gamma"])
ilqr.SetTargetState(p["x_nom"])
ilqr.SetRunningCost(p["Q"], p["R"])
ilqr.SetTerminalCost(p["Qf"])
ilqr.SetInitialState(x_start)
ilqr.SetInitialGuess(np.zeros((1, num_steps - 1)))

st = time.time()
ilqr.Solve()                                               # the first plan, on the model
planned = ilqr.cost.copy()                                 # ... and what it predicts for the whole horizon
ilqr.SetPlant(x_start, plants, control_noise=0.05, seed=1)
stats = ilqr.MPCRun(num_resolves, replan_steps)            # closed loop: plant steps | shift | x0 <- plant | solve, num_resolves times
elapsed = time.time() - st

log = ilqr.plant_log                                       # X (B, n, K+1), U (B, m, K), stage_cost (B, K), steps (B,)
K = num_resolves * replan_steps
err = log.X[:, :, -1] - p["x_nom"]
err[:, 0] = (err[:, 0] + np.pi) % (2.0 * np.pi) - np.pi
stabilised = (np.abs(err[:, 0]) < 0.1) & (np.abs(err[:, 1]) < 0.5) & (log.steps == K)
realised = np.nansum(log.stage_cost, axis=1)
for b in range(0, B, B // 8):
    print(f"plant {b:3d}: ml2 x{scale[b, 0]:.2f} b x{scale[b, 1]:.2f} mgl x{scale[b, 2]:.2f}: angle after {K} steps {log.X[b, 0, -1]:+.3f} rad, "
          f"realised cost {realised[b]:8.3f} over {K} steps (first plan: {planned[b]:8.3f} over {num_steps - 1})")
print(f"{B} plants x {K} closed-loop steps ({num_resolves} re-solves) in {elapsed * 1e3:.1f} ms, {ilqr.plant_kernel_ms():.3f} ms of it in the plant "
      f"kernels; {int(stabilised.sum())} of {B} ({100.0 * stabilised.mean():.1f} %) stabilised; realised cost {realised.min():.3f} .. "
      f"{realised.max():.3f}, median {np.median(realised):.3f} (open-loop prediction {np.median(planned):.3f}; the model's own plant, "
      f"number 0: {realised[0]:.3f})")
