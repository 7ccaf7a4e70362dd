#!/usr/bin/env python
"""Domain-randomised receding-horizon control of the pendulum: every seed swings up ITS OWN plant - inertia, damping and gravity
torque drawn around the nominal ones - from the same start, in one batch on one handle.  With the reference that is one solver
object per System; here SetModelParameters((B, n_params)) gives problem b row b (include/mi_ilqr.h: "Per-problem model
parameters") and the loop of the reference's scripts (acrobot.py:145-155) runs on the device for all of them at once."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from drake_ddp_amd import workloads as W  # noqa: E402
from drake_ddp_amd.ilqr import BatchedIterativeLQR  # noqa: E402
from drake_ddp_amd.models import ModelSystem  # noqa: E402

B, num_resolves, replan_steps = 256, 20, 4
p = W.pendulum_problem()
num_steps, dt = p["N"], p["dt"]
system = ModelSystem(p["model_id"], dt)                    # the nominal plant: [ml2, b, mgl]

rng = np.random.default_rng(0)
scale = rng.uniform([0.8, 0.5, 0.8], [1.2, 1.5, 1.2], (B, 3))
scale[0] = 1.0                                             # seed 0: the nominal plant itself
plants = system.params * scale

ilqr = BatchedIterativeLQR(system, num_steps, B, beta=p["beta"], delta=p["delta"], gamma=p["gamma"])
ilqr.SetModelParameters(plants)                            # (B, 3): one row per seed
ilqr.SetTargetState(p["x_nom"])
ilqr.SetRunningCost(p["Q"], p["R"])
ilqr.SetTerminalCost(p["Qf"])
ilqr.SetInitialState(np.tile(W.pendulum_batch_x0(1)[0], (B, 1)))
ilqr.SetInitialGuess(np.zeros((1, num_steps - 1)))

st = time.time()
ilqr.Solve()
first_cost, first_iters = ilqr.cost.copy(), ilqr.iterations.copy()
stats = ilqr.MPCRun(num_resolves, replan_steps)
elapsed = time.time() - st
log = ilqr.mpc_log                                         # (B, num_resolves, n + 2): x0 of each re-solve | cost | iterations
for b in range(0, B, B // 8):
    print(f"seed {b:2d}: ml2 x{scale[b, 0]:.2f} b x{scale[b, 1]:.2f} mgl x{scale[b, 2]:.2f}: first plan {first_iters[b]:2d} iterations, "
          f"cost {first_cost[b]:8.3f}; angle at the last re-solve {log[b, -1, 0]:+.3f} rad")
print(f"{B} plants x (1 + {num_resolves}) solves in {elapsed * 1e3:.1f} ms; {stats.total_iters} iLQR iterations in the re-solves; "
      f"{stats.n_converged} of {B} converged; first-plan cost {first_cost.min():.3f} .. {first_cost.max():.3f} "
      f"(nominal {first_cost[0]:.3f})")
