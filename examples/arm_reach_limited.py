#!/usr/bin/env python
"""arm_reach.py's task - push the ball 15 cm along +y with the 7-joint arm (n = 27, m = 7) - with joint-torque limits:
control_limits="enforce" and one SetControlLimits call (the reference's method, a no-op there, ilqr.py:158-159).  The base
yaw joint is held to |tau| <= 1 N m, below the push torque of the initial guess, so the guess is projected into the box and the
solution rides the limit on part of the horizon; then a batch of perturbed starts with a receding-horizon loop on the device.
The kernels are the mid-size workgroup family's Limited<M> instantiations (box-QP backward pass, clamped rollouts).

    python examples/arm_reach_limited.py [--coupled]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from drake_ddp_amd import workloads as W  # noqa: E402
from drake_ddp_amd.ilqr import BatchedIterativeLQR, IterativeLinearQuadraticRegulator  # noqa: E402
from drake_ddp_amd.models import ArmAndBall, ArmAndBallCoupled  # noqa: E402

coupled = "--coupled" in sys.argv
p = W.arm27c_problem() if coupled else W.arm27_problem()
num_steps, dt = p["N"], p["dt"]
system_ = (ArmAndBallCoupled if coupled else ArmAndBall)(dt)
u_guess = (W.arm27c_u_guess if coupled else W.arm27_u_guess)(num_steps)
tau_max = np.array([1.0, 14.0, 4.0, 6.0, 2.0, 2.0, 2.0])          # N m per joint

ilqr = IterativeLinearQuadraticRegulator(system_, num_steps, beta=0.5, delta=1e-3, gamma=0, derivs_keypoint_method=None,
                                         control_limits="enforce")
ilqr.SetInitialState(W.arm27_start())
ilqr.SetTargetState(p["x_nom"])
ilqr.SetRunningCost(p["Q"], p["R"])
ilqr.SetTerminalCost(p["Qf"])
ilqr.SetControlLimits(-tau_max, tau_max)
ilqr.SetInitialGuess(u_guess)
states, inputs, solve_time, optimal_cost = ilqr.Solve()
active = (np.abs(inputs) == tau_max[:, None]).sum(axis=1)
print(f"Solved in {solve_time} seconds using iLQR")
print(f"Optimal cost: {optimal_cost}")
print(f"ball: y {states[12, 0]:.3f} -> {states[12, -1]:.3f} m (target {p['x_nom'][12]:.3f})")
print(f"steps on the torque limit per joint: {active.tolist()} of {num_steps - 1}; "
      f"inside the box: {bool(np.all(np.abs(inputs) <= tau_max[:, None]))}")

B, num_resolves, replan_steps = 64, 10, 5
batch = BatchedIterativeLQR(system_, num_steps, B, beta=0.5, delta=1e-3, gamma=0, control_limits="enforce")
batch.SetTargetState(p["x_nom"])
batch.SetRunningCost(p["Q"], p["R"])
batch.SetTerminalCost(p["Qf"])
batch.SetControlLimits(-tau_max, tau_max)
batch.SetInitialState(W.arm27_batch_x0(B))
batch.SetInitialGuess(u_guess)
x, u, _, cost = batch.Solve()
stats = batch.MPCRun(num_resolves, replan_steps)
print(f"{B} starts x (1 + {num_resolves}) solves: {stats.total_iters} iterations in the MPC loop, "
      f"all converged: {stats.n_converged == B}; max |u| / limit = {np.max(np.abs(batch.u_bar) / tau_max[:, None]):.3f}")
