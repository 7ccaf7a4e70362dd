#!/usr/bin/env python
"""Pendulum swing-up with a torque limit |u| <= 1 - swingup_pendulum.py with control_limits="enforce" and one
SetControlLimits call (the reference's method, a no-op there, ilqr.py:158-159).  The bound is below the torque
the unlimited swing-up uses, so the solution pumps energy and rides the limit on part of the horizon."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from drake_ddp_amd.ilqr import IterativeLinearQuadraticRegulator  # noqa: E402
from drake_ddp_amd.models import Pendulum  # noqa: E402

T, dt = 2.0, 1e-2
u_max = 1.0
x0 = np.array([0, 0])
x_nom = np.array([np.pi, 0])
Q = 0.01 * np.diag([0, 1])
R = 0.01 * np.eye(1)
Qf = 100 * np.diag([1, 1])

num_steps = int(T / dt)
ilqr = IterativeLinearQuadraticRegulator(Pendulum(dt), num_steps, control_limits="enforce")
ilqr.SetInitialState(x0)
ilqr.SetTargetState(x_nom)
ilqr.SetRunningCost(dt * Q, dt * R)
ilqr.SetTerminalCost(Qf)
ilqr.SetControlLimits(-u_max, u_max)
ilqr.SetInitialGuess(np.zeros((1, num_steps - 1)))

states, inputs, solve_time, optimal_cost = ilqr.Solve()
active = int(np.sum(np.abs(inputs) == u_max))
print(f"Solved in {solve_time} seconds using iLQR")
print(f"Optimal cost: {optimal_cost}")
print(f"max |u| = {np.abs(inputs).max():.6f} (limit {u_max}); steps on the limit: {active} of {num_steps - 1}")
print(f"final state: {states[:, -1]}  (target {x_nom})")
