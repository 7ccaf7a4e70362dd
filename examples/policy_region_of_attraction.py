#!/usr/bin/env python
"""How far does a solved swing-up policy reach?  The pendulum swing-up of swingup_pendulum.py is solved once; its time-varying
feedback policy u = u_bar - K (x - x_bar) - what the reference's SaveSolution stores K for (ilqr.py:712-733) - is then rolled
out on the GPU from a grid of initial states, each on plants whose mass parameters (m l^2 and m g l) are off by up to +-20 %:
one call, one lane per sample (IterativeLinearQuadraticRegulator.RolloutPolicy).  Prints the fraction of rollouts that end
within a tolerance of the upright target, per mass error."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from drake_ddp_amd.ilqr import IterativeLinearQuadraticRegulator  # noqa: E402
from drake_ddp_amd.models import Pendulum  # noqa: E402

T, dt = 2.0, 1e-2
x_nom = np.array([np.pi, 0])
num_steps = int(T / dt)
system = Pendulum(dt)
ilqr = IterativeLinearQuadraticRegulator(system, num_steps, verbose=False)
ilqr.SetInitialState(np.array([0.0, 0.0]))
ilqr.SetTargetState(x_nom)
ilqr.SetRunningCost(dt * 0.01 * np.diag([0, 1]), dt * 0.01 * np.eye(1))
ilqr.SetTerminalCost(100 * np.diag([1, 1]))
ilqr.SetInitialGuess(np.zeros((1, num_steps - 1)))
_, _, solve_time, cost = ilqr.Solve()
print(f"swing-up solved in {solve_time:.3f} s, cost {cost:.4f}")

# the samples: a 41 x 41 grid of initial (angle, rate) around the start, each on five plants
theta, omega = np.meshgrid(np.linspace(-2.5, 2.5, 41), np.linspace(-6.0, 6.0, 41), indexing="ij")
grid = np.stack([theta.ravel(), omega.ravel()], axis=1)
scales = np.array([0.8, 0.9, 1.0, 1.1, 1.2])
x0 = np.tile(grid, (len(scales), 1))
params = np.tile(system.params, (len(x0), 1))                  # [m l^2, b, m g l]
mass = np.repeat(scales, len(grid))
params[:, 0] *= mass
params[:, 2] *= mass

r = ilqr.RolloutPolicy(x0, params)
tol = 0.1
err = r.x_final - x_nom
err[:, 0] = (err[:, 0] + np.pi) % (2 * np.pi) - np.pi         # angles modulo a turn
reached = np.isfinite(r.cost) & (np.abs(err[:, 0]) < tol) & (np.abs(err[:, 1]) < 10 * tol)
print(f"{len(x0)} rollouts of {num_steps - 1} steps; rollout kernel {ilqr.policy_kernel_ms():.3f} ms")
for sc in scales:
    sel = mass == sc
    print(f"  mass x {sc:.1f}: {reached[sel].mean() * 100:5.1f} % end within {tol} rad of the upright, "
          f"median cost {np.median(r.cost[sel]):.3f}")
print(f"overall: {reached.mean() * 100:.1f} % of the sampled region")
