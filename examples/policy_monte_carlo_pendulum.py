#!/usr/bin/env python
"""How robust is a solved swing-up policy?  Four pendulum swing-ups from different starts are solved in one batch; each problem's
feedback policy u = u_bar - K (x - x_bar) is then evaluated by Monte-Carlo ENTIRELY ON THE GPU (BatchedIterativeLQR.RolloutPolicyStats):
65 536 samples per problem, their starts drawn uniformly from a box around the problem's own start and their plants' mass parameters
(m l^2 and m g l) and damping drawn uniformly within +-10 %, a small actuation noise on top - drawn, rolled out and reduced on the
device, so that one row per problem comes back: how many samples reached the upright, and the mean, spread and worst cost.  Prints
one line per problem."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from drake_ddp_amd.ilqr import BatchedIterativeLQR  # noqa: E402
from drake_ddp_amd.models import Pendulum  # noqa: E402

T, dt, S = 2.0, 1e-2, 65536
x_nom = np.array([np.pi, 0])
num_steps = int(T / dt)
system = Pendulum(dt)
starts = np.array([[0.0, 0.0], [0.5, 0.0], [-0.5, 0.0], [0.0, 1.0]])
B = len(starts)
ilqr = BatchedIterativeLQR(system, num_steps, B)
ilqr.SetInitialState(starts)
ilqr.SetTargetState(x_nom)
ilqr.SetRunningCost(dt * 0.01 * np.diag([0, 1]), dt * 0.01 * np.eye(1))
ilqr.SetTerminalCost(100 * np.diag([1, 1]))
ilqr.SetInitialGuess(np.zeros((1, num_steps - 1)))
ilqr.Solve()
print(f"{B} swing-ups solved, costs {np.array2string(np.asarray(ilqr.cost), precision=3)}")

st = ilqr.RolloutPolicyStats(S, starts, [0.3, 0.6], x0_dist="uniform",                       # a box of starts around each problem's own
                             params_mean=system.params, params_spread=0.1 * np.abs(system.params), params_dist="uniform",
                             goal=[0.1, 1.0],                                                 # |angle - pi| <= 0.1 rad, |rate| <= 1 rad/s at the end
                             control_noise=0.02, seed=2024)
print(f"{S} samples per problem, {num_steps - 1} steps each; rollout kernels {ilqr.policy_kernel_ms():.3f} ms")
for b in range(B):
    print(f"  start ({starts[b, 0]:+.1f}, {starts[b, 1]:+.1f}): success rate {st.success_rate[b]:.4f}, cost mean {st.mean[b]:.3f} "
          f"std {np.sqrt(st.var[b]):.3f} min {st.min[b]:.3f} max {st.max[b]:.3f} (worst: sample {st.argmax[b]})")
