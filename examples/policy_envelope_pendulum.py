#!/usr/bin/env python
"""How wide is the tube around a solved swing-up, and does it stay where it is safe?  Four pendulum swing-ups are solved in one batch;
each problem's feedback policy is then evaluated by Monte-Carlo on the GPU (BatchedIterativeLQR.RolloutPolicyStats) with
envelope=True, controls=True and a safety box: 8192 samples per problem, starts uniform in a box around the problem's own start,
plant parameters within +-10 %, actuation noise - and beside the cost statistics the device reduces, per time step, the mean, spread
and extremes of the states and of the commanded torque over the samples, and counts the samples whose rate never exceeds 9 rad/s.
Prints the tube's half-width at a few steps of problem 0, the largest torque any sample asked for, and the share that stays inside."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from drake_ddp_amd.ilqr import BatchedIterativeLQR  # noqa: E402
from drake_ddp_amd.models import Pendulum  # noqa: E402

T, dt, S = 2.0, 1e-2, 8192
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

rate_max = 9.0
st = ilqr.RolloutPolicyStats(S, starts, [0.3, 0.6], x0_dist="uniform", params_mean=system.params, params_spread=0.1 * np.abs(system.params),
                             goal=[0.1, 1.0], control_noise=0.02, seed=2024,
                             envelope=True, controls=True, safe_box=([-np.inf, -rate_max], [np.inf, rate_max]))
env, ctl, safety = st.envelope, st.control_envelope, st.safety
print(f"{S} samples per problem, {num_steps - 1} steps each; problem 0, angle:")
for t in (0, num_steps // 4, num_steps // 2, 3 * num_steps // 4, num_steps - 1):
    half = 0.5 * (env.max[0, t, 0] - env.min[0, t, 0])
    print(f"step {t:3d}: half-width {half:.4f} rad, mean {env.mean[0, t, 0]:+.4f}, std {np.sqrt(env.var[0, t, 0]):.4f}")
print(f"largest commanded torque of problem 0: {np.abs([ctl.min[0], ctl.max[0]]).max():.3f} (sample {ctl.argmax[0].ravel()[np.argmax(ctl.max[0])]})")
for b in range(B):
    first = np.flatnonzero(safety.exits[b])
    print(f"  start ({starts[b, 0]:+.1f}, {starts[b, 1]:+.1f}): inside the box: {100.0 * safety.safe[b] / S:.2f} %, inside and at the goal "
          f"{100.0 * safety.safe_success[b] / S:.2f} %, success without the box {100.0 * st.success_rate[b]:.2f} %"
          + (f", first exit at step {first[0]}" if first.size else ""))
