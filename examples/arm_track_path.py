#!/usr/bin/env python
"""Tracking a path INSIDE the horizon: the arm + ball task of examples/arm_reach.py (n = 27, m = 7, T = 0.5 s, dt = 1e-2), but the
ball's target is not one point - it moves along a path, 15 cm along +y in B different curves (straight, and bowed towards +x / -x),
and every time index of a solve is pulled towards the path's point at that time (SetTargetTrajectory).  A receding-horizon loop
re-plans every 5 steps; each re-plan's window starts 5 rows further down the path (MPCRun moves the clock), and past the path's end
the target stays at its last point.  One launch for the whole loop, B arms at once.

    python examples/arm_track_path.py"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from drake_ddp_amd import workloads as W  # noqa: E402
from drake_ddp_amd.ilqr import BatchedIterativeLQR  # noqa: E402
from drake_ddp_amd.models import ArmAndBall  # noqa: E402

p = W.arm27_problem()
N, dt = p["N"], p["dt"]
B, num_resolves, replan_steps = 16, 8, 5
T = N + num_resolves * replan_steps                       # rows of the path: the last window ends on its last row

# the ball's path: from where it lies to 15 cm along +y, bowed sideways by up to 3 cm (problem b its own bow)
start = W.arm27_start()
s = np.linspace(0.0, 1.0, T)
bow = np.linspace(-0.03, 0.03, B)
ref = np.tile(p["x_nom"], (B, T, 1))
ref[:, :, 12] = start[12] + 0.15 * s[None, :]
ref[:, :, 11] = start[11] + bow[:, None] * np.sin(np.pi * s)[None, :]

ilqr = BatchedIterativeLQR(ArmAndBall(dt), N, B, beta=0.5, delta=1e-3, gamma=0)
ilqr.SetTargetState(p["x_nom"])                           # (kept, but ignored while the solver holds a reference)
ilqr.SetRunningCost(p["Q"], p["R"])
ilqr.SetTerminalCost(p["Qf"])
ilqr.SetInitialState(np.tile(start, (B, 1)))
ilqr.SetInitialGuess(W.arm27_u_guess(N))
ilqr.SetTargetTrajectory(ref, clock=0)
st = time.time()
x, u, _, cost = ilqr.Solve()
it0 = int(ilqr.iterations.sum())
stats = ilqr.MPCRun(num_resolves, replan_steps)
ms = (time.time() - st) * 1e3
log = ilqr.mpc_log                                        # (B, num_resolves, n + 2): x0 of each re-plan | cost | iterations
print(f"{B} paths x (1 + {num_resolves}) solves in {ms:.1f} ms: {it0} + {stats.total_iters} iLQR iterations, "
      f"all converged: {stats.n_converged == B}; the reference's clock reads {ilqr.target_clock} of {T} rows")
k = np.arange(1, num_resolves + 1) * replan_steps         # the path's row at the start of each re-plan
err = np.hypot(log[:, :, 11] - ref[:, k, 11], log[:, :, 12] - ref[:, k, 12])
for b in (0, B // 2, B - 1):
    print(f"path {b:2d} (bow {bow[b] * 100:+.1f} cm): ball at the last re-plan ({log[b, -1, 11]:.3f}, {log[b, -1, 12]:.3f}) m, the path there "
          f"({ref[b, k[-1], 11]:.3f}, {ref[b, k[-1], 12]:.3f}) m; distance from the path over the loop {err[b].min() * 100:.1f}..{err[b].max() * 100:.1f} cm")
