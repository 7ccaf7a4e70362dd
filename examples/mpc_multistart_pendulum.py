#!/usr/bin/env python
"""Multi-start in the receding-horizon loop: a pendulum swing-up replanned every few steps, G random starts under K seeds each in ONE
batch of G x K problems.  Between two re-solves the seeds of a group are joined on the device
(BatchedIterativeLQR.MPCRunMultiStart): the group's best plan, shifted, goes to every member - unperturbed into the winner's own
slot, plus held torque noise into the others - together with the state to start from, so one bad warm start is not carried from
re-solve to re-solve.  The same starts run beside it with K = 1, the plain loop.  Closed loop with disturbances (SetPlant): every
group has ONE plant, which advances under the winner's policy with process and actuation noise, and every member's next re-solve
starts from the plant's state - one the plan did not predict.  The loop is run one re-solve per call - splitting a run is exact -
so that every re-solve's statuses can be read.  Asserts only what holds by construction: after every re-solve the group's
best cost is no larger than the cost of the slot that continued the previous winner's plan unperturbed, wherever that slot is
eligible.  Prints how many groups end within the goal, and ends with a fixed line."""
import argparse
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from drake_ddp_amd.ilqr import BatchedIterativeLQR  # noqa: E402
from drake_ddp_amd.models import Pendulum  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--groups", type=int, default=64, help="random starts")
ap.add_argument("--seeds", type=int, default=8, help="seeds per start")
ap.add_argument("--resolves", type=int, default=20)
ap.add_argument("--replan", type=int, default=10, help="steps between two re-solves")
ap.add_argument("--steps", type=int, default=200, help="time steps of the horizon (dt = 0.01)")
ap.add_argument("--sigma", type=float, default=0.5, help="standard deviation of the torque noise of the seeds")
ap.add_argument("--disturbance", type=float, default=0.2, help="standard deviation of the plant's actuation noise (its process noise is a tenth)")
args = ap.parse_args()

G, dt, N, R, replan = args.groups, 1e-2, args.steps, args.resolves, min(args.replan, args.steps - 2)
rng = np.random.default_rng(0)
starts = np.stack([rng.uniform(-np.pi, np.pi, G), rng.uniform(-1.0, 1.0, G)], axis=1)
target = np.array([np.pi, 0.0])


def loop(K):
    """-> (G, 2) the groups' plant states after the last segment, (G,) the cost of every group's best member."""
    ilqr = BatchedIterativeLQR(Pendulum(dt), N, G * K)
    ilqr.SetInitialState(np.repeat(starts, K, axis=0))             # group g: problems g K .. g K + K - 1, the same start
    ilqr.SetTargetState(target)
    ilqr.SetRunningCost(dt * 0.01 * np.diag([0, 1]), dt * 0.01 * np.eye(1))
    ilqr.SetTerminalCost(100 * np.diag([1, 1]))
    ilqr.SetInitialGuess(np.zeros((1, N - 1)))
    ms = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        if K > 1:
            ilqr.PerturbInitialGuess(K, 2.0 * args.sigma, seed=2025, round=0, hold=10)
        ilqr.Solve()
        # the same plants and - lane g draws the normals of problem index g - the same disturbances for every K
        ilqr.SetPlant(np.repeat(starts, K, axis=0), state_noise=0.1 * args.disturbance * dt, control_noise=args.disturbance, seed=7)
        for r in range(R):
            before, after = ilqr.MPCRunMultiStart(K, 1, replan, args.sigma, seed=2025, round=r + 1, hold=10)
            ms += ilqr.seeds_kernel_ms()
            cost, st = np.array(ilqr.cost), np.array(ilqr.status) & ~16
            eligible = np.isin(st, (0, 1)) & np.isfinite(cost)
            for g in np.flatnonzero(before.winner >= 0):
                slot = before.problem[g]                           # it continued the winner's plan, unperturbed
                assert not eligible[slot] or after.cost[g] <= cost[slot], (K, r, g)
    row = ilqr.mpc_winner_log([before, after])[:, 0, :]
    print(f"K = {K}: {int((after.winner >= 0).sum())} of {G} groups hold a plan after {R} re-solves, mean best cost {np.nanmean(row[:, 2]):.4f}, "
          f"join kernels {ms:.3f} ms")
    return np.array(ilqr.plant_state)[::K], row[:, 2]


def within_goal(x):
    d = np.abs((x[:, 0] - target[0] + np.pi) % (2.0 * np.pi) - np.pi)
    return (d < 0.3) & (np.abs(x[:, 1]) < 1.0)


x1, c1 = loop(1)
xk, ck = loop(args.seeds)
print(f"groups within the goal after {R * replan} steps: {int(within_goal(x1).sum())} of {G} with K = 1, "
      f"{int(within_goal(xk).sum())} of {G} with K = {args.seeds}")
print("mpc_multistart_pendulum: OK")
