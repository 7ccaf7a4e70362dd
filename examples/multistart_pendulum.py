#!/usr/bin/env python
"""Multi-start swing-up: iLQR is a local method, and from a random start the pendulum's answer depends on the initial torque guess.
G random starts are each solved under K guesses in ONE batch of G x K problems: member 0 of a group starts from the zero guess (the
single start), the others from torques drawn on the GPU and held for a few steps (BatchedIterativeLQR.PerturbInitialGuess); after a
solve every group's losers are reseeded around its winner with a smaller sigma (ReseedFromBest) and solved again; the winners come
back at the end (GatherBest).  Nothing of the size of the guesses crosses the bus between the rounds.  Prints the selection of
every round, in how many groups best-of-K is strictly below member 0 - the same start solved alone - and ends with a fixed line."""
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
ap.add_argument("--seeds", type=int, default=8, help="guesses per start")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=200, help="time steps of the horizon (dt = 0.01)")
ap.add_argument("--sigma", type=float, default=1.0, help="standard deviation of the torque disturbance of round 0")
args = ap.parse_args()

G, K, dt, N = args.groups, args.seeds, 1e-2, args.steps
rng = np.random.default_rng(0)
starts = np.stack([rng.uniform(-np.pi, np.pi, G), rng.uniform(-1.0, 1.0, G)], axis=1)
ilqr = BatchedIterativeLQR(Pendulum(dt), N, G * K)
ilqr.SetInitialState(np.repeat(starts, K, axis=0))                 # group g: problems g K .. g K + K - 1, the same start
ilqr.SetTargetState(np.array([np.pi, 0]))
ilqr.SetRunningCost(dt * 0.01 * np.diag([0, 1]), dt * 0.01 * np.eye(1))
ilqr.SetTerminalCost(100 * np.diag([1, 1]))
ilqr.SetInitialGuess(np.zeros((1, N - 1)))

with warnings.catch_warnings():
    warnings.simplefilter("ignore", RuntimeWarning)
    ilqr.PerturbInitialGuess(K, args.sigma, seed=2025, round=0, hold=10)
    ilqr.Solve()
    single = np.array(ilqr.cost)[::K]                              # member 0 of round 0: the unperturbed start
    for r in range(args.rounds):
        sel = ilqr.SelectBest(K)
        print(f"round {r}: winners {sel.winner.tolist()}, eligible {sel.eligible.tolist()}, mean best cost {sel.cost.mean():.4f}, "
              f"select kernel {ilqr.seeds_kernel_ms():.4f} ms")
        if r == 0:
            assert np.all(sel.cost <= single)                      # the elite slot: best-of-K never loses to the single start
        if r + 1 < args.rounds:
            ilqr.ReseedFromBest(K, args.sigma * 0.5 ** (r + 1), seed=2025, round=r + 1, hold=10)
            ilqr.Solve()
x, u, cost, sel = ilqr.GatherBest(K)
better = int((cost < single).sum())
print(f"best-of-{K} cost is strictly below member 0's in {better} of {G} groups (mean {single.mean():.4f} -> {cost.mean():.4f})")
assert x.shape == (G, 2, N) and u.shape == (G, 1, N - 1) and np.array_equal(cost, sel.cost)
print("multistart_pendulum: OK")
