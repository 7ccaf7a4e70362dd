#!/usr/bin/env python
"""Sampling-based MPC (MPPI / predictive sampling) on the pendulum swing-up: no Jacobians, no line search.  From random starts and a
zero torque guess every problem improves its own plan on the GPU by rounds of { S perturbed copies of the plan, sample 0 the plan
itself; their rollouts; the weighted mean, with temperature = 0 the best sample alone } (BatchedIterativeLQR.MPPIRun) - the
iteration loop never leaves the device.  Three answers per start, side by side: MPPI alone; MPPI followed by Solve(), which polishes
the sampled plan (the run leaves it as the solver's pending guess); and Solve() from the zero guess.  Prints the costs and ends
with a fixed line."""
import argparse
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from drake_ddp_amd.ilqr import BatchedIterativeLQR  # noqa: E402
from drake_ddp_amd.models import Pendulum  # noqa: E402


def make(starts, N, dt):
    ilqr = BatchedIterativeLQR(Pendulum(dt), N, len(starts))
    ilqr.SetInitialState(starts)
    ilqr.SetTargetState(np.array([np.pi, 0]))
    ilqr.SetRunningCost(dt * 0.01 * np.diag([0, 1]), dt * 0.01 * np.eye(1))
    ilqr.SetTerminalCost(100 * np.diag([1, 1]))
    ilqr.SetInitialGuess(np.zeros((1, N - 1)))
    return ilqr


def main(problems=16, samples=256, iterations=30, steps=100, sigma=1.0, temperature=0.0, hold=5, quiet=False):
    """-> dict: mppi_cost (iterations + 1, B) the plan's cost before every round and at the end, polished_cost (B,) after Solve()
    from the sampled plan, solve_cost (B,) of Solve() from the zero guess."""
    dt, N = 1e-2, steps
    rng = np.random.default_rng(0)
    starts = np.stack([rng.uniform(-0.5, 0.5, problems), rng.uniform(-1.0, 1.0, problems)], axis=1)
    say = (lambda *a: None) if quiet else print
    mppi = make(starts, N, dt)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)              # (a solve stopped at max_iters is an outcome here)
        r = mppi.MPPIRun(samples, iterations, sigma, temperature, seed=2025, hold=hold)
        say(f"MPPI alone, {iterations} rounds of {samples} samples: mean cost {r.nominal_cost[0].mean():.4f} -> {r.nominal_cost[-1].mean():.4f}, "
            f"kernels {r.kernel_ms:.3f} ms ({r.kernel_ms / iterations:.4f} ms per round for {problems} problems)")
        mppi.Solve()                                                 # the sampled plan is the pending guess: polish it
        polished = np.array(mppi.cost)
        plain = make(starts, N, dt)
        plain.Solve()
        solve = np.array(plain.cost)
    say(f"MPPI then Solve(): mean cost {polished.mean():.4f} in {np.array(mppi.iterations).mean():.1f} iterations")
    say(f"Solve() from zeros: mean cost {solve.mean():.4f} in {np.array(plain.iterations).mean():.1f} iterations")
    say(f"polished plan at or below the plain solve in {int((polished <= solve).sum())} of {problems} problems")
    return dict(mppi_cost=r.nominal_cost, polished_cost=polished, solve_cost=solve)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=16, help="random starts (more than 4)")
    ap.add_argument("--samples", type=int, default=256, help="samples per problem and round")
    ap.add_argument("--iterations", type=int, default=30)
    ap.add_argument("--steps", type=int, default=100, help="time steps of the horizon (dt = 0.01)")
    ap.add_argument("--sigma", type=float, default=1.0, help="standard deviation of the torque disturbance")
    ap.add_argument("--temperature", type=float, default=0.0, help="0: predictive sampling, the best sample alone")
    ap.add_argument("--hold", type=int, default=5, help="steps a disturbance is held")
    a = ap.parse_args()
    out = main(a.problems, a.samples, a.iterations, a.steps, a.sigma, a.temperature, a.hold)
    if a.temperature == 0.0:
        assert np.all(np.diff(out["mppi_cost"], axis=0) <= 0.0)      # the elite slot: the plan's cost never rises
    assert np.all(out["mppi_cost"][-1] < out["mppi_cost"][0])
    print("mppi_pendulum: OK")
