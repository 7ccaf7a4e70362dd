"""How much disturbance does the pendulum's swing-up policy take?  Solve the swing-up once, then roll the solved feedback policy
u = u_bar - K (x - x_bar) out under process and actuation noise of growing size - S samples per noise level, one GPU lane per
sample, the normals generated on the device (RolloutPolicy's state_noise / control_noise) - and report how many samples still end
near the upright.

    python examples/policy_noise_robustness.py [--samples 4096] [--seed 0]

Every noise level is one problem of a batched solver: the B problems share x0, so they hold the same policy, and each gets its own
sigma row.  common_noise=True gives every level the SAME normals, scaled - the success rates are then monotone in the level up to
the dynamics, not up to sampling error."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from drake_ddp_amd import workloads as W
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    from drake_ddp_amd.models import ModelSystem
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    p = W.pendulum_problem()
    levels = np.array([0.0, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0])          # multiples of the unit disturbance below
    B, N = len(levels), p["N"]
    s = BatchedIterativeLQR(ModelSystem(p["model_id"], p["dt"]), N, B, delta=p["delta"], beta=p["beta"], gamma=p["gamma"])
    s.SetTargetState(p["x_nom"]); s.SetRunningCost(p["Q"], p["R"]); s.SetTerminalCost(p["Qf"])
    s.SetInitialState(np.zeros((B, 2)));                                   # hanging down, at rest (examples/swingup_pendulum.py)
    s.SetInitialGuess(np.zeros((1, N - 1)))
    s.Solve()
    unit_x, unit_u = np.array([1e-3, 1e-2]), np.array([0.05])             # rad, rad/s per step; N m
    x0 = np.broadcast_to(np.array(s.x_bar)[:, None, :, 0], (B, a.samples, 2))
    r = s.RolloutPolicy(x0, state_noise=levels[:, None] * unit_x, control_noise=levels[:, None] * unit_u, seed=a.seed, common_noise=True)
    err = r.x_final - p["x_nom"]
    err[..., 0] = (err[..., 0] + np.pi) % (2.0 * np.pi) - np.pi             # the upright, whichever way round
    ok = (np.abs(err[..., 0]) < 0.1) & (np.abs(err[..., 1]) < 0.5) & (r.steps == N - 1)
    print("pendulum swing-up under noise: %d samples per level, kernel %.3f ms" % (a.samples, s.policy_kernel_ms()))
    print("  level   sigma_theta  sigma_omega  sigma_u   success   median cost")
    for b, k in enumerate(levels):
        print("  %5.2f   %.2e     %.2e     %.2e  %6.1f %%   %.4g" % (k, k * unit_x[0], k * unit_x[1], k * unit_u[0], 100.0 * ok[b].mean(),
                                                                   float(np.median(r.cost[b]))))


if __name__ == "__main__":
    main()
