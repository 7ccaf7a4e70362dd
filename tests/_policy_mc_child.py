"""Helper of tests/test_gpu_policy_mc.py (the passes test): one on-device Monte-Carlo run on a freshly solved pendulum handle, S = 130
with the samples, in THIS process - whose environment decides the window (MI_ILQR_MC_PASS_GROUPS is read once per process).
`python tests/_policy_mc_child.py OUT.npz` writes the ten numbers and the samples; the test calls run() itself for the default."""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELDS = ("n", "counted", "success", "mean", "m2", "min", "max", "argmin", "argmax", "steps_total")


def run():
    from drake_ddp_amd import workloads as W
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    from drake_ddp_amd.models import ModelSystem
    B, S = 3, 130
    p = dict(W.pendulum_problem(), N=40)
    s = BatchedIterativeLQR(ModelSystem(p["model_id"], p["dt"]), p["N"], B, delta=p["delta"], beta=p["beta"], gamma=p["gamma"], device=0,
                            max_iters=3)
    s.SetTargetState(p["x_nom"]); s.SetRunningCost(p["Q"], p["R"]); s.SetTerminalCost(p["Qf"])
    x0b = W.pendulum_batch_x0(B)
    s.SetInitialState(x0b); s.SetInitialGuess(np.zeros((1, p["N"] - 1)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        s.Solve()
    base = np.asarray(s.system.params, dtype=float)
    st = s.RolloutPolicyStats(S, x0b, [0.05, 0.1], params_mean=base, params_spread=0.1 * base, goal=[0.5, np.inf], state_noise=1e-3,
                              control_noise=1e-2, seed=77, first_sample=3, samples=True)
    out = {k: getattr(st, k) for k in FIELDS}
    out.update(x0=st.samples.x0, params=st.samples.params, cost=st.samples.cost, steps=st.samples.steps, passes=s.policy_mc_passes())
    return out


if __name__ == "__main__":
    np.savez(sys.argv[1], **run())
