#!/usr/bin/env python
"""Receding-horizon control of a batch of cheetah-SHAPED models (n=36, m=12), every seed walking at its OWN target speed from its
own start: the loop of the reference's mini_cheetah.py (:147-201) run on one object per seed, in one batch.  Each seed's target
(base x position and velocity) is set per problem with SetTargetState((B, n)), and MPCRun's target_step is (B, n): seed b's base x
target moves by v_b * dt * replan_steps before every re-solve (include/mi_ilqr.h: "Per-problem targets")."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from drake_ddp_amd import workloads as W  # noqa: E402
from drake_ddp_amd.ilqr import BatchedIterativeLQR  # noqa: E402
from drake_ddp_amd.models import Synth36  # noqa: E402

B, num_resolves, replan_steps = 64, 20, 4
p = W.synth36_problem()
num_steps, dt = p["N"], p["dt"]
speeds = W.SYNTH_TARGET_VEL * np.linspace(0.0, 2.0, B)    # one target velocity per seed

x_nom = np.tile(p["x_nom"], (B, 1))
x_nom[:, 0] = speeds * num_steps * dt                      # base x position target at the end of the horizon (mini_cheetah.py:56)
x_nom[:, 18] = speeds                                      # base x velocity target (:57)
x0 = W.synth36_batch_x0(B)

ilqr = BatchedIterativeLQR(Synth36(dt), num_steps, B, beta=0.5, delta=1e-2, gamma=0)
ilqr.SetTargetState(x_nom)
ilqr.SetRunningCost(p["Q"], p["R"])
ilqr.SetTerminalCost(p["Qf"])
ilqr.SetInitialState(x0)
ilqr.SetInitialGuess(W.synth36_u_guess(num_steps))

st = time.time()
ilqr.Solve()
step = np.zeros((B, 36))
step[:, 0] = speeds * dt * replan_steps                    # every seed's base x target moves at its own speed
stats = ilqr.MPCRun(num_resolves, replan_steps, target_step=step)
elapsed = time.time() - st
log = ilqr.mpc_log                                         # (B, num_resolves, n + 2): x0 of each re-solve | cost | iterations
progress = log[:, -1, 0] - x0[:, 0]                        # base x travelled by the start of the last re-solve
wanted = speeds * dt * replan_steps * (num_resolves - 1)   # ... and what the target speed asks for over the same steps
for b in range(0, B, B // 8):
    print(f"seed {b:2d}: target {speeds[b]:.3f} m/s, base x moved {progress[b]:+.4f} m (target {wanted[b]:+.4f} m)")
print(f"{B} seeds at {B} target speeds x (1 + {num_resolves}) solves in {elapsed * 1e3:.1f} ms; {stats.total_iters} iLQR "
      f"iterations in the re-solves; {stats.n_converged} of {B} converged; corr(progress, target) "
      f"{np.corrcoef(progress, wanted)[0, 1]:.3f}")
