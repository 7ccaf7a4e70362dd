"""Parameter identification on one GPU (BatchedIterativeLQR.FitModelParameters; csrc/fit.hpp): kernel time per iteration, the step
evaluations per second that implies, and the NumPy oracle's time for the same work.

    python tools/fit_bench.py [--reps R] [--warmup W] [--batch 1024] [--rows 199] [--iterations 8] [--oracle-problems 4]

Shape: C2's - pendulum, B = 1024, T = 199 transitions per problem (one closed-loop horizon), P = 3 free parameters, starts off by up
to 30 %, noisy data (1e-5) and ftol = 0 so that no problem stops early.  Reported:
  kernel_ms_per_iteration   MI_F_FIT_KERNEL_MS / (I + 1): HIP events from the first evaluation to the closing decision, I + 1 launches
                            of fit_normal_kernel and of fit_update_kernel; `reps` runs after `warmup`: median and min .. max;
  step_evals_per_s          B T G 2 / that time: every lane of fit_normal_kernel - the G = 4 slots of a transition, idle ones
                            included - evaluates the step twice; useful_step_evals_per_s counts the 1 + 2 P a transition needs;
  oracle_ms_per_iteration   tests/fit_np.py on --oracle-problems of the problems, wall time per problem and evaluation, scaled to B.
mppi_rollout_kernel's rate at the same shape (tools/mppi_bench.py: B S (N - 1) step evaluations per rollout) is the project's figure
for a lane-per-item loop over M::step; it is not measured here.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def spread3(v):
    v = np.asarray(v)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=199)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--oracle-problems", type=int, default=4)
    a = ap.parse_args()
    import fit_np as FN
    from drake_ddp_amd import workloads as W
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    from drake_ddp_amd.models import ModelSystem
    from oracle import models_np as M
    p = W.pendulum_problem()
    B, T, I, free = a.batch, a.rows, a.iterations, [0, 1, 2]
    rng = np.random.default_rng(0)
    base = np.array(M.DEFAULT_PARAMS[M.PENDULUM])
    truth = base * (1.0 + 0.1 * rng.uniform(-1, 1, (B, 3)))
    start = truth * (1.0 + 0.3 * rng.uniform(-1, 1, (B, 3)))
    x = np.stack([rng.uniform(-np.pi, np.pi, (B, T)), rng.uniform(-3, 3, (B, T))], axis=2)
    u = rng.uniform(-2, 2, (B, T, 1))
    mo = M.Model(M.PENDULUM, p["dt"])
    # (the pendulum's step, vectorised over the rows: th' = th + dt w', w' = w + dt (u - b w - mgl sin th) / ml2)
    w1 = x[:, :, 1] + p["dt"] * (u[:, :, 0] - truth[:, None, 1] * x[:, :, 1] - truth[:, None, 2] * np.sin(x[:, :, 0])) / truth[:, None, 0]
    xn = np.stack([x[:, :, 0] + p["dt"] * w1, w1], axis=2) + 1e-5 * rng.standard_normal((B, T, 2))
    assert np.allclose(xn[0], FN.predict(mo, truth[0], x[0], u[0]), atol=1e-3)

    s = BatchedIterativeLQR(ModelSystem(p["model_id"], p["dt"]), 4, B, hist_cap=2, pinned_results=False)
    ms, wall = [], []
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        fit = s.FitModelParameters(x, u, xn, free=free, params0=start, iterations=I, ftol=0.0)
        t1 = time.perf_counter()
        if r >= a.warmup:
            ms.append(fit.kernel_ms / (I + 1))
            wall.append((t1 - t0) * 1e3)
    assert np.all(fit.iterations == I), "a problem stopped early: the launches past its end are idle"
    G = 4
    per_it = spread3(ms)
    t0 = time.perf_counter()
    evals = 0
    for b in range(a.oracle_problems):
        o = FN.fit(mo, x[b], u[b], xn[b], start[b], free, iterations=I, ftol=0.0)
        evals += 1 + sum(1 for t in o["trials"] if t[0] is not None)
    oracle_ms = (time.perf_counter() - t0) * 1e3 / max(evals, 1) * B
    out = dict(model="pendulum", B=B, T=T, P=len(free), G=G, iterations=I, kernel_ms_per_iteration=per_it,
               call_wall_ms=spread3(wall), step_evals_per_s=B * T * G * 2 / (per_it["median"] * 1e-3),
               useful_step_evals_per_s=B * T * (1 + 2 * len(free)) / (per_it["median"] * 1e-3), oracle_ms_per_iteration=oracle_ms,
               oracle_problems=a.oracle_problems, worst_relative_parameter_error=float(np.max(np.abs(fit.params / truth - 1.0))),
               accepted=spread3(fit.accepted))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
