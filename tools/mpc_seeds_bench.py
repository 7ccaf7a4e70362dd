"""What joining the seeds between two re-solves of the receding-horizon loop costs, on C2's shape (pendulum swing-up, N = 200, groups
of K = 8 seeds, B = 1024 and B = 65 536 problems), replan_steps = 10, hold = 1 and 10.

    python tools/mpc_seeds_bench.py [--reps R] [--batches 1024,65536] [--holds 1,10]

Per batch size and hold, on ONE solved handle, after two warm-ups, median and range (min .. max) of R repetitions:
  (a) the join kernel by its own events: MPCRunMultiStart(K, 1, ...) then seeds_kernel_ms() - select, shift, reseed and the x0 rows in
      one launch.
  (b) ReseedFromBest by its own events on the same handle (what tools/seeds_bench.py measures): select + reseed, without the shift
      and the x0 rows the composition needs beside it.
  (c) wall clock per re-solve: MPCRunMultiStart(K, 1, ...) against the loop written out in Python - MPCShift, ReseedFromBest, the
      winners' x_bar[:, replan_steps] read back and handed out with mi_ilqr_set_initial, solve_resident.
A tree without MPCRunMultiStart (the parent commit) reports (b) and the composition of (c) alone, so the same file serves both sides
of an A/B.  One JSON line."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, SIGMA, SEED, REPLAN = 8, 0.25, 2025, 10


def _stat(v):
    return dict(median=float(np.median(v)), range=[float(min(v)), float(max(v))])


def run(B, hold, reps):
    from drake_ddp_amd import _capi, workloads as W
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    from drake_ddp_amd.models import ModelSystem
    p = W.pendulum_problem()
    N, G = p["N"], B // K

    def solver():
        s = BatchedIterativeLQR(ModelSystem(p["model_id"], p["dt"]), N, B, delta=p["delta"], beta=p["beta"], gamma=p["gamma"], hist_cap=2,
                                pinned_results=False)
        s.SetTargetState(p["x_nom"]); s.SetRunningCost(p["Q"], p["R"]); s.SetTerminalCost(p["Qf"])
        s.SetInitialState(np.repeat(W.pendulum_batch_x0(G), K, axis=0)); s.SetInitialGuess(np.zeros((1, N - 1)))
        s.PerturbInitialGuess(K, 2.0 * SIGMA, seed=SEED, hold=10)
        s.Solve()
        return s
    out = dict(B=B, K=K, N=N, hold=hold, replan_steps=REPLAN)
    s = solver()
    reseed = []
    for r in range(reps + 2):                                    # (b)
        s.ReseedFromBest(K, SIGMA, seed=SEED, round=r + 1, hold=hold)
        if r >= 2:
            reseed.append(s.seeds_kernel_ms())
        s.solve_resident()
    out["reseed_kernel_ms"] = _stat(reseed)
    s = solver()
    wall = []
    for r in range(reps + 2):                                    # (c), written out
        t0 = time.perf_counter()
        x = np.array(s.x_bar)
        s.MPCShift(REPLAN)
        sel = s.ReseedFromBest(K, SIGMA, seed=SEED, round=r + 1, hold=hold)
        src = np.where(np.repeat(sel.winner, K) >= 0, np.repeat(sel.problem, K), np.arange(B))
        x0 = np.ascontiguousarray(x[src][:, :, REPLAN])
        _capi.check(s._lib.mi_ilqr_set_initial(s._h, _capi.ptr(x0), None), "mi_ilqr_set_initial")
        s.solve_resident()
        if r >= 2:
            wall.append((time.perf_counter() - t0) * 1e3)
    out["composition_wall_ms_per_resolve"] = _stat(wall)
    if hasattr(BatchedIterativeLQR, "MPCRunMultiStart"):
        s = solver()
        join, wall = [], []
        for r in range(reps + 2):                                # (a) and (c)
            t0 = time.perf_counter()
            s.MPCRunMultiStart(K, 1, REPLAN, SIGMA, seed=SEED, round=r + 1, hold=hold)
            if r >= 2:
                wall.append((time.perf_counter() - t0) * 1e3)
                join.append(s.seeds_kernel_ms())
        out["join_kernel_ms"] = _stat(join)
        out["multistart_wall_ms_per_resolve"] = _stat(wall)
        out["join_over_reseed"] = out["join_kernel_ms"]["median"] / out["reseed_kernel_ms"]["median"]
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", default="1024,65536")
    ap.add_argument("--holds", default="1,10")
    args = ap.parse_args()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        print(json.dumps([run(int(b), int(h), args.reps) for b in args.batches.split(",") for h in args.holds.split(",")]))
