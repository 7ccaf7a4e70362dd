"""Time per re-solve of the closed MPC loop (SetPlant + MPCRun; csrc/plant_advance.hpp) on one GPU, beside the only equivalent the
library offered before it and beside the open loop:

    (a) closed-loop MPCRun;
    (b) the Python emulation: RolloutPolicy(S = 1, trajectories=True) for the plant's segment, MPCShift, an x0 upload, solve_resident
        - one host round trip per re-solve (runs on a tree without SetPlant too: --only b);
    (c) the open loop in its host-loop form: MPCShift + solve_resident per re-solve, the launches mi_ilqr_mpc_run itself makes for
        the kernel families and horizons that loop on the host (the pendulum and the quadruped at these shapes take the single-launch
        form otherwise, so the form is spelled out here; it runs on a tree without SetPlant too).

    python tools/closed_loop_bench.py [--reps R] [--warmup W] [--configs pendulum,quad3d] [--resolves K] [--replan r] [--only a,b,c]

Shapes: pendulum B = 1024, N = 200; Quad3D B = 64, N = 40; each without and with noise.  Every repetition starts from the same
solved handle state (a capped solve, then Reset-free re-arming by a fresh Solve()); timed are host wall time of the whole call and
the HIP-event time of the solves (stats.kernel_ms) and of the plant kernels (plant_kernel_ms), all divided by the number of
re-solves; median with min .. max over `reps` after `warmup`.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problem(config):
    from drake_ddp_amd import workloads as W
    if config == "quad3d":
        p, B = W.quad3d_problem(40), 64
        return p, B, W.quad3d_batch_x0(B), W.quad3d_u_guess(40)
    p, B = W.pendulum_problem(), 1024
    return p, B, W.pendulum_batch_x0(B), np.zeros((1, p["N"] - 1))


def noise(config, n):
    if config == "quad3d":
        sx = np.full(n, 1e-3)
        sx[:4] = 0.0
        return sx, 5e-2
    return np.full(n, 3e-3), 1e-2


def solver(p, B, x0, ug, max_iters):
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    from drake_ddp_amd.models import ModelSystem
    s = BatchedIterativeLQR(ModelSystem(p["model_id"], p["dt"]), p["N"], B, delta=p["delta"], beta=p["beta"], gamma=p["gamma"],
                            hist_cap=2, pinned_results=False, max_iters=max_iters)
    s.SetTargetState(p["x_nom"]); s.SetRunningCost(p["Q"], p["R"]); s.SetTerminalCost(p["Qf"])
    s.SetInitialState(x0); s.SetInitialGuess(ug)
    return s


def summary(rows):
    a = np.asarray(rows)
    return {k: dict(median=float(np.median(a[:, i])), min=float(a[:, i].min()), max=float(a[:, i].max()))
            for i, k in enumerate(("wall_ms", "solve_kernel_ms", "plant_kernel_ms"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--configs", default="pendulum,quad3d")
    ap.add_argument("--resolves", type=int, default=8)
    ap.add_argument("--replan", type=int, default=4)
    ap.add_argument("--only", default="a,b,c")
    ap.add_argument("--max-iters", type=int, default=20)
    args = ap.parse_args()
    warnings.simplefilter("ignore", RuntimeWarning)
    R, r, only = args.resolves, args.replan, set(args.only.split(","))
    out = dict(resolves=R, replan_steps=r, reps=args.reps, warmup=args.warmup, results={})
    for config in args.configs.split(","):
        p, B, x0, ug = problem(config)
        n = x0.shape[1]
        s = solver(p, B, x0, ug, args.max_iters)
        has_plant = hasattr(s, "SetPlant")
        for noisy in (False, True):
            sx, su = noise(config, n)
            kw = dict(state_noise=sx, control_noise=su, seed=11) if noisy else {}
            rows = {k: [] for k in "abc"}
            for rep in range(args.warmup + args.reps):
                for which in "abc":
                    if which not in only or (which == "a" and not has_plant):
                        continue
                    s.SetInitialState(x0); s.SetInitialGuess(ug)
                    s.Solve()
                    plant_ms = 0.0
                    if which == "a":
                        s.SetPlant(x0, **kw)
                        t0 = time.perf_counter()
                        st = s.MPCRun(R, r)
                        wall, solve_ms, plant_ms = time.perf_counter() - t0, st.kernel_ms, s.plant_kernel_ms()
                        s.ClearPlant()
                    elif which == "c":
                        solve_ms = 0.0
                        t0 = time.perf_counter()
                        for k in range(R):
                            s.MPCShift(r)
                            solve_ms += s.solve_resident().kernel_ms
                        wall = time.perf_counter() - t0
                    else:
                        from drake_ddp_amd import _capi
                        x, solve_ms = np.ascontiguousarray(x0), 0.0
                        t0 = time.perf_counter()
                        for k in range(R):
                            ro = s.RolloutPolicy(x[:, None, :], trajectories=True, first_sample=0, **(dict(kw, seed=11 + k) if noisy else {}))
                            x = np.ascontiguousarray(ro.X[:, 0, :, r])
                            s.MPCShift(r)
                            _capi.check(s._lib.mi_ilqr_set(s._h, _capi.F_X0, _capi.ptr(x), x.nbytes), "mi_ilqr_set")
                            solve_ms += s.solve_resident().kernel_ms
                        wall = time.perf_counter() - t0
                    if rep >= args.warmup:
                        rows[which].append((wall * 1e3 / R, solve_ms / R, plant_ms / R))
            out["results"]["%s%s" % (config, "_noise" if noisy else "")] = {
                dict(a="closed_loop", b="python_emulation", c="host_loop_without_plant")[k]: summary(v) for k, v in rows.items() if v}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
