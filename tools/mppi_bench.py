"""Sampling-based MPC on one GPU (BatchedIterativeLQR.MPPIRun; csrc/mppi.hpp): kernel time per iteration, the rollout / update split, and
the host emulation the on-device loop replaces.

    python tools/mppi_bench.py [--reps R] [--warmup W] [--configs c2,c5] [--samples 256,1024] [--iterations 10] [--emulate-up-to P] [--split]

Shapes: C2's - pendulum, B = 1024, N = 200 - and C5's - Synth36, B = 64, N = 40 - at S = 256 and 1024 samples per problem, I = 10
iterations from the workload's own initial guess; sigma 0.5 (pendulum) / 0.05 (chain), held 5 steps, temperature of the order of the
costs' spread.  Per shape:
  kernel_ms_per_iteration   MI_F_SEEDS_KERNEL_MS / I: HIP events around the whole run (staging, I x { rollout, update }, the closing
                            rollout, the hand-over), `reps` runs after `warmup`: median and min .. max;
  stored_variant            what a variant that STORES the applied controls would move per iteration - B S (N-1) m doubles written
                            by the rollout and read by the update - and the time that takes at the HBM rate the guide measures
                            (6.3 TB/s), to set beside the update kernel's time: regenerating the normals is what is built;
  emulation                 the same iteration on the host, timed in the same session where B S <= --emulate-up-to: sampling in NumPy
                            (PerturbInitialGuess-style: base + sigma z, held), a (B S)-problem handle whose pending guess is the
                            samples and one RolloutPolicy on it (cold: no gains, the open-loop cost), the weights and the blend in
                            NumPy - wall time per iteration, and its three parts.
--split: one more run per shape under `rocprofv3 --kernel-trace --stats` in a child process (a trace of its own, no counters): the
summed time of mppi_rollout_kernel and of mppi_update_kernel per iteration; the child runs under a time limit, and when it fails or
does not end the tool ends there and starts nothing more on the GPU.  Prints one JSON line."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12
CHILD_TIMEOUT_S = 300              # the profiled child: one run of a shape that takes seconds


def problem(config):
    from drake_ddp_amd import workloads as W
    if config == "c5":
        p, B = W.synth36_problem(40), 64
        return p, B, W.synth36_batch_x0(B), W.synth36_u_guess(40), 0.05, 1e-3
    p, B = W.pendulum_problem(), 1024
    return p, B, W.pendulum_batch_x0(B), np.zeros((1, p["N"] - 1)), 0.5, 10.0


def solver(p, B, **kw):
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    from drake_ddp_amd.models import ModelSystem
    s = BatchedIterativeLQR(ModelSystem(p["model_id"], p["dt"]), p["N"], B, delta=p["delta"], beta=p["beta"], gamma=p["gamma"],
                            hist_cap=2, pinned_results=False, **kw)
    s.SetTargetState(p["x_nom"]); s.SetRunningCost(p["Q"], p["R"]); s.SetTerminalCost(p["Qf"])
    return s


def spread3(v):
    v = np.asarray(v)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def run_once(config, S, iterations):
    p, B, x0, ug, sigma, T = problem(config)
    s = solver(p, B)
    s.SetInitialState(x0); s.SetInitialGuess(ug)
    return s, s.MPPIRun(S, iterations, sigma, T, seed=1, hold=5)


def emulate(config, S, reps, warmup):
    """One iteration on the host: -> wall ms and its parts."""
    p, B, x0, ug, sigma, T = problem(config)
    N, n = p["N"], x0.shape[1]
    u = np.array(np.broadcast_to(np.asarray(ug, dtype=float).reshape(-1, N - 1), (B,) + np.asarray(ug).reshape(-1, N - 1).shape))
    m = u.shape[1]
    e = solver(p, B * S)
    e.SetInitialState(np.repeat(x0, S, axis=0))
    x0s = np.repeat(x0, S, axis=0)[:, None, :]
    parts = dict(wall=[], sample=[], rollout=[], blend=[])
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        rng = np.random.default_rng(i)
        z = np.repeat(rng.standard_normal((B, S, m, (N - 1 + 4) // 5)), 5, axis=3)[..., :N - 1]
        v = u[:, None] + sigma * z
        v[:, 0] = u
        t1 = time.perf_counter()
        e.Reset(); e.SetInitialGuess(v.reshape(B * S, m, N - 1))
        e._push_problem()
        L = e.RolloutPolicy(x0s).cost.reshape(B, S)
        t2 = time.perf_counter()
        w = np.exp(-(L - L.min(axis=1, keepdims=True)) / T)
        w /= w.sum(axis=1, keepdims=True)
        u = np.einsum("bs,bskt->bkt", w, v)
        t3 = time.perf_counter()
        if i >= warmup:
            for k, dt in (("wall", t3 - t0), ("sample", t1 - t0), ("rollout", t2 - t1), ("blend", t3 - t2)):
                parts[k].append(1e3 * dt)
    return {k + "_ms": spread3(v) for k, v in parts.items()}


def split(config, S, iterations):
    """The child under rocprofv3's kernel trace: summed kernel times by name, per iteration."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--child", config, str(S), str(iterations)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit("mppi_bench: the profiled child for %s S=%d did not end within %d s; nothing more is started" % (config, S, CHILD_TIMEOUT_S))
        if r.returncode != 0:       # an abort, a fault: the tool ends here and starts nothing more on the GPU
            raise SystemExit("mppi_bench: the profiled child for %s S=%d ended with status %d; nothing more is started\n%s"
                             % (config, S, r.returncode, r.stdout[-2000:]))
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise SystemExit("mppi_bench: the profiler left no kernel statistics for %s S=%d\n%s" % (config, S, r.stdout[-2000:]))
        out = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                for key in ("mppi_rollout_kernel", "mppi_update_kernel", "mppi_stage_kernel", "mppi_handover_kernel"):
                    if key in row["Name"]:
                        out[key + "_ms_per_iteration"] = out.get(key + "_ms_per_iteration", 0.0) + float(row["TotalDurationNs"]) * 1e-6 / iterations
                        out[key + "_calls"] = out.get(key + "_calls", 0) + int(row["Calls"])
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--configs", default="c2,c5")
    ap.add_argument("--samples", default="256,1024")
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--emulate-up-to", type=int, default=262144, help="largest B S the host emulation builds a handle for")
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--child", nargs=3, metavar=("CONFIG", "S", "I"), help="one run and nothing else (what --split profiles)")
    a = ap.parse_args()
    warnings.simplefilter("ignore", RuntimeWarning)
    if a.child:
        run_once(a.child[0], int(a.child[1]), int(a.child[2]))
        return
    out = {}
    for config in a.configs.split(","):
        for S in (int(v) for v in a.samples.split(",")):
            p, B, x0, ug, sigma, T = problem(config)
            N, m = p["N"], np.asarray(ug).reshape(-1, p["N"] - 1).shape[0]
            s = solver(p, B)
            s.SetInitialState(x0)
            ms, last = [], None
            for i in range(a.warmup + a.reps):
                s.Reset(); s.SetInitialGuess(ug)
                last = s.MPPIRun(S, a.iterations, sigma, T, seed=1, hold=5)
                if i >= a.warmup:
                    ms.append(last.kernel_ms / a.iterations)
            moved = 2.0 * B * S * (N - 1) * m * 8
            res = dict(B=B, N=N, S=S, m=m, iterations=a.iterations, kernel_ms_per_iteration=spread3(ms),
                       sample_steps_per_s=B * S * (N - 1) / (np.median(ms) * 1e-3),
                       nominal_cost_mean=[float(last.nominal_cost[0].mean()), float(last.nominal_cost[-1].mean())],
                       ess_mean=float(np.nanmean(last.ess)),
                       stored_variant=dict(bytes_per_iteration=moved, ms_at_hbm_rate=1e3 * moved / HBM_BYTES_PER_S))
            del s
            if B * S <= a.emulate_up_to:
                res["emulation"] = emulate(config, S, max(2, a.reps // 2), 1)
            if a.split:
                res["split"] = split(config, S, a.iterations)
            out["%s_S%d" % (config, S)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
