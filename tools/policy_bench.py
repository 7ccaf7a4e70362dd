"""Sample-steps per second of the policy rollout (BatchedIterativeLQR.RolloutPolicy, csrc/policy_rollout.hpp) on one GPU, beside the
only equivalent the library offered before it: a (B S)-problem handle with the policy replicated by set_state and one
stage_rollout(0.0).

    python tools/policy_bench.py [--reps R] [--warmup W] [--configs pendulum,quad3d] [--samples 64,1024] [--emulate-up-to P] [--noise]

Shapes: pendulum B = 1024, N = 200; Quad3D B = 64, N = 40; each at S = 64 and S = 1024 samples per problem.  The policy is what a
capped solve leaves on the handle; the samples are the problems' own x0 plus seeded perturbations (all rollouts run to the end).
Both paths are timed with HIP events around their ONE kernel (policy_kernel_ms / last_kernel_ms): `reps` launches after `warmup`,
median and the min .. max spread; sample-steps/s = B S (N - 1) / kernel time.  The emulation's handle holds the whole solver state
of B S problems (fx alone is B S n^2 (N-1) doubles: 27 GB for Quad3D at S = 1024, which still runs), so it runs where B S <=
--emulate-up-to (default 65536: everything but the pendulum at S = 1024, a 1 M-problem handle) - the rates are per sample-step and
compare across S.  --noise: the same rollouts again with process and actuation noise (state_noise / control_noise: the noisy
kernels of csrc/policy_rollout.hpp, a Philox block and its Box-Muller normals per four components and step) and the ratio of the
two kernel times.  --mc: the whole call instead - RolloutPolicy on host arrays plus the NumPy reduction against RolloutPolicyStats
(csrc/policy_mc.hpp), wall and kernel times (mc_bench).  --mc --envelope [--host-fold N]: RolloutPolicyStats plain, with state envelopes,
and with both envelopes and a safety box, beside RolloutPolicy(trajectories=True) plus the NumPy fold (envelope_bench).  Prints one
JSON line."""
import argparse
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problem(config):
    from drake_ddp_amd import workloads as W
    if config == "quad3d":
        p, B = W.quad3d_problem(40), 64
        return p, B, W.quad3d_batch_x0(B), W.quad3d_u_guess(40), 1e-3
    p, B = W.pendulum_problem(), 1024
    return p, B, W.pendulum_batch_x0(B), np.zeros((1, p["N"] - 1)), 0.05


def noise(config, n):
    """sigma_x (n,), sigma_u: about 1e-3 of the state scale and 1e-2 of the control scale; the quadruped's attitude quaternion gets none"""
    if config == "quad3d":
        sx = np.full(n, 1e-3)
        sx[:4] = 0.0
        return sx, 5e-2
    return np.full(n, 3e-3), 1e-2


def solver(p, B, **kw):
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    from drake_ddp_amd.models import ModelSystem
    s = BatchedIterativeLQR(ModelSystem(p["model_id"], p["dt"]), p["N"], B, delta=p["delta"], beta=p["beta"], gamma=p["gamma"],
                            hist_cap=2, pinned_results=False, **kw)
    s.SetTargetState(p["x_nom"]); s.SetRunningCost(p["Q"], p["R"]); s.SetTerminalCost(p["Qf"])
    return s


def summary(ms, work):
    ms = np.asarray(ms)
    med = float(np.median(ms))
    return dict(kernel_ms=med, kernel_ms_min=float(ms.min()), kernel_ms_max=float(ms.max()), sample_steps_per_s=work / (med * 1e-3))


def spread3(v):
    v = np.asarray(v)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def mc_bench(a):
    """--mc: the WHOLE call, old path against new, at S = 1024 samples per problem (pendulum B = 1024, N = 200: 10^6 samples; Quad3D
    B = 64, N = 40).  (a) what a caller did before: draw the starts in NumPy, RolloutPolicy on the host arrays, reduce the costs in
    NumPy (count, mean, M2, min, max, argmin, argmax) - wall time, and its three parts; the call and the reduction run on the very
    samples the device draws (seed 7, fetched once with samples=True), so both kernels roll out the same starts; (b) RolloutPolicyStats - wall time.  Beside
    them the kernel times (HIP events): policy_rollout_kernel and the Monte-Carlo kernel (its passes summed, the fold not included),
    without and with noise.  `reps` timed calls after `warmup`, the two paths alternated twice: median [min .. max] of 2 x reps."""
    import time
    out = {}
    for config in a.configs.split(","):
        p, B, x0b, ug, sigma = problem(config)
        N, n, S = p["N"], x0b.shape[1], 1024
        s = solver(p, B, max_iters=5)
        s.SetInitialState(x0b); s.SetInitialGuess(ug)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            s.Solve()
        res = dict(B=B, S=S, N=N)
        # the SAME samples for both kernels: what the device draws for seed 7, fed back to RolloutPolicy as host arrays
        x0_same = s.RolloutPolicyStats(S, x0b, sigma * np.ones(n), seed=7, samples=True).samples.x0
        for label, nz in (("no_noise", {}), ("noise", dict(zip(("state_noise", "control_noise"), noise(config, n))))):
            old, new = dict(wall=[], draw=[], call=[], reduce=[], kernel=[]), dict(wall=[], kernel=[])
            for rnd in range(2):
                for i in range(a.warmup + a.reps):
                    t0 = time.perf_counter()
                    rng = np.random.default_rng(rnd * 1000 + i)
                    x0 = x0b[:, None, :] + sigma * rng.standard_normal((B, S, n))     # (the caller's draw: timed, then set aside)
                    t1 = time.perf_counter()
                    r = s.RolloutPolicy(x0_same, seed=7, **nz)
                    t2 = time.perf_counter()
                    ok = (r.steps == N - 1) & np.isfinite(r.cost)
                    c = np.where(ok, r.cost, np.nan)
                    cnt = ok.sum(axis=1)
                    mean = np.nansum(c, axis=1) / cnt
                    red = (cnt, mean, np.nansum((c - mean[:, None]) ** 2, axis=1), np.nanmin(c, axis=1), np.nanmax(c, axis=1),
                           np.nanargmin(c, axis=1), np.nanargmax(c, axis=1), r.steps.sum(axis=1))
                    t3 = time.perf_counter()
                    if i >= a.warmup:
                        for k, v in (("wall", t3 - t0), ("draw", t1 - t0), ("call", t2 - t1), ("reduce", t3 - t2)):
                            old[k].append(1e3 * v)
                        old["kernel"].append(s.policy_kernel_ms())
                for i in range(a.warmup + a.reps):
                    t0 = time.perf_counter()
                    st = s.RolloutPolicyStats(S, x0b, sigma * np.ones(n), seed=7, **nz)
                    t1 = time.perf_counter()
                    if i >= a.warmup:
                        new["wall"].append(1e3 * (t1 - t0))
                        new["kernel"].append(s.policy_kernel_ms())
            res[label] = dict(host_arrays={k + "_ms": spread3(v) for k, v in old.items()}, on_device={k + "_ms": spread3(v) for k, v in new.items()},
                              wall_speedup=float(np.median(old["wall"]) / np.median(new["wall"])),
                              kernel_ratio=float(np.median(new["kernel"]) / np.median(old["kernel"])),
                              counted_host=int(red[0].sum()), counted_device=int(st.counted.sum()))
        out["%s_S%d" % (config, S)] = res
    print(json.dumps(out))


def host_fold(r, lo, hi):
    """What a caller did before the device reduced them: RolloutPolicy's trajectories X (B, S, n, N) / U to per-step count, mean, M2,
    min, max, argmin, argmax over the samples, and the box counts, in vectorised NumPy."""
    out = []
    for V in (r.X, r.U):
        ok = np.isfinite(V)
        cnt = ok.sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.nansum(np.where(ok, V, np.nan), axis=1) / cnt
            m2 = np.nansum(np.where(ok, V - mean[:, None], np.nan) ** 2, axis=1)
        out.append((cnt, mean, m2, np.min(np.where(ok, V, np.inf), axis=1), np.max(np.where(ok, V, -np.inf), axis=1),
                    np.argmin(np.where(ok, V, np.inf), axis=1), np.argmax(np.where(ok, V, -np.inf), axis=1)))
    with np.errstate(invalid="ignore"):
        outside = ((r.X < lo[:, None, :, None]) | (r.X > hi[:, None, :, None])).any(axis=2)      # (B, S, N)
    ran = np.isfinite(r.X).all(axis=(2, 3))
    ever = outside.any(axis=2)
    first = np.where(ever, np.argmax(outside, axis=2), -1)
    exits = np.stack([np.bincount(f[f >= 0], minlength=r.X.shape[3]) for f in first])
    out.append((ran.sum(axis=1), (ran & ~ever).sum(axis=1), exits))
    return out


def envelope_bench(a):
    """--mc --envelope: the WHOLE call with what a run observes beside the cost (csrc/policy_env.hpp), S = 1024 samples per problem:
    (a) plain RolloutPolicyStats, (b) with state envelopes, (c) with state and control envelopes and a box - alternated, `reps` timed
    calls after `warmup` in each of two rounds: median [min .. max] of the wall times, and the rollout kernels' own milliseconds.
    --host-fold N: also (d), N times: RolloutPolicy(trajectories=True) on starts drawn in NumPy plus the NumPy reduction (host_fold) -
    the only equivalent there was; it uses nothing this feature added, so with --reps 0 it runs on an older checkout as well."""
    import time
    out = {}
    for config in a.configs.split(","):
        p, B, x0b, ug, sigma = problem(config)
        N, n, S = p["N"], x0b.shape[1], 1024
        s = solver(p, B, max_iters=5)
        s.SetInitialState(x0b); s.SetInitialGuess(ug)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            s.Solve()
        spread = sigma * np.ones(n)
        lo, hi = np.full((B, n), -np.inf), x0b + 3.0 * sigma               # a box most samples stay in for a while
        res = dict(B=B, S=S, N=N, state_window_bytes=8 * B * N * n * S)
        if a.reps > 0:
            forms = (("plain", {}), ("states", dict(envelope=True)), ("all", dict(envelope=True, controls=True, safe_box=(lo, hi))))
            wall, kern = {k: [] for k, _ in forms}, {k: [] for k, _ in forms}
            for rnd in range(2):
                for i in range(a.warmup + a.reps):
                    for k, more in forms:                                  # alternated: a, b, c, a, b, c, ...
                        t0 = time.perf_counter()
                        st = s.RolloutPolicyStats(S, x0b, spread, seed=7, **more)
                        t1 = time.perf_counter()
                        if i >= a.warmup:
                            wall[k].append(1e3 * (t1 - t0)); kern[k].append(s.policy_kernel_ms())
                        res["passes_" + k] = s.policy_mc_passes()
                        if st.safety is not None:
                            res["safe_share"] = float(st.safety.safe.sum() / (B * S))
                        del st                                             # (an observing result is tens of MB: freed outside the next call's clock)
            res["on_device"] = {k: dict(wall_ms=spread3(wall[k]), rollout_kernel_ms=spread3(kern[k])) for k, _ in forms}
            res["states_over_plain"] = float(np.median(wall["states"]) / np.median(wall["plain"]))
            res["all_over_plain"] = float(np.median(wall["all"]) / np.median(wall["plain"]))
        if a.host_fold > 0:
            x0_same = x0b[:, None, :] + sigma * np.random.default_rng(7).standard_normal((B, S, n))     # (drawn here: any build runs this part)
            parts = dict(wall=[], call=[], reduce=[])
            for i in range(a.host_fold):
                t0 = time.perf_counter()
                r = s.RolloutPolicy(x0_same, trajectories=True, seed=7)
                t1 = time.perf_counter()
                red = host_fold(r, lo, hi)
                t2 = time.perf_counter()
                for k, v in (("wall", t2 - t0), ("call", t1 - t0), ("reduce", t2 - t1)):
                    parts[k].append(1e3 * v)
                del r
            res["host_fold"] = {k + "_ms": spread3(v) for k, v in parts.items()}
            res["host_fold_safe_share"] = float(red[2][1].sum() / (B * S))
            if "on_device" in res:
                res["host_fold_over_states"] = float(np.median(parts["wall"]) / np.median(wall["states"]))
        out["%s_S%d" % (config, S)] = res
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--configs", default="pendulum,quad3d")
    ap.add_argument("--samples", default="64,1024")
    ap.add_argument("--emulate-up-to", type=int, default=65536)
    ap.add_argument("--noise", action="store_true")
    ap.add_argument("--mc", action="store_true")
    ap.add_argument("--envelope", action="store_true")
    ap.add_argument("--host-fold", type=int, default=0)
    a = ap.parse_args()
    if a.mc and a.envelope:
        return envelope_bench(a)
    if a.mc:
        return mc_bench(a)
    out = {}
    for config in a.configs.split(","):
        p, B, x0b, ug, sigma = problem(config)
        N, n = p["N"], x0b.shape[1]
        s = solver(p, B, max_iters=5)
        s.SetInitialState(x0b); s.SetInitialGuess(ug)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            s.Solve()
        pol = dict(x_bar=np.array(s.x_bar), u_bar=np.array(s.u_bar), K=np.array(s.K))
        for S in (int(v) for v in a.samples.split(",")):
            rng = np.random.default_rng(S)
            x0 = x0b[:, None, :] + sigma * rng.standard_normal((B, S, n))
            work = float(B) * S * (N - 1)
            ms = []
            for i in range(a.warmup + a.reps):
                r = s.RolloutPolicy(x0)
                if i >= a.warmup:
                    ms.append(s.policy_kernel_ms())
            res = dict(B=B, S=S, N=N, full_rollouts=int((r.steps == N - 1).sum()), policy_rollout=summary(ms, work))
            if a.noise:
                sx, su = noise(config, n)
                ms_n = []
                for i in range(a.warmup + a.reps):
                    rn = s.RolloutPolicy(x0, state_noise=sx, control_noise=su, seed=S)
                    if i >= a.warmup:
                        ms_n.append(s.policy_kernel_ms())
                res["policy_rollout_noise"] = dict(summary(ms_n, work), full_rollouts=int((rn.steps == N - 1).sum()))
                res["noise_slowdown"] = res["policy_rollout_noise"]["kernel_ms"] / res["policy_rollout"]["kernel_ms"]
            if B * S <= a.emulate_up_to:
                e = solver(p, B * S)
                e.set_state(**{k: np.repeat(v, S, axis=0) for k, v in pol.items()})
                e.SetInitialState(x0.reshape(B * S, n))
                ms = []
                for i in range(a.warmup + a.reps):
                    _, _, L, _ = e.stage_rollout(0.0)
                    if i >= a.warmup:
                        ms.append(e.last_kernel_ms())
                res["emulation"] = summary(ms, work)
                res["speedup"] = res["emulation"]["kernel_ms"] / res["policy_rollout"]["kernel_ms"]
                fin = np.isfinite(r.cost.ravel())
                res["max_rel_cost_difference"] = float(np.max(np.abs(L[fin] - r.cost.ravel()[fin]) / np.abs(L[fin])))
                del e
            out["%s_S%d" % (config, S)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
