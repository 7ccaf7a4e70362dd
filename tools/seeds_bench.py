"""What joining the seeds of a multi-start costs on the device and on the host, on C2's shape (pendulum swing-up, N = 200, groups of
K = 8 seeds, B = 1024 and B = 65 536 problems).

    python tools/seeds_bench.py [--reps R] [--host-reps H] [--batches 1024,65536]

Per batch size, on ONE solved handle:
  (a) ReseedFromBest by its own kernel events (seeds_kernel_ms): select + rebuild B guesses in one launch.  Every repetition
      follows a fresh solve, so the kernel reads the winners from u_bar, the case of a multi-start loop.
  (b) the host round trip it replaces, wall clock: mi_ilqr_get of cost, status and u_bar, the NumPy statement of the reseed
      (tests/seeds_np.py) and mi_ilqr_set_initial of the new guesses.
  (c) the kernel's HBM floor: the bytes it must move - B m (N-1) 8 written, the winners' rows G m (N-1) 8 and the cost, status and
      sigma rows read - over the bandwidth of a hipMemcpyAsync device-to-device copy of B m (N-1) 8 bytes measured in the same
      process (2 x bytes / time: a copy reads and writes).
Warm-up first, medians over the repetitions, the spread (min .. max) beside them.  One JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, SIGMA, SEED, HOLD = 8, 0.5, 2025, 10


def copy_bandwidth(nbytes, reps):
    """GB/s of a device-to-device hipMemcpyAsync of `nbytes` on the null stream: 2 x nbytes over the median event time."""
    hip = C.CDLL("libamdhip64.so")
    chk = lambda rc: None if rc == 0 else (_ for _ in ()).throw(RuntimeError(f"HIP error {rc}"))   # noqa: E731
    src, dst, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    chk(hip.hipMalloc(C.byref(src), C.c_size_t(nbytes))); chk(hip.hipMalloc(C.byref(dst), C.c_size_t(nbytes)))
    chk(hip.hipMemset(src, 1, C.c_size_t(nbytes)))
    chk(hip.hipEventCreate(C.byref(e0))); chk(hip.hipEventCreate(C.byref(e1)))
    ms = []
    for r in range(reps + 2):
        chk(hip.hipEventRecord(e0, None))
        chk(hip.hipMemcpyAsync(dst, src, C.c_size_t(nbytes), 3, None))          # hipMemcpyDeviceToDevice
        chk(hip.hipEventRecord(e1, None))
        chk(hip.hipEventSynchronize(e1))
        t = C.c_float()
        chk(hip.hipEventElapsedTime(C.byref(t), e0, e1))
        if r >= 2:
            ms.append(float(t.value))
    for p in (src, dst):
        chk(hip.hipFree(p))
    chk(hip.hipEventDestroy(e0)); chk(hip.hipEventDestroy(e1))
    return 2.0 * nbytes / (np.median(ms) * 1e-3) / 1e9, ms


def run(B, reps, host_reps):
    import seeds_np as SN
    from drake_ddp_amd import _capi, workloads as W
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    from drake_ddp_amd.models import ModelSystem
    p = W.pendulum_problem()
    N, m, G = p["N"], 1, B // K
    s = BatchedIterativeLQR(ModelSystem(p["model_id"], p["dt"]), N, B, delta=p["delta"], beta=p["beta"], gamma=p["gamma"], hist_cap=2,
                            pinned_results=False)
    s.SetTargetState(p["x_nom"]); s.SetRunningCost(p["Q"], p["R"]); s.SetTerminalCost(p["Qf"])
    s.SetInitialState(np.repeat(W.pendulum_batch_x0(G), K, axis=0)); s.SetInitialGuess(np.zeros((1, N - 1)))
    s.PerturbInitialGuess(K, SIGMA, seed=SEED, hold=HOLD)
    perturb_ms = s.seeds_kernel_ms()
    s.solve_resident()
    dev, select_ms = [], []
    for r in range(reps + 2):                                  # (a)
        s.ReseedFromBest(K, SIGMA, seed=SEED, round=r + 1, hold=HOLD)
        if r >= 2:
            dev.append(s.seeds_kernel_ms())
        s.solve_resident()
        s.SelectBest(K)
        if r >= 2:
            select_ms.append(s.seeds_kernel_ms())
    sigma = np.full((B, m), SIGMA)
    host, parts = [], []
    for r in range(host_reps + 1):                             # (b)
        t0 = time.perf_counter()
        cost, status, u = np.array(s.cost), np.array(s.status), np.array(s.u_bar)
        t1 = time.perf_counter()
        guess, _ = SN.reseed(u, cost, status, K, sigma, SEED, r + 1, HOLD)
        t2 = time.perf_counter()
        guess = np.ascontiguousarray(guess)
        _capi.check(s._lib.mi_ilqr_reset(s._h), "mi_ilqr_reset")
        _capi.check(s._lib.mi_ilqr_set_initial(s._h, None, _capi.ptr(guess)), "mi_ilqr_set_initial")
        _capi.check(s._lib.mi_ilqr_synchronize(s._h), "mi_ilqr_synchronize")
        t3 = time.perf_counter()
        if r >= 1:
            host.append((t3 - t0) * 1e3)
            parts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
        s.solve_resident()
    nbytes = B * m * (N - 1) * 8
    bw, copy_ms = copy_bandwidth(nbytes, reps)                  # (c)
    moved = nbytes + G * m * (N - 1) * 8 + B * (8 + 4 + 8 * m)
    floor_ms = moved / (bw * 1e9) * 1e3
    a, b = float(np.median(dev)), float(np.median(host))
    get_ms, spec_ms, set_ms = (float(np.median([q[i] for q in parts])) for i in range(3))
    return dict(B=B, K=K, N=N, reseed_kernel_ms=a, reseed_kernel_ms_range=[min(dev), max(dev)], select_kernel_ms=float(np.median(select_ms)),
                perturb_kernel_ms=perturb_ms, host_round_trip_ms=b, host_round_trip_ms_range=[min(host), max(host)],
                host_get_ms=get_ms, host_numpy_ms=spec_ms, host_set_ms=set_ms, host_transfers_only_ms=get_ms + set_ms,
                copy_GBps=bw, copy_ms=float(np.median(copy_ms)), bytes_moved=moved, floor_ms=floor_ms,
                host_over_device=b / a, transfers_over_device=(get_ms + set_ms) / a, device_over_floor=a / floor_ms)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--batches", default="1024,65536")
    args = ap.parse_args()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        print(json.dumps([run(int(b), args.reps, args.host_reps) for b in args.batches.split(",")]))
