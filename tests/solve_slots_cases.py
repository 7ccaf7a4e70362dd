"""The sequences of tests/test_gpu_solve_slots.py, written once and run two ways: `pipelined` - cold solves enqueued back to back
with mi_ilqr_solve_async on one handle, which puts them on its two solve slots - and blocking, every solve waited
for before the next call.  The blocking run is the reference: the test starts it in a child process under MI_ILQR_SOLVE_SLOTS=1
(tests/_solve_slots_child.py; the switch is read once per process) and compares everything bitwise.

Every case returns a dict of arrays.  Per-solve results are read from the handle's ring after the last solve (the ring scalars of
solve k live in ring slot k % 32 whatever the solve slot); the per-iteration log is compared over the rows the LAST solve wrote
(row < iterations; rows behind them are leftovers of earlier solves on the same arrays, which the two runs do not share)."""
import ctypes as C
import warnings

import numpy as np

from drake_ddp_amd import _capi
from drake_ddp_amd import workloads as W
from drake_ddp_amd.ilqr import BatchedIterativeLQR
from drake_ddp_amd.models import ModelSystem

STATE_FIELDS = ("x_bar", "u_bar", "K", "kappa", "dV_coeff", "fx", "fu")
STAT_FIELDS = ("total_iters", "total_ls_trials", "n_converged", "n_max_iters", "n_ls_failed", "max_iters_seen", "best_cost",
               "best_index", "n_internal", "n_not_pd")
RING = 32


_hip = None


def hip():
    """The HIP runtime libmi_ilqr.so itself runs on, for the few raw calls the cases make on the library's pointers and stream: the
    copy this process has loaded (after `import torch` that is torch's own, which the library then shares; else the system's)."""
    global _hip
    if _hip is None:
        _capi.load()
        with open("/proc/self/maps") as f:
            paths = {ln.split()[-1] for ln in f if "libamdhip64" in ln}
        assert len(paths) == 1, f"one HIP runtime per process, found {sorted(paths)}"
        _hip = C.CDLL(paths.pop())
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        _hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _hip.hipFree.argtypes = [C.c_void_p]
        _hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        _hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    return _hip


D2H, D2D = 2, 3


def dev_read(ptr, shape, dtype):
    out = np.empty(shape, dtype=dtype)
    assert hip().hipMemcpy(_capi.ptr(out), ptr, out.nbytes, D2H) == 0
    return out


def make(N, B, **kw):
    p = W.pendulum_problem()
    s = BatchedIterativeLQR(ModelSystem(p["model_id"], p["dt"]), N, B, delta=p["delta"], beta=p["beta"], gamma=p["gamma"], device=0,
                            pinned_results=False, **kw)
    s.SetTargetState(p["x_nom"]); s.SetRunningCost(p["Q"], p["R"]); s.SetTerminalCost(p["Qf"])
    s.solves = 0
    return s


def input_sets(N, B):
    """Two sets of (x0, u_guess), per problem, far enough apart that their solves differ in cost and iteration counts."""
    rng = np.random.default_rng(20 * N + B)
    xa = np.ascontiguousarray(W.pendulum_batch_x0(max(B, 8))[:B])
    xb = np.ascontiguousarray(xa[::-1] * 0.7 + 0.1)
    ua = 0.05 * rng.standard_normal((B, 1, N - 1))
    ub = -0.3 + 0.1 * rng.standard_normal((B, 1, N - 1))
    return (xa, ua), (xb, ub)


def set_inputs(s, x0, ug):
    """mi_ilqr_set_initial alone (Solve()'s _push_problem would send the costs as well)."""
    _capi.check(s._lib.mi_ilqr_set_initial(s._h, _capi.ptr(x0), _capi.ptr(ug)), "mi_ilqr_set_initial")


def start(s, x0, ug):
    s.SetInitialState(x0); s.SetInitialGuess(ug)
    s._push_problem()


def cold(s, pipelined):
    s.rearm(cold=True)
    if pipelined:
        s.solve_resident_async()
    else:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            s.solve_resident()
    s.solves += 1


def ring_results(s, count):
    """cost, iterations, status, trials of the last `count` solves, (count, B) each, and their statistics records - collected here."""
    stats = s.collect(count)
    out = {}
    cur = (s.solves - 1) % RING
    for name, which, typestr, size in (("ring_cost", _capi.F_COST, "<f8", 8), ("ring_iters", _capi.I_ITERS, "<i4", 4),
                                       ("ring_status", _capi.I_STATUS, "<i4", 4), ("ring_trials", _capi.I_LS_TRIALS, "<i4", 4)):
        p, nb = C.c_void_p(), C.c_size_t()
        _capi.check(s._lib.mi_ilqr_device_ptr(s._h, which, C.byref(p), C.byref(nb)), "mi_ilqr_device_ptr")
        base = p.value - cur * s.B * size
        ring = dev_read(base, (RING, s.B), np.dtype(typestr))
        out[name] = np.stack([ring[(s.solves - count + i) % RING] for i in range(count)])
    out["stats"] = np.array([[float(getattr(st, f)) for f in STAT_FIELDS] for st in stats])
    return out


def state(s):
    out = {f: getattr(s, f) for f in STATE_FIELDS}
    it = s.iterations
    hist = s.history
    rows = np.arange(hist.shape[1])[None, :, None] < np.minimum(it, hist.shape[1])[:, None, None]
    out["hist"] = np.where(rows, hist, 0.0)
    out.update(cost=s.cost, iterations=it, status=s.status, ls_trials=s.ls_trials, kp_count=s.keypoint_count,
               kp_list=s.keypoint_list, x0=s._get(_capi.F_X0, (s.B, s.n)))
    return out


def sequence(N, B, pipelined, alternate, count=6, **kw):
    s = make(N, B, **kw)
    sets = input_sets(N, B)
    start(s, *sets[0])
    for k in range(count):
        if alternate:
            set_inputs(s, *sets[k % 2])
        cold(s, pipelined)
    out = ring_results(s, count)
    out.update(state(s))
    return s, out


def case_alternating(pipelined):
    return sequence(20, 64, pipelined, True)[1]


def case_alternating_long(pipelined):
    return sequence(200, 8, pipelined, True)[1]


def case_repeated(pipelined):
    return sequence(20, 64, pipelined, False)[1]


def case_partial_inputs(pipelined):
    """x0 alone and u_guess alone between the solves: each input has copies of its own."""
    s = make(20, 64)
    (xa, ua), (xb, ub) = input_sets(20, 64)
    start(s, xa, ua)
    for k, (x0, ug) in enumerate(((None, None), (xb, None), (None, ub), (xa, None), (None, None))):
        if x0 is not None or ug is not None:
            set_inputs(s, x0, ug)
        cold(s, pipelined)
    out = ring_results(s, 5)
    out.update(state(s))
    return out


def case_warm(pipelined):
    N, B = 20, 64
    s = make(N, B)
    sets = input_sets(N, B)
    start(s, *sets[0])
    for k in range(4):
        set_inputs(s, *sets[k % 2])
        cold(s, pipelined)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        st = s.solve_resident()                      # warm, straight behind them: continues from the last enqueued solve's state
    s.solves += 1
    out = ring_results(s, 5)
    out["warm_stats"] = np.array([float(getattr(st, f)) for f in STAT_FIELDS])
    out.update(state(s))
    return out


def case_consumers(pipelined):
    N, B = 20, 64
    s = make(N, B)
    sets = input_sets(N, B)
    start(s, *sets[0])
    for k in range(4):
        set_inputs(s, *sets[k % 2])
        cold(s, pipelined)
    out = state(s)                                   # mi_ilqr_get of every field, no collect in between
    rng = np.random.default_rng(5)
    r = s.RolloutPolicy(sets[1][0][:, None, :] + 0.01 * rng.standard_normal((B, 3, 2)), trajectories=True)
    out.update(policy_cost=r.cost, policy_x_final=r.x_final, policy_steps=r.steps, policy_X=r.X, policy_U=r.U)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        st = s.MPCRun(3, 2)
    out["mpc_stats"] = np.array([float(getattr(st, f)) for f in STAT_FIELDS])
    out["mpc_log"] = s.mpc_log
    out.update({"mpc_" + f: getattr(s, f) for f in STATE_FIELDS})
    return out


def case_stream_order(pipelined):
    """The cost and x_bar of the last solve, read by copies enqueued on the stream mi_ilqr_get_stream returns - nothing waits on the
    host between the last solve and those copies."""
    N, B = 20, 64
    s = make(N, B)
    sets = input_sets(N, B)
    start(s, *sets[0])
    for k in range(4):
        set_inputs(s, *sets[k % 2])
        cold(s, pipelined)
    stream, p, q, nb = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t()
    _capi.check(s._lib.mi_ilqr_get_stream(s._h, C.byref(stream)), "mi_ilqr_get_stream")
    _capi.check(s._lib.mi_ilqr_device_ptr(s._h, _capi.F_COST, C.byref(p), C.byref(nb)), "mi_ilqr_device_ptr")
    _capi.check(s._lib.mi_ilqr_device_ptr(s._h, _capi.F_X_BAR, C.byref(q), C.byref(nb)), "mi_ilqr_device_ptr")
    h_, nx = hip(), B * 2 * N * 8
    dst = C.c_void_p()
    assert h_.hipMalloc(C.byref(dst), B * 8 + nx) == 0
    try:
        assert h_.hipMemcpyAsync(dst.value, p.value, B * 8, D2D, stream.value) == 0
        assert h_.hipMemcpyAsync(dst.value + B * 8, q.value, nx, D2D, stream.value) == 0
        assert h_.hipStreamSynchronize(stream.value) == 0
        out = {"stream_cost": dev_read(dst.value, (B,), np.float64), "stream_x_bar": dev_read(dst.value + B * 8, (B, 2, N), np.float64)}
    finally:
        h_.hipFree(dst)
    s.collect(1)
    return out


def case_sink(pipelined):
    """A handle with a result sink set: its solves write the caller's page-locked arrays."""
    N, B = 20, 64
    s = make(N, B)
    sets = input_sets(N, B)
    start(s, *sets[0])
    sizes = (B * 2 * N, B * (N - 1), B)
    mem = [C.c_void_p() for _ in sizes]
    for m_, k in zip(mem, sizes):
        _capi.check(s._lib.mi_ilqr_host_alloc(k * 8, C.byref(m_)), "mi_ilqr_host_alloc")
    try:
        _capi.check(s._lib.mi_ilqr_set_result_sink(s._h, *mem), "mi_ilqr_set_result_sink")
        for k in range(3):
            set_inputs(s, *sets[k % 2])
            cold(s, pipelined)
        out = ring_results(s, 3)
        for name, m_, k in zip(("sink_x", "sink_u", "sink_cost"), mem, sizes):
            out[name] = np.ctypeslib.as_array(C.cast(m_, C.POINTER(C.c_double)), (k,)).copy()
        out.update(state(s))
        _capi.check(s._lib.mi_ilqr_set_result_sink(s._h, None, None, None), "mi_ilqr_set_result_sink")
    finally:
        for m_ in mem:
            s._lib.mi_ilqr_host_free(m_)
    return out


def case_tiny(pipelined):
    return sequence(20, 2, pipelined, True, count=4)[1]


def case_limited(pipelined):
    N, B = 20, 64
    s = make(N, B, control_limits="enforce")
    s.SetControlLimits(-0.4, 0.6)
    sets = input_sets(N, B)
    start(s, *sets[0])
    for k in range(4):
        set_inputs(s, *sets[k % 2])
        cold(s, pipelined)
    out = ring_results(s, 4)
    out.update(state(s))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        st = s.solve_resident()                      # warm: S2 of the last solve's slot comes along
    out["warm_stats"] = np.array([float(getattr(st, f)) for f in STAT_FIELDS])
    out.update({"warm_" + f: getattr(s, f) for f in STATE_FIELDS})
    return out


def _used_bytes():
    free, total = C.c_size_t(), C.c_size_t()
    assert hip().hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return total.value - free.value


def case_lazy(pipelined):
    """Device memory a handle takes: create plus blocking solves (`pipelined` adds three pipelined ones on top)."""
    N, B = 200, 1024
    w = make(N, B); start(w, *input_sets(N, B)[0]); cold(w, False); del w        # (the runtime's own first allocations)
    before = _used_bytes()
    s = make(N, B)
    start(s, *input_sets(N, B)[0])
    cold(s, False); cold(s, False)
    out = {"blocking_bytes": np.array([_used_bytes() - before])}
    if pipelined:
        for _ in range(3):
            cold(s, True)
        s.collect(3)
        out["pipelined_bytes"] = np.array([_used_bytes() - before])
    return out


CASES = {f[5:]: g for f, g in list(globals().items()) if f.startswith("case_")}


def run_all(pipelined, names=None):
    out = {}
    for name in names or CASES:
        for k, v in CASES[name](pipelined).items():
            out[name + "/" + k] = np.asarray(v)
    return out
