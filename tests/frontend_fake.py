"""A recording stand-in for libmi_ilqr.so, and the script of front-end calls traced through it (tests/test_frontend_call_trace.py).

`FakeLibrary` answers every `mi_ilqr_*` name: it records (name, selector or None, byte count or None, data) - data: the scalar
arguments as ints, then the doubles of every input buffer as float.hex strings -, zero-fills the output buffers and returns OK or the
code scripted for (name, selector).  Installed as `_capi._lib`, `_capi.load()` returns it: the classes of drake_ddp_amd/ilqr.py run
on it without a built library and without a GPU.  mi_ilqr_destroy / mi_ilqr_host_free run when objects are collected and are left
out of the record.

`SCENARIOS` is the script; `run(install)` plays it and returns {label: {"calls": [...], "returns": ...}} plus the table of distinct
buffers the calls point into.  The committed record, tests/frontend_trace.json, is what the commit BEFORE the front end was split
into argcheck.py / results.py / ilqr.py answered; it was written with this file run against a checkout of that commit:

    git worktree add /tmp/parent <that commit>
    PYTHONPATH=/tmp/parent python tests/frontend_fake.py --record tests/frontend_trace.json
"""
import ctypes as C
import json
import os
import sys

import numpy as np

UNTRACED = ("mi_ilqr_destroy", "mi_ilqr_host_free")
HANDLE = 0x1000


def _doubles(addr, count):
    return [] if not addr else [float(v).hex() for v in (C.c_double * count).from_address(addr)]


def _addr(p):
    return p.value if isinstance(p, C.c_void_p) else p


class FakeLibrary:
    def __init__(self, m, codes=None):
        self.m, self.codes, self.calls, self._blocks = m, dict(codes or {}), [], []

    def __getattr__(self, name):
        if not name.startswith("mi_ilqr_"):
            raise AttributeError(name)

        def call(*args):
            return self._call(name, args)
        return call

    def _zero(self, p, nbytes):
        if _addr(p):
            C.memset(_addr(p), 0, nbytes)

    def _call(self, name, a):
        if name in UNTRACED:
            return None
        if name == "mi_ilqr_strerror":
            return b"error of the stand-in"
        which = nbytes = None
        data = []
        if name == "mi_ilqr_create":
            d = a[0]._obj
            self.n, self.md, self.N, self.B, self.n_params = d.n, d.m, d.N, d.B, d.n_params
            data = [getattr(d, f) if "double" not in str(t) else float(getattr(d, f)).hex()
                    for f, t in d._fields_ if f != "model_params"] + [float(v).hex() for v in d.model_params[:d.n_params]]
            a[1]._obj.value = HANDLE
        elif name == "mi_ilqr_host_alloc":
            nbytes = a[0]
            self._blocks.append(bytearray(nbytes))
            a[1]._obj.value = C.addressof((C.c_char * nbytes).from_buffer(self._blocks[-1]))
        elif name == "mi_ilqr_set":
            which, nbytes = a[1], a[3]
            data = _doubles(a[2], nbytes // 8)
        elif name in ("mi_ilqr_get", "mi_ilqr_get_int"):
            which, nbytes = a[1], a[3]
            self._zero(a[2], nbytes)
        elif name in ("mi_ilqr_get_mpc_log", "mi_ilqr_get_cycles"):
            nbytes = a[2]
            self._zero(a[1], nbytes)
        elif name == "mi_ilqr_set_cost":
            for p, k in zip(a[1:], (self.n * self.n, self.md * self.md, self.n * self.n, self.n)):
                data += ["-"] if p is None else _doubles(p, k)
        elif name in ("mi_ilqr_set_initial", "mi_ilqr_set_initial_shared"):
            k = self.md * (self.N - 1) * (1 if name.endswith("shared") else self.B)
            data = _doubles(a[1], self.B * self.n) + (["-"] if a[2] is None else _doubles(a[2], k))
        elif name == "mi_ilqr_set_control_limits":
            k = self.m * (self.B if a[3] else 1)
            data = [a[3]] + _doubles(a[1], k) + _doubles(a[2], k)
        elif name in ("mi_ilqr_rollout", "mi_ilqr_forward"):
            data = _doubles(a[1], self.B)
        elif name in ("mi_ilqr_solve", "mi_ilqr_collect_stats"):
            C.memset(C.addressof(a[1]._obj), 0, C.sizeof(a[1]._obj))
        elif name == "mi_ilqr_collect_stats_n":
            data = [a[1]]
            C.memset(C.addressof(a[2]), 0, C.sizeof(a[2]))
        elif name == "mi_ilqr_solve_into":
            B, n, md, N = self.B, self.n, self.md, self.N
            for p, k in zip(a[1:4], (B * n * N, B * md * (N - 1), B)):
                self._zero(p, 8 * k)
            k = a[5]
            data = [a[4], k] + [int(a[6][i]) for i in range(k)] + [int(a[8][i]) for i in range(k)]
            for i in range(k):
                self._zero(a[7][i], int(a[8][i]))
            C.memset(C.addressof(a[9]._obj), 0, C.sizeof(a[9]._obj))
            a[10]._obj.value = 0
        elif name == "mi_ilqr_mpc_run":
            data = [a[1], a[2]] + (["-"] if a[3] is None else _doubles(a[3], self.n))
            C.memset(C.addressof(a[4]._obj), 0, C.sizeof(a[4]._obj))
        elif name == "mi_ilqr_policy_rollout":
            B, n, md, N, S = self.B, self.n, self.md, self.N, a[1]
            data = [S] + _doubles(a[2], B * S * n) + (["-"] if a[3] is None else _doubles(a[3], B * S * self.n_params))
            for p, k in zip(a[4:], (8 * B * S, 8 * B * S * n, 4 * B * S, 8 * B * S * n * N, 8 * B * S * md * (N - 1))):
                data.append(0 if p is None else 1)
                self._zero(p, k)
        elif name == "mi_ilqr_last_kernel_ms":
            a[1]._obj.value = 0.0
        elif name in ("mi_ilqr_mpc_shift", "mi_ilqr_set_timing"):
            data = [a[1]]
        elif name not in ("mi_ilqr_reset", "mi_ilqr_rearm_initial_guess", "mi_ilqr_solve_async", "mi_ilqr_linearize", "mi_ilqr_backward"):
            raise AssertionError(f"the stand-in does not know {name}")
        self.calls.append([name, which, nbytes, data])
        return self.codes.get((name, which), 0)


# ---------------------------------------------------------------- what a call returned, as JSON
def encode(v):
    if isinstance(v, np.ndarray):
        flat = v.ravel()
        return {"dtype": str(v.dtype), "shape": list(v.shape), "contiguous": bool(v.flags["C_CONTIGUOUS"]),
                "data": [float(x).hex() for x in flat] if v.dtype.kind == "f" else [int(x) for x in flat]}
    if isinstance(v, (tuple, list)):
        return [encode(x) for x in v]
    if isinstance(v, C.Structure):
        return {"struct": type(v).__name__, **{f: getattr(v, f) for f, _ in v._fields_}}
    if isinstance(v, (bool, np.bool_)) or v is None or isinstance(v, str):
        return v if v is None or isinstance(v, str) else bool(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return float(v).hex()
    if hasattr(type(v), "__slots__"):
        return {"class": type(v).__name__, **{k: encode(getattr(v, k)) for k in type(v).__slots__ if not k.startswith("__")}}
    raise TypeError(f"cannot record a {type(v).__name__}")


# ---------------------------------------------------------------- the solvers
B, N = 3, 5
NO_REF = "no_ref"        # scripted: a get of MI_F_X_REF answers E_BAD_ARG - the handle holds no reference trajectory


def make(kind, lib_codes, install, **options):
    """-> (solver, fake): `plain` Pendulum B = 3, N = 5; `padded` the same system with m_dev = 4; `single` the drop-in class."""
    from drake_ddp_amd import _capi, ilqr
    from drake_ddp_amd.models import Pendulum
    codes = {}
    for c in lib_codes:
        codes.update({NO_REF: {("mi_ilqr_get", _capi.F_X_REF): _capi.E_BAD_ARG}}[c] if isinstance(c, str) else c)
    system = Pendulum(1e-2)
    if kind == "padded":
        system.m_dev = 4
    fake = FakeLibrary(system.m, codes)
    install(fake)
    if kind == "single":
        s = ilqr.IterativeLinearQuadraticRegulator(system, N, verbose=False, **options)
        s.SetInitialState(np.array([0.1, -0.2]))
    else:
        s = ilqr.BatchedIterativeLQR(system, N, B, **options)
        s.SetInitialState(np.arange(B * s.n, dtype=np.float64).reshape(B, s.n) / 8)
    s.SetTargetState(np.array([np.pi, 0.0]))
    s.SetRunningCost(np.diag([1.0, 0.5]), np.array([[0.25]]))
    s.SetTerminalCost(np.diag([10.0, 2.0]))
    return s, fake


def _grid(*shape):
    return (np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape) + 1) / 16


def _each(*steps):
    """A scenario of several steps on one solver: every step's return (or refusal) is recorded."""
    def play(s):
        out = []
        for step in steps:
            try:
                out.append(encode(step(s)))
            except (ValueError, RuntimeError) as e:
                out.append({"raises": type(e).__name__, "message": str(e)})
        return out
    return play


def _solve(s):
    r = s.Solve()
    return r[0], r[1], r[3]         # (the wall time is not the front end's to repeat)


def _per_problem(s):
    s.SetRunningCost(_grid(B, 2, 2) + np.eye(2), _grid(B, 1, 1))
    s.SetTerminalCost(_grid(B, 2, 2) + 2 * np.eye(2))
    s.SetTargetState(_grid(B, 2))
    s.SetInitialGuess(_grid(B, 1, N - 1))
    return _solve(s)


def _codes():
    from drake_ddp_amd import _capi
    return _capi


BATCHED = {
    "solve_shared": _each(lambda s: s.SetInitialGuess(_grid(1, N - 1)), _solve, _solve),
    "solve_per_problem": _each(_per_problem, lambda s: s.cost_matrices),
    "target_trajectory_cleared": _each(lambda s: s.SetTargetTrajectory(None), lambda s: s.target_trajectory, lambda s: s.target_clock),
    "model_parameters": _each(lambda s: s.SetModelParameters(_grid(B, s.system.params.size)), lambda s: s.SetModelParameters(_grid(s.system.params.size)),
                              lambda s: s.SetModelParameters(None), lambda s: s.model_params),
    "mpc_run": _each(lambda s: s.MPCRun(2, 1), lambda s: s.MPCRun(2, 1, np.array([0.5, 0.25])), lambda s: s.x_nom,
                     lambda s: s.MPCRun(1, 2, _grid(B, 2)), lambda s: s.x_nom, lambda s: s.mpc_log),
    "stages": _each(lambda s: s.stage_rollout(0.5), lambda s: s.stage_forward(np.array([1.0, 2.0, 3.0])), lambda s: s.stage_linearize(),
                    lambda s: s.stage_backward()),
    "rollout_policy": _each(lambda s: s.RolloutPolicy(_grid(2, 2)),
                            lambda s: s.RolloutPolicy(_grid(B, 2, 2), state_noise=0.5, control_noise=[0.25], seed=7, first_sample=3, common_noise=True),
                            lambda s: s.RolloutPolicy(_grid(2, 2)),
                            lambda s: s.RolloutPolicy(_grid(2, 2), _grid(2, s.system.params.size), trajectories=True)),
    "rollout_policy_stats": _each(lambda s: s.RolloutPolicyStats(4, [0.0, 0.0], [0.5, 0.25]),
                                  lambda s: s.RolloutPolicyStats(4, _grid(B, 2), [0.5, 0.25], x0_dist="uniform", goal=[0.5, np.inf],
                                                                 params_mean=_grid(s.system.params.size), params_spread=_grid(s.system.params.size) / 4,
                                                                 state_noise=[0.5, 0.25], seed=9, first_sample=8, samples=True, envelope=True,
                                                                 controls=True, safe_box=(None, [1.0, np.inf])),
                                  lambda s: s.policy_mc_passes(), lambda s: s.policy_kernel_ms()),
    "plant": _each(lambda s: s.SetPlant(_grid(B, 2), _grid(s.system.params.size), state_noise=0.125, control_noise=_grid(B, 1), seed=5,
                                        common_noise=True, feedback=False, clock=11),
                   lambda s: s.SetPlant([0.5, 0.25]), lambda s: s.plant_state, lambda s: s.plant_clock, lambda s: s.MPCRun(2, 1),
                   lambda s: s.plant_log, lambda s: s.plant_kernel_ms(), lambda s: s.ClearPlant()),
    "multi_start": _each(lambda s: s.PerturbInitialGuess(3, 0.5, seed=4, round=1, hold=2), lambda s: s.SelectBest(3),
                         lambda s: s.ReseedFromBest(1, _grid(B, 1), 2, 3, 1), lambda s: s.GatherBest(3), lambda s: s.seeds_kernel_ms()),
    "solve_multi_start": _each(lambda s: s.SolveMultiStart(3, 2, [0.5], seed=6, hold=2, shrink=0.5)),
    "mpc_run_multi_start": _each(lambda s: (setattr(s, "_sel", s.MPCRunMultiStart(3, 2, 1, 0.25, seed=3, round=5, hold=2)), s._sel)[1],
                                 lambda s: s.mpc_winner_log(s._sel), lambda s: s.mpc_winner_log(s._sel[:1]),
                                 lambda s: s.MPCRunMultiStart(1, 1, 3, _grid(B, 1), target_step=[0.5, 0.25]), lambda s: s.x_nom),
    "mppi": _each(lambda s: s.SetInitialGuess(_grid(1, N - 1)), lambda s: s.MPPIRun(8, 2, [0.5], 0.25, seed=2, first_sample=16, hold=2, shift=1)),
    "state": _each(*(eval("lambda s: s." + k) for k in                                      # noqa: S307
                     ("x_bar", "u_bar", "K", "kappa", "dV_coeff", "fx", "fu", "cost", "history", "iteration_cycles", "iterations", "status",
                      "ls_trials", "keypoint_count", "keypoint_list", "percentage_derivs", "cluster_stats", "stage_cycles")),
                   lambda s: s.set_state(x_bar=_grid(B, 2, N), u_bar=_grid(B, 1, N - 1), K=_grid(B, 1, 2, N - 1), kappa=_grid(B, 1, N - 1),
                                         dV_coeff=_grid(B, N - 1), fx=_grid(B, 2, 2, N - 1), fu=_grid(B, 2, 1, N - 1))),
    "resident": _each(lambda s: s.last_kernel_ms(), lambda s: s.set_timing(2), lambda s: s.Reset(), lambda s: s.rearm(), lambda s: s.rearm(False),
                      lambda s: s.MPCShift(2), lambda s: s.solve_resident(), lambda s: s.solve_resident_async(), lambda s: s.collect(1),
                      lambda s: s.SetTargetStateResident([1.0, 2.0]), lambda s: s.SetTargetStateResident(_grid(B, 2))),
}
# on a handle that answers a get of MI_F_X_REF with OK: the solver "holds a reference trajectory"
TRACKING = _each(lambda s: s.SetTargetTrajectory(_grid(4, 2), clock=2), lambda s: s.target_trajectory, lambda s: s.target_clock,
                 lambda s: s.SetTargetTrajectory(_grid(B, 2, 2)), lambda s: s.MPCRun(2, 1), lambda s: s.MPCRun(2, 1, [0.5, 0.25]),
                 lambda s: s.RolloutPolicy(_grid(2, 2)), lambda s: s.RolloutPolicyStats(4, [0.0, 0.0], [0.5, 0.25]),
                 lambda s: s.SetPlant([0.5, 0.25]), lambda s: s.MPCRunMultiStart(3, 2, 1, 0.25, target_step=[0.5, 0.25]))
LIMITS = _each(lambda s: s.SetControlLimits(-1.0, 2.0), lambda s: s.SetControlLimits([-1.0], [np.inf]),
               lambda s: s.SetControlLimits(-_grid(B, 1), _grid(B, 1)), lambda s: s.SetControlLimits(None, None))
SINGLE = {
    "solve": _each(lambda s: s.SetInitialGuess(_grid(1, N - 1)), _solve),
    "rollout_policy": _each(lambda s: s.RolloutPolicy(_grid(2, 2), trajectories=True, control_noise=0.5)),
    "plant": _each(lambda s: s.SetPlant(np.array([0.5, 0.25]), clock=3), lambda s: s.plant_state, lambda s: s.MPCRun(2, 1), lambda s: s.plant_log),
    "state": _each(*(eval("lambda s: s." + k) for k in ("x_bar", "u_bar", "K", "kappa", "dV_coeff", "fx", "fu", "percentage_derivs"))),   # noqa: S307
}


def _refused(name, which_name, code_name):
    c = _codes()
    return {(name, getattr(c, which_name)): getattr(c, code_name)}


def scenarios():
    """-> [(label, kind, scripted codes, constructor options, play)]"""
    out = []
    for kind in ("plain", "padded"):
        for label, play in BATCHED.items():
            out.append((f"{kind}/{label}", kind, (NO_REF,), {}, play))
        for label in ("solve_shared", "solve_per_problem", "state", "stages"):
            out.append((f"{kind}/pageable/{label}", kind, (NO_REF,), {"pinned_results": False}, BATCHED[label]))
        out.append((f"{kind}/tracking", kind, (), {}, TRACKING))
        out.append((f"{kind}/limits", kind, (NO_REF,), {"control_limits": "enforce"}, LIMITS))
        out.append((f"{kind}/limits_ignored", kind, (NO_REF,), {}, LIMITS))
    ref_refused = _refused("mi_ilqr_set", "F_X_REF", "E_UNSUPPORTED")
    out.append(("plain/reference_refused_no_plant", "plain", (ref_refused, _refused("mi_ilqr_get", "F_PLANT_STATE", "E_BAD_ARG")), {},
                _each(lambda s: s.SetTargetTrajectory(_grid(4, 2)))))
    out.append(("plain/reference_refused_plant", "plain", (ref_refused,), {}, _each(lambda s: s.SetTargetTrajectory(_grid(4, 2)))))
    seeds = _each(lambda s: s.SelectBest(3), lambda s: s.MPCRunMultiStart(3, 2, 1, 0.25), lambda s: s.MPPIRun(8, 2, [0.5], 0.25))
    out.append(("plain/seeds_unsupported", "plain", (NO_REF, _refused("mi_ilqr_set", "F_SEEDS_RUN", "E_UNSUPPORTED")), {}, seeds))
    out.append(("plain/seeds_bad_arg", "plain", (NO_REF, _refused("mi_ilqr_set", "F_SEEDS_RUN", "E_BAD_ARG")), {},
                _each(lambda s: s.MPCRunMultiStart(3, 2, 1, 0.25))))
    for label, play in SINGLE.items():
        out.append((f"single/{label}", "single", (NO_REF,), {}, play))
    out.append(("single/pageable/solve", "single", (NO_REF,), {"pinned_results": False}, SINGLE["solve"]))
    out.append(("single/tracking", "single", (), {}, _each(lambda s: s.SetTargetTrajectory(_grid(4, 2), 1), lambda s: s.target_trajectory,
                                                            lambda s: s.SetTargetTrajectory(None))))
    return out


def run(install, only=None):
    """Play the script -> {label: {"calls": .., "returns": ..}}; calls as [name, selector, byte count, data]."""
    record = {}
    for label, kind, codes, options, play in scenarios():
        if only is not None and label != only:
            continue
        s, fake = make(kind, codes, install, **options)
        returns = play(s)
        record[label] = {"calls": fake.calls, "returns": returns}
        del s
    return record


def _walk(v, data):
    """v with the "data" of every recorded array, however deep, put through `data`."""
    if isinstance(v, list):
        return [_walk(x, data) for x in v]
    if isinstance(v, dict):
        return {k: data(x) if k == "data" else _walk(x, data) for k, x in v.items()}
    return v


def pack(record):
    """The record with the data of every call and of every returned array replaced by its index in a table of the distinct buffers
    (most repeat a few)."""
    buffers, index = [], {}

    def data(buf):
        key = json.dumps(buf)
        if key not in index:
            index[key] = len(buffers)
            buffers.append(buf)
        return index[key]
    return {"scenarios": {label: {"calls": [c[:3] + [data(c[3])] for c in r["calls"]], "returns": _walk(r["returns"], data)}
                          for label, r in record.items()}, "buffers": buffers}


def unpack(packed):
    data = packed["buffers"].__getitem__
    return {label: {"calls": [c[:3] + [data(c[3])] for c in r["calls"]], "returns": _walk(r["returns"], data)}
            for label, r in packed["scenarios"].items()}


def main(argv):
    if len(argv) != 3 or argv[1] != "--record":
        sys.exit("usage: python tests/frontend_fake.py --record FILE")
    sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # (behind PYTHONPATH: another checkout's package wins)
    from drake_ddp_amd import _capi

    def install(fake):
        _capi._lib = fake
    with open(argv[2], "w") as f:
        json.dump(pack(run(install)), f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv)
