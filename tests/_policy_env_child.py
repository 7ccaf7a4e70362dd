"""Helper of tests/test_gpu_policy_env.py: the pendulum case - B = 3, N = 40 (80 state rows: a full row tile and a ragged one),
S = 130 (three groups, a ragged tail), state and control noise, sampled parameters, first_sample = 3, both envelopes and a box - run
in THIS process, whose environment decides the window (MI_ILQR_MC_PASS_GROUPS is read once per process).
`python tests/_policy_env_child.py OUT.npz` writes what run() returns; the test calls run() itself for the default window."""
import functools
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, S, FIRST = 3, 130, 3
TEN = ("n", "counted", "success", "mean", "m2", "min", "max", "argmin", "argmax", "steps_total")
ENV = ("count", "mean", "m2", "min", "max", "argmin", "argmax")
GOAL = [0.5, np.inf]


@functools.lru_cache(maxsize=None)
def setup():
    """-> (a freshly solved pendulum handle, the keywords of the Monte-Carlo calls on it without S and first_sample, x_nom)"""
    from drake_ddp_amd import workloads as W
    from drake_ddp_amd.ilqr import BatchedIterativeLQR
    from drake_ddp_amd.models import ModelSystem
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
    kw = dict(x0_mean=x0b, x0_spread=[0.05, 0.1], params_mean=base, params_spread=0.1 * base, goal=GOAL, state_noise=1e-3, control_noise=1e-2,
              seed=77)
    return s, kw, np.asarray(p["x_nom"], dtype=float)


def stats(s, kw, count=S, first=FIRST, **more):
    k = dict(kw)
    return s.RolloutPolicyStats(count, k.pop("x0_mean"), k.pop("x0_spread"), first_sample=first, **k, **more)


def trajectories(s, kw, st, first=FIRST):
    """RolloutPolicy's trajectories of the samples `st` holds, under the same stream."""
    return s.RolloutPolicy(st.samples.x0, params=st.samples.params, trajectories=True, state_noise=kw["state_noise"],
                           control_noise=kw["control_noise"], seed=kw["seed"], first_sample=first)


def box_between(X):
    """A box from the trajectories X (B, S, n, N) alone: per problem, the velocity's upper bound half way between the two middle
    values of the samples' largest velocities - about half of the samples cross it, none sits on it -, the angle unbounded below
    and bounded above by the largest angle any sample reaches (a value exactly on a bound: inside)."""
    n = X.shape[2]
    lo, hi = np.full((X.shape[0], n), -np.inf), np.full((X.shape[0], n), np.inf)
    top = np.sort(np.nanmax(X[:, :, 1, :], axis=2), axis=1)
    h = X.shape[1] // 2
    hi[:, 1] = 0.5 * (top[:, h - 1] + top[:, h]) if X.shape[1] > 1 else top[:, 0]
    hi[:, 0] = np.nanmax(X[:, :, 0, :], axis=(1, 2))
    return lo, hi


def raw(s, which, shape):
    from drake_ddp_amd import _capi
    out = np.empty(shape)
    _capi.check(s._lib.mi_ilqr_get(s._h, which, _capi.ptr(out), out.nbytes), "mi_ilqr_get")
    return out


def run():
    from drake_ddp_amd import _capi
    s, kw, _ = setup()
    plain = stats(s, kw, samples=True)                                               # before any observing call on this handle
    r = trajectories(s, kw, plain)
    lo, hi = box_between(r.X)
    st = stats(s, kw, samples=True, envelope=True, controls=True, safe_box=(lo, hi))
    out = {"passes": s.policy_mc_passes(), "box_lo": lo, "box_hi": hi, "X": r.X, "U": r.U}
    out["raw_x"] = raw(s, _capi.F_POLICY_MC_ENVELOPE, (B, s.N, s.n, 8))
    out["raw_u"] = raw(s, _capi.F_POLICY_MC_ENVELOPE_U, (B, s.N - 1, s._md, 8))
    out["raw_safety"] = raw(s, _capi.F_POLICY_MC_SAFETY, (B, 3 + s.N))
    for tag, res in (("plain", plain), ("obs", st)):
        out.update({"%s_%s" % (tag, k): getattr(res, k) for k in TEN})
        out.update({"%s_x0" % tag: res.samples.x0, "%s_params" % tag: res.samples.params, "%s_cost" % tag: res.samples.cost,
                    "%s_steps" % tag: res.samples.steps})
    out.update({"env_" + k: getattr(st.envelope, k) for k in ENV})
    out.update({"cenv_" + k: getattr(st.control_envelope, k) for k in ENV})
    out.update({"safety_" + k: getattr(st.safety, k) for k in ("n", "ran", "safe", "safe_success", "exits")})
    return out


if __name__ == "__main__":
    np.savez(sys.argv[1], **run())
