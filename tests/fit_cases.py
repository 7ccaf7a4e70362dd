"""The identification problems tests/test_fit_oracle.py and tests/test_gpu_fit.py share: per kind a model, its free parameters, B true
parameter rows (the defaults with the free entries moved by up to 10 %), B starts (the truth with the free entries off by a
uniform +-spread) and T noise-free transitions per problem generated with the oracle's step on the TRUE row - random states and
controls for the small models, one rollout per problem from the workload's initial states under its initial guess plus control
noise for the large ones, so that the states are ones the model meets (ground and ball contact included)."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fit_np as FN  # noqa: E402
from oracle import models_np as M  # noqa: E402

# kind: model id, dt, free parameters, the start's spread.  The free sets of the six recovery cases are identifiable in such data.
KINDS = {
    "pendulum": (M.PENDULUM, 1e-2, [0, 1, 2], 0.3), "acrobot": (M.ACROBOT, 4e-3, [1, 7, 8], 0.3), "cart_pole": (M.CARTPOLE, 1e-2, [0, 1, 2], 0.3),
    "cart_pole_with_wall": (M.CARTPOLE_WALL, 1e-2, [0, 1, 2], 0.2), "synth36": (M.SYNTH36, 2e-2, [0, 3], 0.2),
    "planar_quad": (M.PLANAR_QUAD, 4e-3, [0], 0.2), "quad3d": (M.QUAD3D, 4e-3, [0], 0.2), "arm27": (M.ARM27, 1e-2, [0, 3, 7], 0.2),
    "arm27c": (M.ARM27C, 1e-2, [0, 3], 0.2),
}
RECOVERY = ("pendulum", "acrobot", "cart_pole", "synth36", "arm27", "quad3d")


class Case:
    pass


def _random_rows(kind, rng, B, T):
    U = rng.uniform
    if kind == "pendulum":
        return np.stack([U(-np.pi, np.pi, (B, T)), U(-3, 3, (B, T))], axis=2), U(-2, 2, (B, T, 1))
    if kind == "acrobot":
        return np.concatenate([U(-np.pi, np.pi, (B, T, 2)), U(-2, 2, (B, T, 2))], axis=2), U(-2, 2, (B, T, 1))
    lo = -0.6 if kind == "cart_pole_with_wall" else -1.0
    return np.concatenate([U(lo, 0.3, (B, T, 1)), U(-np.pi, np.pi, (B, T, 1)), U(-2, 2, (B, T, 2))], axis=2), U(-10, 10, (B, T, 1))


def _rollout_inputs(kind, rng, B, T):
    from drake_ddp_amd import workloads as W
    x0, ug, s = {"synth36": (W.synth36_batch_x0, W.synth36_u_guess, 0.3), "planar_quad": (W.planar_quad_batch_x0, W.planar_quad_u_guess, 0.5),
                 "quad3d": (W.quad3d_batch_x0, W.quad3d_u_guess, 0.5), "arm27": (W.arm27_batch_x0, W.arm27_u_guess, 0.3),
                 "arm27c": (W.arm27_batch_x0, W.arm27c_u_guess, 0.3)}[kind]
    u = ug(T + 1).T[None] + s * rng.standard_normal((B, T, ug(2).shape[0]))
    return x0(B), u


# The arm's contact is not smooth: from the default first damping 1e-3 the ORACLE spends up to four of its eight trials on
# rejections (seed 0: problem 1 ends at 4.6e-3) - with mu0 = 1 and the data of seed 2 it accepts all eight and ends at 1.6e-15 or
# below in every problem: the case the recovery tests are about.  FIT_KW: what a kind's recovery runs pass on both sides.
SEEDS = {"arm27": 2}
FIT_KW = {"arm27": dict(damping=1.0)}


@functools.lru_cache(maxsize=None)
def case(kind, B=3, T=70, seed=None):
    seed = SEEDS.get(kind, 0) if seed is None else seed
    mid, dt, free, spread = KINDS[kind]
    rng = np.random.default_rng(1000 * sorted(KINDS).index(kind) + seed)
    c = Case()
    c.kind, c.model_id, c.dt, c.free, c.B, c.T = kind, mid, dt, list(free), B, T
    c.n, c.m = M.MODEL_DIMS[mid]
    base = np.array(M.DEFAULT_PARAMS[mid], dtype=float)
    c.truth = np.tile(base, (B, 1))
    c.truth[:, free] *= 1.0 + 0.1 * rng.uniform(-1, 1, (B, len(free)))
    c.start = c.truth.copy()
    c.start[:, free] *= 1.0 + spread * rng.choice([-1.0, 1.0], (B, len(free))) * rng.uniform(0.5, 1.0, (B, len(free)))
    c.models = [M.Model(mid, dt, c.truth[b]) for b in range(B)]
    if kind in ("pendulum", "acrobot", "cart_pole", "cart_pole_with_wall"):
        c.x, c.u = _random_rows(kind, rng, B, T)
        c.x_next = np.stack([FN.predict(c.models[b], c.truth[b], c.x[b], c.u[b]) for b in range(B)])
    else:
        x0, c.u = _rollout_inputs(kind, rng, B, T)
        X = np.empty((B, T + 1, c.n))
        X[:, 0] = x0
        for b in range(B):
            for t in range(T):
                X[b, t + 1] = c.models[b].step_unchecked(X[b, t], c.u[b, t])
        c.x, c.x_next = np.ascontiguousarray(X[:, :-1]), np.ascontiguousarray(X[:, 1:])
    assert np.isfinite(c.x_next).all(), kind
    for a in (c.x, c.u, c.x_next, c.truth, c.start):
        a.setflags(write=False)
    return c


def oracle_fit(c, b, **kw):
    a = dict(theta0=c.start[b], free=c.free, **FIT_KW.get(c.kind, {}))
    a.update(kw)
    return FN.fit(c.models[b], c.x[b], c.u[b], c.x_next[b], **a)


def rel_error(c, params):
    """(B,) the worst relative error of the free entries against the truth."""
    params = np.asarray(params).reshape(-1, c.truth.shape[1])
    return np.max(np.abs(params[:, c.free] - c.truth[: len(params), c.free]) / np.abs(c.truth[: len(params), c.free]), axis=1)
