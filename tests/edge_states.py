"""Single states of the small built-in models where the golden trajectories never go (tests/test_gpu_edge_steps.py): angles up to
1e4 rad, velocities up to 1e3, the acrobot's q2 at multiples of pi (M12 extremal), the cart-pole's wall gap phi / sigma across
[-800, 800] and at 0.  Built from a seed without any libm call, so they come out bit for bit on every machine; truth of one step
and of its Jacobian: tests/golden/edge_<model>.npz (oracle/gen_edge_step_golden.py - oracle/models_np.py's own step functions
evaluated in mpmath), as `hi` and `lo` = (truth - hi) / ulp(hi), float32, like the primitives' fixtures."""
import hashlib
import os

import numpy as np

SEED = 20261017
B = 256
MODELS = ("pendulum", "acrobot", "cartpole", "cartpole_wall")
MODEL_ID = {"pendulum": 0, "acrobot": 1, "cartpole": 2, "cartpole_wall": 3}       # oracle/models_np.py
DT = {"pendulum": 1e-2, "acrobot": 0.004, "cartpole": 1e-2, "cartpole_wall": 1e-2}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def states(model):
    """(x (B, n), u (B, 1))."""
    rng = np.random.default_rng(SEED + MODEL_ID[model])
    ang = lambda k: np.concatenate([rng.uniform(-1e4, 1e4, k - k // 4), rng.uniform(-4.0, 4.0, k // 4)])      # noqa: E731
    vel = lambda k: np.concatenate([rng.uniform(-1e3, 1e3, k // 2), rng.uniform(-5.0, 5.0, k - k // 2)])       # noqa: E731
    if model == "pendulum":
        return np.stack([ang(B), rng.permutation(vel(B))], axis=1), rng.uniform(-2.0, 2.0, (B, 1))
    if model == "acrobot":
        q2 = ang(B)
        q2[::2] = rng.integers(-3000, 3001, B // 2) * np.pi                  # the doubles at k pi (one rounding of the product)
        q2[:8:2] = np.array([0.0, 1.0, -1.0, 2.0]) * np.pi
        return np.stack([rng.permutation(ang(B)), q2, rng.permutation(vel(B)), rng.permutation(vel(B))], axis=1), rng.uniform(-5.0, 5.0, (B, 1))
    x = np.stack([rng.uniform(-2.0, 2.0, B), rng.permutation(ang(B)), rng.permutation(vel(B)), rng.permutation(vel(B))], axis=1)
    if model == "cartpole_wall":
        # gap phi = px + l sin(theta) - rad - face, in units of sigma: with theta = 0 (even rows) px sets it to g up to round-off -
        # 0, +-800, +-745, +-36.7 (where the softplus's exp leaves the double's range and its log1p's argument drops below an ulp)
        # and a uniform sweep; odd rows keep a general angle, px = face + rad + g sigma - l S with S uniform in [-1, 1]
        face, rad, sig, l = -0.45, 0.05, 0.01, 0.5                           # models_np.DEFAULT_PARAMS[CARTPOLE_WALL]
        g = rng.uniform(-800.0, 800.0, B)
        g[:18:2] = [0.0, 800.0, -800.0, 745.0, -745.0, 36.7, -36.7, 0.88, -0.88]
        S = rng.uniform(-1.0, 1.0, B)
        S[::2] = 0.0
        x[::2, 1] = 0.0
        x[:, 0] = (face + rad) + g * sig - l * S
    return x, rng.uniform(-10.0, 10.0, (B, 1))


def digest(model):
    x, u = states(model)
    return hashlib.sha1(np.ascontiguousarray(np.concatenate([x, u], axis=1)).tobytes()).hexdigest()


def load(model):
    with np.load(os.path.join(GOLDEN, "edge_%s.npz" % model)) as z:
        return {k: z[k] for k in z.files}


def value(hi, lo):
    """hi + lo ulp(hi) in long double."""
    return hi.astype(np.longdouble) + lo.astype(np.longdouble) * np.spacing(np.abs(hi)).astype(np.longdouble)


def worst(a, hi, lo):
    """Per output component: the largest |a - truth| over the batch (axis 0)."""
    return np.max(np.abs(a.astype(np.longdouble) - value(hi, lo)), axis=0).astype(np.float64)
