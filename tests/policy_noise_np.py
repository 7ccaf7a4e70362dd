"""NumPy statement of the noisy policy rollouts (include/mi_ilqr.h: "Process and actuation noise"; csrc/philox.hpp,
csrc/policy_rollout.hpp with NZ = true): the Philox4x32-10 block cipher in uint64 arithmetic, the Box-Muller normals by the
device's counter layout, and tests/policy_rollout_np.py's rollout_sample with the disturbances added.

    key     = (seed mod 2^32, seed div 2^32)
    counter = (first_sample + s, t, common ? 0 : b, j)      j = i / 4 for state component i, 256 + k / 4 for control component k
    normal of a component = Box-Muller of the block's words: (w0, w1) -> z0, z1 and (w2, w3) -> z2, z3

    u_t     = u_bar_t - K_t (x_t - x_bar_t)   [clamped]                 the COMMANDED control: what U and the cost see
    x_{t+1} = f(x_t, u_t + sigma_u o xi^u_t) + sigma_x o xi^x_t
"""
import numpy as np

from oracle import models_np as M

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
SHIFT = np.uint64(32)
CONTROL_BLOCK = 256                     # the control stream's first block


def philox4x32_10(ctr, key):
    """ctr (..., 4), key (..., 2) (broadcast against each other), words as integers < 2^32 -> (..., 4) uint64 array of output words."""
    ctr, key = np.asarray(ctr, dtype=np.uint64), np.asarray(key, dtype=np.uint64)
    shape = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    c = [np.broadcast_to(ctr[..., i], shape).copy() for i in range(4)]
    k = [np.broadcast_to(key[..., i], shape).copy() for i in range(2)]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                    # (32 x 32 bits: the product fits a uint64)
        c = [(p1 >> SHIFT) ^ c[1] ^ k[0], p1 & MASK, (p0 >> SHIFT) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return np.stack(c, axis=-1)


def box_muller(wa, wb):
    """Two words -> two standard normals (arrays broadcast): u_a = (wa + 1/2) 2^-32 and u_b likewise are exact in fp64."""
    ua = (np.asarray(wa, dtype=np.float64) + 0.5) * 2.0 ** -32
    ub = (np.asarray(wb, dtype=np.float64) + 0.5) * 2.0 ** -32
    r = np.sqrt(-2.0 * np.log(ua))
    return r * np.cos(2.0 * np.pi * ub), r * np.sin(2.0 * np.pi * ub)


def _stream(seed, first_sample, common, b, s, t, count, first_block):
    """`count` normals of one stream for every (s, t) of the broadcast integer arrays s, t: (..., count)."""
    seed = int(seed)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    s, t = np.broadcast_arrays(np.asarray(s, dtype=np.uint64), np.asarray(t, dtype=np.uint64))
    blocks = (count + 3) // 4
    ctr = np.empty(s.shape + (blocks, 4), dtype=np.uint64)
    ctr[..., 0] = (np.uint64(first_sample) + s)[..., None]
    ctr[..., 1] = t[..., None]
    ctr[..., 2] = np.uint64(0 if common else b)
    ctr[..., 3] = np.uint64(first_block) + np.arange(blocks, dtype=np.uint64)
    assert int(ctr[..., 0].max(initial=0)) < 2 ** 32
    w = philox4x32_10(ctr, key)
    z = np.empty(s.shape + (blocks, 4))
    z[..., 0], z[..., 1] = box_muller(w[..., 0], w[..., 1])
    z[..., 2], z[..., 3] = box_muller(w[..., 2], w[..., 3])
    return z.reshape(s.shape + (4 * blocks,))[..., :count]


def state_normals(seed, first_sample, common, b, s, t, n):
    """xi^x of problem b for the samples s and steps t (integer arrays, broadcast): (..., n)."""
    return _stream(seed, first_sample, common, b, s, t, n, 0)


def control_normals(seed, first_sample, common, b, s, t, m):
    """xi^u likewise: (..., m)."""
    return _stream(seed, first_sample, common, b, s, t, m, CONTROL_BLOCK)


def rollout_sample_noisy(model, x0, x_bar, u_bar, K, Q, R, Qf, x_nom, sigma_x, sigma_u, zx, zu, u_min=None, u_max=None):
    """policy_rollout_np.rollout_sample with the disturbances sigma_x o zx[t] on the state and sigma_u o zu[t] on the applied
    control; zx (N-1, n), zu (N-1, m).  -> cost, x_final (n,), steps, X (n, N), U (m, N-1): U is the commanded control."""
    n, N = x_bar.shape
    m = u_bar.shape[0]
    bad = M.INFEASIBLE_FUNCS.get(model.model_id)
    X, U = np.full((n, N), np.nan), np.full((m, N - 1), np.nan)
    x = np.array(x0, dtype=float).reshape(n)
    X[:, 0] = x
    L, steps = 0.0, 0
    alive = bool(np.isfinite(x).all())
    for t in range(N - 1):
        if not alive:
            break
        u = u_bar[:, t] - K[:, :, t] @ (x - x_bar[:, t])
        if u_min is not None:
            u = np.clip(u, u_min, u_max)
        with np.errstate(all="ignore"):
            xn = model.step_unchecked(x, u + sigma_u * zu[t]) + sigma_x * zx[t]
        if not np.isfinite(xn).all() or (bad is not None and bad(list(xn), model.params)):
            alive = False
            break
        dx = x - x_nom
        L += dx @ Q @ dx + u @ R @ u
        U[:, t] = u
        X[:, t + 1] = xn
        x = xn
        steps += 1
    if alive:
        dx = x - x_nom
        L += dx @ Qf @ dx
    else:
        L = np.inf
    return L, x, steps, X, U


def rollout_noisy(make_model, x0, params, x_bar, u_bar, K, Q, R, Qf, x_nom, sigma, seed=0, first_sample=0, common=False,
                  u_min=None, u_max=None, shift=0.0):
    """The batched form, the arguments of policy_rollout_np.rollout plus sigma (B, n + m) = sigma_x | sigma_u and the stream.
    `shift` is added to every normal (the reference's own sensitivity to the last digits of the normals).
    -> cost (B,S), x_final (B,S,n), steps (B,S) int32, X (B,S,n,N), U (B,S,m,N-1)."""
    B, S, n = x0.shape
    N, m = x_bar.shape[2], u_bar.shape[1]
    row = lambda a, b, nd: a if a is None or np.ndim(a) == nd else a[b]   # noqa: E731
    cost, xf, steps = np.empty((B, S)), np.empty((B, S, n)), np.empty((B, S), dtype=np.int32)
    X, U = np.empty((B, S, n, N)), np.empty((B, S, m, N - 1))
    ss, tt = np.arange(S)[:, None], np.arange(N - 1)[None, :]
    for b in range(B):
        zx = state_normals(seed, first_sample, common, b, ss, tt, n) + shift
        zu = control_normals(seed, first_sample, common, b, ss, tt, m) + shift
        shared = make_model(params[b]) if np.ndim(params) == 2 else None
        for s in range(S):
            model = shared if shared is not None else make_model(params[b, s])
            cost[b, s], xf[b, s], steps[b, s], X[b, s], U[b, s] = rollout_sample_noisy(
                model, x0[b, s], x_bar[b], u_bar[b], K[b], row(Q, b, 2), row(R, b, 2), row(Qf, b, 2), row(x_nom, b, 1),
                sigma[b, :n], sigma[b, n:], zx[s], zu[s], row(u_min, b, 1), row(u_max, b, 1))
    return cost, xf, steps, X, U


# ---------------------------------------------------------------- what the tests share
TEST_SEED = 0x123456789ABCDE            # the stream of the moment tests (CPU: this file's; GPU: the device's): both key words non-zero
NORMAL_TOL = 4e-14                      # |z - z_exact|: three functions good to 2 ulp and one product, 6 ulp at |z| <= 6.77 = 9e-15; x 4


def assert_moments(z):
    """z (S, T, C): samples x steps x components of one stream.  Mean, variance and the correlations between neighbouring samples,
    steps and components, each within five standard deviations of its estimator under independence."""
    cnt = z.size
    assert abs(z.mean()) <= 5.0 / np.sqrt(cnt), z.mean()
    assert abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / cnt), z.var()
    for axis, what in enumerate(("samples", "steps", "components")):
        a, b = np.moveaxis(z, axis, 0)[:-1], np.moveaxis(z, axis, 0)[1:]
        r = float(np.mean((a - a.mean()) * (b - b.mean())) / (a.std() * b.std()))
        assert abs(r) <= 5.0 / np.sqrt(a.size), (what, r)
    assert np.abs(z).max() <= np.sqrt(66.0 * np.log(2.0)) + NORMAL_TOL
