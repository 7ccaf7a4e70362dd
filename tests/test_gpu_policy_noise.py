"""Process and actuation noise of the Monte-Carlo policy rollouts on the device (RolloutPolicy's state_noise / control_noise,
MI_F_POLICY_NOISE / MI_F_POLICY_STREAM; csrc/philox.hpp, csrc/policy_rollout.hpp with NZ = true) against the NumPy statement of
the same thing (tests/policy_noise_np.py): the generator read through a plant that passes the disturbances through, rollouts of
solved policies on every kernel family, the equivalences with the noise-free path, and the isolation of failing samples.

Tolerance against the oracle: the rule of tests/test_gpu_policy_rollout.py - 1e-9 relative + 10 x the oracle's own spread - where
the spread now is the largest change of the oracle under a one-ulp perturbation of x0 in both directions AND under every normal
moved by +-4e-14 (what a device normal may differ from the oracle's by: policy_noise_np.NORMAL_TOL).  The sigmas - about 1e-3
of the state scale, 1e-2 of the control scale - keep that spread below 1e-6 relative, which _reference asserts with the oracle alone."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "plugins"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import policy_noise_np as PN  # noqa: E402
import test_gpu_policy_rollout as TP  # noqa: E402  (its cached handles with a policy on them, its comparison rule)

pytestmark = pytest.mark.gpu

B = TP.B
S_VALUES = TP.S_VALUES
S_MAX = TP.S_MAX
SEED = PN.TEST_SEED
FIELDS = ("cost", "x_final", "steps", "X", "U")


def _same(r, q, sel=slice(None)):
    return all(np.array_equal(getattr(r, a)[:, sel], getattr(q, a)[:, sel], equal_nan=True) for a in FIELDS)


# ---------------------------------------------------------------- 1. the generator through the public interface
PROBE_N, PROBE_M = 40, 16


@functools.lru_cache(maxsize=None)
def _probe(batch):
    """A cold handle on the noise probe (examples/plugins/models.py: x+ = 0 x + u): the policy is zero, so with x0 = 0 the states
    after the first ARE the disturbances."""
    import models as PM
    from drake_ddp_amd import plugin
    sys_ = plugin.build_model(*PM.NOISEPROBE_SPEC)(0.01)
    assert (sys_.n, sys_.m) == (PROBE_N, PROBE_M)

    def make(N):
        p = dict(model_id=sys_.model_id, dt=0.01, N=N, delta=1e-3, beta=0.5, gamma=0.0, Q=np.eye(PROBE_N), R=np.eye(PROBE_M),
                 Qf=np.eye(PROBE_N), x_nom=np.zeros(PROBE_N))
        return TP._solver(p, system=sys_, batch=batch)
    return {N: make(N) for N in (5, 2)}


def _grid(S, N):
    """sample and step indices of a call, to broadcast: (S, 1), (1, N-1)"""
    return np.arange(S)[:, None], np.arange(N - 1)[None, :]


@pytest.mark.parametrize("N", [5, 2])
def test_the_state_and_control_streams(N):
    S = 130                                                           # three waves, the last one ragged
    s = _probe(2)[N]
    x0 = np.zeros((2, S, PROBE_N))
    ss, tt = _grid(S, N)
    r = s.RolloutPolicy(x0, trajectories=True, state_noise=1.0, seed=SEED)
    assert np.all(r.steps == N - 1) and np.all(r.X[..., 0] == 0.0) and np.all(r.U == 0.0)
    worst = 0.0
    for b in range(2):
        z = PN.state_normals(SEED, 0, False, b, ss, tt, PROBE_N)      # (S, N-1, n)
        e = np.abs(np.moveaxis(r.X[b, :, :, 1:], 1, 2) - z).max()
        worst = max(worst, e)
        assert e <= PN.NORMAL_TOL, (b, e)
        assert np.array_equal(r.x_final[b], r.X[b, :, :, -1])
    # the cost is the commanded (zero) control's and the noisy states': sum of squares with unit matrices
    assert np.allclose(r.cost, (r.X ** 2).sum(axis=(2, 3)), rtol=1e-12, atol=0.0)
    c = s.RolloutPolicy(x0, trajectories=True, control_noise=1.0, seed=SEED)
    for b in range(2):
        z = PN.control_normals(SEED, 0, False, b, ss, tt, PROBE_M)
        e = np.abs(np.moveaxis(c.X[b, :, :PROBE_M, 1:], 1, 2) - z).max()
        worst = max(worst, e)
        assert e <= PN.NORMAL_TOL, (b, e)
    assert np.all(c.X[:, :, PROBE_M:, :] == 0.0) and np.all(c.U == 0.0) and np.all(c.steps == N - 1)      # U: the COMMANDED controls
    print("noise probe N=%d: worst |device normal - oracle normal| %.2e" % (N, worst))


def test_sigma_rows_seeds_common_and_first_sample():
    S, N = 130, 5
    s = _probe(2)[N]
    x0 = np.zeros((2, S, PROBE_N))
    one = s.RolloutPolicy(x0, trajectories=True, state_noise=1.0, control_noise=1.0, seed=SEED)
    # per-problem rows scale exactly: problem 1 with twice the sigma of problem 0; per-component rows too
    sx = np.ones((2, PROBE_N)); sx[1] = 2.0
    su = np.ones((2, PROBE_M)); su[1] = 2.0
    two = s.RolloutPolicy(x0, trajectories=True, state_noise=sx, control_noise=su, seed=SEED)
    assert np.array_equal(two.X[0], one.X[0]) and np.array_equal(two.X[1], 2.0 * one.X[1])
    comp = np.arange(PROBE_N, dtype=float)
    only_x = s.RolloutPolicy(x0, trajectories=True, state_noise=1.0, seed=SEED)
    scaled = s.RolloutPolicy(x0, trajectories=True, state_noise=comp, seed=SEED)
    assert np.array_equal(scaled.X, only_x.X * comp[None, None, :, None]) and np.all(scaled.X[:, :, 0, :] == 0.0)
    # the same seed twice; another seed; a seed that differs in the key's high word only
    again = s.RolloutPolicy(x0, trajectories=True, state_noise=1.0, control_noise=1.0, seed=SEED)
    assert _same(again, one)
    for other in (SEED + 1, SEED + 2 ** 32):
        o = s.RolloutPolicy(x0, trajectories=True, state_noise=1.0, control_noise=1.0, seed=other)
        assert not np.array_equal(o.X[..., 1:], one.X[..., 1:]) and np.all(o.X[..., 1:] != one.X[..., 1:])
    # common random numbers
    assert not np.array_equal(one.X[0], one.X[1])
    com = s.RolloutPolicy(x0, trajectories=True, state_noise=1.0, control_noise=1.0, seed=SEED, common_noise=True)
    assert np.array_equal(com.X[0], com.X[1]) and np.array_equal(com.X[0], one.X[0])
    # a later window of the same stream: S = 66 from first_sample = 64 is samples 64 .. 129 of the S = 130 call
    win = s.RolloutPolicy(x0[:, :66], trajectories=True, state_noise=1.0, control_noise=1.0, seed=SEED, first_sample=64)
    assert _same(win, type(one)(*(getattr(one, a)[:, 64:130] for a in FIELDS)))
    # the last sample numbers there are
    top = s.RolloutPolicy(x0[:, :3], trajectories=True, state_noise=1.0, seed=SEED, first_sample=2 ** 32 - 3)
    z = PN.state_normals(SEED, 2 ** 32 - 3, False, 1, *_grid(3, N), PROBE_N)
    assert np.abs(np.moveaxis(top.X[1, :, :, 1:], 1, 2) - z).max() <= PN.NORMAL_TOL


def test_moments_on_the_device():
    """B = 1, S = 4096, N = 5: the stream of tests/test_policy_noise_oracle.py's moment test, with its bounds."""
    s = _probe(1)[5]
    x0 = np.zeros((1, 4096, PROBE_N))
    r = s.RolloutPolicy(x0, trajectories=True, state_noise=1.0, seed=SEED)
    PN.assert_moments(np.moveaxis(r.X[0, :, :, 1:], 1, 2))
    c = s.RolloutPolicy(x0, trajectories=True, control_noise=1.0, seed=SEED)
    PN.assert_moments(np.moveaxis(c.X[0, :, :PROBE_M, 1:], 1, 2))


def test_the_selectors_through_the_c_abi():
    from drake_ddp_amd import _capi
    s = _probe(2)[5]
    lib, h = s._lib, s._h
    w = PROBE_N + PROBE_M
    s.RolloutPolicy(np.zeros((2, 3, PROBE_N)))                         # (clears whatever an earlier test left)
    got, st = np.full((2, w), -1.0), np.full(3, -1.0)
    assert lib.mi_ilqr_get(h, _capi.F_POLICY_NOISE, _capi.ptr(got), got.nbytes) == _capi.OK and np.all(got == 0.0)     # not set: zeros
    rows = np.arange(2 * w, dtype=float).reshape(2, w)
    assert lib.mi_ilqr_set(h, _capi.F_POLICY_NOISE, _capi.ptr(rows), rows.nbytes) == _capi.OK
    stream = np.array([2.0 ** 53 - 1, 2.0 ** 32 - 1, 1.0])
    assert lib.mi_ilqr_set(h, _capi.F_POLICY_STREAM, _capi.ptr(stream), 24) == _capi.OK
    for bad in (rows[:, :-1].copy(), np.zeros((2, w + 1))):
        assert lib.mi_ilqr_set(h, _capi.F_POLICY_NOISE, _capi.ptr(bad), bad.nbytes) == _capi.E_BAD_SHAPE
    for v in (-1.0, np.nan, np.inf):
        bad = rows.copy(); bad[1, 7] = v
        assert lib.mi_ilqr_set(h, _capi.F_POLICY_NOISE, _capi.ptr(bad), bad.nbytes) == _capi.E_BAD_ARG
    assert lib.mi_ilqr_set(h, _capi.F_POLICY_NOISE, None, rows.nbytes) == _capi.E_BAD_ARG
    assert lib.mi_ilqr_set(h, _capi.F_POLICY_STREAM, _capi.ptr(stream), 16) == _capi.E_BAD_SHAPE
    for bad in ([-1.0, 0, 0], [2.0 ** 53, 0, 0], [0.5, 0, 0], [np.nan, 0, 0], [0, -1.0, 0], [0, 2.0 ** 32, 0], [0, 1.5, 0], [0, 0, 2.0],
                [0, 0, 0.5], [0, 0, np.nan]):
        assert lib.mi_ilqr_set(h, _capi.F_POLICY_STREAM, _capi.ptr(np.array(bad, dtype=float)), 24) == _capi.E_BAD_ARG, bad
    # the refused calls changed nothing
    assert lib.mi_ilqr_get(h, _capi.F_POLICY_NOISE, _capi.ptr(got), got.nbytes) == _capi.OK and np.array_equal(got, rows)
    assert lib.mi_ilqr_get(h, _capi.F_POLICY_STREAM, _capi.ptr(st), 24) == _capi.OK and np.array_equal(st, stream)
    assert lib.mi_ilqr_get(h, _capi.F_POLICY_STREAM, _capi.ptr(st), 8) == _capi.E_BAD_SHAPE
    # first_sample + S > 2^32 is refused by the rollout itself; S = 1 still fits
    x0, cost = np.zeros((2, 2, PROBE_N)), np.empty((2, 2))
    call = lambda S_: lib.mi_ilqr_policy_rollout(h, S_, _capi.ptr(x0), None, _capi.ptr(cost), None, None, None, None)   # noqa: E731
    assert call(2) == _capi.E_BAD_ARG and call(1) == _capi.OK
    # the rows survive a reset; clearing returns the zeros
    assert lib.mi_ilqr_reset(h) == _capi.OK
    assert lib.mi_ilqr_get(h, _capi.F_POLICY_NOISE, _capi.ptr(got), got.nbytes) == _capi.OK and np.array_equal(got, rows)
    assert lib.mi_ilqr_set(h, _capi.F_POLICY_NOISE, None, 0) == _capi.OK
    assert lib.mi_ilqr_get(h, _capi.F_POLICY_NOISE, _capi.ptr(got), got.nbytes) == _capi.OK and np.all(got == 0.0)
    assert call(2) == _capi.OK                                         # (no noise: the sample counter is not used)
    assert lib.mi_ilqr_set(h, _capi.F_POLICY_STREAM, _capi.ptr(np.zeros(3)), 24) == _capi.OK
    s._policy_noise_set = False


def test_a_sigma_on_a_padding_control_is_refused():
    from drake_ddp_amd import _capi
    c = _padded()
    s = c.s
    w = c.n + 4
    rows = np.zeros((B, w)); rows[:, c.n:c.n + 3] = 0.1
    assert s._lib.mi_ilqr_set(s._h, _capi.F_POLICY_NOISE, _capi.ptr(rows), rows.nbytes) == _capi.OK
    bad = rows.copy(); bad[2, c.n + 3] = 1e-3
    assert s._lib.mi_ilqr_set(s._h, _capi.F_POLICY_NOISE, _capi.ptr(bad), bad.nbytes) == _capi.E_BAD_ARG
    user = np.zeros((B, c.n + 3))                                      # (the row has the DEVICE's number of controls)
    assert s._lib.mi_ilqr_set(s._h, _capi.F_POLICY_NOISE, _capi.ptr(user), user.nbytes) == _capi.E_BAD_SHAPE
    assert s._lib.mi_ilqr_set(s._h, _capi.F_POLICY_NOISE, None, 0) == _capi.OK


# ---------------------------------------------------------------- 2. rollouts against the oracle
def _sigma(name, n, m):
    """sigma_x (n,), sigma_u (m,): about 1e-3 of the state scale and 1e-2 of the control scale of each problem."""
    sx, su = {"pendulum": (3e-3, 1e-2), "pendulum_throughput": (3e-3, 1e-2), "acrobot": (2e-3, 1e-2), "arm27": (1e-3, 5e-2),
              "quad3d": (1e-3, 5e-2), "chainx": (1e-3, 1e-2)}[name]
    sx, su = np.full(n, sx), np.full(m, su)
    if name == "quad3d":
        sx[:4] = 0.0                                                   # the attitude quaternion gets no noise of its own
    return sx, su


class _Ctx:
    pass


@functools.lru_cache(maxsize=None)
def _padded():
    """The (37, 3) chainx plugin of test_gpu_policy_rollout.py::test_padding_controls - n > 32, four device controls - with a policy."""
    import plugin_steps as PS
    from oracle import models_np as M
    nq, m, ne, dt, N = 16, 3, 5, 0.02, 12
    c = _Ctx()
    c.n = n = 2 * nq + ne
    sys_ = TP._plugins()[0](dt)
    assert sys_.m == m and sys_.m_dev == 4
    c.p = dict(model_id=sys_.model_id, dt=dt, N=N, delta=1e-3, beta=0.6, gamma=0.0, Q=dt * np.eye(n), R=dt * 0.1 * np.eye(m),
               Qf=5.0 * np.eye(n), x_nom=np.zeros(n))
    rng = np.random.default_rng(8)
    c.x0b = 0.3 * rng.standard_normal((B, n))
    c.s = TP._solver(c.p, system=sys_, max_iters=3)
    c.s.SetInitialState(c.x0b); c.s.SetInitialGuess(np.zeros((m, N - 1)))
    TP._solve(c.s)
    c.x_bar, c.u_bar, c.K = np.array(c.s.x_bar), np.array(c.s.u_bar), np.array(c.s.K)
    c.x0 = c.x0b[:, None, :] + 0.01 * rng.standard_normal((B, S_MAX, n)); c.x0[:, 0] = c.x0b
    c.base = np.tile(sys_.params, (B, 1))
    c.params = sys_.params[None, None, :] * rng.uniform(0.8, 1.2, (B, S_MAX, sys_.params.size))
    c.make_model = lambda row: M.Model.custom(n, m, PS.chainx_step(nq, m, ne), row, dt)
    return c


def _case(name):
    return _padded() if name == "chainx" else TP._ctx(name)


def _oracle_with_spread(c, x0, params, sigma, seed, u_min=None, u_max=None):
    """The noisy oracle's result for every sample and its own spread (cost, X, U per sample): x0 one ulp up and down, every normal
    4e-14 up and down."""
    p = c.p
    run = lambda x, shift: PN.rollout_noisy(c.make_model, x, params, c.x_bar, c.u_bar, c.K, p["Q"], p["R"], p["Qf"], p["x_nom"], sigma,   # noqa: E731
                                            seed, 0, False, u_min, u_max, shift)
    ref = run(x0, 0.0)
    sp = [np.zeros(ref[0].shape) for _ in range(3)]
    for alt in (run(np.nextafter(x0, np.inf), 0.0), run(np.nextafter(x0, -np.inf), 0.0), run(x0, PN.NORMAL_TOL), run(x0, -PN.NORMAL_TOL)):
        with np.errstate(invalid="ignore"):
            sp[0] = np.fmax(sp[0], np.abs(alt[0] - ref[0]))
            sp[1] = np.fmax(sp[1], np.nanmax(np.abs(alt[3] - ref[3]), axis=(2, 3)))
            sp[2] = np.fmax(sp[2], np.nanmax(np.abs(alt[4] - ref[4]), axis=(2, 3)))
    return ref, sp


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = _case(name)
    n, m = c.x0.shape[2], c.u_bar.shape[1]
    sigma = np.tile(np.concatenate(_sigma(name, n, m)), (B, 1)) * np.array([1.0, 0.5, 2.0])[:, None]      # (a row per problem)
    ref, sp = _oracle_with_spread(c, c.x0, c.base, sigma, SEED + 17)
    TP._assert_spread_small(ref, sp)
    return sigma, ref, sp


CASES = ["pendulum", "pendulum_throughput", "acrobot", "arm27", "quad3d", "chainx"]


@pytest.mark.parametrize("S", S_VALUES)
@pytest.mark.parametrize("name", CASES)
def test_against_the_oracle(name, S):
    c = _case(name)
    n = c.x0.shape[2]
    sigma, ref, sp = _reference(name)
    r = c.s.RolloutPolicy(c.x0[:, :S], trajectories=True, state_noise=sigma[:, :n], control_noise=sigma[:, n:], seed=SEED + 17)
    TP._compare(r, ref, sp, S, report="%s with noise" % name)
    free = c.s.RolloutPolicy(c.x0[:, :S], trajectories=True)           # the noise does move the rollouts, by about its size
    with np.errstate(invalid="ignore"):
        assert np.all(np.nanmax(np.abs(r.X - free.X), axis=(1, 2, 3)) > 0.1 * sigma[:, :n].max(axis=1))
    lean = c.s.RolloutPolicy(c.x0[:, :S], state_noise=sigma[:, :n], control_noise=sigma[:, n:], seed=SEED + 17)
    assert lean.X is None and np.array_equal(lean.cost, r.cost) and np.array_equal(lean.x_final, r.x_final)
    c.s.RolloutPolicy(c.x0[:, :1])                                     # (leave the shared handle without noise)


def test_noise_with_per_sample_parameters_and_active_limits():
    c = TP._ctx("pendulum")
    p = c.p
    S = 65
    lo, hi = np.array([[-0.4], [-0.2], [-1.0]]), np.array([[0.3], [0.5], [0.1]])
    rng = np.random.default_rng(21)
    x0 = c.x0b[:, None, :] + 1.5 * rng.standard_normal((B, S, 2))      # far enough out that the feedback saturates
    prm = np.ascontiguousarray(c.params[:, :S])
    sigma = np.tile([3e-3, 3e-3, 5e-2], (B, 1))
    s = TP._solver(p, control_limits="enforce")
    s.SetControlLimits(lo, hi)
    s.set_state(x_bar=c.x_bar, u_bar=c.u_bar, K=c.K)
    r = s.RolloutPolicy(x0, prm, trajectories=True, state_noise=sigma[:, :2], control_noise=sigma[:, 2:], seed=5)
    assert np.all(r.U >= lo[:, None, :, None]) and np.all(r.U <= hi[:, None, :, None])       # the commanded control, exactly inside
    assert np.any(r.U == lo[:, None, :, None]) and np.any(r.U == hi[:, None, :, None])
    ref, sp = _oracle_with_spread(c, x0, prm, sigma, 5, lo, hi)
    TP._assert_spread_small(ref, sp)
    TP._compare(r, ref, sp, S, report="pendulum clamped, per-sample parameters, with noise")


# ---------------------------------------------------------------- 3. equivalences
@pytest.mark.parametrize("name", ["pendulum", "quad3d", "chainx"])
def test_zero_sigma_and_clearing(name):
    c = _case(name)
    S = 65
    n, m = c.x0.shape[2], c.u_bar.shape[1]
    x0 = np.ascontiguousarray(c.x0[:, :S])
    before = c.s.RolloutPolicy(x0, trajectories=True)
    zero = c.s.RolloutPolicy(x0, trajectories=True, state_noise=0.0, control_noise=np.zeros((B, m)), seed=3)       # the noisy kernel, both streams skipped
    for a in FIELDS:
        assert np.all((getattr(zero, a) == getattr(before, a)) | (np.isnan(getattr(zero, a)) & np.isnan(getattr(before, a)))), a
    sx = np.zeros((B, n)); sx[1] = _sigma("chainx" if name == "chainx" else name, n, m)[0]
    mixed = c.s.RolloutPolicy(x0, trajectories=True, state_noise=sx, seed=3)                                         # ... and per problem
    assert _same(type(mixed)(*(getattr(mixed, a)[[0, 2]] for a in FIELDS)), type(before)(*(getattr(before, a)[[0, 2]] for a in FIELDS)))
    assert not np.array_equal(mixed.X[1], before.X[1])
    after = c.s.RolloutPolicy(x0, trajectories=True)                                                                 # cleared: the noise-free kernel
    assert _same(after, before)
    got = np.full((B, n + c.s._md), -1.0)
    from drake_ddp_amd import _capi
    assert c.s._lib.mi_ilqr_get(c.s._h, _capi.F_POLICY_NOISE, _capi.ptr(got), got.nbytes) == _capi.OK and np.all(got == 0.0)


@pytest.mark.parametrize("name", ["pendulum", "pendulum_throughput", "arm27"])
def test_a_solve_after_a_noisy_rollout_is_the_solve_without(name):
    c = TP._ctx(name)
    p, x0b, ug, mode, _ = TP._cases()[name]()
    n, m = c.x0.shape[2], c.u_bar.shape[1]
    got = []
    for with_rollout in (True, False):
        s = TP._solver(p, max_iters=6, kernel_mode=mode)
        s.SetInitialState(x0b); s.SetInitialGuess(ug)
        TP._solve(s)
        if with_rollout:
            r = s.RolloutPolicy(c.x0[:, :65], trajectories=True, state_noise=_sigma(name, n, m)[0], control_noise=_sigma(name, n, m)[1], seed=9)
            assert np.isfinite(r.cost).any()
        s.SetInitialState(x0b)
        TP._solve(s)
        got.append([np.array(a) for a in (s.x_bar, s.u_bar, s.K, s.cost, s.iterations)])
    for a, b_ in zip(*got):
        assert np.array_equal(a, b_)


# ---------------------------------------------------------------- 4. isolation
@pytest.mark.parametrize("name", ["pendulum", "quad3d"])
def test_a_nan_x0_leaves_its_wave_neighbours_alone(name):
    c = TP._ctx(name)
    S = 65
    n, m = c.x0.shape[2], c.u_bar.shape[1]
    kw = dict(trajectories=True, state_noise=_sigma(name, n, m)[0], control_noise=_sigma(name, n, m)[1], seed=12)
    clean = np.ascontiguousarray(c.x0[:, :S])
    bad = clean.copy()
    bad[:, 30, n - 1] = np.nan
    r_ok, r_bad = c.s.RolloutPolicy(clean, **kw), c.s.RolloutPolicy(bad, **kw)
    others = [s_ for s_ in range(S) if s_ != 30]
    assert np.isfinite(r_ok.cost).all()
    assert np.all(r_bad.cost[:, 30] == np.inf) and np.all(r_bad.steps[:, 30] == 0) and np.isnan(r_bad.X[:, 30][..., 1:]).all()
    assert np.array_equal(r_bad.x_final[:, 30], bad[:, 30], equal_nan=True)
    assert _same(r_bad, r_ok, others)                                  # bitwise
    c.s.RolloutPolicy(clean[:, :1])


def test_a_huge_sigma_ends_one_problems_samples_only():
    c = TP._ctx("pendulum")
    S, N = 65, c.p["N"]
    x0 = np.ascontiguousarray(c.x0[:, :S])
    sx = np.tile(_sigma("pendulum", 2, 1)[0], (B, 1))
    mild = c.s.RolloutPolicy(x0, trajectories=True, state_noise=sx, seed=14)
    sx[1] = np.finfo(np.float64).max                                   # sigma z overflows wherever |z| > 1: the sample ends there at the latest
    r = c.s.RolloutPolicy(x0, trajectories=True, state_noise=sx, seed=14)
    z = PN.state_normals(14, 0, False, 1, *_grid(S, N), 2)             # (S, N-1, 2)
    first = np.argmax((np.abs(z) > 1.0 + 1e-9).any(axis=2), axis=1)
    assert np.all((np.abs(z) > 1.0 + 1e-9).any(axis=(1, 2))) and np.all(first < N - 2)
    assert np.all(r.cost[1] == np.inf) and np.all(r.steps[1] <= first) and np.all(r.steps[1] < N - 1)
    assert np.isfinite(r.x_final[1]).all()                             # the last state they held
    for s_ in range(S):
        t = r.steps[1, s_]
        assert np.isfinite(r.X[1, s_, :, :t + 1]).all() and np.isnan(r.X[1, s_, :, t + 1:]).all() and np.isnan(r.U[1, s_, :, t:]).all()
    assert np.isfinite(mild.cost).all()
    assert _same(type(r)(*(getattr(r, a)[[0, 2]] for a in FIELDS)), type(mild)(*(getattr(mild, a)[[0, 2]] for a in FIELDS)))
    c.s.RolloutPolicy(x0[:, :1])
