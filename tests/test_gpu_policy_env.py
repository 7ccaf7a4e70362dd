"""Envelopes and the safety box of the on-device Monte-Carlo (RolloutPolicyStats(envelope=, controls=, safe_box=); MI_F_POLICY_MC_BOX /
_OBSERVE / _ENVELOPE / _ENVELOPE_U / _SAFETY; csrc/policy_env.hpp) against the NumPy mirror (tests/policy_env_np.py) folded over the
DEVICE'S OWN trajectories: every test makes a run with samples=True, hands the samples to RolloutPolicy(trajectories=True) under the
same noise, seed and first_sample, and folds what comes back.  On the pendulum and Quad3D the two rollouts agree bit for bit
(DESIGN 4.2h), so every accumulator, every finalised field and every safety counter is compared BITWISE; the control-limited Arm27
handle is held to the same (its costs are bit for bit in tests/test_gpu_policy_mc.py, and so its trajectories were measured to be).
The merge of split calls is exact in its integer and extreme fields and within the bounds of tests/test_policy_env_oracle.py in its
moments."""
import functools
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "plugins"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _policy_env_child as CH  # noqa: E402
import policy_env_np as EN  # noqa: E402
import test_gpu_policy_mc as TM  # noqa: E402  (its handles and its mixed start distribution)
import test_gpu_policy_rollout as TP  # noqa: E402

pytestmark = pytest.mark.gpu

SEED, FIRST = TM.SEED, TM.FIRST


def _bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _raw(s, with_u=True, with_box=True):
    from drake_ddp_amd import _capi
    B = s.B
    return (CH.raw(s, _capi.F_POLICY_MC_ENVELOPE, (B, s.N, s.n, 8)),
            CH.raw(s, _capi.F_POLICY_MC_ENVELOPE_U, (B, s.N - 1, s._md, 8)) if with_u else None,
            CH.raw(s, _capi.F_POLICY_MC_SAFETY, (B, 3 + s.N)) if with_box else None)


def _check_envelope(env, raw, V, first, what):
    """env: a PolicyEnvelope; raw: the accumulators it was finalised from, cut like it; V: RolloutPolicy's X or U."""
    acc = EN.fold(EN.rows_of(V), first)
    assert _bits(raw, acc), (what, "accumulators", int((raw != acc).sum()))
    f = EN.finalise(acc)
    for k in EN.FIELDS:
        assert _bits(getattr(env, k), f[k]), (what, k)
    return f


def _check_safety(safety, raw, X, lo, hi, x_nom, goal, S, what):
    B, N = X.shape[0], X.shape[3]
    want = np.zeros((B, 3 + N), dtype=np.int64)
    for b in range(B):
        ran, safe, succ, exits = EN.box(np.transpose(X[b], (0, 2, 1)), lo[b], hi[b], x_nom, np.broadcast_to(goal, (B, X.shape[2]))[b])
        want[b, :3], want[b, 3:] = (ran, safe, succ), exits
    assert _bits(raw, want.astype(np.float64)), (what, raw, want)
    assert _bits(safety.ran, want[:, 0]) and _bits(safety.safe, want[:, 1]) and _bits(safety.safe_success, want[:, 2])
    assert _bits(safety.exits, want[:, 3:]) and np.all(safety.n == S)
    assert _bits(safety.survival, 1.0 - np.cumsum(want[:, 3:], axis=1) / float(S))
    return want


# ---------------------------------------------------------------- 1. the pendulum: both envelopes and a box
@functools.lru_cache(maxsize=None)
def _case1():
    return CH.run()


def test_pendulum_envelopes_and_box():
    o = _case1()
    s, kw, x_nom = CH.setup()
    S, N = CH.S, s.N
    X, U, lo, hi = o["X"], o["U"], o["box_lo"], o["box_hi"]
    assert X.shape == (CH.B, S, 2, N) and N * 2 == 80 and o["passes"] == 1
    # the ranges, with the mirror alone, before anything is compared
    ran, safe, succ, exits = EN.box(np.transpose(X[1], (0, 2, 1)), lo[1], hi[1], x_nom, np.array(CH.GOAL))
    cut = 1.0 - safe / S
    assert 0.1 <= cut <= 0.9 and (exits > 0).sum() >= 2, (cut, exits)
    assert np.isfinite(X).all()
    print("pendulum: the box cuts off %.0f %% of problem 1's samples, exits at %d steps" % (100 * cut, (exits > 0).sum()))

    class _R:
        pass
    env, cenv, saf = _R(), _R(), _R()
    for k in CH.ENV:
        setattr(env, k, o["env_" + k]); setattr(cenv, k, o["cenv_" + k])
    for k in ("n", "ran", "safe", "safe_success", "exits"):
        setattr(saf, k, o["safety_" + k])
    saf.survival = 1.0 - np.cumsum(saf.exits, axis=-1) / saf.n[:, None]
    f = _check_envelope(env, o["raw_x"], X, CH.FIRST, "pendulum states")
    _check_envelope(cenv, o["raw_u"], U, CH.FIRST, "pendulum controls")
    want = _check_safety(saf, o["raw_safety"], X, lo, hi, x_nom, CH.GOAL, S, "pendulum box")
    assert np.all(f["count"] == S) and np.all(f["m2"][:, 1:] > 0.0) and np.all(f["argmin"] >= CH.FIRST) and np.all(f["argmax"] < CH.FIRST + S)
    assert np.all(want[:, 0] == S) and np.all(want[:, 1] < S) and np.all(want[:, 2] <= want[:, 1])
    # a value exactly on a bound is inside: the largest angle any sample reaches IS the angle's bound, and nobody left through it
    assert np.array_equal(f["max"][:, :, 0].max(axis=1), hi[:, 0])


# ---------------------------------------------------------------- 2. the degenerate shapes
@functools.lru_cache(maxsize=None)
def _two_step_handle():
    c = TP._ctx("pendulum")
    s = TP._solver(dict(c.p, N=2))
    s.set_state(x_bar=np.ascontiguousarray(c.x_bar[:, :, :2]), u_bar=np.ascontiguousarray(c.u_bar[:, :, :1]),
                K=np.ascontiguousarray(c.K[:, :, :, :1]))
    return s, c


@pytest.mark.parametrize("S", [1, 64, 65])
def test_pendulum_two_steps(S):
    """N = 2: four state rows, one control row; S = 1, a full wave, one lane into the second tile."""
    s, c = _two_step_handle()
    kw = dict(state_noise=1e-3, control_noise=1e-2, seed=SEED, first_sample=FIRST)
    lo, hi = [-np.inf, -np.inf], c.x0b + np.array([0.0, 0.05])                       # half of the draws start above the angle's bound
    st = s.RolloutPolicyStats(S, c.x0b, [0.05, 0.1], samples=True, envelope=True, controls=True, safe_box=(lo, hi), goal=[np.inf, 0.5], **kw)
    raw_x, raw_u, raw_s = _raw(s)
    r = s.RolloutPolicy(st.samples.x0, trajectories=True, **kw)
    _check_envelope(st.envelope, raw_x, r.X, FIRST, "N=2 states S=%d" % S)
    _check_envelope(st.control_envelope, raw_u, r.U, FIRST, "N=2 controls S=%d" % S)
    _check_safety(st.safety, raw_s, r.X, np.broadcast_to(lo, (TP.B, 2)), hi, np.asarray(c.p["x_nom"], dtype=float), [np.inf, 0.5], S, "N=2 box S=%d" % S)
    assert st.envelope.count.shape == (TP.B, 2, 2) and st.control_envelope.count.shape == (TP.B, 1, 1) and st.safety.exits.shape == (TP.B, 2)


# ---------------------------------------------------------------- 3. Quad3D: a part of the samples ends early
def test_quad3d_a_part_of_the_samples_ends():
    s = TM._handle("quad3d")[0]
    mean, spread, x0, o = TM._mixed_case()
    S, n, N = x0.shape[1], x0.shape[2], s.N
    ended = ~np.isfinite(o[0][1])
    assert 0.25 <= ended.mean() <= 0.75, ended.mean()                                # the oracle's share, before anything is compared
    kw = dict(seed=SEED, first_sample=FIRST)
    box = (None, np.full(n, np.inf))
    st = s.RolloutPolicyStats(S, mean, spread, x0_dist="uniform", samples=True, envelope=True, controls=True, safe_box=box, **kw)
    raw_x, raw_u, raw_s = _raw(s)
    r = s.RolloutPolicy(st.samples.x0, trajectories=True, **kw)
    assert np.array_equal(~np.isfinite(r.cost[1]), ended)
    f = _check_envelope(st.envelope, raw_x, r.X, FIRST, "quad3d states")
    _check_envelope(st.control_envelope, raw_u[:, :, :s.m], r.U, FIRST, "quad3d controls")
    assert np.all(raw_u[:, :, s.m:, 4:6] == 0.0) or s._md == s.m                     # padding controls: exact zeros
    want = _check_safety(st.safety, raw_s, r.X, np.full((TP.B, n), -np.inf), np.full((TP.B, n), np.inf), np.asarray(TP._ctx("quad3d").p["x_nom"], dtype=float),
                         np.inf, S, "quad3d box")
    fin = np.isfinite(r.X).all(axis=(2, 3))                                          # (B, S): the samples with a finite trajectory
    assert np.array_equal(want[:, 0], fin.sum(axis=1)) and want[1, 0] == S - ended.sum() and np.array_equal(want[:, 0], want[:, 1])
    # count falls below S exactly where the samples have ended: per step the samples that still hold a state
    alive = np.isfinite(r.X).all(axis=2).sum(axis=1)                                 # (B, N)
    assert np.array_equal(st.envelope.count, np.broadcast_to(alive[:, :, None], (TP.B, N, n)))
    assert np.all(st.envelope.count[1, 0] == S) and np.all(st.envelope.count[1, -1] == S - ended.sum()) and np.all(st.envelope.count[[0, 2]] == S)
    # the survivors' moments, against a plain NumPy mean over them
    t = N - 1
    surv = np.isfinite(r.X[1, :, :, t]).all(axis=1)
    ref = r.X[1, surv, :, t].mean(axis=0)
    assert np.all(np.abs(f["mean"][1, t] - ref) <= 1e-12 * np.abs(r.X[1, surv, :, t]).max(axis=0) + 1e-300)


# ---------------------------------------------------------------- 4. the control envelope: padding and limits
@functools.lru_cache(maxsize=None)
def _short(name, limited=False):
    """B = 2, N = 6: a handle with a policy on it (three iterations), control-limited on request (half of what the plan asks for)."""
    from drake_ddp_amd import workloads as W
    p = {"quad3d": W.quad3d_problem, "arm27": W.arm27_problem}[name](6)
    x0b = {"quad3d": W.quad3d_batch_x0, "arm27": W.arm27_batch_x0}[name](2)
    ug = {"quad3d": W.quad3d_u_guess, "arm27": W.arm27_u_guess}[name](6)
    s = TP._solver(p, batch=2, max_iters=3)
    s.SetInitialState(x0b); s.SetInitialGuess(ug)
    TP._solve(s)
    if not limited:
        return s, x0b, None
    x_bar, u_bar, K = np.array(s.x_bar), np.array(s.u_bar), np.array(s.K)
    sl = TP._solver(p, batch=2, control_limits="enforce")
    lim = 0.5 * np.abs(u_bar).max(axis=2) + 1e-3
    sl.SetControlLimits(-lim, lim)
    sl.set_state(x_bar=x_bar, u_bar=u_bar, K=K)
    return sl, x0b, lim


def test_quad3d_control_envelope_is_cut_to_the_users_controls():
    s, x0b, _ = _short("quad3d")
    S = 70
    kw = dict(state_noise=1e-4, control_noise=1e-3, seed=SEED, first_sample=FIRST)
    st = s.RolloutPolicyStats(S, x0b, 1e-3 * np.ones(s.n), samples=True, envelope=True, controls=True, **kw)
    raw_x, raw_u, _ = _raw(s, with_box=False)
    r = s.RolloutPolicy(st.samples.x0, trajectories=True, **kw)
    assert s._md == 12 and s.n >= 33 and st.safety is None
    assert st.control_envelope.count.shape == (2, 5, s.m) and r.U.shape == (2, S, s.m, 5) and raw_u.shape == (2, 5, 12, 8)
    _check_envelope(st.envelope, raw_x, r.X, FIRST, "short quad3d states")
    _check_envelope(st.control_envelope, raw_u[:, :, :s.m], r.U, FIRST, "short quad3d controls")
    if s._md > s.m:                                                                  # the padding controls: S exact zeros per row
        pad = raw_u[:, :, s.m:]
        assert np.all(pad[..., 0] == S) and np.all(pad[..., 1:6] == 0.0) and np.all(pad[..., 6:] == FIRST)


def test_arm27_limited_control_envelope_respects_the_limits():
    from drake_ddp_amd import _capi
    s, x0b, lim = _short("arm27", limited=True)
    S = 70
    kw = dict(seed=SEED, first_sample=FIRST)
    st = s.RolloutPolicyStats(S, x0b, 1e-3 * np.ones(s.n), samples=True, controls=True, **kw)
    raw_u = CH.raw(s, _capi.F_POLICY_MC_ENVELOPE_U, (s.B, s.N - 1, s._md, 8))
    r = s.RolloutPolicy(st.samples.x0, trajectories=True, **kw)
    assert st.envelope is None and st.safety is None
    f = _check_envelope(st.control_envelope, raw_u[:, :, :s.m], r.U, FIRST, "limited arm27 controls")
    u_max = np.broadcast_to(lim[:, None, :], f["max"].shape)
    assert np.all(st.control_envelope.max <= u_max) and np.all(st.control_envelope.min >= -u_max)
    sat = f["max"] == u_max                                                          # where the mirror saturates, so does the device
    assert sat.any() and np.array_equal(st.control_envelope.max == u_max, sat)


# ---------------------------------------------------------------- 5. window independence
def test_the_result_does_not_depend_on_the_window():
    here = dict(_case1())                                                            # this process: the default window, one pass
    assert here.pop("passes") == 1
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "one_group_per_pass.npz")
        env = dict(os.environ, MI_ILQR_MC_PASS_GROUPS="1")                            # three passes, the accumulators carried between them
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_policy_env_child.py"), out], env=env, timeout=300,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        there = dict(np.load(out))
    assert int(there.pop("passes")) == 3
    assert set(here) == set(there)
    for k in here:
        assert _bits(here[k], there[k]), k


# ---------------------------------------------------------------- 6. split calls and merge
def test_merge_of_two_calls_is_one_call():
    o = _case1()
    s, kw, x_nom = CH.setup()
    box = (o["box_lo"], o["box_hi"])
    more = dict(envelope=True, controls=True, safe_box=box)
    a = CH.stats(s, kw, 64, CH.FIRST, **more)
    b = CH.stats(s, kw, 66, CH.FIRST + 64, **more)
    m = a.merge(b)
    for k in CH.TEN:
        if k not in ("mean", "m2"):
            assert np.array_equal(getattr(m, k), o["obs_" + k]), k
    for k in ("n", "ran", "safe", "safe_success", "exits"):
        assert _bits(getattr(m.safety, k), o["safety_" + k]), k
    worst = [0.0, 0.0]
    for tag, got, V in (("env_", m.envelope, o["X"]), ("cenv_", m.control_envelope, o["U"])):
        for k in ("count", "min", "max", "argmin", "argmax"):
            assert _bits(getattr(got, k), o[tag + k]), (tag, k)
        rows = EN.rows_of(V)
        for idx in np.ndindex(rows.shape[:3]):
            b_mean, b_m2 = EN.moment_bounds(rows[idx])
            e_mean, e_m2 = abs(got.mean[idx] - o[tag + "mean"][idx]), abs(got.m2[idx] - o[tag + "m2"][idx])
            if b_mean > 0:
                worst[0] = max(worst[0], e_mean / b_mean)
            if b_m2 > 0:
                worst[1] = max(worst[1], e_m2 / b_m2)
            assert e_mean <= b_mean and e_m2 <= b_m2, (tag, idx, e_mean, b_mean, e_m2, b_m2)
    print("merge of split calls: worst |merged - one call| / bound: mean %.3f, M2 %.3f" % tuple(worst))


# ---------------------------------------------------------------- 7. off means off
def test_off_means_off():
    o = _case1()
    s, kw, _ = CH.setup()
    for k in CH.TEN + ("x0", "params", "cost", "steps"):                             # the observing call: the plain call's numbers, bitwise
        assert _bits(o["obs_" + k], o["plain_" + k]), k
    again = CH.stats(s, kw, samples=True)                                            # a plain call AFTER observing ones: what it was before any
    assert again.envelope is None and again.control_envelope is None and again.safety is None and s.policy_mc_passes() == 1
    for k in CH.TEN:
        assert _bits(getattr(again, k), o["plain_" + k]), k
    for k in ("x0", "params", "cost", "steps"):
        assert _bits(getattr(again.samples, k), o["plain_" + k]), k
    from drake_ddp_amd import _capi
    one, rows = np.empty(1), np.empty((CH.B, 8, 10))
    assert s._lib.mi_ilqr_get(s._h, _capi.F_POLICY_MC_OBSERVE, _capi.ptr(one), 8) == _capi.OK and one[0] == 0.0    # the settings are back
    for which in (_capi.F_POLICY_MC_ENVELOPE, _capi.F_POLICY_MC_ENVELOPE_U, _capi.F_POLICY_MC_SAFETY):             # ... and that run produced none
        assert s._lib.mi_ilqr_get(s._h, which, _capi.ptr(rows), 8) == _capi.E_BAD_ARG


def test_a_solve_after_an_observing_run_is_the_solve_without():
    p, x0b, ug, mode, sigma = TP._cases()["pendulum"]()
    got = []
    for with_run in (True, False):
        s = TP._solver(p, max_iters=6, kernel_mode=mode)
        s.SetInitialState(x0b); s.SetInitialGuess(ug)
        TP._solve(s)
        if with_run:
            st = s.RolloutPolicyStats(130, x0b, sigma * np.ones(2), state_noise=1e-4, seed=SEED, envelope=True, controls=True,
                                      safe_box=([-10.0, -10.0], [10.0, 10.0]))
            assert np.all(st.counted > 0) and np.all(st.envelope.count > 0)
        s.SetInitialState(x0b)
        TP._solve(s)
        got.append([np.array(a) for a in (s.x_bar, s.u_bar, s.K, s.cost, s.iterations)])
    for a, b_ in zip(*got):
        assert np.array_equal(a, b_)


# ---------------------------------------------------------------- 8. refusals through the C ABI
def test_the_c_abi_refuses_and_keeps_what_it_had():
    from drake_ddp_amd import _capi
    c = TP._ctx("pendulum")
    s = TP._solver(c.p)
    s.set_state(x_bar=c.x_bar, u_bar=c.u_bar, K=c.K)
    s._push_costs()
    lib, h, B, n, N = s._lib, s._h, TP.B, 2, s.N
    st_ = lambda which, a, nbytes=None: lib.mi_ilqr_set(h, which, _capi.ptr(a), (0 if a is None else a.nbytes) if nbytes is None else nbytes)   # noqa: E731
    gt_ = lambda which, a, nbytes=None: lib.mi_ilqr_get(h, which, _capi.ptr(a), a.nbytes if nbytes is None else nbytes)   # noqa: E731
    run = lambda *v: st_(_capi.F_POLICY_MC_RUN, np.array(v, dtype=np.float64))   # noqa: E731
    obs = lambda v: st_(_capi.F_POLICY_MC_OBSERVE, np.array([v], dtype=np.float64))   # noqa: E731
    env, envu, saf = np.empty((B, N, n, 8)), np.empty((B, N - 1, 1, 8)), np.empty((B, 3 + N))
    rows = np.zeros((B, 12))
    rows[:, :n] = c.x0b; rows[:, n:2 * n] = 0.05; rows[:, 2 * n:3 * n] = np.inf; rows[:, 6:9] = c.base
    assert st_(_capi.F_POLICY_MC_DIST, rows) == _capi.OK
    box = np.hstack([c.x0b - 0.5, c.x0b + 0.5])
    # before any run: nothing to read; the settings read back
    for which, a in ((_capi.F_POLICY_MC_ENVELOPE, env), (_capi.F_POLICY_MC_ENVELOPE_U, envu), (_capi.F_POLICY_MC_SAFETY, saf)):
        assert gt_(which, a) == _capi.E_BAD_ARG
    assert obs(3.0) == _capi.OK and st_(_capi.F_POLICY_MC_BOX, box) == _capi.OK
    back, one = np.empty_like(box), np.empty(1)

    def unchanged(results=None):
        assert gt_(_capi.F_POLICY_MC_BOX, back) == _capi.OK and np.array_equal(back, box)
        assert gt_(_capi.F_POLICY_MC_OBSERVE, one) == _capi.OK and one[0] == 3.0
        if results is not None:
            e, u, f = np.empty_like(env), np.empty_like(envu), np.empty_like(saf)
            assert gt_(_capi.F_POLICY_MC_ENVELOPE, e) == gt_(_capi.F_POLICY_MC_ENVELOPE_U, u) == gt_(_capi.F_POLICY_MC_SAFETY, f) == _capi.OK
            assert _bits(e, results[0]) and _bits(u, results[1]) and _bits(f, results[2])
    unchanged()
    assert run(70, 0, 0, 0, 0) == _capi.OK
    assert gt_(_capi.F_POLICY_MC_ENVELOPE, env) == gt_(_capi.F_POLICY_MC_ENVELOPE_U, envu) == gt_(_capi.F_POLICY_MC_SAFETY, saf) == _capi.OK
    assert np.all(env[..., 0] == 70) and np.all(saf[:, 0] == 70)
    res = (env.copy(), envu.copy(), saf.copy())
    # wrong sizes
    assert st_(_capi.F_POLICY_MC_BOX, box, box.nbytes - 8) == _capi.E_BAD_SHAPE and st_(_capi.F_POLICY_MC_BOX, None, box.nbytes) == _capi.E_BAD_ARG
    assert st_(_capi.F_POLICY_MC_OBSERVE, one, 16) == _capi.E_BAD_SHAPE and gt_(_capi.F_POLICY_MC_OBSERVE, one, 4) == _capi.E_BAD_SHAPE
    assert gt_(_capi.F_POLICY_MC_BOX, back, 8) == _capi.E_BAD_SHAPE
    for which, a in ((_capi.F_POLICY_MC_ENVELOPE, env), (_capi.F_POLICY_MC_ENVELOPE_U, envu), (_capi.F_POLICY_MC_SAFETY, saf)):
        assert gt_(which, a, a.nbytes - 8) == _capi.E_BAD_SHAPE
        assert st_(which, a) == _capi.E_BAD_ARG                                      # read-only
    unchanged(res)
    # a NaN, an inverted box, observe values that are none
    for i, j, v in ((1, 0, np.nan), (1, n, np.nan), (2, 1, np.inf), (0, n + 1, -np.inf), (1, 0, c.x0b[1, 0] + 0.6)):
        bad = box.copy()
        bad[i, j] = v
        assert st_(_capi.F_POLICY_MC_BOX, bad) == _capi.E_BAD_ARG, (i, j, v)
    for v in (4.0, -1.0, 0.5, np.nan, np.inf):
        assert obs(v) == _capi.E_BAD_ARG, v
    unchanged(res)
    assert run(0, 0, 0, 0, 0) == _capi.E_BAD_ARG                                     # a refused run keeps the last results too
    unchanged(res)
    # a run that observes less: what it does not produce is refused, what it does is replaced
    assert obs(1.0) == _capi.OK and st_(_capi.F_POLICY_MC_BOX, None) == _capi.OK and run(5, 0, 0, 0, 0) == _capi.OK
    assert gt_(_capi.F_POLICY_MC_ENVELOPE, env) == _capi.OK and np.all(env[..., 0] == 5)
    assert gt_(_capi.F_POLICY_MC_ENVELOPE_U, envu) == _capi.E_BAD_ARG and gt_(_capi.F_POLICY_MC_SAFETY, saf) == _capi.E_BAD_ARG
    assert obs(0.0) == _capi.OK and run(5, 0, 0, 0, 0) == _capi.OK
    assert gt_(_capi.F_POLICY_MC_ENVELOPE, env) == _capi.E_BAD_ARG
    zero = np.empty_like(box)
    assert gt_(_capi.F_POLICY_MC_BOX, zero) == _capi.OK and np.all(zero == 0.0)       # no box: zeros
    # the box and the bits survive a reset
    assert obs(2.0) == _capi.OK and st_(_capi.F_POLICY_MC_BOX, box) == _capi.OK and lib.mi_ilqr_reset(h) == _capi.OK
    assert gt_(_capi.F_POLICY_MC_BOX, back) == _capi.OK and np.array_equal(back, box) and gt_(_capi.F_POLICY_MC_OBSERVE, one) == _capi.OK and one[0] == 2.0


def test_python_refuses_before_anything_is_sent():
    s, kw, _ = CH.setup()
    before = CH.stats(s, kw)
    for more in (dict(envelope=1), dict(controls="yes"), dict(safe_box=([0.0, 0.0],)), dict(safe_box=([1.0, 0.0], [0.0, 0.0])),
                 dict(safe_box=([np.nan, 0.0], None)), dict(safe_box=(np.zeros(3), None))):
        with pytest.raises(ValueError, match="RolloutPolicyStats"):
            CH.stats(s, kw, **more)
    after = CH.stats(s, kw)
    assert all(_bits(getattr(after, k), getattr(before, k)) for k in CH.TEN)


# ---------------------------------------------------------------- 9. the example
def test_the_example():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "policy_envelope_pendulum.py")], timeout=300,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert len(re.findall(r"^step\s+\d+: half-width", r.stdout, re.M)) >= 3, r.stdout
    m = re.search(r"inside the box: ([0-9.]+) %", r.stdout)
    assert m and 0.0 <= float(m.group(1)) <= 100.0, r.stdout
