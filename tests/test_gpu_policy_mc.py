"""Monte-Carlo on the device (BatchedIterativeLQR.RolloutPolicyStats; MI_F_POLICY_MC_DIST / _RUN / _STATS / _SAMPLES; csrc/policy_mc.hpp)
against the NumPy statement of the same thing (tests/policy_mc_np.py) and against RolloutPolicy: the draws through the noise probe,
the rollouts of the drawn samples bit for bit those of RolloutPolicy on every kernel family's handle, the ten numbers against
NumPy and the mirror of the device's reduction order, the goal test, ended samples, the window passes, the handle left as it was,
the refusals of the C ABI, and the example.

Tolerance of mean and M2 (the exact fields - S, counted, success, steps_total, min, max, argmin, argmax - are compared exactly).
The device and the mirror oracle (policy_mc_np.mirror_moments) run the SAME merges in the SAME order on the same per-sample costs,
each merge being  n = nA + nB, delta = mB - mA, w = nB / n, q = (nA nB) / n, mean = mA + delta w, M2 = (M2A + M2B) + (delta delta) q:
at most eight roundings, and the only licensed difference is contraction (the compiler may fuse a multiply into the add behind it,
which removes one of them).  A sample's cost passes through the 6 merges of its group's butterfly and at most G folds, G the groups
of the problem.  With every intermediate mean bounded by max|c| and every rounding relative eps of a quantity bounded by the final
one, the two evaluations differ by at most
    |mean - mean'| <= 8 eps (6 + G) max_s |c_s|
    |M2 - M2'|     <= 8 eps (6 + G) (sum_s (c_s - mean)^2 + S max_s |c_s| |mean|)
(the second term of the M2 bound: an error of the means, up to the first bound, enters M2 through delta^2 q <= S |delta| max|c|).
tests/test_policy_mc_oracle.py checks the same bound against a two-pass extended-precision reduction.  Every comparison prints the
worst ratio it saw."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "plugins"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import policy_mc_np as MC  # noqa: E402
import policy_noise_np as PN  # noqa: E402
import test_gpu_policy_rollout as TP  # noqa: E402  (its cached handles with a policy on them)

pytestmark = pytest.mark.gpu

B = TP.B
SEED = PN.TEST_SEED
FIRST = 5                                  # first_sample of the rollout tests: sample numbers are not sample indices
S_VALUES = (1, 64, 65, 130)                # one lane, a full wave, one lane into the second wave, three waves with a ragged tail
FIELDS = MC.FIELDS
WORST = {"mean": 0.0, "m2": 0.0}


def _ten(st):
    return np.stack([np.asarray(getattr(st, k), dtype=np.float64) for k in FIELDS], axis=1)


def _same_ten(a, b):
    return np.array_equal(_ten(a), _ten(b), equal_nan=True)


# ---------------------------------------------------------------- 1. the draws
PROBE_N = 40


@functools.lru_cache(maxsize=None)
def _probe():
    import test_gpu_policy_noise as TN
    return TN._probe(2)[2]                 # B = 2, N = 2, cold: ten x0 blocks


def _probe_rows():
    rng = np.random.default_rng(31)
    mean = rng.standard_normal((2, PROBE_N)) * 10.0 ** rng.integers(-3, 4, (2, PROBE_N))
    spread = rng.uniform(0.1, 2.0, (2, PROBE_N)) * 10.0 ** rng.integers(-2, 2, (2, PROBE_N))     # per component and per problem
    spread[:, 5] = 0.0
    spread[1, 17] = 0.0
    mean[0, 5] = -0.0
    return mean, spread


def _draw_tol(dist, mean, spread):
    """What a drawn x0 may differ from the oracle's by: normal - NORMAL_TOL spread + 2 ulp(|mean| + 6.77 spread); uniform - the
    oracle's d is exact, only the final multiply-add may round differently: 2 ulp(|mean| + spread)."""
    if dist == "normal":
        return PN.NORMAL_TOL * spread + 2.0 * np.spacing(np.abs(mean) + 6.77 * spread)
    return 2.0 * np.spacing(np.abs(mean) + spread)


@pytest.mark.parametrize("dist", ["normal", "uniform"])
def test_the_draws(dist):
    s, S = _probe(), 130
    mean, spread = _probe_rows()
    st = s.RolloutPolicyStats(S, mean, spread, x0_dist=dist, seed=SEED, samples=True)
    x0 = st.samples.x0
    assert x0.shape == (2, S, PROBE_N) and st.samples.params is None and np.all(st.n == S) and np.all(st.counted == S)
    worst = 0.0
    for b in range(2):
        ref = MC.draw_x0(dist, mean[b], spread[b], SEED, 0, False, b, np.arange(S))
        tol = _draw_tol(dist, mean[b], spread[b])
        if dist == "uniform":
            assert np.all(np.abs(x0[b] - mean[b]) <= spread[b])
        err = np.abs(x0[b] - ref)
        assert np.all(err <= tol[None, :]), (b, float(np.max(err / tol[None, :])))
        worst = max(worst, float(np.max(err / tol[None, :])))
        zero = spread[b] == 0.0
        assert np.array_equal(x0[b][:, zero], np.broadcast_to(mean[b][zero], (S, int(zero.sum()))))       # spread 0: the mean's bits
    assert np.all(np.signbit(x0[0, :, 5]))                                                                   # ... -0.0 included
    print("draws %s: worst |device - oracle| / tolerance %.3f" % (dist, worst))
    # the same seed twice; another seed; a seed that differs in the key's high word only
    again = s.RolloutPolicyStats(S, mean, spread, x0_dist=dist, seed=SEED, samples=True)
    assert np.array_equal(again.samples.x0, x0) and _same_ten(again, st)
    moving = spread != 0.0
    for other in (SEED + 1, SEED + 2 ** 32):
        o = s.RolloutPolicyStats(S, mean, spread, x0_dist=dist, seed=other, samples=True)
        assert np.all((o.samples.x0 != x0)[:, :, moving[0] & moving[1]])
    # common random numbers: with the same rows both problems draw the same states; without, different ones
    com = s.RolloutPolicyStats(S, mean[0], spread[0], x0_dist=dist, seed=SEED, common_noise=True, samples=True)
    assert np.array_equal(com.samples.x0[0], com.samples.x0[1]) and np.array_equal(com.samples.x0[0], x0[0])
    own = s.RolloutPolicyStats(S, mean[0], spread[0], x0_dist=dist, seed=SEED, samples=True)
    assert not np.array_equal(own.samples.x0[0], own.samples.x0[1]) and np.array_equal(own.samples.x0[0], x0[0])
    # a later window of the same sample set: S = 66 from first_sample = 64 is samples 64 .. 129, bitwise
    win = s.RolloutPolicyStats(66, mean, spread, x0_dist=dist, seed=SEED, first_sample=64, samples=True)
    assert np.array_equal(win.samples.x0, x0[:, 64:]) and np.array_equal(win.samples.cost, st.samples.cost[:, 64:])
    assert np.array_equal(win.samples.steps, st.samples.steps[:, 64:])
    # the last sample numbers there are
    top = s.RolloutPolicyStats(3, mean, spread, x0_dist=dist, seed=SEED, first_sample=2 ** 32 - 3, samples=True)
    for b in range(2):
        ref = MC.draw_x0(dist, mean[b], spread[b], SEED, 2 ** 32 - 3, False, b, np.arange(3))
        assert np.all(np.abs(top.samples.x0[b] - ref) <= _draw_tol(dist, mean[b], spread[b])[None, :]), b
    assert np.all(top.argmin >= 2 ** 32 - 3) and np.all(top.argmax <= 2 ** 32 - 1)


# ---------------------------------------------------------------- 2. the rollouts are RolloutPolicy's
HANDLES = ["pendulum", "acrobot_lane", "arm27_limited", "quad3d"]


@functools.lru_cache(maxsize=None)
def _handle(name):
    """-> (solver with a policy on it, x0 means (B, n), x0 spread, parameter means or None, N)"""
    if name == "acrobot_lane":                                   # the lane-per-problem kernels' policy layout
        p, x0b, ug, _, sigma = TP._cases()["acrobot"]()
        s = TP._solver(p, max_iters=3, kernel_mode="throughput")
        s.SetInitialState(x0b); s.SetInitialGuess(ug)
        TP._solve(s)
        return s, x0b, sigma, None, p["N"]
    if name == "arm27_limited":                                  # a control-limited handle: the clamp is active
        c = TP._ctx("arm27")
        s = TP._solver(c.p, control_limits="enforce")
        lim = 0.5 * np.abs(c.u_bar).max(axis=2) + 1e-3           # (B, m): half of what each control's plan asks for
        s.SetControlLimits(-lim, lim)
        s.set_state(x_bar=c.x_bar, u_bar=c.u_bar, K=c.K)
        return s, c.x0b, 1e-3, None, c.p["N"]
    c = TP._ctx(name)
    sigma = TP._cases()[name]()[4]
    return c.s, c.x0b, sigma, c.base[0], c.p["N"]               # (pendulum, quad3d: the parameters are sampled too)


def _noise(noisy):
    return dict(state_noise=1e-4, control_noise=1e-3) if noisy else {}


@functools.lru_cache(maxsize=None)
def _run(name, S, noisy):
    """One on-device Monte-Carlo with the samples, and RolloutPolicy fed with those samples under the same stream."""
    s, mean, sigma, base, N = _handle(name)
    kw = dict(seed=SEED, first_sample=FIRST, **_noise(noisy))
    prm = {} if base is None else dict(params_mean=base, params_spread=0.05 * np.abs(base))
    st = s.RolloutPolicyStats(S, mean, sigma * np.ones(mean.shape[1]), samples=True, **prm, **kw)
    r = s.RolloutPolicy(st.samples.x0, st.samples.params, **kw)
    return st, r


@pytest.mark.parametrize("noisy", [False, True], ids=["noise_off", "noise_on"])
@pytest.mark.parametrize("name", HANDLES)
def test_the_rollouts_are_rollout_policys(name, noisy):
    """cost and steps of every drawn sample, bit for bit: policy_mc.hpp repeats policy_rollout_kernel's loop and hands it the drawn
    state the way a loaded one arrives (without that, Quad3D costs differed in the last bits - 9 of 192 at S = 64 by up
    to 8.57e-16 relative - because a * b + c * d was contracted around the other product)."""
    for S in S_VALUES:
        st, r = _run(name, S, noisy)
        assert st.samples.cost.shape == (B, S) and st.samples.steps.dtype == np.int32
        assert np.array_equal(st.samples.steps, r.steps), (name, S)
        same = st.samples.cost == r.cost
        assert same.all(), (name, S, int((~same).sum()), float(np.max(np.abs(st.samples.cost[~same] - r.cost[~same]) / np.abs(r.cost[~same]))))
        if _handle(name)[3] is not None:
            base = _handle(name)[3]
            assert np.all(np.abs(st.samples.params - base) <= 0.05 * np.abs(base)) and st.samples.params.std() > 0.0


FURTHER = ["planar_quad", "synth36", "cartpole_wall", "acrobot", "pendulum_throughput"]


@pytest.mark.parametrize("name", FURTHER)
def test_further_models_roll_out_as_rollout_policy_does(name):
    """The same comparison on the models the list above leaves out - PlanarQuad (the other model that can fail), Synth36, the cart-pole
    with its wall, the acrobot on its wave-per-problem handle, the pendulum on a lane-per-problem one - with sampled parameters,
    noise off and on, S = 65 and 130: bit for bit on the MI355X this was measured on.  The interface promises the same arithmetic up
    to FMA contraction (include/mi_ilqr.h); this test holds the BUILD to what it was measured to give, so that a compiler or a
    kernel change that breaks it shows."""
    for noisy in (False, True):
        for S in (65, 130):
            st, r = _run(name, S, noisy)
            assert np.array_equal(st.samples.steps, r.steps), (name, S, noisy)
            same = st.samples.cost == r.cost
            assert same.all(), (name, S, noisy, int((~same).sum()))


# ---------------------------------------------------------------- 3. the statistics
def _check_stats(st, cost, steps, N, first, success=None, what=""):
    """The ten numbers of every problem against NumPy on the returned per-sample results: module docstring."""
    for b in range(cost.shape[0]):
        want = MC.stats(cost[b], steps[b], N, first_sample=first, success=None if success is None else success[b])
        for k in ("n", "counted", "success", "steps_total", "min", "max", "argmin", "argmax"):
            assert getattr(st, k)[b] == want[k], (what, b, k, getattr(st, k)[b], want[k])
        if want["counted"] == 0:
            assert np.isnan(st.mean[b]) and np.isnan(st.m2[b])
            continue
        counted = (steps[b] == N - 1) & np.isfinite(cost[b])
        b_mean, b_m2 = MC.moment_bounds(cost[b], counted, want["mean"])
        e_mean, e_m2 = abs(st.mean[b] - want["mean"]), abs(st.m2[b] - want["m2"])
        assert e_mean <= b_mean and e_m2 <= b_m2, (what, b, e_mean, b_mean, e_m2, b_m2)
        WORST["mean"] = max(WORST["mean"], e_mean / b_mean)
        WORST["m2"] = max(WORST["m2"], e_m2 / b_m2 if b_m2 else 0.0)


@pytest.mark.parametrize("name", HANDLES)
def test_the_statistics(name):
    s, mean, sigma, base, N = _handle(name)
    for S in S_VALUES:
        for noisy in (False, True):
            st, _ = _run(name, S, noisy)
            _check_stats(st, st.samples.cost, st.samples.steps, N, FIRST, what="%s S=%d" % (name, S))
            assert np.all(st.success == st.counted) and np.all(st.n == S)                      # the default goal: all +inf
            if S > 1:
                assert np.all(st.var > 0.0) and np.all(st.min < st.mean) and np.all(st.mean < st.max)
    # samples=False: the same ten numbers, bitwise
    st, _ = _run(name, 130, True)
    prm = {} if base is None else dict(params_mean=base, params_spread=0.05 * np.abs(base))
    lean = s.RolloutPolicyStats(130, mean, sigma * np.ones(mean.shape[1]), seed=SEED, first_sample=FIRST, **prm, **_noise(True))
    assert lean.samples is None and _same_ten(lean, st)
    # a constructed tie: spread 0, every sample the same - argmin = argmax = first_sample, M2 exactly zero
    tie = s.RolloutPolicyStats(130, mean, 0.0 * mean, seed=SEED, first_sample=FIRST, samples=True)
    assert np.all(tie.samples.cost == tie.samples.cost[:, :1]) and np.array_equal(tie.samples.x0, np.broadcast_to(mean[:, None, :], (B, 130, mean.shape[1])))
    assert np.all(tie.argmin == FIRST) and np.all(tie.argmax == FIRST) and np.all(tie.m2 == 0.0)
    assert np.array_equal(tie.mean, tie.samples.cost[:, 0]) and np.array_equal(tie.min, tie.max)
    print("statistics %s: worst |device - mirror| / bound: mean %.3f, M2 %.3f" % (name, WORST["mean"], WORST["m2"]))


def test_merge_of_two_calls_is_one_call():
    """PolicyStats.merge of the windows [FIRST, FIRST + 64) and [FIRST + 64, FIRST + 130) against the one call: the fold of whole
    groups in the same order - bitwise."""
    s, mean, sigma, base, N = _handle("pendulum")
    one, _ = _run("pendulum", 130, True)
    kw = dict(params_mean=base, params_spread=0.05 * np.abs(base), seed=SEED, **_noise(True))
    a = s.RolloutPolicyStats(64, mean, sigma * np.ones(2), first_sample=FIRST, **kw)
    b_ = s.RolloutPolicyStats(66, mean, sigma * np.ones(2), first_sample=FIRST + 64, **kw)
    m = a.merge(b_)
    for k in ("n", "counted", "success", "steps_total", "min", "max", "argmin", "argmax"):
        assert np.array_equal(getattr(m, k), getattr(one, k)), k
    for b in range(B):
        counted = np.isfinite(one.samples.cost[b])
        b_mean, b_m2 = MC.moment_bounds(one.samples.cost[b], counted, one.mean[b])
        assert abs(m.mean[b] - one.mean[b]) <= b_mean and abs(m.m2[b] - one.m2[b]) <= b_m2


# ---------------------------------------------------------------- 4. the goal
@pytest.mark.parametrize("name", ["pendulum", "quad3d"])
def test_the_goal(name):
    s, mean, sigma, base, N = _handle(name)
    S = 130
    st, r = _run(name, S, True)
    x_nom = TP._ctx(name).p["x_nom"]
    n = mean.shape[1]
    dev = np.abs(r.x_final - x_nom[None, None, :])                                  # RolloutPolicy's final states of the same samples
    comp, prob = 1, 1
    d = np.sort(dev[prob, :, comp])
    g = 0.5 * (d[S // 2 - 1] + d[S // 2])                                           # between two samples: half of them inside, none on the edge
    assert d[S // 2 - 1] < g < d[S // 2]
    goal = np.full((B, n), np.inf)
    goal[prob, comp] = g
    kw = dict(params_mean=base, params_spread=0.05 * np.abs(base), seed=SEED, first_sample=FIRST, **_noise(True))
    got = s.RolloutPolicyStats(S, mean, sigma * np.ones(n), goal=goal, **kw)
    want = (np.isfinite(r.cost) & (dev <= goal[:, None, :]).all(axis=2)).sum(axis=1)
    assert np.array_equal(got.success, want) and 0 < want[prob] < st.counted[prob] and np.array_equal(np.delete(want, prob), np.delete(st.counted, prob))
    assert np.array_equal(got.success_rate, want / S)
    assert np.array_equal(_ten(got)[:, [0, 1, 3, 4, 5, 6, 7, 8, 9]], _ten(st)[:, [0, 1, 3, 4, 5, 6, 7, 8, 9]])         # nothing else moves
    zero = s.RolloutPolicyStats(S, mean, sigma * np.ones(n), goal=np.zeros(n), **kw)
    assert np.all(zero.success == 0) and np.array_equal(zero.counted, st.counted)
    inf = s.RolloutPolicyStats(S, mean, sigma * np.ones(n), goal=np.full(n, np.inf), **kw)
    assert np.array_equal(inf.success, inf.counted) and _same_ten(inf, st)


# ---------------------------------------------------------------- 5. ended samples
def test_a_problem_whose_samples_all_end():
    from oracle import models_np as M
    c = TP._ctx("quad3d")
    s, mean, sigma, base, N = _handle("quad3d")
    n, S = mean.shape[1], 130
    vmax = M.DEFAULT_PARAMS[M.QUAD3D][6]
    bad = mean.copy()
    bad[1, n - 1] = 2.0 * vmax                                   # test_failing_samples_do_not_leak's x0: no step brings it back
    spread = sigma * np.ones((B, n))
    spread[1] = 0.0
    kw = dict(seed=SEED, first_sample=FIRST, **_noise(True))
    st = s.RolloutPolicyStats(S, bad, spread, samples=True, **kw)
    r = s.RolloutPolicy(st.samples.x0, **kw)
    assert np.all(r.cost[1] == np.inf) and np.all(st.samples.cost[1] == np.inf) and np.array_equal(st.samples.steps, r.steps)
    assert st.n[1] == S and st.counted[1] == 0 and st.success[1] == 0 and np.isnan(st.mean[1]) and np.isnan(st.m2[1])
    assert st.min[1] == np.inf and st.max[1] == -np.inf and st.argmin[1] == -1 and st.argmax[1] == -1
    assert st.steps_total[1] == int(r.steps[1].sum()) and np.isnan(st.var[1]) and st.success_rate[1] == 0.0
    _check_stats(st, st.samples.cost, st.samples.steps, N, FIRST, what="all of problem 1 end")
    ok_spread = spread.copy()
    ok_spread[1] = sigma
    ok = s.RolloutPolicyStats(S, mean, ok_spread, **kw)                              # problem 1 benign
    assert ok.counted[1] == S
    assert np.array_equal(_ten(st)[[0, 2]], _ten(ok)[[0, 2]])                         # problems 0 and 2: bitwise what they were


@functools.lru_cache(maxsize=None)
def _mixed_case():
    """A start distribution chosen with the ORACLE alone, on the CPU: problem 1's last joint rate uniform in (0, 2 k v_max), the
    first k of a short list for which between a quarter and three quarters of its samples end early (a rate far above v_max ends
    a sample at its first step, a small one never does: the share falls with k).  The other problems start at their own x0."""
    from oracle import models_np as M
    from policy_rollout_np import rollout
    c = TP._ctx("quad3d")
    p = c.p
    n, S = c.x0b.shape[1], 130
    vmax = M.DEFAULT_PARAMS[M.QUAD3D][6]
    args = (c.x_bar, c.u_bar, c.K, p["Q"], p["R"], p["Qf"], p["x_nom"])
    for k in (1.0, 0.75, 1.5, 0.5, 2.0, 0.35, 3.0):
        mean, spread = c.x0b.copy(), np.zeros((B, n))
        mean[1, n - 1] = spread[1, n - 1] = k * vmax
        x1 = MC.draw_x0("uniform", mean[1], spread[1], SEED, FIRST, False, 1, np.arange(S))
        o1 = rollout(c.make_model, x1[None], c.base[1:2], *(a[1:2] for a in args[:3]), *args[3:])
        if 0.25 <= (~np.isfinite(o1[0][0])).mean() <= 0.75:
            break
    x0 = np.stack([MC.draw_x0("uniform", mean[b], spread[b], SEED, FIRST, False, b, np.arange(S)) for b in range(B)])
    o = rollout(c.make_model, x0, c.base, *args)
    return mean, spread, x0, o


def test_a_problem_of_which_a_part_ends():
    s, _, _, _, N = _handle("quad3d")
    mean, spread, x0, o = _mixed_case()
    S = x0.shape[1]
    ended = ~np.isfinite(o[0][1])
    share = ended.mean()
    assert 0.25 <= share <= 0.75, share                                               # the oracle's share, before anything is compared
    assert np.isfinite(o[0][[0, 2]]).all()
    st = s.RolloutPolicyStats(S, mean, spread, x0_dist="uniform", seed=SEED, first_sample=FIRST, samples=True)
    assert np.all(np.abs(st.samples.x0 - x0) <= 2.0 * np.spacing(np.abs(mean) + spread)[:, None, :])
    assert np.array_equal(~np.isfinite(st.samples.cost[1]), ended) and np.array_equal(st.samples.steps, o[2])
    assert st.counted[1] == S - int(ended.sum()) and 0 < st.counted[1] < S and st.counted[0] == st.counted[2] == S
    assert st.steps_total[1] == int(o[2][1].sum())
    _check_stats(st, st.samples.cost, st.samples.steps, N, FIRST, what="a part of problem 1 ends")      # the moments: over the survivors
    print("mixed: %d of %d samples of problem 1 end early; worst ratios so far: mean %.3f, M2 %.3f" % (ended.sum(), S, WORST["mean"], WORST["m2"]))


# ---------------------------------------------------------------- 6. passes
def test_the_result_does_not_depend_on_the_window():
    import _policy_mc_child as child
    here = child.run()                                                               # this process: the default window (one pass)
    assert here.pop("passes") == 1
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "one_group_per_pass.npz")
        env = dict(os.environ, MI_ILQR_MC_PASS_GROUPS="1")                            # three passes, the accumulator carried between them
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_policy_mc_child.py"), out], env=env, timeout=300,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        there = dict(np.load(out))
    assert int(there.pop("passes")) == 3                                              # the switch was read: S = 130 is three groups
    assert set(here) == set(there)
    for k in here:
        assert np.array_equal(here[k], there[k], equal_nan=True), k
    assert np.all(here["n"] == 130) and np.all(here["counted"] > 0)


# ---------------------------------------------------------------- 7. the handle is only read; refusals
@pytest.mark.parametrize("name", ["pendulum", "pendulum_throughput", "arm27"])
def test_a_solve_after_a_run_is_the_solve_without(name):
    p, x0b, ug, mode, sigma = TP._cases()[name]()
    got = []
    for with_run in (True, False):
        s = TP._solver(p, max_iters=6, kernel_mode=mode)
        s.SetInitialState(x0b); s.SetInitialGuess(ug)
        TP._solve(s)
        if with_run:
            st = s.RolloutPolicyStats(130, x0b, sigma * np.ones(x0b.shape[1]), state_noise=1e-4, seed=SEED, samples=True)
            assert np.all(st.counted > 0)
        s.SetInitialState(x0b)
        TP._solve(s)
        got.append([np.array(a) for a in (s.x_bar, s.u_bar, s.K, s.cost, s.iterations)])
    for a, b_ in zip(*got):
        assert np.array_equal(a, b_)


def test_the_c_abi_refuses_and_keeps_what_it_had():
    from drake_ddp_amd import _capi
    c = TP._ctx("pendulum")
    s = TP._solver(c.p)
    s.set_state(x_bar=c.x_bar, u_bar=c.u_bar, K=c.K)
    s._push_costs()
    lib, h = s._lib, s._h
    n, npar, W = 2, 3, 3 * 2 + 2 * 3
    st_ = lambda which, a, nbytes=None: lib.mi_ilqr_set(h, which, _capi.ptr(a), (0 if a is None else a.nbytes) if nbytes is None else nbytes)   # noqa: E731
    gt_ = lambda which, a, nbytes=None: lib.mi_ilqr_get(h, which, _capi.ptr(a), a.nbytes if nbytes is None else nbytes)   # noqa: E731
    run = lambda *v: st_(_capi.F_POLICY_MC_RUN, np.array(v, dtype=np.float64))   # noqa: E731
    stats, smp = np.empty((B, 10)), np.empty((B, 5, n + npar + 2))
    # before anything is set
    assert run(5, 0, 0, 0, 0) == _capi.E_BAD_ARG                                     # no DIST rows
    assert gt_(_capi.F_POLICY_MC_STATS, stats) == _capi.E_BAD_ARG and gt_(_capi.F_POLICY_MC_SAMPLES, smp) == _capi.E_BAD_ARG
    passes = np.zeros(1, dtype=np.int32)
    assert lib.mi_ilqr_get_int(h, _capi.I_POLICY_MC_PASSES, _capi.ptr(passes), 4) == _capi.E_BAD_ARG
    rows = np.zeros((B, W))
    rows[:, :n] = c.x0b; rows[:, n:2 * n] = 0.05; rows[:, 2 * n:3 * n] = np.inf
    rows[:, 3 * n:3 * n + npar] = c.base; rows[:, 3 * n + npar:] = 0.01
    assert st_(_capi.F_POLICY_MC_DIST, rows) == _capi.OK
    back = np.empty_like(rows)
    assert gt_(_capi.F_POLICY_MC_DIST, back) == _capi.OK and np.array_equal(back, rows)
    # refused rows leave the rows
    assert st_(_capi.F_POLICY_MC_DIST, rows, rows.nbytes - 8) == _capi.E_BAD_SHAPE
    assert st_(_capi.F_POLICY_MC_DIST, None, rows.nbytes) == _capi.E_BAD_ARG
    for col, v in ((0, np.nan), (0, np.inf), (n, -1e-9), (n, np.inf), (n, np.nan), (2 * n, -0.5), (2 * n, np.nan), (3 * n, -np.inf),
                   (3 * n + npar, -1.0), (3 * n + npar, np.inf)):
        bad = rows.copy()
        bad[1, col] = v
        assert st_(_capi.F_POLICY_MC_DIST, bad) == _capi.E_BAD_ARG, (col, v)
    assert gt_(_capi.F_POLICY_MC_DIST, back) == _capi.OK and np.array_equal(back, rows)
    # a run, then refused runs: the statistics stay
    assert run(5, 0, 1, 1, 0) == _capi.OK
    assert gt_(_capi.F_POLICY_MC_STATS, stats) == _capi.OK and np.all(stats[:, 0] == 5) and np.all(stats[:, 1] == 5)
    assert gt_(_capi.F_POLICY_MC_STATS, stats, stats.nbytes - 8) == _capi.E_BAD_SHAPE
    assert lib.mi_ilqr_get_int(h, _capi.I_POLICY_MC_PASSES, _capi.ptr(passes), 4) == _capi.OK and passes[0] == 1
    assert lib.mi_ilqr_get_int(h, _capi.I_POLICY_MC_PASSES, _capi.ptr(passes), 8) == _capi.E_BAD_SHAPE
    assert gt_(_capi.F_POLICY_MC_SAMPLES, smp) == _capi.E_BAD_ARG                     # that run kept no samples
    ms = np.empty(1)
    assert gt_(_capi.F_POLICY_KERNEL_MS, ms) == _capi.OK and ms[0] > 0.0
    five = np.zeros(5); five[0] = 5
    assert st_(_capi.F_POLICY_MC_RUN, five, 32) == _capi.E_BAD_SHAPE and st_(_capi.F_POLICY_MC_RUN, None, 40) == _capi.E_BAD_ARG
    assert gt_(_capi.F_POLICY_MC_RUN, five) == _capi.E_BAD_ARG                        # write-only
    assert st_(_capi.F_POLICY_MC_STATS, stats) == _capi.E_BAD_ARG and st_(_capi.F_POLICY_MC_SAMPLES, smp) == _capi.E_BAD_ARG   # read-only
    for v in ((0, 0, 0, 0, 0), (-3, 0, 0, 0, 0), (2.5, 0, 0, 0, 0), (np.nan, 0, 0, 0, 0), (2.0 ** 32 + 1, 0, 0, 0, 0), (5, 2, 0, 0, 0),
              (5, 0, -1, 0, 0), (5, 0, 0, 0.5, 0), (5, 0, 0, 0, 3)):
        assert run(*v) == _capi.E_BAD_ARG, v
    stream = np.array([7.0, 2.0 ** 32 - 2, 0.0])
    assert st_(_capi.F_POLICY_STREAM, stream) == _capi.OK
    assert run(3, 0, 0, 0, 0) == _capi.E_BAD_ARG and run(2, 0, 0, 0, 1) == _capi.OK   # first_sample + S > 2^32; = 2^32
    two = np.empty((B, 2, n + npar + 2))
    assert gt_(_capi.F_POLICY_MC_SAMPLES, two) == _capi.OK and gt_(_capi.F_POLICY_MC_SAMPLES, smp) == _capi.E_BAD_SHAPE
    assert np.array_equal(two[:, :, n:n + npar], np.broadcast_to(c.base[:, None, :], (B, 2, npar)))           # not drawn: the problem's row
    after = np.empty((B, 10))
    assert gt_(_capi.F_POLICY_MC_STATS, after) == _capi.OK and np.all(after[:, 0] == 2) and np.all(after[:, 7] >= 2.0 ** 32 - 2)
    assert run(0, 0, 0, 0, 0) == _capi.E_BAD_ARG
    again = np.empty((B, 10))
    assert gt_(_capi.F_POLICY_MC_STATS, again) == _capi.OK and np.array_equal(again, after)
    assert gt_(_capi.F_POLICY_MC_SAMPLES, two) == _capi.OK
    # the rows survive a reset; (NULL, 0) clears them
    assert lib.mi_ilqr_reset(h) == _capi.OK
    assert gt_(_capi.F_POLICY_MC_DIST, back) == _capi.OK and np.array_equal(back, rows)
    assert st_(_capi.F_POLICY_MC_DIST, None) == _capi.OK and run(2, 0, 0, 0, 0) == _capi.E_BAD_ARG


def test_sample_params_on_a_model_without_parameters_is_unsupported():
    from drake_ddp_amd import _capi, plugin
    from drake_ddp_amd import workloads as W
    body = """
    const T w = x[1] + dt * (u[0] - 0.1 * x[1] - 4.0 * mi_sin(x[0]));
    xn[0] = x[0] + dt * w;
    xn[1] = w;
"""
    make = plugin.build_model("pp_noparams", 2, 1, body, [], "small")                # (test_gpu_policy_rollout's parameterless plugin)
    q = W.pendulum_problem()
    s = TP._solver(dict(q, N=10), system=make(q["dt"]))
    rows = np.zeros((B, 6)); rows[:, 2:4] = 0.1; rows[:, 4:] = np.inf
    assert s._lib.mi_ilqr_set(s._h, _capi.F_POLICY_MC_DIST, _capi.ptr(rows), rows.nbytes) == _capi.OK
    v = np.array([4.0, 0.0, 0.0, 1.0, 0.0])
    assert s._lib.mi_ilqr_set(s._h, _capi.F_POLICY_MC_RUN, _capi.ptr(v), v.nbytes) == _capi.E_UNSUPPORTED
    with pytest.raises(ValueError, match="no parameters"):
        s.RolloutPolicyStats(4, np.zeros(2), 0.1 * np.ones(2), params_mean=[])
    st = s.RolloutPolicyStats(4, np.zeros(2), 0.1 * np.ones(2))                      # the refusal left a working handle
    assert np.all(st.counted == 4) and np.all(st.steps_total == 4 * 9)


def test_a_handle_that_holds_a_reference_is_refused():
    from drake_ddp_amd import _capi
    c = TP._ctx("quad3d")
    s = TP._solver(c.p)
    n = c.x0b.shape[1]
    st = s.RolloutPolicyStats(4, c.x0b, 1e-3 * np.ones(n))                           # a cold handle runs (zero policy), and leaves its rows
    before = _ten(st)
    s.SetTargetTrajectory(np.tile(c.p["x_nom"], (3, 1)))
    v = np.array([4.0, 0.0, 0.0, 0.0, 0.0])
    assert s._lib.mi_ilqr_set(s._h, _capi.F_POLICY_MC_RUN, _capi.ptr(v), v.nbytes) == _capi.E_UNSUPPORTED
    with pytest.raises(ValueError, match="reference trajectory"):
        s.RolloutPolicyStats(4, c.x0b, 1e-3 * np.ones(n))
    out = np.empty((B, 10))
    assert s._lib.mi_ilqr_get(s._h, _capi.F_POLICY_MC_STATS, _capi.ptr(out), out.nbytes) == _capi.OK
    assert np.array_equal(out, before, equal_nan=True)                                # the last statistics are in place
    s.SetTargetTrajectory(None)
    assert _same_ten(s.RolloutPolicyStats(4, c.x0b, 1e-3 * np.ones(n)), st)


# ---------------------------------------------------------------- 8. the example
def test_the_example():
    import re
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "policy_monte_carlo_pendulum.py")], timeout=300,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    rates = [float(v) for v in re.findall(r"success rate ([0-9.]+)", r.stdout)]
    assert len(rates) == 4 and all(0.0 <= v <= 1.0 for v in rates), r.stdout
    print(r.stdout)
