"""tests/closed_loop_np.py - the NumPy statement of the plant of the closed MPC loop - tied to the policy-rollout oracles it is built
on; the host-side argument checks of SetPlant; the six selectors in the header and its ctypes mirror.  CPU only."""
import os
import re

import numpy as np
import pytest

import closed_loop_np as CL
import policy_noise_np as PN
from common import load_golden
from oracle import models_np as M
from policy_rollout_np import rollout_sample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi_ilqr.h")


def _policy(name):
    g, prob = load_golden(name)
    return g, prob, M.Model(prob["model_id"], prob["dt"], prob.get("params"))


@pytest.mark.parametrize("name", ["pendulum_stage", "acrobot_stage"])
@pytest.mark.parametrize("steps", [1, 7])
def test_without_mismatch_the_plant_follows_the_plan(name, steps):
    """No mismatch, no noise, feedback on: from x_bar[:, 0] the plant reproduces x_bar[:, :steps + 1] of a trajectory that is a rollout
    of its own controls (the golden's accepted line-search trial).  Tolerance: the oracle rollouts' own spread - the largest change
    of the plant's states under a one-ulp perturbation of the start in both directions - times 10, plus 1e-12 relative."""
    g, prob, model = _policy(name)
    x_bar, u_bar, K = g["roll_x"], g["roll_u"], g["pre_K"]
    args = (x_bar, u_bar, K, prob["Q"], prob["R"], prob["x_nom"], steps)
    xf, done, X, U, L = CL.plant_segment(model, x_bar[:, 0], *args)
    assert done == steps
    spread = 0.0
    for d in (np.inf, -np.inf):
        alt = CL.plant_segment(model, np.nextafter(x_bar[:, 0], d), *args)
        spread = max(spread, np.abs(alt[2] - X).max(), np.abs(alt[0] - xf).max())
    scale = np.abs(x_bar[:, :steps + 1]).max()
    assert spread <= 1e-6 * scale
    got = np.concatenate([X, xf[:, None]], axis=1)
    assert np.abs(got - x_bar[:, :steps + 1]).max() <= 1e-12 * scale + 10.0 * spread
    assert np.abs(U - u_bar[:, :steps]).max() <= 1e-12 * np.abs(u_bar).max() + 10.0 * np.abs(K[..., :steps]).max() * spread
    # the log's cost is the stage cost of the policy rollouts: their total is its sum plus the terminal term
    tot, xe, st, Xr, Ur = rollout_sample(model, x_bar[:, 0], x_bar[:, :steps + 1], u_bar[:, :steps], K[..., :steps], prob["Q"], prob["R"],
                                         np.zeros_like(prob["Q"]), prob["x_nom"])
    assert st == steps and np.array_equal(Xr[:, :steps], X) and np.array_equal(Ur, U) and np.array_equal(xe, xf)
    acc = 0.0
    for v in L:
        acc += v
    assert acc == tot


@pytest.mark.parametrize("feedback", [True, False])
def test_offsets_limits_and_feedback_off(feedback):
    g, prob, model = _policy("pendulum_stage")
    x_bar, u_bar, K = g["pre_x_bar"], g["pre_u_bar"], g["pre_K"]
    lo, hi = np.array([-0.05]), np.array([0.02])
    x = x_bar[:, 0] + np.array([0.3, -0.2])
    xf, done, X, U, L = CL.plant_segment(model, x, x_bar, u_bar, K, prob["Q"], prob["R"], prob["x_nom"], 5, feedback=feedback, u_min=lo, u_max=hi)
    assert done == 5 and U.min() >= lo[0] and U.max() <= hi[0]
    xs = np.array(x)
    for t in range(5):
        u = np.clip(u_bar[:, t] - (K[:, :, t] @ (xs - x_bar[:, t]) if feedback else 0.0), lo, hi)
        assert np.array_equal(X[:, t], xs) and np.array_equal(U[:, t], u)
        dx = xs - prob["x_nom"]
        assert L[t] == dx @ prob["Q"] @ dx + u @ prob["R"] @ u
        xs = model.step(xs, u)
    assert np.array_equal(xf, xs)


def test_with_noise_it_is_sample_0_of_the_noisy_policy_rollout():
    """Bitwise: the same NumPy code path, and the counter (0, k, b, j) is sample 0's at step t = k."""
    g, prob, _ = _policy("acrobot_stage")
    n, m, B, steps, seed = 4, 1, 3, 6, PN.TEST_SEED
    rng = np.random.default_rng(3)
    x_bar, u_bar, K = (np.ascontiguousarray(np.broadcast_to(g[k], (B,) + g[k].shape)) for k in ("pre_x_bar", "pre_u_bar", "pre_K"))
    x0 = x_bar[:, :, 0] + 0.01 * rng.standard_normal((B, n))
    base = np.asarray(M.DEFAULT_PARAMS[prob["model_id"]], dtype=float)
    params = base[None, :] * rng.uniform(0.9, 1.1, (B, base.size))
    sigma = np.tile([2e-3] * n + [1e-2] * m, (B, 1)) * np.array([1.0, 0.5, 2.0])[:, None]
    make = lambda row: M.Model(prob["model_id"], prob["dt"], row)   # noqa: E731
    for common in (False, True):
        ref = PN.rollout_noisy(make, x0[:, None, :], params, x_bar, u_bar, K, prob["Q"], prob["R"], prob["Qf"], prob["x_nom"], sigma, seed, 0, common)
        xf, done, X, U, L = CL.advance(make, x0, params, x_bar, u_bar, K, prob["Q"], prob["R"], prob["x_nom"], steps, sigma, seed, 0, common)
        assert np.all(done == steps)
        assert np.array_equal(X, ref[3][:, 0, :, :steps]) and np.array_equal(xf, ref[3][:, 0, :, steps]) and np.array_equal(U, ref[4][:, 0, :, :steps])
        # ... and the clock carries the stream: two segments are one
        x1, d1, X1, U1, L1 = CL.advance(make, x0, params, x_bar, u_bar, K, prob["Q"], prob["R"], prob["x_nom"], 2, sigma, seed, 0, common)
        sh = lambda a: a[..., 2:]   # noqa: E731
        x2, d2, X2, U2, L2 = CL.advance(make, x1, params, sh(x_bar), sh(u_bar), sh(K), prob["Q"], prob["R"], prob["x_nom"], steps - 2, sigma, seed, 2, common)
        assert np.array_equal(np.concatenate([X1, X2], axis=2), X) and np.array_equal(x2, xf) and np.array_equal(np.concatenate([L1, L2], axis=1), L)
    zx, zu = CL.plant_normals(seed, False, 2, 5, 3, n, m)
    assert np.array_equal(zx, PN.state_normals(seed, 0, False, 2, np.zeros(1, int)[:, None], np.arange(5, 8)[None, :], n)[0])
    assert np.array_equal(zu, PN.control_normals(seed, 0, False, 2, np.zeros(1, int)[:, None], np.arange(5, 8)[None, :], m)[0])


def test_a_plant_that_ends_keeps_its_state():
    g, prob, model = _policy("pendulum_stage")
    x_bar, u_bar, K = g["pre_x_bar"], g["pre_u_bar"], g["pre_K"]
    zx = np.zeros((4, 2)); zx[2] = 1.0
    zu = np.zeros((4, 1))
    big = np.array([np.finfo(float).max, np.finfo(float).max])
    xf, done, X, U, L = CL.plant_segment(model, x_bar[:, 0], x_bar, u_bar, K, prob["Q"], prob["R"], prob["x_nom"], 4, big, np.zeros(1), zx * 2.0, zu)
    assert done == 2 and np.isfinite(xf).all() and np.array_equal(xf, X[:, 2])
    assert np.isfinite(X[:, :3]).all() and np.isnan(X[:, 3]).all() and np.isfinite(U[:, :2]).all() and np.isnan(U[:, 2:]).all()
    assert np.isfinite(L[:2]).all() and np.isnan(L[2:]).all()


# ---------------------------------------------------------------- check_plant_args
def test_check_plant_args_broadcasts():
    from drake_ddp_amd.ilqr import check_plant_args as chk
    B, n, m, P = 3, 2, 1, 3
    x, p, noise, stream = chk(np.array([1.0, 2.0]), None, None, None, 0, False, True, 0, B, n, m, P)
    assert x.shape == (B, n) and x.flags["C_CONTIGUOUS"] and np.array_equal(x[2], [1.0, 2.0]) and p is None and noise is None
    assert np.array_equal(stream, [0.0, 0.0, 0.0, 1.0])
    xs = np.arange(6.0).reshape(B, n)
    x, p, noise, stream = chk(xs[::-1], np.ones(P), 0.5, np.array([0.25]), 2 ** 53 - 1, True, False, 2 ** 32 - 1, B, n, m, P, m_dev=4)
    assert np.array_equal(x, xs[::-1]) and x.flags["C_CONTIGUOUS"] and p.shape == (B, P) and p.flags["C_CONTIGUOUS"]
    assert noise.shape == (B, n + 4) and np.all(noise[:, :n] == 0.5) and np.all(noise[:, n] == 0.25) and np.all(noise[:, n + 1:] == 0.0)
    assert np.array_equal(stream, [2.0 ** 53 - 1, 2.0 ** 32 - 1, 1.0, 0.0])
    x, p, noise, stream = chk(xs, np.ones((B, P)), np.ones((B, n)), None, 1, 0, 1, 5.0, B, n, m, P)
    assert np.all(noise[:, :n] == 1.0) and np.all(noise[:, n:] == 0.0) and np.array_equal(stream, [1.0, 5.0, 0.0, 1.0])
    x, p, noise, stream = chk(xs, None, None, np.ones(m), 0, False, True, 0, B, n, m, 0)       # a parameterless model
    assert p is None and np.all(noise[:, :n] == 0.0)


def test_check_plant_args_refuses():
    from drake_ddp_amd.ilqr import check_plant_args as chk
    B, n, m, P = 3, 2, 1, 3
    xs = np.zeros((B, n))
    ok = dict(params=None, state_noise=None, control_noise=None, seed=0, common_noise=False, feedback=True, clock=0)

    def bad(match=None, x=xs, n_params=P, **kw):
        a = dict(ok, **kw)
        with pytest.raises(ValueError, match=match):
            chk(x, a["params"], a["state_noise"], a["control_noise"], a["seed"], a["common_noise"], a["feedback"], a["clock"], B, n, m, n_params)

    for x in (np.zeros(n + 1), np.zeros((B + 1, n)), np.zeros((B, n, 1)), 1.0, "x"):
        bad(x=x)
    for v in (np.nan, np.inf, -np.inf):
        x = xs.copy(); x[1, 1] = v
        bad("NaN or infinity in x", x=x)
        p = np.ones((B, P)); p[2, 0] = v
        bad("NaN or infinity in params", params=p)
        bad("state_noise", state_noise=v)
        bad("control_noise", control_noise=np.array([v]))
    for p in (np.ones(P + 1), np.ones((B + 1, P)), np.ones((B, P, 1))):
        bad(params=p)
    bad("no parameters", params=np.zeros((B, 0)), n_params=0)
    bad("negative", state_noise=-1e-3)
    bad("negative", control_noise=np.array([[0.1], [-0.1], [0.1]]))
    for s in (np.ones(n + 1), np.ones((B + 1, n)), np.ones((B, n, 1))):
        bad("state_noise", state_noise=s)
    for s in (np.ones(m + 1), np.ones((B, m + 1))):
        bad("control_noise", control_noise=s)
    for v in (-1, 2 ** 53, 0.5, np.nan, "1", True):
        bad("seed", seed=v)
    for v in (-1, 2 ** 32, 1.5, np.inf, None):
        bad("clock", clock=v)
    for v in (2, -1, 0.5, None, "yes"):
        bad("common_noise", common_noise=v)
        bad("feedback", feedback=v)


def test_set_plant_raises_before_it_touches_the_handle():
    """The methods themselves, on objects that have no handle at all (no device, no library call can have happened)."""
    from drake_ddp_amd import ilqr

    class _System:
        params = np.array([0.25, 0.1, 4.905])

    for cls, B in ((ilqr.BatchedIterativeLQR, 3), (ilqr.IterativeLinearQuadraticRegulator, 1)):
        for name in ("SetPlant", "ClearPlant", "plant_kernel_ms"):
            assert callable(getattr(cls, name))
        for name in ("plant_state", "plant_clock", "plant_log"):
            assert isinstance(getattr(cls, name), property)
        s = object.__new__(cls)
        s.B, s.n, s.m, s._md, s.N, s.system = B, 2, 1, 1, 10, _System()
        with pytest.raises(ValueError):
            s.SetPlant(np.zeros(3))
        with pytest.raises(ValueError):
            s.SetPlant(np.zeros(2), np.full(3, np.nan))
        with pytest.raises(ValueError):
            s.SetPlant(np.zeros(2), control_noise=-1.0)
    single = object.__new__(ilqr.IterativeLinearQuadraticRegulator)
    single.B, single.n, single.m, single._md, single.N, single.system = 1, 2, 1, 1, 10, _System()
    with pytest.raises(ValueError, match=r"x must be \(2,\)"):                 # the drop-in class takes (n,) only
        single.SetPlant(np.zeros((1, 2)))


# ---------------------------------------------------------------- the C ABI
SELECTORS = {"MI_F_PLANT_STATE": 21, "MI_F_PLANT_PARAMS": 22, "MI_F_PLANT_NOISE": 23, "MI_F_PLANT_STREAM": 24, "MI_F_PLANT_LOG": 25,
             "MI_F_PLANT_KERNEL_MS": 26}


def test_the_header_declares_the_selectors_and_no_new_entry_point():
    from drake_ddp_amd import _capi
    with open(HEADER) as f:
        src = f.read()
    values = {k: int(v) for k, v in re.findall(r"\b(MI_F_[A-Z0-9_]+)\s*=\s*(\d+)", src)}
    for name, v in SELECTORS.items():
        assert values[name] == v and getattr(_capi, name[3:]) == v, name
    assert len(set(values.values())) == len(values)
    shapes = {"MI_F_PLANT_STATE": "(B,n)", "MI_F_PLANT_PARAMS": "(B,n_params)", "MI_F_PLANT_NOISE": "(B,n+m)", "MI_F_PLANT_STREAM": "(4,)",
              "MI_F_PLANT_LOG": "(B,num_resolves*replan_steps,n+m+1)", "MI_F_PLANT_KERNEL_MS": "(1,)"}
    for name, shape in shapes.items():
        line = next(ln for ln in src.splitlines() if re.search(r"\b%s\s*=" % name, ln))
        assert shape in line, line
    assert re.search(r"#define MI_ILQR_ABI_VERSION 10\b", src) and _capi.ABI_VERSION == 10
    declared = re.findall(r"^(?:int|void|const char\s*\*|size_t|double)\s*(mi_ilqr_\w+)\(", src, re.M)
    assert len(declared) == len(set(declared)) == 48 and set(declared) == set(_capi.EXPORTS)
    flat = " ".join(re.sub(r"\n\s*\*", " ", src).split())
    for phrase in ("counter = (0, k, common ? 0 : b, j)", "SAMPLE 0 of a policy rollout", "x0 <- the plant's state", "Default 0 | 0 | 0 | 1",
                   "before anything is launched", "Independent of MI_F_POLICY_NOISE", "A refused call changes nothing"):
        assert phrase in flat, phrase


def test_the_library_refuses_a_null_handle():
    from drake_ddp_amd import _capi
    lib = _capi.load()
    assert lib.mi_ilqr_abi_version() == 10
    v = np.zeros(4)
    for which in SELECTORS.values():
        assert lib.mi_ilqr_set(None, which, _capi.ptr(v), v.nbytes) == _capi.E_BAD_ARG
        assert lib.mi_ilqr_get(None, which, _capi.ptr(v), v.nbytes) == _capi.E_BAD_ARG
