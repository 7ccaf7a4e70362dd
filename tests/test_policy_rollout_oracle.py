"""tests/policy_rollout_np.py - the NumPy statement of mi_ilqr_policy_rollout - tied to the reference and pinned in its
conventions.  CPU only."""
import numpy as np
import pytest

from common import load_golden, rel_err
from oracle import models_np as M
from policy_rollout_np import rollout_sample


@pytest.mark.parametrize("name", ["pendulum_stage", "acrobot_stage"])
def test_reproduces_the_references_rollout(name):
    """eps = 1 and the golden's kappa: roll_x / roll_u / roll_L as the unmodified reference generated them, to the 1e-10 relative
    test_stage_level holds the device to."""
    g, prob = load_golden(name)
    model = M.Model(prob["model_id"], prob["dt"], prob.get("params"))
    L, xf, steps, X, U = rollout_sample(model, g["x0"], g["pre_x_bar"], g["pre_u_bar"], g["pre_K"], prob["Q"], prob["R"], prob["Qf"],
                                        prob["x_nom"], eps=1.0, kappa=g["pre_kappa"])
    assert steps == prob["N"] - 1
    assert rel_err(X, g["roll_x"]) < 1e-10 and rel_err(U, g["roll_u"]) < 1e-10
    assert abs(L - float(g["roll_L"])) <= 1e-10 * abs(float(g["roll_L"]))
    assert np.array_equal(xf, X[:, -1])


def test_zero_gains_is_the_open_loop_simulation():
    g, prob = load_golden("acrobot_stage")
    model = M.Model(prob["model_id"], prob["dt"])
    n, N = g["pre_x_bar"].shape
    u = g["pre_u_bar"]
    L, xf, steps, X, U = rollout_sample(model, g["x0"], g["pre_x_bar"], u, np.zeros_like(g["pre_K"]), prob["Q"], prob["R"], prob["Qf"],
                                        prob["x_nom"])
    x, Lo = np.array(g["x0"], float), 0.0
    for t in range(N - 1):
        assert np.array_equal(X[:, t], x) and np.array_equal(U[:, t], u[:, t])
        dx = x - prob["x_nom"]
        Lo += dx @ prob["Q"] @ dx + u[:, t] @ prob["R"] @ u[:, t]
        x = model.step(x, u[:, t])
    dx = x - prob["x_nom"]
    Lo += dx @ prob["Qf"] @ dx
    assert steps == N - 1 and np.array_equal(xf, x) and L == Lo


def test_clamp_convention():
    """The clamp applies to the whole feedback law, before the step and before the cost."""
    model = M.Model(M.PENDULUM, 0.01)
    N = 6
    x_bar, u_bar, K = np.zeros((2, N)), np.full((1, N - 1), 0.5), np.full((1, 2, N - 1), 4.0)
    args = (np.eye(2), np.eye(1), np.eye(2), np.zeros(2))
    L, xf, steps, X, U = rollout_sample(model, [1.0, 0.0], x_bar, u_bar, K, *args, u_min=np.array([-0.3]), u_max=np.array([0.2]))
    free = rollout_sample(model, [1.0, 0.0], x_bar, u_bar, K, *args)
    assert (free[4] < -0.3).any()                                    # the law itself leaves the box ...
    assert U.min() == -0.3 and U.max() <= 0.2 and steps == N - 1     # ... the clamped rollout does not
    x, Lo = np.array([1.0, 0.0]), 0.0
    for t in range(N - 1):
        u = np.clip(u_bar[:, t] - K[:, :, t] @ (x - x_bar[:, t]), -0.3, 0.2)
        Lo += x @ x + u @ u
        x = model.step(x, u)
    assert L == Lo + x @ x and np.array_equal(xf, x)


def test_infeasible_step_convention():
    """A planar-quadruped state one step away from a velocity planar_quad_infeasible flags: the sample ends there."""
    model = M.Model(M.PLANAR_QUAD, 0.002)
    n, m = model.n, model.m
    N = 5
    x0 = np.zeros(n); x0[1] = 0.5                                    # trunk in the air, at rest
    ok = rollout_sample(model, x0, np.zeros((n, N)), np.zeros((m, N - 1)), np.zeros((m, n, N - 1)), np.eye(n), np.eye(m), np.eye(n),
                        np.zeros(n))
    assert ok[2] == N - 1 and np.isfinite(ok[0])
    x_fast = x0.copy()
    u = np.zeros((m, N - 1)); u[0, 1] = 5000.0                       # a torque at step 1 that carries a joint rate across the bound
    assert not M.planar_quad_infeasible(list(model.step_unchecked(x_fast, u[:, 0])), model.params)
    L, xf, steps, X, U = rollout_sample(model, x_fast, np.zeros((n, N)), u, np.zeros((m, n, N - 1)), np.eye(n), np.eye(m), np.eye(n),
                                        np.zeros(n))
    assert M.planar_quad_infeasible(list(model.step_unchecked(X[:, 1], u[:, 1])), model.params)
    assert steps == 1 and L == np.inf
    assert np.array_equal(xf, X[:, 1]) and np.isfinite(X[:, :2]).all() and np.isnan(X[:, 2:]).all()
    assert np.isfinite(U[:, :1]).all() and np.isnan(U[:, 1:]).all()
    # a non-finite x0 ends the sample before its first step
    x_nan = x0.copy(); x_nan[2] = np.nan
    L, xf, steps, X, U = rollout_sample(model, x_nan, np.zeros((n, N)), np.zeros((m, N - 1)), np.zeros((m, n, N - 1)), np.eye(n), np.eye(m),
                                        np.eye(n), np.zeros(n))
    assert steps == 0 and L == np.inf and np.isnan(xf[2]) and np.isnan(X[:, 1:]).all() and np.isnan(U).all()
    assert np.array_equal(X[:, 0], x_nan, equal_nan=True)
