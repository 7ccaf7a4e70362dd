"""The NumPy statement of parameter identification (tests/fit_np.py) on its own: it recovers the truth from noise-free transitions,
lowers the cost at every accepted trial, and ends with the statuses the rules give where they are constructed.  No GPU, no library.

Recovery bound: 1e-10 relative on every free parameter after 8 trials - the bound the device is held to in tests/test_gpu_fit.py.
The residual is zero at the truth, so the fixed point does not depend on the finite-difference Jacobians; measured with the cases of
tests/fit_cases.py (B = 3, T = 70, starts off by 15 - 30 % resp. 10 - 20 %), the worst problem per model: pendulum 1.2e-15, acrobot
1.3e-14, cart-pole 2.3e-15, 36-state chain 0, arm + ball 1.6e-15, 3-D quadruped 0."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fit_cases as FC  # noqa: E402
import fit_np as FN  # noqa: E402
from oracle import models_np as M  # noqa: E402


@pytest.mark.parametrize("kind", FC.RECOVERY)
def test_the_oracle_recovers_the_truth(kind):
    c = FC.case(kind)
    spread = FC.KINDS[kind][3]
    off = np.abs(c.start[:, c.free] / c.truth[:, c.free] - 1.0)
    assert off.max() <= spread + 1e-12 and off.min() >= 0.5 * spread - 1e-12  # the start is really off
    for b in range(c.B):
        r = FC.oracle_fit(c, b, iterations=8)
        err = np.max(np.abs(r["params"][c.free] - c.truth[b, c.free]) / np.abs(c.truth[b, c.free]))
        print(kind, b, "relative error", err, "cost", r["cost0"], "->", r["cost"], "status", r["status"])
        assert err <= 1e-10, (kind, b, err)
        assert r["status"] in (FN.CONVERGED, FN.MAX_ITERS) and r["cost"] < 1e-12 * r["cost0"]
        fixed = [k for k in range(c.truth.shape[1]) if k not in c.free]
        assert np.array_equal(r["params"][fixed], c.start[b, fixed])           # the other parameters stay at params0


@pytest.mark.parametrize("kind,b", (("pendulum", 0), ("arm27", 1)))
def test_the_cost_falls_at_every_accepted_trial(kind, b):
    c = FC.case(kind, seed=0)                                                  # (the arm's problem 1 of seed 0: rejections first)
    rng = np.random.default_rng(3)
    xn = c.x_next[b] + 1e-4 * rng.standard_normal(c.x_next[b].shape)           # noisy data: the cost ends above zero
    r = FN.fit(c.models[b], c.x[b], c.u[b], xn, c.start[b], c.free, iterations=12, ftol=0.0)
    kept = [r["cost0"]]
    for cost, accepted in r["trials"]:
        if accepted:
            assert cost < kept[-1]
            kept.append(cost)
        else:
            assert cost is None or not cost < kept[-1]
    assert r["accepted"] == len(kept) - 1 >= 3 and r["cost"] == kept[-1] > 0.0 and r["iterations"] == len(r["trials"])
    if kind == "arm27":
        assert not all(acc for _, acc in r["trials"])                          # ... and a rejection does raise mu and try again


def test_bad_data_and_stalled_where_constructed():
    c = FC.case("pendulum")
    mo = c.models[0]
    r = FN.fit(mo, c.x[0], c.u[0], c.x_next[0], c.start[0], c.free, count=0)
    assert r["status"] == FN.BAD_DATA and r["cost"] == np.inf and r["cost0"] == np.inf and np.array_equal(r["params"], c.start[0])
    assert r["iterations"] == 0
    bad = c.start[0].copy()
    bad[0] = 0.0                                                               # ml2 = 0: every prediction divides by zero
    r = FN.fit(mo, c.x[0], c.u[0], c.x_next[0], bad, [1, 2])
    assert r["status"] == FN.BAD_DATA and not np.isfinite(r["cost"]) and np.array_equal(r["params"], bad) and r["iterations"] == 0
    # u = 0 and omega = 0 at theta = 0: the pendulum stays where it is whatever its parameters - none of them is visible, the
    # gradient and the normal matrix are zero, D = I, delta = 0: no trial lowers the cost, mu climbs to its ceiling
    T = 5
    x = np.zeros((T, 2))
    u = np.zeros((T, 1))
    xn = np.tile([1e-3, 0.0], (T, 1))                                          # (a residual nothing explains)
    r = FN.fit(mo, x, u, xn, c.start[0], [1], damping=1e9, iterations=20)
    assert r["status"] == FN.STALLED and r["damping"] == 1e12 and r["accepted"] == 0 and r["iterations"] == 4
    assert np.array_equal(r["params"], c.start[0]) and r["cost"] == r["cost0"] > 0.0
    assert not r["normal_matrix"].any() and not r["gradient"].any()


def test_bounds_hold_the_result():
    c = FC.case("pendulum")
    k = c.free[1]
    lo = np.full(3, -np.inf)
    lo[k] = 1.05 * c.truth[0, k]
    r = FN.fit(c.models[0], c.x[0], c.u[0], c.x_next[0], c.start[0], c.free, bounds=(lo, np.full(3, np.inf)), iterations=12)
    free = FC.oracle_fit(c, 0, iterations=12)
    assert r["params"][k] == lo[k] and r["cost"] > free["cost"]


def test_a_plugin_step_goes_through_model_custom():
    import plugin_steps as PS
    nq, m, ne, dt = 16, 3, 5, 0.02
    truth = np.array([4.0, 0.5, 6.0, 2.0])
    mo = M.Model.custom(2 * nq + ne, m, PS.chainx_step(nq, m, ne), truth, dt)
    rng = np.random.default_rng(5)
    x, u = 0.5 * rng.standard_normal((20, mo.n)), rng.uniform(-1, 1, (20, m))
    xn = FN.predict(mo, truth, x, u)
    r = FN.fit(mo, x, u, xn, truth * np.array([1.2, 0.8, 1.0, 1.0]), [0, 1], iterations=8)
    assert np.max(np.abs(r["params"] / truth - 1.0)) <= 1e-10
