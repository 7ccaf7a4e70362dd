"""tests/golden/edge_<model>.npz are what oracle/gen_edge_step_golden.py writes today from the states tests/edge_states.py rebuilds:
digest of the states, a fixed sample regenerated with mpmath bit for bit, and the fp64 NumPy oracle close to that truth (it is the
yardstick of tests/test_gpu_edge_steps.py)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import edge_states as E  # noqa: E402

SAMPLE = 7


@pytest.mark.parametrize("model", E.MODELS)
def test_states_and_a_sample_of_the_truth_regenerate(model):
    g = E.load(model)
    assert str(g["sha1"]) == E.digest(model)
    x, u = E.states(model)
    assert np.abs(x[:, 1 if model != "pendulum" else 0]).max() > 9e3 and np.abs(x[:, -1]).max() > 9e2
    if model == "cartpole_wall":
        gap = (x[::2, 0] - 0.05 + 0.45) / 0.01                              # theta = 0 rows
        assert gap.min() < -790 and gap.max() > 790 and np.abs(gap).min() < 1e-9
    pytest.importorskip("mpmath")
    from oracle import gen_edge_step_golden as G
    new = G.arrays(model, sample=SAMPLE)
    for k, v in new.items():
        if v.ndim == 0:
            assert str(v) == str(g[k])
        else:
            assert v.dtype == g[k].dtype and np.array_equal(v, g[k][::SAMPLE], equal_nan=True), (model, k)


@pytest.mark.parametrize("model", E.MODELS)
def test_the_fp64_oracle_is_near_the_truth(model):
    """The yardstick itself: oracle/models_np.py in fp64 against its own formulas in mpmath - relative to each component's largest
    magnitude, 1e-9 (angles of 1e4 rad cost libm nothing, the softplus at +-800 sigma neither)."""
    from oracle import models_np as M
    g = E.load(model)
    x, u = E.states(model)
    mod = M.Model(E.MODEL_ID[model], E.DT[model])
    xn = np.array([mod.step_unchecked(x[b], u[b]) for b in range(E.B)])
    J = np.array([np.hstack(mod.jac_ad(x[b], u[b])) for b in range(E.B)])
    assert np.all(E.worst(xn, g["xn_hi"], g["xn_lo"]) <= 1e-9 * np.abs(g["xn_hi"]).max(axis=0))
    assert np.all(E.worst(J, g["J_hi"], g["J_lo"]) <= 1e-9 * np.maximum(np.abs(g["J_hi"]).max(axis=0), 1e-300))
