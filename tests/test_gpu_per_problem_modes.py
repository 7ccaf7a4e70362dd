"""Mode changes of the per-problem arrays on ONE handle: per-problem cost matrices with a shared target that changes under them
(the lane-per-problem kernels read that target from a broadcast the host caches), per-problem targets and back, per-problem model
parameters and back, shared matrices again - on the lane-per-problem, the wave-per-problem and the clustered workgroup kernels.
The other suites check each mode against a fresh shared handle; here every step runs on a handle that has been through the steps
before it, where a stale cached upload or a mode that was not really left would show.

Every step is Reset() and a cold solve from the same x0 and guess on the one handle H, compared BITWISE (x, u, K, L, it, st, ls)
with a fresh handle configured directly - GPU against GPU, no tolerance.  Cases, weight sets and sizes are those of
tests/test_gpu_cost_matrices.py (the smallest that still take each path, for the reasons given there); the parameter groups those of
tests/test_gpu_model_params.py.  T0 is the case's x_nom, T1 = T0 + 0.2 on the first coordinate (0.05 for Synth36).

The guard of step 3 - the cost under T1 differs from the cost under T0 for EVERY problem, so a stale target cannot pass - holds for
the reference: on the CPU the C oracle converged (status 0) on every problem of the three cases under both targets, and the smallest
relative cost difference between T0 and T1 was 8.7 % (pendulum), 12.6 % (acrobot) and 4.0 % (Synth36)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu


def _param_groups(name):
    import test_gpu_model_params as MP
    return {"acrobot_tp": MP._acrobot, "pendulum": MP._pendulum, "synth36": MP._synth36}[name]()[-1]


@pytest.mark.parametrize("name", ["acrobot_tp", "pendulum", "synth36"])
def test_mode_changes_on_one_handle_equal_fresh_handles(name):
    import test_gpu_cost_matrices as CM
    import test_gpu_model_params as MP
    p, B, kw, x0, ug = CM.CASES[name]()
    ws = CM._weights(p)
    rows = CM._stacked(ws, B)
    T0 = np.array(p["x_nom"], dtype=np.float64)
    T1 = T0.copy()
    T1[0] += 0.05 if name == "synth36" else 0.2
    T01 = np.ascontiguousarray(np.stack([T1 if b % 2 else T0 for b in range(B)]))
    prm = MP._rows(_param_groups(name), B)

    def set_rows(s):
        s.SetRunningCost(rows[0], rows[1]); s.SetTerminalCost(rows[2])

    def fresh(target, per_problem_weights=True, params=None):
        s = CM._solver(p, B, **kw)
        if per_problem_weights:
            set_rows(s)
        s.SetTargetState(target)
        if params is not None:
            s.SetModelParameters(params)
        return CM._solve(s, x0, ug)

    H = CM._solver(p, B, **kw)

    def step(tag, want):
        H.Reset()
        got = CM._solve(H, x0, ug)
        CM._assert_rows_equal(got, want, slice(None), (name, tag))
        return got

    # 1. interleaved weight rows, target T0
    set_rows(H)
    H.SetTargetState(T0)
    r1 = step("1: rows, T0", fresh(T0))
    # 2. nothing changed: the uploads are skipped
    step("2: repeated", r1)
    # 3. the shared target changes under the per-problem weights
    H.SetTargetState(T1)
    r3 = step("3: rows, T1", fresh(T1))
    assert np.all(r3["L"] != r1["L"]), (name, "T1 does not move every problem's cost: step 3 proves nothing")
    # 4. per-problem targets, T0 and T1 alternating
    H.SetTargetState(T01)
    step("4: rows, T0 / T1 by b % 2", fresh(T01))
    # 5. one target again: the cached broadcast must not still hold T1
    H.SetTargetState(T0)
    step("5: rows, T0 again", r1)
    # 6. per-problem model parameters, and back
    H.SetModelParameters(prm)
    step("6: rows, T0, parameter rows", fresh(T0, params=prm))
    H.SetModelParameters(None)
    step("6: parameters dropped", r1)
    # 7. shared matrices again
    CM._set_weights(H, ws[0])
    step("7: shared set 0, T0", fresh(T0, per_problem_weights=False))
