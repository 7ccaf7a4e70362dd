"""The model and seeds of tests/test_gpu_dual2_overloads.py are chosen so that its flip budget can be 0: the NumPy oracle, run again
with x0 moved by one ulp either way, keeps its own iteration and line-search-trial counts on every one of the 256 problems - no
decision of these solves sits at round-off.  (A sample here; every problem was checked when the case was chosen.)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

STRIDE = int(os.environ.get("MI_DUAL2_ORACLE_STRIDE", "8"))


def test_oracle_counts_survive_one_ulp_of_x0():
    import plugin_steps as PS
    import test_gpu_dual2_overloads as T
    from oracle import models_np as M
    from oracle.ilqr_np import OracleILQR
    c = T.CASE
    x0, ug = T.problems()
    model = M.Model.custom(2, 1, PS.endstop2_step, np.array(T.ENDSTOP2_DEFAULTS), c["dt"])

    def counts(x):
        o = OracleILQR(model, c["N"], c["delta"], c["beta"], 0.0, jacobian="ad")
        o.set_problem(x, c["x_nom"], c["dt"] * c["Q"], c["dt"] * c["R"], c["Qf"], ug)
        hist = o.solve()[3]
        return len(hist), int(sum(h[2] for h in hist))
    moved = []
    for b in range(0, c["B"], STRIDE):
        base = counts(x0[b])
        if any(counts(np.nextafter(x0[b], d)) != base for d in (np.inf, -np.inf)):
            moved.append(b)
    assert not moved, moved
