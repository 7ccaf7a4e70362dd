"""Writes tests/golden/prim_<name>.npz: the scalar primitives of the device models (csrc/dual.hpp, csrc/fastmath.hpp) in mpmath at
50 digits, at the inputs tests/primitive_probes.py rebuilds from its seed.

    python -m oracle.gen_primitive_golden [name ...]

prim_kpi.npz holds the inputs that need mpmath themselves (the doubles nearest k pi / 2).  Per primitive: `x_sha1` (digest of the
inputs), `hi` / `lo` (the value: the correctly rounded double and the remainder in ulps of it, float32), `d_hi` / `d_lo` (the derivative at primitive_probes.deriv_index, for the primitives whose derivative is not another
primitive's value) and `fd_hi` / `fd_lo` (the derivative at primitive_probes.fd_inputs).  tests/test_primitive_golden.py
regenerates a sample of every array.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

DPS = 50
OWN_DERIV = ("rcp", "log1p", "sqrt", "softplus")       # sin' = cos, cos' = -sin, exp' = exp: the value fixtures serve


def arrays(prim, sample=None):
    """The fixture's arrays; `sample` = a stride: every sample-th point only (the CPU test's regeneration)."""
    import mpmath as mp
    import primitive_probes as P
    mp.mp.dps = DPS
    st = slice(None, None, sample)
    x = P.inputs(prim)
    out = {"x_sha1": np.array(P.digest(x)), "fd_x_sha1": np.array(P.digest(P.fd_inputs(prim)))}
    out["hi"], out["lo"] = P.truth(mp, prim, x[st])
    if prim in OWN_DERIV:
        out["d_hi"], out["d_lo"] = P.truth(mp, prim, x[P.deriv_index(prim)][st], deriv=True)
    out["fd_hi"], out["fd_lo"] = P.truth(mp, prim, P.fd_inputs(prim)[st], deriv=True)
    return out


def kpi():
    """The doubles nearest k pi / 2 for primitive_probes.KPI_NEAR / KPI_FAR."""
    import mpmath as mp
    import primitive_probes as P
    mp.mp.dps = DPS
    return {name: np.array([float(int(k) * mp.pi / 2) for k in ks()]) for name, ks in (("near", P.KPI_NEAR), ("far", P.KPI_FAR))}


def main(names):
    import primitive_probes as P
    if not names or "kpi" in names:
        np.savez_compressed(os.path.join(P.GOLDEN, "prim_kpi.npz"), **kpi())          # (first: the trig inputs read it)
        names = [n for n in names if n != "kpi"]
    for prim in names or P.PRIMS:
        a = arrays(prim)
        path = os.path.join(P.GOLDEN, "prim_%s.npz" % prim)
        np.savez_compressed(path, **a)
        print(prim, a["hi"].size, "points,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
