"""Writes tests/golden/edge_<model>.npz: one step of the small built-in models, and its Jacobian, at the edge states of
tests/edge_states.py - oracle/models_np.py's own step functions evaluated in mpmath at 50 digits, by swapping the primitives of
oracle/dual.py the module calls (D.sin, D.cos, D.softplus ...) for mpmath ones that also carry a gradient (unittest.mock.patch.object;
neither file is edited).

    python -m oracle.gen_edge_step_golden [model ...]

Arrays: `sha1` (digest of the states), `xn_hi` / `xn_lo` (B, n), `J_hi` / `J_lo` (B, n, n + m) = [fx fu]."""
import os
import sys
from unittest import mock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

DPS = 50


def _mp_dual(mp):
    class MD:
        """value + gradient row in mpf"""
        __array_priority__ = 1000

        def __init__(self, v, d):
            self.v, self.d = v, d

        @staticmethod
        def lift(o, like):
            return o if isinstance(o, MD) else MD(mp.mpf(o), [mp.mpf(0)] * len(like.d))

        def __add__(self, o):
            o = MD.lift(o, self)
            return MD(self.v + o.v, [a + b for a, b in zip(self.d, o.d)])
        __radd__ = __add__

        def __sub__(self, o):
            o = MD.lift(o, self)
            return MD(self.v - o.v, [a - b for a, b in zip(self.d, o.d)])

        def __rsub__(self, o):
            return MD.lift(o, self) - self

        def __mul__(self, o):
            o = MD.lift(o, self)
            return MD(self.v * o.v, [a * o.v + b * self.v for a, b in zip(self.d, o.d)])
        __rmul__ = __mul__

        def __truediv__(self, o):
            o = MD.lift(o, self)
            q = self.v / o.v
            return MD(q, [(a - q * b) / o.v for a, b in zip(self.d, o.d)])

        def __rtruediv__(self, o):
            return MD.lift(o, self) / self

        def __neg__(self):
            return MD(-self.v, [-a for a in self.d])

    def chain(f, df):
        return lambda a: MD(f(a.v), [df(a.v) * t for t in a.d])
    softplus = lambda t: mp.log1p(mp.exp(t)) if t < 0 else t + mp.log1p(mp.exp(-t))      # noqa: E731
    prims = dict(sin=chain(mp.sin, mp.cos), cos=chain(mp.cos, lambda t: -mp.sin(t)), exp=chain(mp.exp, mp.exp),
                 log1p=chain(mp.log1p, lambda t: 1 / (1 + t)), sqrt=chain(mp.sqrt, lambda t: 1 / (2 * mp.sqrt(t))),
                 softplus=chain(softplus, lambda t: 1 / (1 + mp.exp(-t))))
    return MD, prims


def arrays(model, sample=None):
    import mpmath as mp
    import edge_states as E
    import primitive_probes as P
    from oracle import dual as D, models_np as M
    mp.mp.dps = DPS
    MD, prims = _mp_dual(mp)
    mid = E.MODEL_ID[model]
    n, m = M.MODEL_DIMS[mid]
    x, u = E.states(model)
    xu = np.concatenate([x, u], axis=1)[::sample]
    p = [mp.mpf(float(v)) for v in M.DEFAULT_PARAMS[mid]]
    dt = mp.mpf(float(E.DT[model]))
    out = {k: np.empty(s, t) for k, s, t in (("xn_hi", (len(xu), n), float), ("xn_lo", (len(xu), n), np.float32),
                                             ("J_hi", (len(xu), n, n + m), float), ("J_lo", (len(xu), n, n + m), np.float32))}
    with mock.patch.multiple(D, **prims):
        for b, row in enumerate(xu):
            seed = [MD(mp.mpf(float(v)), [mp.mpf(int(i == j)) for j in range(n + m)]) for i, v in enumerate(row)]
            res = M.STEP_FUNCS[mid](seed[:n], seed[n:], p, dt)
            for i, r in enumerate(res):
                out["xn_hi"][b, i], out["xn_lo"][b, i] = P.to_pair(mp, r.v)
                for j in range(n + m):
                    out["J_hi"][b, i, j], out["J_lo"][b, i, j] = P.to_pair(mp, r.d[j])
    out["sha1"] = np.array(E.digest(model))
    return out


def main(names):
    import edge_states as E
    for model in names or E.MODELS:
        a = arrays(model)
        path = os.path.join(E.GOLDEN, "edge_%s.npz" % model)
        np.savez_compressed(path, **a)
        print(model, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
