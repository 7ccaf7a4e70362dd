"""Probe plugins for the scalar primitives every device model is written on (csrc/dual.hpp, csrc/fastmath.hpp): mi_sin, mi_cos,
mi_rcp, mi_exp, mi_log1p, mi_sqrt, mi_softplus.  Shared by the fixture generator (oracle/gen_primitive_golden.py), the CPU
test of the fixtures (tests/test_primitive_golden.py) and the GPU test (tests/test_gpu_primitives.py).

A probe is a plugin model (drake_ddp_amd/plugin.py) whose step() is diagonal: xn[i] = f_i(x[i]), one primitive per state
slot.  The controls are read and never enter a value, so fu is exactly zero and a slot's result is the primitive's, bit for
bit (a "+ 0.0 * u[0]" would turn the gains' 0 * (inf - inf) = NaN into every slot of a problem with one non-finite input).
Through the existing stage entries:

  stage_rollout(1.0)          x[:, i, 1] = f_i(x0_i)             the double overloads
  stage_linearize(), "ad"     fx[:, i, i, 0] = f_i'(x0_i)        the Dual1 derivative rules; every other entry exactly 0
  stage_linearize(), "fd"     the same diagonal by central differences of the double overloads

Inputs are rebuilt from SEED by inputs(); truth (mpmath, 50 digits) lives in tests/golden/prim_<name>.npz as the correctly
rounded double `hi` and the remainder `lo` = (truth - hi) / ulp(hi) as float32 (in ulps of hi: a plain fp64 remainder of a
result near 2^-500 would not fit a float32, and two doubles per point would put a fixture above the size a committed file may
have).  error = |(dev - hi) / ulp(hi) - lo|, exact in fp64 whenever dev is within a factor of two of hi.
"""
import os

import numpy as np

SEED = 20261016
PRIMS = ("sin", "cos", "rcp", "exp", "log1p", "sqrt", "softplus")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DERIV_STRIDE = 8                      # derivative truth of rcp / log1p / sqrt / softplus: every 8th point (file size)
FD_H = 2.0 ** -17                     # central-difference step of the "fd" cases: x on a 2^-30 grid, so x +- h is exact
FD_POINTS = 1024

# step() text of one slot
CALL = {"sin": "mi_sin", "cos": "mi_cos", "rcp": "mi_rcp", "exp": "mi_exp", "log1p": "mi_log1p", "sqrt": "mi_sqrt",
        "softplus": "mi_softplus"}

# Bounds in ulp of the result (the project's own: tools/ubench/trig_acc.hip fails at 4 ulp, and for sin / cos results below 1e-6
# at 1e-15 absolute; mi_rcp: fma(r, e, r) rounds once, 0.5 ulp, and the residual of two Newton steps from a seed good to 2^-14 is
# below another 0.5; sqrt is correctly rounded; softplus = exp 1 + log1p 2 + one rounding).
VALUE_ULP = {"sin": 4.0, "cos": 4.0, "rcp": 1.0, "exp": 4.0, "log1p": 4.0, "sqrt": 0.5, "softplus": 4.0}
TRIG_SMALL, TRIG_ABS = 1e-6, 1e-15
# Dual1 rules with the seed d = 1 (the product with d is exact).  An error of e ulp in a factor is at most 2 e ulp in a result of
# another binade position, hence the factors of two:
#   sin' = fast_cos(v), cos' = -fast_sin(v), exp' = exp(v): the value primitives themselves                       4
#   rcp' = -(r * r): r within 1 ulp, twice, carried over (x 2), + the product's rounding                          2 (1 + 1) + 0.5
#   sqrt' = fast_rcp(2 r): r within 0.5 ulp, the reciprocal within 1, carried over                                2 (0.5 + 1) + 0.5
#   log1p' = 1 / (1 + v): the sum within 0.5 ulp, carried over, + the IEEE division's rounding                    2 (0.5) + 0.5
#   softplus' = r or t r, r = fast_rcp(1 + t), t = fast_exp_nonpos: the value's figure (exp 1 + reciprocal 1, carried over)   4
DERIV_ULP = {"sin": 4.0, "cos": 4.0, "exp": 4.0, "rcp": 4.5, "sqrt": 3.5, "log1p": 1.5, "softplus": 4.0}
TINY = 2.0 ** -1022                   # softplus / logistic below it: compared absolutely against it (a flush is allowed)

# "fd" cases: range of x and max |f'''| on it (+- h included)
#   sin, cos on [-1, 1]:       |f'''| <= 1
#   rcp on [1, 4]:             f''' = -6 / x^4, largest at x = 1 - h: 6 (1 + 5 h)            -> 6.001
#   exp on [-8, 0]:            f''' = exp(x) <= exp(h)                                        -> 1.001
#   log1p on [2^-10, 1]:       f''' = 2 / (1 + x)^3 <= 2
#   sqrt on [1, 4]:            f''' = 3/8 x^(-5/2), largest at x = 1 - h                      -> 0.376
#   softplus on [-8, 8]:       f''' = s (1 - s) (1 - 2 s), s = logistic: max 1 / (6 sqrt 3)   -> 0.09623
FD_RANGE = {"sin": (-1.0, 1.0, 1.0), "cos": (-1.0, 1.0, 1.0), "rcp": (1.0, 4.0, 6.001), "exp": (-8.0, 0.0, 1.001),
            "log1p": (2.0 ** -10, 1.0, 2.0), "sqrt": (1.0, 4.0, 0.376), "softplus": (-8.0, 8.0, 0.09623)}


def ref_value(mp, prim, x):
    """The primitive in mpmath (x an mpf)."""
    return {"sin": mp.sin, "cos": mp.cos, "rcp": lambda t: 1 / t, "exp": mp.exp, "log1p": mp.log1p, "sqrt": mp.sqrt,
            "softplus": lambda t: mp.log1p(mp.exp(t)) if t < 0 else t + mp.log1p(mp.exp(-t))}[prim](x)


def ref_deriv(mp, prim, x):
    return {"sin": mp.cos, "cos": lambda t: -mp.sin(t), "rcp": lambda t: -1 / (t * t), "exp": mp.exp,
            "log1p": lambda t: 1 / (1 + t), "sqrt": lambda t: 1 / (2 * mp.sqrt(t)),
            "softplus": lambda t: 1 / (1 + mp.exp(-t))}[prim](x)


def _logu(rng, e0, e1, k):
    """k magnitudes, log-uniform over [2^e0, 2^e1) up to the mantissa's uniformity: ldexp of a uniform mantissa, no libm call (the
    inputs must come out of the seed bit for bit on every machine)."""
    return np.ldexp(rng.uniform(1.0, 2.0, k), rng.integers(e0, e1, k).astype(np.int32))


def _near(c, k, width, rng):
    """k points around c: half of them the doubles next to c (c + j ulp, j = -k/4 .. k/4), half uniform in c +- width."""
    j = np.arange(-(k // 4), k - k // 2 - k // 4)
    a = c + j * np.spacing(abs(c) if c != 0.0 else 2.0 ** -1000)
    return np.concatenate([a, c + rng.uniform(-width, width, k - a.size)])


def KPI_NEAR():
    return np.arange(-2048, 2049)


def KPI_FAR():
    return np.concatenate([s * (2 ** 20 + np.arange(-384, 385)) for s in (-1, 1)])


def _trig_inputs():
    rng = np.random.default_rng(SEED)
    seg = []
    for r in (4.0, 1e2, 1e4, 3e6):
        seg.append(("uniform %g" % r, "ulp", rng.uniform(-r, r, 15000)))
    # the doubles nearest k pi / 2, |k| <= 2048 and |k| = 2^20 + (-384 .. 384): rounded from mpmath's pi by the generator and kept in
    # tests/golden/prim_kpi.npz (they cannot be rebuilt in fp64)
    with np.load(os.path.join(GOLDEN, "prim_kpi.npz")) as z:
        near, far = z["near"], z["far"]
    assert near.size == KPI_NEAR().size and far.size == KPI_FAR().size
    seg.append(("k pi/2, |k| <= 2048", "ulp", near))
    seg.append(("k pi/2, |k| ~ 2^20", "ulp", far))
    seg.append(("zeros and subnormals", "ulp", np.array([0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1040, -2.0 ** -1040, 2.0 ** -1023, -2.0 ** -1023])))
    big = np.maximum(_logu(rng, 21, 51, 1011), 3e6) * rng.choice([-1.0, 1.0], 1011)
    seg.append(("3e6 .. 2^51", "bounded", big))
    seg.append(("nan, +-inf", "nan", np.array([np.nan, np.inf, -np.inf])))
    return seg


def _rcp_inputs():
    rng = np.random.default_rng(SEED + 1)
    mag = _logu(rng, -500, 500, 63600)
    p2 = np.ldexp(1.0, np.arange(-500, 501, dtype=np.int32))
    return [("log-uniform 2^-500 .. 2^500", "ulp", mag * rng.choice([-1.0, 1.0], mag.size)),
            ("powers of two", "ulp", np.concatenate([p2, -p2])),
            # fast_rcp's Newton steps meet 0 x inf: NaN for 0 and +-inf (stated in fastmath.hpp), not IEEE 1 / x
            ("0, +-inf, nan", "nan", np.array([0.0, -0.0, np.inf, -np.inf, np.nan, np.nan]))]


def _exp_inputs():
    rng = np.random.default_rng(SEED + 2)
    return [("uniform -745 .. 0", "ulp", rng.uniform(-745.0, 0.0, 32768)), ("uniform -40 .. 0", "ulp", rng.uniform(-40.0, 0.0, 16384)),
            ("uniform -1 .. 0", "ulp", rng.uniform(-1.0, 0.0, 16382)), ("ends", "ulp", np.array([0.0, -745.0]))]


def _log1p_inputs():
    rng = np.random.default_rng(SEED + 3)
    return [("uniform 0 .. 1", "ulp", rng.uniform(0.0, 1.0, 49152)), ("log-uniform 2^-60 .. 1", "ulp", _logu(rng, -60, 0, 16382)),
            ("ends", "ulp", np.array([0.0, 1.0]))]


def _sqrt_inputs():
    rng = np.random.default_rng(SEED + 4)
    r = rng.integers(1, 2 ** 26, 16384).astype(np.float64)
    return [("log-uniform 2^-60 .. 2^60", "ulp", _logu(rng, -60, 60, 49152)), ("exact squares", "ulp", r * r)]


def _softplus_inputs():
    rng = np.random.default_rng(SEED + 5)
    ln53, fold = 53.0 * 0.6931471805599453, 0.881373587019543          # ln 2^53, -ln(sqrt 2 - 1) = asinh 1
    seg = [("uniform 40", "ulp", rng.uniform(-40.0, 40.0, 24576)), ("uniform 800", "ulp", rng.uniform(-800.0, 800.0, 24576)),
           ("around 0", "ulp", _near(0.0, 2048, 1e-3, rng))]
    for s in (1.0, -1.0):
        seg.append(("around %+.4f (t = 2^-53)" % (s * ln53), "ulp", _near(s * ln53, 2048, 1e-2, rng)))
        seg.append(("around %+.4f (log1p fold)" % (s * fold), "ulp", _near(s * fold, 2560, 1e-2, rng)))
        seg.append(("around %+d (exp clamp)" % (s * 745), "ulp", _near(s * 745.0, 2560, 2.0, rng)))
    return seg


_INPUTS = {"sin": _trig_inputs, "cos": _trig_inputs, "rcp": _rcp_inputs, "exp": _exp_inputs, "log1p": _log1p_inputs,
           "sqrt": _sqrt_inputs, "softplus": _softplus_inputs}


def segments(prim):
    """[(label, kind, slice)] and the input array of a primitive: kind "ulp" = measured against the fixture, "bounded" = finite
    and |f| <= 1 (+ the bound), "nan" = the result is NaN."""
    seg = _INPUTS[prim]()
    x = np.concatenate([s[2] for s in seg])
    out, at = [], 0
    for label, kind, a in seg:
        out.append((label, kind, slice(at, at + a.size)))
        at += a.size
    assert x.size >= 2 ** 16, (prim, x.size)
    return out, x


def inputs(prim):
    return segments(prim)[1]


def measured(prim):
    """Mask of the inputs whose result is compared with the fixture."""
    seg, x = segments(prim)
    m = np.zeros(x.size, bool)
    for _, kind, sl in seg:
        m[sl] = kind == "ulp"
    return m


def deriv_index(prim):
    """Indices of the inputs whose derivative has truth of its own (sin, cos, exp: every measured one, from the value fixtures)."""
    return np.nonzero(measured(prim))[0][::DERIV_STRIDE]


def fd_inputs(prim):
    lo, hi, _ = FD_RANGE[prim]
    rng = np.random.default_rng(SEED + 100 + PRIMS.index(prim))
    g = 2.0 ** 30
    return rng.integers(int(np.ceil(lo * g)), int(np.floor(hi * g)) + 1, FD_POINTS).astype(np.float64) / g


def to_pair(mp, t):
    """mpf -> (hi, lo in ulps of hi as float32)."""
    hi = float(t)
    if not np.isfinite(hi):
        return hi, np.float32(0.0)
    return hi, np.float32(float((t - mp.mpf(hi)) / mp.mpf(float(np.spacing(abs(hi))))))


def truth(mp, prim, x, deriv=False):
    f = ref_deriv if deriv else ref_value
    hi, lo = np.empty(x.size), np.empty(x.size, np.float32)
    for i, xi in enumerate(x):
        if np.isfinite(xi) and not (prim == "rcp" and xi == 0.0):
            hi[i], lo[i] = to_pair(mp, f(mp, prim, mp.mpf(float(xi))))
        else:
            hi[i], lo[i] = np.nan, 0.0
    return hi, lo


def digest(x):
    """What a fixture keeps of its inputs (the arrays themselves would double its size)."""
    import hashlib
    return hashlib.sha1(np.ascontiguousarray(x, dtype=np.float64).tobytes()).hexdigest()


def load(prim):
    with np.load(os.path.join(GOLDEN, "prim_%s.npz" % prim)) as z:
        return {k: z[k] for k in z.files}


def ulp_error(dev, hi, lo):
    """|dev - (hi + lo ulp(hi))| / ulp(hi)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs((dev - hi) / np.spacing(np.abs(hi)) - lo.astype(np.float64))


# ---------------------------------------------------------------------------------------------------------------- the probes
# name -> (n, m, family, primitive of every slot).  Family 0 has six slots: two probes.
def _cycle(n):
    return tuple(PRIMS[i % len(PRIMS)] for i in range(n))


PROBES = {
    "probe_small_a": (6, 1, "small", ("sin", "cos", "rcp", "exp", "log1p", "sqrt")),
    "probe_small_b": (6, 1, "small", ("softplus", "softplus", "sin", "cos", "rcp", "sqrt")),
    "probe_mid": (12, 4, "large", _cycle(12)),
    "probe_large": (36, 4, "large", _cycle(36)),
}


def body(slots):
    lines = ["    xn[%d] = %s(x[%d]);" % (i, CALL[p], i) for i, p in enumerate(slots)]
    return "\n".join(lines + ["    (void)u; (void)p; (void)dt;"])


def specs():
    """plugin.build_models' tuples."""
    return [(name, n, m, body(slots), [], fam) for name, (n, m, fam, slots) in PROBES.items()]


def pack(slots, pools, B):
    """Spread every primitive's inputs over the slots that evaluate it: launches of B problems, x0 (L, B, n) (slots whose pool
    has run out evaluate 1.0), and per primitive the (launch, slot) order in which unpack() reads the results back."""
    n = len(slots)
    where = {p: [i for i, q in enumerate(slots) if q == p] for p in pools}
    L = max(-(-pools[p].size // (B * len(where[p]))) for p in pools if where[p])
    x0 = np.ones((L, B, n))
    for p, x in pools.items():
        c = len(where[p])
        if c == 0:
            continue
        buf = np.ones(L * c * B)
        buf[:x.size] = x
        buf = buf.reshape(L, c, B)
        for j, i in enumerate(where[p]):
            x0[:, :, i] = buf[:, j, :]
    return x0, where


def unpack(out, where, pools):
    """out (L, B, n) -> {primitive: results in the order of its pool}."""
    res = {}
    for p, x in pools.items():
        if where[p]:
            res[p] = np.stack([out[:, :, i] for i in where[p]], axis=1).reshape(-1)[:x.size]
    return res
