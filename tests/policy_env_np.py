"""NumPy statement of what an on-device Monte-Carlo run observes beside the cost (include/mi_ilqr.h, "Envelopes and a safety box";
csrc/policy_env.hpp): the left fold of a row's samples into count | K | s1 | s2 | min | max | argmin | argmax, its finalisation, the
box rules and the merge of two windows.  Every operation is one rounded IEEE double operation per element, in the device's order, so
the fold is the device's bit for bit."""
import numpy as np

FIELDS = ("count", "mean", "m2", "min", "max", "argmin", "argmax")


def empty(shape=()):
    acc = np.zeros(tuple(shape) + (8,))
    acc[..., 4], acc[..., 5], acc[..., 6], acc[..., 7] = np.inf, -np.inf, -1.0, -1.0
    return acc


def fold(V, first_sample=0, acc=None):
    """V (..., S): the rows' values in sample order, sample s being global sample first_sample + s.  acc (..., 8) or None - empty:
    the accumulators so far.  Returns the accumulators after the S samples: a loop over the samples, vectorised over the rows."""
    V = np.asarray(V, dtype=np.float64)
    acc = empty(V.shape[:-1]) if acc is None else np.array(acc, dtype=np.float64)
    cnt, K, s1, s2, mn, mx, amin, amax = (acc[..., k].copy() for k in range(8))
    for s in range(V.shape[-1]):
        v = V[..., s]
        ok = np.isfinite(v)
        K = np.where(ok & (cnt == 0.0), v, K)
        with np.errstate(invalid="ignore", over="ignore"):
            d = v - K
            n1, n2 = s1 + d, s2 + d * d
        s1, s2, cnt = np.where(ok, n1, s1), np.where(ok, n2, s2), np.where(ok, cnt + 1.0, cnt)
        g = float(first_sample + s)
        with np.errstate(invalid="ignore"):
            lo, hi = ok & (v < mn), ok & (v > mx)
        mn, amin = np.where(lo, v, mn), np.where(lo, g, amin)
        mx, amax = np.where(hi, v, mx), np.where(hi, g, amax)
    return np.stack([cnt, K, s1, s2, mn, mx, amin, amax], axis=-1)


def fold_windows(V, window, first_sample=0):
    """The same fold carried through windows of `window` samples."""
    acc = None
    for s0 in range(0, V.shape[-1], window):
        acc = fold(V[..., s0:s0 + window], first_sample + s0, acc)
    return acc if acc is not None else empty(V.shape[:-1])


def finalise(acc):
    """-> dict of FIELDS: mean = K + s1 / count, M2 = max(0, s2 - s1 s1 / count); count 0: mean = M2 = NaN."""
    cnt, K, s1, s2 = (acc[..., k] for k in range(4))
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = K + s1 / cnt
        m2 = np.maximum(0.0, s2 - s1 * s1 / cnt)
    e = cnt == 0
    return dict(count=cnt.astype(np.int64), mean=np.where(e, np.nan, mean), m2=np.where(e, np.nan, m2), min=acc[..., 4].copy(),
                max=acc[..., 5].copy(), argmin=acc[..., 6].astype(np.int64), argmax=acc[..., 7].astype(np.int64))


def merge(a, b):
    """Two finalised dicts, a the window of the lower sample numbers: counts add, extrema by strict comparison (ties keep a), the
    moments by Chan's merge; a count-0 side leaves the other's numbers."""
    nA, nB = a["count"].astype(np.float64), b["count"].astype(np.float64)
    n = nA + nB
    with np.errstate(invalid="ignore", divide="ignore"):
        delta = b["mean"] - a["mean"]
        mean = a["mean"] + delta * (nB / n)
        m2 = (a["m2"] + b["m2"]) + (delta * delta) * ((nA * nB) / n)
    mean = np.where(nB == 0, a["mean"], np.where(nA == 0, b["mean"], mean))
    m2 = np.where(nB == 0, a["m2"], np.where(nA == 0, b["m2"], m2))
    lo, hi = b["min"] < a["min"], b["max"] > a["max"]
    return dict(count=a["count"] + b["count"], mean=mean, m2=m2, min=np.where(lo, b["min"], a["min"]), max=np.where(hi, b["max"], a["max"]),
                argmin=np.where(lo, b["argmin"], a["argmin"]), argmax=np.where(hi, b["argmax"], a["argmax"]))


def two_pass(v):
    """Extended-precision reference of one row: (count, mean, M2) over its finite values, two passes in np.longdouble."""
    x = np.asarray(v, dtype=np.float64)
    x = x[np.isfinite(x)].astype(np.longdouble)
    if x.size == 0:
        return 0, np.nan, np.nan
    mean = x.sum() / x.size
    return x.size, mean, ((x - mean) ** 2).sum()


def moment_bounds(v):
    """What the fold's finalised mean and M2 of one row may differ from two_pass's by - the standard bounds of recursive summation of
    S terms, on the shifted data d = v - K: |mean - ref| <= 2 S eps max|d| + eps |K|, |M2 - ref| <= 4 S eps sum d^2."""
    x = np.asarray(v, dtype=np.float64)
    x = x[np.isfinite(x)]
    if x.size == 0:
        return 0.0, 0.0
    eps = np.finfo(np.float64).eps
    d = x - x[0]
    return 2.0 * x.size * eps * float(np.max(np.abs(d))) + eps * abs(float(x[0])), 4.0 * x.size * eps * float(np.sum(d * d))


def box(X, lo, hi, x_nom, goal):
    """X (S, N, n): the samples' states, NaN from the step at which a sample ended; lo, hi, x_nom, goal (n,).  -> ran, safe,
    safe_success (integers) and exits (N,): a state is outside if x < lo or x > hi for some i (a NaN never is, a value on a bound is
    inside); exits[t] counts the samples whose FIRST outside state is x_t; the box only observes."""
    X = np.asarray(X, dtype=np.float64)
    S, N, n = X.shape
    with np.errstate(invalid="ignore"):
        outside = ((X < lo) | (X > hi)).any(axis=2)                        # (S, N)
        near = (np.abs(X[:, N - 1, :] - x_nom) <= goal).all(axis=1)
    ran = np.isfinite(X).all(axis=(1, 2))
    ever = outside.any(axis=1)
    first = np.argmax(outside, axis=1)
    exits = np.bincount(first[ever], minlength=N).astype(np.int64)
    safe = ran & ~ever
    return int(ran.sum()), int(safe.sum()), int((safe & near).sum()), exits


def rows_of(X):
    """RolloutPolicy's X (B, S, n, N) (or U (B, S, m, N-1)) -> the rows the device folds, (B, N, n, S)."""
    return np.ascontiguousarray(np.transpose(X, (0, 3, 2, 1)))
