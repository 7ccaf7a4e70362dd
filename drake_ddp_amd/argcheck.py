"""The argument checks of the front end (ilqr.py): each `check_*` turns a public method's arguments into the arrays and numbers the C
ABI takes, or raises ValueError - before anything reaches the library.  They stand on four primitives, `numbers`, `integer`, `rows`
and `flag`, which take the caller's name (`who`) and the argument's, so every message is worded where it is raised.  NumPy and the
constants of _capi only: nothing here loads the library.

The messages are part of the interface (tests/test_frontend_messages.py holds them), and so is which of two bad arguments is
reported: the order of the checks.  Kept as they grew, on purpose:
 - check_noise_args shows an out-of-range integer as int(v) (`got 9007199254740992`), a wrong-typed one as {v!r}; every other
   function shows {v!r} for both (`got 9007199254740992.0`).
 - check_mc_args takes S and first_sample as Python or NumPy ints only; a whole-number float is refused there, accepted elsewhere.
 - the shape phrase is `(B, k) or (k,)` in SetModelParameters and SetPlant, `(k,) or (B, k)` in RolloutPolicyStats.
 - check_mppi_args takes seed, hold and sigma_u through check_seed_args(1, ..): their errors come in that function's order.
 - check_model_params and check_target_trajectory name no argument in "not an array of numbers"; check_target_trajectory's clock is
   anything int() takes that equals its int - True and 3.0 pass.
"""
import numpy as np

from . import _capi

_INT, _FLOAT, _BOOL = (int, np.integer), (float, np.floating), (bool, np.bool_)


def numbers(v, who, name=None):
    """v as a float64 array, or ValueError."""
    try:
        return np.asarray(v, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{who}: {name + ' is ' if name else ''}not an array of numbers ({e})") from None


def integer(v, who, name, lo, end, rng, floats=True, show_int=False):
    """v as an int in [lo, end) - end None: no upper end -, or ValueError "<who>: <name> must be an integer <rng>; got <v!r>".  A bool
    is no integer; a float that is a whole number is one unless floats=False.  show_int: an integer out of range is shown as int(v)."""
    ok = not isinstance(v, _BOOL) and isinstance(v, _INT + (_FLOAT if floats else ()))
    if ok and isinstance(v, _FLOAT):
        ok = bool(np.isfinite(v) and v == np.floor(v))
    if ok and lo <= int(v) and (end is None or int(v) < end):
        return int(v)
    raise ValueError(f"{who}: {name} must be an integer {rng}; got {int(v) if ok and show_int else repr(v)}")


def rows(v, who, name, B, k, *, scalar=False, b_first=False, finite=True, nonneg=None, pad=None):
    """v, (k,) or (B, k) - scalar=True: or a scalar -, as (B, k) float64 rows (a broadcast view), or ValueError.  name None: the
    messages name no argument.  b_first: the shape phrase is "(B, k) or (k,)".  finite=False: infinities pass, NaN does not.  nonneg: a
    negative entry is refused, with these words behind "negative entry in <name>".  pad: the rows are written into the leading
    columns of a fresh contiguous (B, pad) array of zeros."""
    a = numbers(v, who, name)
    if a.shape not in ((k,), (B, k)) + (((),) if scalar else ()):
        forms = f"({B}, {k}) or ({k},)" if b_first else f"({k},) or ({B}, {k})"
        raise ValueError(f"{who}: {name or 'parameters'} must be {'a scalar, ' if scalar else ''}{forms}; got {a.shape}")
    if np.isnan(a).any() or (finite and not np.isfinite(a).all()):
        raise ValueError(f"{who}: NaN{' or infinity' if finite else ''}{' in ' + name if name else ''}")
    if nonneg is not None and (a < 0.0).any():
        raise ValueError(f"{who}: negative entry in {name}{nonneg}")
    if pad is None:
        return np.broadcast_to(a, (B, k))
    out = np.zeros((B, pad))
    out[:, :k] = a
    return out


def flag(v, who, name, ints=False):
    """v as a bool; ints=True: 0 and 1 are flags too."""
    if isinstance(v, _BOOL) or (ints and isinstance(v, _INT) and v in (0, 1)):
        return bool(v)
    raise ValueError(f"{who}: {name} must be True or False; got {v!r}")


def _sigmas(who, state_noise, control_noise, B, n, m, m_dev):
    """None when both are None, else the (B, n + m_dev) rows sigma_x | sigma_u: scalar, (n,) / (m,) or (B, n) / (B, m); None: zeros."""
    if state_noise is None and control_noise is None:
        return None
    def sigma(v, k, name, pad):
        return np.zeros((B, pad)) if v is None else rows(v, who, name, B, k, scalar=True, nonneg=" (standard deviations)", pad=pad)

    return np.hstack([sigma(state_noise, n, "state_noise", n), sigma(control_noise, m, "control_noise", m_dev)])


def check_model_params(params, B, n_params):
    """SetModelParameters' argument as a contiguous (B, n_params) float64 array ((n_params,) is broadcast to rows), or None for
    None.  ValueError for any other shape and for NaN / infinity - decided here, before anything reaches the device."""
    if params is None:
        return None
    if n_params == 0:
        raise ValueError("SetModelParameters: this model has no parameters")
    return np.ascontiguousarray(rows(params, "SetModelParameters", None, B, n_params, b_first=True))


def check_target_trajectory(x_ref, clock, B, n):
    """SetTargetTrajectory's arguments as a contiguous (B, T, n) float64 array ((T, n) is broadcast to the batch; None for None) and
    the clock as an int.  ValueError for any other shape, T = 0, NaN / infinity and a clock that is not an integer in [0, 2^30) -
    decided here, before anything reaches the device."""
    try:
        c = int(clock)
        ok = c == clock and 0 <= c < 2 ** 30
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"SetTargetTrajectory: clock must be an integer in [0, 2^30); got {clock!r}")
    if x_ref is None:
        return None, c
    a = numbers(x_ref, "SetTargetTrajectory")
    if a.ndim == 2 and a.shape[1] == n:
        a = np.broadcast_to(a, (B,) + a.shape)
    elif not (a.ndim == 3 and a.shape[0] == B and a.shape[2] == n):
        raise ValueError(f"SetTargetTrajectory: the reference must be (T, {n}) or ({B}, T, {n}); got {a.shape}")
    if a.shape[1] < 1:
        raise ValueError("SetTargetTrajectory: the reference needs at least one row (T >= 1)")
    if not np.isfinite(a).all():
        raise ValueError("SetTargetTrajectory: NaN or infinity")
    return np.ascontiguousarray(a), c


def check_rollout_args(x0, params, B, n, n_params):
    """RolloutPolicy's arguments as contiguous (B, S, n) and (B, S, n_params) float64 arrays (None for params=None).
    ValueError for a wrong rank or size and for NaN / infinity in params - decided here, before anything reaches the device.
    A non-finite x0 is data: that sample ends before its first step."""
    x0 = numbers(x0, "RolloutPolicy", "x0")
    if x0.ndim == 2 and x0.shape[1] == n and x0.shape[0] >= 1:
        x0 = np.broadcast_to(x0, (B,) + x0.shape)
    elif not (x0.ndim == 3 and x0.shape[0] == B and x0.shape[1] >= 1 and x0.shape[2] == n):
        raise ValueError(f"RolloutPolicy: x0 must be ({B}, S, {n}) or (S, {n}) with S >= 1; got {x0.shape}")
    S = x0.shape[1]
    if params is not None:
        if n_params == 0:
            raise ValueError("RolloutPolicy: this model has no parameters")
        params = numbers(params, "RolloutPolicy", "params")
        if params.shape == (S, n_params):
            params = np.broadcast_to(params, (B, S, n_params))
        elif params.shape != (B, S, n_params):
            raise ValueError(f"RolloutPolicy: params must be ({B}, {S}, {n_params}) or ({S}, {n_params}); got {params.shape}")
        if not np.isfinite(params).all():
            raise ValueError("RolloutPolicy: NaN or infinity in params")
        params = np.ascontiguousarray(params)
    return np.ascontiguousarray(x0), params


def check_noise_args(state_noise, control_noise, seed, first_sample, common_noise, B, n, m, m_dev=None, S=None):
    """RolloutPolicy's disturbance arguments -> (rows, stream): rows is None when both sigmas are None (no noise), else the
    contiguous (B, n + m_dev) float64 array sigma_x | sigma_u with zeros on the padding controls (m_dev: the device's number of
    controls, default m); stream is the float64 triple seed | first_sample | common.  state_noise: scalar, (n,) or (B, n);
    control_noise: scalar, (m,) or (B, m); one of them None: zeros.  ValueError - decided here, before anything reaches the device -
    for any other shape, a negative, NaN or infinite sigma, a seed that is no integer in [0, 2^53), a first_sample that is no integer
    in [0, 2^32) or - S given - with first_sample + S > 2^32."""
    who = "RolloutPolicy"
    seed = integer(seed, who, "seed", 0, 1 << 53, "in [0, 2^53)", show_int=True)
    first_sample = integer(first_sample, who, "first_sample", 0, 1 << 32, "in [0, 2^32)", show_int=True)
    if S is not None and first_sample + int(S) > (1 << 32):
        raise ValueError(f"RolloutPolicy: first_sample + S must not exceed 2^32; got {first_sample} + {int(S)}")
    stream = np.array([seed, first_sample, 1.0 if common_noise else 0.0], dtype=np.float64)
    return _sigmas(who, state_noise, control_noise, B, n, m, m if m_dev is None else int(m_dev)), stream


def check_plant_args(x, params, state_noise, control_noise, seed, common_noise, feedback, clock, B, n, m, n_params, m_dev=None):
    """SetPlant's arguments -> (x, params, noise, stream): x the contiguous (B, n) float64 states ((n,) is broadcast to rows); params
    None or the contiguous (B, n_params) rows ((n_params,) broadcast); noise None when both sigmas are None, else the (B, n + m_dev)
    rows sigma_x | sigma_u of check_noise_args (the same forms: scalar, (n,) / (m,), (B, n) / (B, m)); stream the float64 quadruple
    seed | clock | common | feedback.  ValueError - decided here, before anything reaches the device - for any other shape, NaN or
    infinity in x or params, params for a model without parameters, a negative, NaN or infinite sigma, a seed that is no integer in
    [0, 2^53), a clock that is no integer in [0, 2^32), common_noise or feedback that is no bool (or 0 / 1)."""
    who = "SetPlant"
    x = np.ascontiguousarray(rows(x, who, "x", B, n, b_first=True))
    if params is not None:
        if n_params == 0:
            raise ValueError("SetPlant: this model has no parameters")
        params = np.ascontiguousarray(rows(params, who, "params", B, n_params, b_first=True))
    seed = integer(seed, who, "seed", 0, 1 << 53, "in [0, 2^53)", show_int=True)       # (check_noise_args' rules, in its order)
    clock = integer(clock, who, "clock", 0, 1 << 32, "in [0, 2^32)", show_int=True)
    noise = _sigmas(who, state_noise, control_noise, B, n, m, m if m_dev is None else int(m_dev))
    stream = np.array([seed, clock, flag(common_noise, who, "common_noise", ints=True), flag(feedback, who, "feedback", ints=True)],
                      dtype=np.float64)
    return x, params, noise, stream


MC_DISTS = {"normal": _capi.MC_DIST_NORMAL, "uniform": _capi.MC_DIST_UNIFORM}


def check_mc_args(S, x0_mean, x0_spread, B, n, n_params, *, x0_dist="normal", params_mean=None, params_spread=None, params_dist="uniform",
                  goal=None, samples=False, first_sample=0):
    """RolloutPolicyStats' sampler arguments -> (rows, run): rows the contiguous (B, 3 n + 2 n_params) float64 array x0_mean | x0_spread |
    goal | p_mean | p_spread (MI_F_POLICY_MC_DIST), run the float64 quintuple S | x0_dist | p_dist | sample_params | samples
    (MI_F_POLICY_MC_RUN).  Means, spreads and goal: (k,) or (B, k); goal None: +inf everywhere (success = counted); params_mean None:
    the parameters are not sampled (params_spread alone is refused; params_mean alone: spread zero).  ValueError - decided here, before
    anything reaches the device - for any other shape, a NaN, a mean or spread that is not finite, a negative spread or goal, an S
    that is no integer >= 1 or with first_sample + S > 2^32, an unknown distribution, parameters on a model without any."""
    who = "RolloutPolicyStats"
    S = integer(S, who, "S", 1, None, ">= 1", floats=False)
    first_sample = integer(first_sample, who, "first_sample", 0, 1 << 32, "in [0, 2^32)", floats=False)
    if first_sample + S > (1 << 32):
        raise ValueError(f"RolloutPolicyStats: first_sample + S must not exceed 2^32; got {first_sample} + {S}")
    for name, d in (("x0_dist", x0_dist), ("params_dist", params_dist)):
        if d not in MC_DISTS:
            raise ValueError(f"RolloutPolicyStats: {name} must be 'normal' or 'uniform'; got {d!r}")
    out = np.zeros((B, 3 * n + 2 * n_params))
    out[:, :n] = rows(x0_mean, who, "x0_mean", B, n)
    out[:, n:2 * n] = rows(x0_spread, who, "x0_spread", B, n, nonneg="")
    out[:, 2 * n:3 * n] = np.inf if goal is None else rows(goal, who, "goal", B, n, finite=False, nonneg="")
    sample_params = params_mean is not None
    if params_spread is not None and not sample_params:
        raise ValueError("RolloutPolicyStats: params_spread needs params_mean")
    if sample_params:
        if n_params == 0:
            raise ValueError("RolloutPolicyStats: this model has no parameters")
        out[:, 3 * n:3 * n + n_params] = rows(params_mean, who, "params_mean", B, n_params)
        if params_spread is not None:
            out[:, 3 * n + n_params:] = rows(params_spread, who, "params_spread", B, n_params, nonneg="")
    run = np.array([S, MC_DISTS[x0_dist], MC_DISTS[params_dist], 1.0 if sample_params else 0.0, 1.0 if samples else 0.0], dtype=np.float64)
    return out, run


def check_mc_observe(envelope, controls, safe_box, B, n):
    """RolloutPolicyStats' observing arguments -> (bits, box): bits the value of MI_F_POLICY_MC_OBSERVE (1 state envelopes, 2 control
    envelopes), box None or the contiguous (B, 2 n) float64 rows lo | hi of MI_F_POLICY_MC_BOX.  safe_box: None or a pair (lo, hi),
    each None - unbounded - or (n,) / (B, n) with +-inf for an unbounded component.  ValueError - decided here, before anything
    reaches the device - for a flag that is no bool, a safe_box that is no pair, any other shape, a NaN, or lo > hi anywhere."""
    who = "RolloutPolicyStats"
    envelope, controls = flag(envelope, who, "envelope"), flag(controls, who, "controls")
    bits = (_capi.MC_OBSERVE_X if envelope else 0) | (_capi.MC_OBSERVE_U if controls else 0)
    if safe_box is None:
        return bits, None
    if not isinstance(safe_box, (tuple, list)) or len(safe_box) != 2:
        raise ValueError("RolloutPolicyStats: safe_box must be a pair (lo, hi)")
    box = np.empty((B, 2 * n))
    for j, (name, v, dflt) in enumerate((("safe_box lo", safe_box[0], -np.inf), ("safe_box hi", safe_box[1], np.inf))):
        box[:, j * n:(j + 1) * n] = dflt if v is None else rows(v, who, name, B, n, finite=False)
    if (box[:, :n] > box[:, n:]).any():
        raise ValueError("RolloutPolicyStats: safe_box has lo > hi")
    return bits, box


def check_seed_args(K, B, m, sigma_u=None, seed=0, round=0, hold=1, m_dev=None, what="PerturbInitialGuess"):   # noqa: A002
    """The multi-start arguments -> (K, rows, seed, round, hold): K the group size as an int, rows None for sigma_u=None (SelectBest,
    GatherBest) or the contiguous (B, m_dev) float64 sigma_u rows with zeros on the padding controls (m_dev: the device's number of
    controls, default m); sigma_u: scalar, (m,) or (B, m).  ValueError - decided here, before anything reaches the library - for a K
    that is no integer >= 1 or does not divide B, a hold that is no integer in [1, 2^31), a seed that is no integer in [0, 2^53), a
    round that is no integer in [0, 2^32), any other shape of sigma_u and a negative, NaN or infinite entry in it."""
    K = integer(K, what, "K", 1, 1 << 31, "in [1, 2^31)")
    if B % K != 0:
        raise ValueError(f"{what}: K must divide the batch: {B} problems are no whole number of groups of {K}")
    seed = integer(seed, what, "seed", 0, 1 << 53, "in [0, 2^53)")
    round = integer(round, what, "round", 0, 1 << 32, "in [0, 2^32)")   # noqa: A001
    hold = integer(hold, what, "hold", 1, 1 << 31, "in [1, 2^31)")
    if sigma_u is None:
        return K, None, seed, round, hold
    sigma = rows(sigma_u, what, "sigma_u", B, m, scalar=True, nonneg=" (standard deviations)", pad=m if m_dev is None else int(m_dev))
    return K, sigma, seed, round, hold


def check_mppi_args(S, iterations, B, m, N, sigma_u, temperature, seed=0, first_sample=0, hold=1, shift=0, m_dev=None, what="MPPIRun"):
    """The sampling-based MPC arguments -> (S, iterations, rows, temperature, seed, first_sample, hold, shift): the integers as ints,
    rows the contiguous (B, m_dev) float64 sigma_u rows with zeros on the padding controls (sigma_u: scalar, (m,) or (B, m)).
    ValueError - decided here, before anything reaches the library - for an S that is no integer in [1, 2^31 - 64], an iterations or hold that is no integer in [1, 2^31), a
    seed that is no integer in [0, 2^53), a first_sample that is no integer in [0, 2^32), first_sample + iterations S > 2^32, a shift
    that is no integer in [0, N - 2], a temperature that is no number >= 0 (NaN included), a missing sigma_u, any other shape of it
    and a negative, NaN or infinite entry in it."""
    S = integer(S, what, "S", 1, (1 << 31) - 63, "in [1, 2^31 - 64]")
    iterations = integer(iterations, what, "iterations", 1, 1 << 31, "in [1, 2^31)")
    if sigma_u is None:
        raise ValueError(f"{what}: sigma_u is required")
    _, sigma, seed, _, hold = check_seed_args(1, B, m, sigma_u, seed, 0, hold, m_dev, what)
    first_sample = integer(first_sample, what, "first_sample", 0, 1 << 32, "in [0, 2^32)")
    if first_sample + iterations * S > 1 << 32:
        raise ValueError(f"{what}: first_sample + iterations S must not exceed 2^32 (iteration i draws samples first_sample + i S ..)")
    shift = integer(shift, what, "shift", 0, N - 1, f"in [0, {N - 2}]")
    ok = not isinstance(temperature, _BOOL) and isinstance(temperature, _INT + _FLOAT)
    if not ok or not temperature >= 0.0:
        raise ValueError(f"{what}: temperature must be a number >= 0 (0: the best sample alone); got {temperature!r}")
    return S, iterations, sigma, float(temperature), seed, first_sample, hold, shift


def check_fit_args(x, u, x_next, B, n, m, n_params, *, free, params0, count=None, weights=None, damping=1e-3, bounds=None, iterations=20,
                   ftol=1e-12, fd_rel=1e-6, fd_floor=1e-8, apply=False, m_dev=None, what="FitModelParameters"):
    """The parameter-identification arguments -> (data, wrows, start, brows, run): data the contiguous (B, T, 2 n + m_dev) float64 rows
    x | u | x_next with zeros on the padding controls and in the rows past a problem's count (MI_F_FIT_DATA), wrows the (B, n + 1)
    rows w | count, start the (B, n_params + 1) rows theta0 | mu0, brows None or the (2, n_params) rows lower | upper, run the
    float64 vector iterations | ftol | fd_rel | fd_floor | apply | P | free.. (MI_F_FIT_RUN).  x, x_next: (B, T, n), u: (B, T, m),
    T >= 1; free: strictly increasing indices below n_params, between 1 and 8 of them; count: None - T - or (B,) integers in
    [0, T]; weights: None - ones - or (n,) / (B, n), >= 0; params0: (B, n_params) or (n_params,) (the caller resolves None to the
    rows the solver holds); damping: a scalar or (B,), > 0; bounds: None or a pair (lo, hi), each None or (n_params,), +-inf allowed.
    ValueError - decided here, before anything reaches the library - for a model without parameters, any other rank or shape, a
    NaN or an infinity in a row a problem uses, in weights, params0 or damping, a NaN in bounds or lo > hi, a free list that is
    empty, too long, not increasing or out of range, a count outside [0, T], an iterations that is no integer in [0, 2^20], an ftol
    that is no number >= 0, an fd_rel or fd_floor that is no number > 0, an apply that is no bool."""
    who = what
    if n_params == 0:
        raise ValueError(f"{who}: this model has no parameters")
    arrs = []
    T = None
    for name, v, k in (("x", x, n), ("u", u, m), ("x_next", x_next, n)):
        a = numbers(v, who, name)
        if a.ndim != 3 or a.shape[0] != B or a.shape[2] != k or a.shape[1] < 1 or (T is not None and a.shape[1] != T):
            raise ValueError(f"{who}: {name} must be ({B}, {'T' if T is None else T}, {k}) with T >= 1; got {a.shape}")
        T = a.shape[1]
        arrs.append(a)
    try:
        free = list(free)
    except TypeError:
        raise ValueError(f"{who}: free must be a list of parameter indices; got {free!r}") from None
    if not 1 <= len(free) <= _capi.FIT_MAX_FREE:
        raise ValueError(f"{who}: free must hold between 1 and {_capi.FIT_MAX_FREE} parameter indices; got {len(free)}")
    free = [integer(v, who, f"free[{i}]", 0, n_params, f"in [0, {n_params - 1}]") for i, v in enumerate(free)]
    if any(b_ <= a_ for a_, b_ in zip(free, free[1:])):
        raise ValueError(f"{who}: free must be strictly increasing; got {free}")
    if count is None:
        cnt = np.full(B, T, dtype=np.int64)
    else:
        c = numbers(count, who, "count")
        if c.shape != (B,) or not np.isfinite(c).all() or (c != np.floor(c)).any() or (c < 0).any() or (c > T).any():
            raise ValueError(f"{who}: count must be ({B},) integers in [0, {T}]; got {count!r}")
        cnt = c.astype(np.int64)
    used = np.arange(T)[None, :] < cnt[:, None]
    for name, a in zip(("x", "u", "x_next"), arrs):
        if not np.isfinite(a[used]).all():
            raise ValueError(f"{who}: NaN or infinity in {name}")
    md = m if m_dev is None else int(m_dev)
    data = np.zeros((B, T, 2 * n + md))
    data[:, :, :n], data[:, :, n:n + m], data[:, :, n + md:] = arrs
    data[~used] = 0.0
    wrows = np.empty((B, n + 1))
    wrows[:, :n] = 1.0 if weights is None else rows(weights, who, "weights", B, n, nonneg="")
    wrows[:, n] = cnt
    start = np.empty((B, n_params + 1))
    if params0 is None:
        raise ValueError(f"{who}: params0 is required")
    start[:, :n_params] = rows(params0, who, "params0", B, n_params, b_first=True)
    d = numbers(damping, who, "damping")
    if d.shape not in ((), (B,)) or not np.isfinite(d).all() or not (d > 0.0).all():
        raise ValueError(f"{who}: damping must be a scalar or ({B},), finite and > 0; got {damping!r}")
    start[:, n_params] = d
    brows = None
    if bounds is not None:
        if not isinstance(bounds, (tuple, list)) or len(bounds) != 2:
            raise ValueError(f"{who}: bounds must be a pair (lo, hi)")
        brows = np.empty((2, n_params))
        for j, (name, v, dflt) in enumerate((("bounds lo", bounds[0], -np.inf), ("bounds hi", bounds[1], np.inf))):
            if v is None:
                brows[j] = dflt
                continue
            a = numbers(v, who, name)
            if a.shape != (n_params,):
                raise ValueError(f"{who}: {name} must be ({n_params},); got {a.shape}")
            if np.isnan(a).any():
                raise ValueError(f"{who}: NaN in {name}")
            brows[j] = a
        if (brows[0] > brows[1]).any():
            raise ValueError(f"{who}: bounds has lo > hi")
    iterations = integer(iterations, who, "iterations", 0, (1 << 20) + 1, "in [0, 2^20]")
    nums = {}
    for name, v, strict in (("ftol", ftol, False), ("fd_rel", fd_rel, True), ("fd_floor", fd_floor, True)):
        ok = not isinstance(v, _BOOL) and isinstance(v, _INT + _FLOAT) and np.isfinite(v) and (v > 0.0 if strict else v >= 0.0)
        if not ok:
            raise ValueError(f"{who}: {name} must be a finite number {'> 0' if strict else '>= 0'}; got {v!r}")
        nums[name] = float(v)
    apply = flag(apply, who, "apply")   # noqa: A001
    run = np.array([iterations, nums["ftol"], nums["fd_rel"], nums["fd_floor"], 1.0 if apply else 0.0, len(free)] + free, dtype=np.float64)
    return np.ascontiguousarray(data), wrows, start, brows, run
