"""What the calls of the front end (ilqr.py) return: plain holders of NumPy arrays, built from the rows the C ABI's selectors hand
back (include/mi_ilqr.h names the columns), with the statistics that are derived on the host - variances, survival, Chan's merge
of two windows of samples.  NumPy only: nothing here knows the library.
"""
import numpy as np


class PolicySamples:
    """The samples of a RolloutPolicyStats(..., samples=True) call: x0 (B, S, n), params (B, S, n_params) - None when the parameters
    were not sampled -, cost (B, S) and steps (B, S) int32: what RolloutPolicy takes and returns for the same samples."""
    __slots__ = ("x0", "params", "cost", "steps")

    def __init__(self, x0, params, cost, steps):
        self.x0, self.params, self.cost, self.steps = x0, params, cost, steps


class MPPIResult:
    """What MPPIRun did (include/mi_ilqr.h: "Sampling-based MPC"): u (B, m, N-1) the final nominal plans, unshifted; per iteration and
    problem, (I, B): best_sample - the sample of least finite cost, -1 when none was finite -, best_cost (+inf then), finite - the
    number of samples with a finite cost - and ess, the effective sample size 1 / sum w^2 (NaN without a finite sample);
    nominal_cost (I + 1, B): the nominal's own cost at the start of every iteration and, row I, of the final nominal; kernel_ms: the
    run's kernels, first to last."""
    __slots__ = ("u", "best_sample", "best_cost", "finite", "ess", "nominal_cost", "kernel_ms")

    def __init__(self, u, best_sample, best_cost, finite, ess, nominal_cost, kernel_ms):
        self.u, self.best_sample, self.best_cost, self.finite = u, best_sample, best_cost, finite
        self.ess, self.nominal_cost, self.kernel_ms = ess, nominal_cost, kernel_ms

    @classmethod
    def from_rows(cls, u, best, cost, kernel_ms):
        """best (I, B, 3) and cost (I + 1, B, 2) as MI_F_SEEDS_BEST / MI_F_SEEDS_COST return them."""
        return cls(u, best[:, :, 0].astype(np.int64), np.ascontiguousarray(best[:, :, 1]), best[:, :, 2].astype(np.int64),
                   np.ascontiguousarray(cost[:-1, :, 1]), np.ascontiguousarray(cost[:, :, 0]), kernel_ms)

    def __repr__(self):
        return f"MPPIResult(iterations={self.best_cost.shape[0]}, nominal_cost[-1]={self.nominal_cost[-1].tolist()})"


class ParamFit:
    """What FitModelParameters found (include/mi_ilqr.h: "Parameter identification"): params (B, n_params) - the rows
    SetModelParameters takes -; cost0, cost (B,): the weighted squared one-step prediction error at the start and at params; damping
    (B,): the Levenberg-Marquardt mu to carry into a following call; iterations - trials made -, accepted, status (FIT_CONVERGED /
    FIT_MAX_ITERS / FIT_STALLED / FIT_BAD_DATA of _capi) and count - the rows each problem used -, (B,) integers; gradient (B, P) and
    normal_matrix (B, P, P): g = sum J' W r and H = sum J' W J at params, over the free parameters in the order of `free`;
    kernel_ms: the run's kernels, first to last.  inv(normal_matrix) cost / (count n - P) is the usual covariance estimate of the
    fitted entries; it is the caller's to form."""
    __slots__ = ("params", "cost0", "cost", "damping", "iterations", "accepted", "status", "count", "gradient", "normal_matrix", "kernel_ms")

    def __init__(self, params, cost0, cost, damping, iterations, accepted, status, count, gradient, normal_matrix, kernel_ms):
        self.params, self.cost0, self.cost, self.damping = params, cost0, cost, damping
        self.iterations, self.accepted, self.status, self.count = iterations, accepted, status, count
        self.gradient, self.normal_matrix, self.kernel_ms = gradient, normal_matrix, kernel_ms

    @classmethod
    def from_rows(cls, result, normal, n_params, P, kernel_ms):
        """result (B, n_params + 7) and normal (B, P + P P) as MI_F_FIT_RESULT / MI_F_FIT_NORMAL return them."""
        col = lambda k: np.ascontiguousarray(result[:, n_params + k])   # noqa: E731
        icol = lambda k: result[:, n_params + k].astype(np.int64)   # noqa: E731
        return cls(np.ascontiguousarray(result[:, :n_params]), col(0), col(1), col(2), icol(3), icol(4), icol(5), icol(6),
                   np.ascontiguousarray(normal[:, :P]), np.ascontiguousarray(normal[:, P:]).reshape(-1, P, P), kernel_ms)

    def _without_batch_axis(self):
        return ParamFit(*(getattr(self, k)[0] for k in self.__slots__[:-1]), self.kernel_ms)

    def __repr__(self):
        return f"ParamFit(status={np.asarray(self.status).tolist()}, cost={np.asarray(self.cost).tolist()})"


class SeedSelection:
    """What SelectBest found in every group of K seeds (include/mi_ilqr.h: "Multi-start"), (G,) arrays: winner - the member index of
    the eligible member of least cost, -1 when no member is eligible -, its cost (+inf then) and the number of eligible members."""
    __slots__ = ("K", "winner", "cost", "eligible")

    def __init__(self, K, winner, cost, eligible):
        self.K, self.winner, self.cost, self.eligible = K, winner, cost, eligible

    @classmethod
    def from_rows(cls, K, rows):
        return cls(int(K), rows[:, 0].astype(np.int64), np.ascontiguousarray(rows[:, 1]), rows[:, 2].astype(np.int64))

    @property
    def problem(self):
        """(G,) the winners as problem numbers g K + winner; -1 for a group without a winner."""
        g = np.arange(self.winner.size) * self.K
        return np.where(self.winner >= 0, g + self.winner, -1)

    def __repr__(self):
        return f"SeedSelection(K={self.K}, winner={self.winner.tolist()}, eligible={self.eligible.tolist()})"


def _chan(nA, meanA, m2A, nB, meanB, m2B):
    """include/mi_ilqr.h's merge of (count, mean, M2), A the operand of the lower sample numbers; a count-0 side leaves the other's."""
    fA, fB = nA.astype(np.float64), nB.astype(np.float64)
    n = fA + fB
    with np.errstate(invalid="ignore", divide="ignore"):
        delta = meanB - meanA
        mean = meanA + delta * (fB / n)
        m2 = (m2A + m2B) + (delta * delta) * ((fA * fB) / n)
    return (np.where(fB == 0, meanA, np.where(fA == 0, meanB, mean)), np.where(fB == 0, m2A, np.where(fA == 0, m2B, m2)))


class PolicyEnvelope:
    """Per-step statistics over the samples of a RolloutPolicyStats(..., envelope=True / controls=True) call, arrays (B, N, n) - for
    the controls (B, N-1, m): count, the samples that held a finite value at that step (a sample that ended leaves its later
    steps out); mean, m2 (the sum of squared deviations), min, max over those; argmin / argmax the global sample numbers of min /
    max (-1 where count is 0, and there mean = m2 = NaN, min = +inf, max = -inf)."""
    __slots__ = ("count", "mean", "m2", "min", "max", "argmin", "argmax")

    def __init__(self, count, mean, m2, min, max, argmin, argmax):   # noqa: A002
        self.count, self.mean, self.m2, self.min, self.max, self.argmin, self.argmax = count, mean, m2, min, max, argmin, argmax

    @classmethod
    def from_raw(cls, raw):
        """raw (..., 8): the accumulators count | K | s1 | s2 | min | max | argmin | argmax of MI_F_POLICY_MC_ENVELOPE, finalised by
        the header's formulas mean = K + s1 / count, M2 = max(0, s2 - s1 s1 / count)."""
        cnt, K, s1, s2 = (raw[..., k] for k in range(4))
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = K + s1 / cnt
            m2 = np.maximum(0.0, s2 - s1 * s1 / cnt)
        empty = cnt == 0
        return cls(cnt.astype(np.int64), np.where(empty, np.nan, mean), np.where(empty, np.nan, m2), raw[..., 4].copy(), raw[..., 5].copy(),
                   raw[..., 6].astype(np.int64), raw[..., 7].astype(np.int64))

    @property
    def var(self):
        """The sample variance, m2 / (count - 1); NaN with fewer than two values."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.count > 1, self.m2 / (self.count - 1), np.nan)

    def merge(self, other):
        """The envelope of self's samples and those of a DISJOINT, LATER window (other): counts add, extrema by comparison with ties
        to self - exact -, mean and m2 by Chan's merge - correct to round-off, not the bits of one call."""
        mean, m2 = _chan(self.count, self.mean, self.m2, other.count, other.mean, other.m2)
        lo, hi = other.min < self.min, other.max > self.max
        return PolicyEnvelope(self.count + other.count, mean, m2, np.where(lo, other.min, self.min), np.where(hi, other.max, self.max),
                              np.where(lo, other.argmin, self.argmin), np.where(hi, other.argmax, self.argmax))


class PolicySafety:
    """The safety box of a RolloutPolicyStats(..., safe_box=(lo, hi)) call: of n samples per problem `ran` held finite states at all
    N steps, `safe` of those never left the box and `safe_success` of those also ended within `goal` of the target, (B,) each;
    exits (B, N): the samples whose FIRST state outside the box is x_t (the box only observes: a sample goes on)."""
    __slots__ = ("n", "ran", "safe", "safe_success", "exits")

    def __init__(self, n, ran, safe, safe_success, exits):
        self.n, self.ran, self.safe, self.safe_success, self.exits = n, ran, safe, safe_success, exits

    @classmethod
    def from_rows(cls, n, rows):
        """rows: the (B, 3 + N) array of MI_F_POLICY_MC_SAFETY."""
        r = rows.astype(np.int64)
        return cls(np.asarray(n, dtype=np.int64), r[:, 0], r[:, 1], r[:, 2], r[:, 3:])

    @property
    def survival(self):
        """(B, N): the share of the samples that have not left the box up to and including step t, 1 - cumsum(exits) / n."""
        return 1.0 - np.cumsum(self.exits, axis=-1) / np.asarray(self.n)[..., None]

    def merge(self, other):
        """Integer counters: they add, exactly."""
        return PolicySafety(self.n + other.n, self.ran + other.ran, self.safe + other.safe, self.safe_success + other.safe_success,
                            self.exits + other.exits)


class PolicyStats:
    """What RolloutPolicyStats returns, (B,) arrays: n samples, of which `counted` ran to the end with a finite cost and `success`
    also ended within `goal` of the target; mean, m2 (the sum of squared deviations), min, max over the counted samples; argmin /
    argmax the global sample numbers of min / max (-1 without a counted sample); steps_total the steps of all n samples.
    samples: None or a PolicySamples.  envelope, control_envelope: None or a PolicyEnvelope; safety: None or a PolicySafety."""
    __slots__ = ("n", "counted", "success", "mean", "m2", "min", "max", "argmin", "argmax", "steps_total", "samples", "envelope",
                 "control_envelope", "safety")

    def __init__(self, n, counted, success, mean, m2, min, max, argmin, argmax, steps_total, samples=None, envelope=None,   # noqa: A002
                 control_envelope=None, safety=None):
        self.n, self.counted, self.success, self.mean, self.m2 = n, counted, success, mean, m2
        self.min, self.max, self.argmin, self.argmax, self.steps_total, self.samples = min, max, argmin, argmax, steps_total, samples
        self.envelope, self.control_envelope, self.safety = envelope, control_envelope, safety

    @classmethod
    def from_rows(cls, rows, samples=None):
        """rows: the (B, 10) array of MI_F_POLICY_MC_STATS."""
        i = lambda k: rows[:, k].astype(np.int64)   # noqa: E731
        return cls(i(0), i(1), i(2), rows[:, 3].copy(), rows[:, 4].copy(), rows[:, 5].copy(), rows[:, 6].copy(), i(7), i(8), i(9), samples)

    @property
    def var(self):
        """The sample variance of the counted costs, m2 / (counted - 1); NaN with fewer than two."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.counted > 1, self.m2 / (self.counted - 1), np.nan)

    @property
    def success_rate(self):
        return self.success / self.n

    def merge(self, other):
        """Chan's merge with the result of a DISJOINT, LATER window of samples (first_sample): how a sample set split over calls or
        ranks is put together.  self is operand A of include/mi_ilqr.h's merge; a side without a counted sample leaves the other's
        numbers as they are; ties of min / max keep self's sample.  envelope, control_envelope and safety are joined too where both
        sides hold them (else None): their counts, exits, extrema and argmin / argmax exactly, their mean / m2 correct to round-off
        (Chan's merge of two finalised halves is not the one left fold's bits)."""
        both = lambda k: None if getattr(self, k) is None or getattr(other, k) is None else getattr(self, k).merge(getattr(other, k))   # noqa: E731
        mean, m2 = _chan(self.counted, self.mean, self.m2, other.counted, other.mean, other.m2)
        lo, hi = other.min < self.min, other.max > self.max
        return PolicyStats(self.n + other.n, self.counted + other.counted, self.success + other.success, mean, m2,
                           np.where(lo, other.min, self.min), np.where(hi, other.max, self.max), np.where(lo, other.argmin, self.argmin),
                           np.where(hi, other.argmax, self.argmax), self.steps_total + other.steps_total, None, both("envelope"),
                           both("control_envelope"), both("safety"))


class PlantLog:
    """The closed loop's record (plant_log), K = num_resolves * replan_steps steps of the last MPCRun on a solver that holds a plant:
    X (B, n, K+1) - the state at every step, the plant's current state last -, U (B, m, K) the commanded controls, stage_cost (B, K)
    the l_k and steps (B,) the steps each plant completed in that run; NaN where a plant that ended did not get to (its X keeps
    the state it stopped in, in column `steps` and - the current state - in the last one)."""
    __slots__ = ("X", "U", "stage_cost", "steps")

    def __init__(self, X, U, stage_cost, steps):
        self.X, self.U, self.stage_cost, self.steps = X, U, stage_cost, steps

    def _without_batch_axis(self):
        return PlantLog(*(a[0] for a in (self.X, self.U, self.stage_cost, self.steps)))


class PolicyRollout:
    """What RolloutPolicy returns: cost, x_final, steps and - asked for - the trajectories X, U (else None)."""
    __slots__ = ("cost", "x_final", "steps", "X", "U")

    def __init__(self, cost, x_final, steps, X=None, U=None):
        self.cost, self.x_final, self.steps, self.X, self.U = cost, x_final, steps, X, U

    def _without_batch_axis(self):
        return PolicyRollout(*(None if a is None else a[0] for a in (self.cost, self.x_final, self.steps, self.X, self.U)))
