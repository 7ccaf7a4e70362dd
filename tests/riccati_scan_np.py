"""NumPy statement of the time-parallel backward pass of the wave-per-problem kernels (csrc/ilqr_small.hpp: backward_scan), and
the inputs of the small-state backward tests (test_riccati_scan_oracle.py on the CPU, test_gpu_small_backward.py on the device).

The scan: step t's second-order expansion is an element a_t = (A, b, C, eta, J) = (fx_t, -fu_t luu^-1 lu_t, fu_t luu^-1 fu_t^T,
-lx_t, lxx), the terminal one (0, 0, 0, -lf_x, lf_xx), elements compose by
    a_i (x) a_j:  M = (I + C_i J_j)^-1, W = A_j M, V = (M A_i)^T,
                  A = W A_i, b = W (b_i + C_i eta_j) + b_j, C = W C_i A_j^T + C_j, eta = V (eta_j - J_j b_i) + eta_i, J = V J_j A_i + J_i
and (Vxx, Vx) at step t is (J, -eta) of a_t (x) ... (x) a_{N-1}.  The device deals chunks of ceil(N / 64) consecutive elements to
its 64 lanes in reverse time order, composes each chunk, runs an inclusive Kogge-Stone scan over the lanes (four shifts inside the
16-lane rows, then two row broadcasts) and finally the reference recursion over each chunk from the scan's value at its right edge.
Same elements, same composition, same chunking and scan order here; P = I + C_i J_j is inverted the way the device does it
(n = 2: adjugate / determinant, n > 2: Gauss-Jordan without pivoting) or with np.linalg.inv."""
import functools

import numpy as np

LANES = 64


def gj_unpivoted(P):
    """(P^-1, smallest |pivot|) by Gauss-Jordan without row exchanges (ilqr_small.hpp: ric_invert, n > 2)."""
    n = P.shape[0]
    a, Mi, piv = P.copy(), np.eye(n), np.inf
    for k in range(n):
        piv = min(piv, abs(a[k, k]))
        ip = 1.0 / a[k, k]
        a[k] *= ip; Mi[k] *= ip
        for i in range(n):
            if i != k:
                f = a[i, k]
                a[i] -= f * a[k]; Mi[i] -= f * Mi[k]
    return Mi, piv


class Scan:
    """One backward pass of an OracleILQR's current x_bar / u_bar / fx / fu, the scan's way.  After run(): K (m, n, N-1),
    kappa (m, N-1), dV (N-1), min_pivot (smallest unpivoted Gauss-Jordan pivot of any P), cond_P (largest cond(P)) and the two
    quantities the device's guard looks at (backward_scan, phase (4)).  gain_gap, n > 2: every lane that started its recursion
    from the scan's value computes the gain K of its first step once more from the Vxx its neighbour's recursion arrives at; the
    largest difference from the gain it wrote, relative to the largest such gain over the lanes.  edge_gap, n = 2: the largest
    relative disagreement (upper triangle, max-norm) between the Vxx a lane's recursion reaches at the left edge of its chunk and
    the scan's own J there."""
    GAIN_TOL = 2e-12                                             # ilqr_small.hpp: kScanGainTol
    EDGE_TOL = 1e-10                                             # ilqr_small.hpp: kScanEdgeTol

    def __init__(self, o, invert="device"):
        assert o.m == 1, "rank-one control term: C = fu luu^-1 fu^T with scalar luu"
        self.o, self.invert = o, invert
        self.min_pivot, self.cond_P = np.inf, 0.0

    # -- elements
    def identity(self):
        n = self.o.n
        return (np.eye(n), np.zeros(n), np.zeros((n, n)), np.zeros(n), np.zeros((n, n)))

    def element(self, t):
        o, n, N = self.o, self.o.n, self.o.N
        if t >= N:
            return self.identity()
        if t == N - 1:
            lfx = 2 * o.Qf @ o.x_bar[:, -1] - 2 * o.x_nom @ o.Qf
            return (np.zeros((n, n)), np.zeros(n), np.zeros((n, n)), -lfx, 2 * o.Qf)
        fx, fu = o.fx[:, :, t], o.fu[:, 0, t]
        r2i = 1.0 / (2 * o.R[0, 0])
        lx = 2 * o.Q @ o.x_bar[:, t] - 2 * o.x_nom @ o.Q
        return (fx.copy(), -fu * o.u_bar[0, t], np.outer(fu * r2i, fu), -lx, 2 * o.Q)

    def inverse(self, P):
        n = P.shape[0]
        self.cond_P = max(self.cond_P, float(np.linalg.cond(P)))
        Mi, piv = gj_unpivoted(P)
        if n > 2:
            self.min_pivot = min(self.min_pivot, piv)
        if self.invert == "inv":
            return np.linalg.inv(P)
        if n == 2:
            idet = 1.0 / (P[0, 0] * P[1, 1] - P[0, 1] * P[1, 0])
            return np.array([[P[1, 1], -P[0, 1]], [-P[1, 0], P[0, 0]]]) * idet
        return Mi

    def combine(self, ei, ej):
        """ei (x) ej, ei earlier in time (ilqr_small.hpp: ric_combine; C and J are mirrored from their upper triangles there)."""
        Ai, bi, Ci, ei_, Ji = ei
        Aj, bj, Cj, ej_, Jj = ej
        n = Ai.shape[0]
        Mi = self.inverse(np.eye(n) + Ci @ Jj)
        W, MA = Aj @ Mi, Mi @ Ai
        C = W @ Ci @ Aj.T + Cj
        J = MA.T @ Jj @ Ai + Ji
        C, J = np.triu(C) + np.triu(C, 1).T, np.triu(J) + np.triu(J, 1).T
        return (W @ Ai, W @ (bi + Ci @ ej_) + bj, C, MA.T @ (ej_ - Jj @ bi) + ei_, J)

    # -- the pass
    def run(self):
        o = self.o
        n, m, N = o.n, o.m, o.N
        chunk = (N + LANES - 1) // LANES
        e0 = [(LANES - 1 - l) * chunk for l in range(LANES)]
        S = []
        for l in range(LANES):
            if e0[l] >= N:
                S.append(self.identity())
                continue
            s = self.element(e0[l])
            for k in range(1, chunk):
                s = self.combine(s, self.element(e0[l] + k))
            S.append(s)
        ident = self.identity()
        for d in (1, 2, 4, 8):                                   # row_shr:d - inside the 16-lane rows
            S = [self.combine(S[l], S[l - d] if l % 16 >= d else ident) for l in range(LANES)]
        S = [self.combine(S[l], S[(l // 16) * 16 - 1] if (l // 16) in (1, 3) else ident) for l in range(LANES)]   # row_bcast:15
        S = [self.combine(S[l], S[31] if l >= 32 else ident) for l in range(LANES)]                                # row_bcast:31
        self.K = np.zeros((m, n, N - 1)); self.kappa = np.zeros((m, N - 1)); self.dV = np.zeros(N - 1)
        Q2, R2 = 2 * o.Q, 2 * o.R
        recursed, self.edge_gap = [], 0.0
        for l in range(LANES):
            t_hi = e0[l] + chunk - 1
            if t_hi >= N - 1:
                t_hi = N - 2
                Vx = 2 * o.Qf @ o.x_bar[:, -1] - 2 * o.x_nom @ o.Qf
                Vxx = 2 * o.Qf
            else:
                Vx, Vxx = -S[l - 1][3], S[l - 1][4]
            for t in range(t_hi, e0[l] - 1, -1):
                x, u, fx, fu = o.x_bar[:, t], o.u_bar[:, t], o.fx[:, :, t], o.fu[:, :, t]
                lx, lu = Q2 @ x - 2 * o.x_nom @ o.Q, R2 @ u
                Qx, Qu = lx + fx.T @ Vx, lu + fu.T @ Vx
                Qxx, Quu, Qux = Q2 + fx.T @ Vxx @ fx, R2 + fu.T @ Vxx @ fu, fu.T @ Vxx @ fx
                Qi = np.linalg.inv(Quu)
                self.kappa[:, t] = Qi @ Qu
                self.K[:, :, t] = Qi @ Qux
                self.dV[t] = Qu @ Qi @ Qu
                Vx = Qx - Qu @ Qi @ Qux
                Vxx = Qxx - Qux.T @ Qi @ Qux
            recursed.append(Vxx)
            if t_hi >= e0[l]:
                sJ, iu = S[l][4], np.triu_indices(n)
                self.edge_gap = max(self.edge_gap, float(np.abs(Vxx - sJ)[iu].max() / max(np.abs(sJ).max(), 1e-300)))
        d = s = 0.0
        for l in range(1, LANES):
            t1 = e0[l] + chunk - 1
            if t1 < N - 1:
                fx, fu, Vr = o.fx[:, :, t1], o.fu[:, 0, t1], recursed[l - 1]
                Bm = fu @ Vr
                Kr = (Bm @ fx) / (R2[0, 0] + Bm @ fu)
                d, s = max(d, float(np.abs(Kr - self.K[0, :, t1]).max())), max(s, float(np.abs(Kr).max()))
        self.gain_gap = d / s if s > 0 else 0.0
        return self

    def guard(self):
        """(the quantity the device's guard looks at for this n, its threshold)"""
        return (self.edge_gap, self.EDGE_TOL) if self.o.n == 2 else (self.gain_gap, self.GAIN_TOL)

    def fires(self):
        v, tol = self.guard()
        return not v <= tol


# ---------------------------------------------------------------------------------------------------------------------------
# Inputs of the small-state backward tests: B = 8 seeded problems per (model, N) - a random start, a random control guess, the
# oracle's own rollout and Jacobians (forward(inf)) - and the cost scalings of each.
# ---------------------------------------------------------------------------------------------------------------------------
B = 8


def problem(model, N):
    from drake_ddp_amd import workloads as W
    if model == "pendulum":
        return dict(W.pendulum_problem(), N=N)
    return {"acrobot": W.acrobot_problem, "cartpole": W.cartpole_problem, "cartpole_wall": W.cartpole_wall_problem}[model](N)


def _starts(model, rng):
    if model == "pendulum":
        return np.stack([rng.uniform(-np.pi, np.pi, B), rng.uniform(-1.0, 1.0, B)], axis=1), 0.2
    if model == "acrobot":
        return rng.uniform(-0.1, 0.1, (B, 4)), 0.2
    if model == "cartpole":
        x0 = np.zeros((B, 4)); x0[:, 0] = rng.uniform(-0.2, 0.2, B); x0[:, 1] = rng.uniform(-0.3, 0.3, B)
        return x0, 1.0
    x0 = np.zeros((B, 4)); x0[:, 1] = np.pi + 0.5 + rng.uniform(-0.2, 0.2, B)       # (the C4 starts: the pole falls into the wall)
    return x0, 1.0


SEEDS = {"pendulum": 11, "acrobot": 12, "cartpole": 13, "cartpole_wall": 14}


@functools.lru_cache(maxsize=None)
def trajectories(model, N):
    """(x0 (B, n), u_guess (B, 1, N-1), x_bar (B, n, N), fx (B, n, n, N-1), fu (B, n, 1, N-1)) of the committed seeds: the
    oracle's rollout of the guess and its forward-mode Jacobians along it.  They do not depend on the cost matrices."""
    from common import make_oracle
    prob = problem(model, N)
    rng = np.random.default_rng(SEEDS[model] * 1000 + N)
    x0, amp = _starts(model, rng)
    ug = rng.uniform(-amp, amp, (B, 1, N - 1))
    xs, fxs, fus = [], [], []
    for b in range(B):
        o = make_oracle(prob)
        o.set_problem(x0[b], prob["x_nom"], prob["Q"], prob["R"], prob["Qf"], ug[b])
        o.forward(np.inf)
        xs.append(o.x_bar.copy()); fxs.append(o.fx.copy()); fus.append(o.fu.copy())
    out = (x0, ug, np.stack(xs), np.stack(fxs), np.stack(fus))
    for a in out:
        a.setflags(write=False)
    return out


# label -> (R scale, Qf scale, dense Qf)
COSTS = {"own": (1.0, 1.0, False), "R1e-3": (1e-3, 1.0, False), "R1e-6": (1e-6, 1.0, False),
         "Qf100": (1.0, 100.0, False), "R1e-3_Qf100": (1e-3, 100.0, False), "R1e-6_Qf100": (1e-6, 100.0, False),
         "denseQf": (1.0, 1.0, True)}
COSTS_N2 = dict(COSTS, **{"R1e-9": (1e-9, 1.0, False), "R1e-9_Qf100": (1e-9, 100.0, False)})


def cost_labels(model):
    return list(COSTS_N2 if model == "pendulum" else COSTS)


def cost_matrices(prob, label):
    """(Q, R, Qf) of a scaling: the workload's Q, R x rs, Qf x qs; "denseQf": Qf rotated by a seeded orthogonal matrix, so that
    the terminal J is not diagonal (symmetric positive definite as before)."""
    rs, qs, dense = COSTS_N2[label]
    Qf = qs * prob["Qf"]
    if dense:
        n = Qf.shape[0]
        w = np.diag(Qf) * np.linspace(1.0, 0.25, n)              # (the workloads' Qf are diagonal; distinct eigenvalues)
        U, _ = np.linalg.qr(np.random.default_rng(5).standard_normal((n, n)))
        Qf = (U * w) @ U.T
        Qf = 0.5 * (Qf + Qf.T)
    return prob["Q"], rs * prob["R"], Qf


def asymmetric(Q):
    """Q made asymmetric by one ulp of its largest entry: outside the class of the fast backward forms, so the host picks the
    reference's recursion verbatim (mi_ilqr.hip: classify_cost)."""
    Q = np.array(Q, float)
    Q[0, 1] += np.spacing(np.abs(Q).max())
    return Q


def oracle_for(model, N, label, b, asym=False):
    """The NumPy oracle holding problem b's inputs under a cost scaling, backward() not yet run."""
    from common import make_oracle
    prob = problem(model, N)
    Q0, R, Qf = cost_matrices(prob, label)
    Q_ = asymmetric(Q0) if asym else Q0
    x0, ug, xb, fx, fu = trajectories(model, N)
    o = make_oracle(dict(prob, Q=Q_, R=R, Qf=Qf))
    o.set_problem(x0[b], prob["x_nom"], Q_, R, Qf, ug[b])
    o.x_bar, o.fx, o.fu = xb[b].copy(), fx[b].copy(), fu[b].copy()
    return o


@functools.lru_cache(maxsize=None)
def reference(model, N, label, asym=False):
    """Per problem of the case: (K, kappa, dV) of the extended-precision pass and the fp64 NumPy pass's distance from it, computed
    once and shared by every test on these inputs.  Returns (list of (Kx, kx, dx), e_ref (B,), cond(Quu) (B,))."""
    from common import backward_extended
    refs, e_ref, cond = [], np.zeros(B), np.zeros(B)
    for b in range(B):
        o = oracle_for(model, N, label, b, asym)
        o.backward()
        Kx, kx, dx, cond[b] = backward_extended(o)
        for r_, x_ in zip((o.K, o.kappa, o.dV), (Kx, kx, dx)):
            e_ref[b] = max(e_ref[b], float(np.max(np.abs(r_ - x_))) / float(np.max(np.abs(x_))))
        refs.append((Kx, kx, dx))
    return refs, e_ref, cond


def distance(dev, ref):
    """common.backward_errors' measure of (K, kappa, dV) against an extended-precision (Kx, kx, dx)."""
    return max(float(np.max(np.abs(d_ - x_))) / float(np.max(np.abs(x_))) for d_, x_ in zip(dev, ref))
