"""ORACLE of control-limited iLQR (test infrastructure): oracle.ilqr_np.OracleILQR with box control limits.

The semantics of include/mi_ilqr.h: mi_ilqr_set_control_limits, restated in NumPy:
  rollout   u_t = clip(u_bar_t - eps kappa_t - K_t (x_t - x_bar_t), u_min, u_max) in every trial; the expected improvement is
            -(eps sum_t dV_t - eps^2 / 2 S2), S2 = sum_t kappa_t^T Quu_t kappa_t of the last backward pass;
  backward  per step the box QP  du* = argmin 1/2 du^T Quu du + Qu^T du,  u_min - u_bar_t <= du <= u_max - u_bar_t,
            kappa_t = -du*, clamped rows of K zero, free rows Quu_ff^-1 Qux_f, the general value update (the reference's
            arithmetic when nothing is clamped); a Quu that is not positive definite stops the solve (status NOT_PD).
"""
import math

import numpy as np

from oracle.ilqr_np import OracleILQR, LinesearchFailed  # noqa: F401


def _clip(v, lo, hi):
    """clip by comparisons, a NaN stays NaN (as the kernels do)."""
    v = np.where(v < lo, lo, v)
    return np.where(v > hi, hi, v)


def box_qp(Quu, Qu, lo, hi):
    """argmin 1/2 d^T Quu d + Qu^T d on lo <= d <= hi for m = 1, 2 -> (d, clamped flags, pd).  The construction of
    the kernels' box_qp_step: the unconstrained minimiser (explicit inverse) if inside, else the best edge in the order
    u0 = lo0, u0 = hi0, u1 = lo1, u1 = hi1 (infinite edges skipped), ties to the earlier edge."""
    m = len(Qu)
    Quu = np.asarray(Quu, float)
    if m == 1:
        pd = bool(Quu[0, 0] > 0 and np.isfinite(Quu[0, 0]))
    else:
        det = Quu[0, 0] * Quu[1, 1] - Quu[0, 1] * Quu[1, 0]
        pd = bool(Quu[0, 0] > 0 and det > 0 and np.all(np.isfinite(Quu)) and np.isfinite(det))
    if not pd:
        return np.zeros(m), [False] * m, False
    Qi = _inv(Quu)
    d = -(Qi @ Qu)
    cl = [False] * m
    if m == 1:
        if d[0] < lo[0]:
            d[0], cl[0] = lo[0], True
        elif d[0] > hi[0]:
            d[0], cl[0] = hi[0], True
        return d, cl, True
    if not (d[0] < lo[0] or d[0] > hi[0] or d[1] < lo[1] or d[1] > hi[1]):
        return d, cl, True
    best = math.inf
    for e in range(4):
        fx, fr = e >> 1, 1 - (e >> 1)
        v = hi[fx] if e & 1 else lo[fx]
        if not np.isfinite(v):
            continue
        f = -(Qu[fr] + Quu[fr, fx] * v) / Quu[fr, fr]
        cf = False
        if f < lo[fr]:
            f, cf = lo[fr], True
        elif f > hi[fr]:
            f, cf = hi[fr], True
        c = np.zeros(2)
        c[fx], c[fr] = v, f
        obj = 0.5 * (c @ Quu @ c) + Qu @ c
        if obj < best:
            best = obj
            d = c
            cl = [False, False]
            cl[fx], cl[fr] = True, cf
    return d, cl, True


def _inv(A):
    """The kernels' closed-form inverse of an m <= 2 matrix (invert_small)."""
    if A.shape[0] == 1:
        return np.array([[1.0 / A[0, 0]]])
    idet = 1.0 / (A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0])
    return np.array([[A[1, 1] * idet, -A[0, 1] * idet], [-A[1, 0] * idet, A[0, 0] * idet]])


class LimitedOracleILQR(OracleILQR):
    """OracleILQR with box control limits u_min <= u <= u_max ((m,) arrays, +-inf allowed)."""

    def __init__(self, model, N, *args, u_min=None, u_max=None, **kw):
        super().__init__(model, N, *args, **kw)
        self.u_min = np.full(self.m, -np.inf) if u_min is None else np.asarray(u_min, float).reshape(self.m)
        self.u_max = np.full(self.m, np.inf) if u_max is None else np.asarray(u_max, float).reshape(self.m)
        self.S2 = 0.0
        self.clamped = np.zeros((self.m, self.N - 1), dtype=bool)
        self.not_pd = False

    def rollout(self, eps):
        n, m, N = self.n, self.m, self.N
        x = np.zeros((n, N))
        u = np.zeros((m, N - 1))
        x[:, 0] = self.x0
        L = 0.0
        sdv = 0.0
        for t in range(N - 1):
            v = self.u_bar[:, t] - eps * self.kappa[:, t] - self.K[:, :, t] @ (x[:, t] - self.x_bar[:, t])
            u[:, t] = _clip(v, self.u_min, self.u_max)
            try:
                x[:, t + 1] = self.model.step(x[:, t], u[:, t])
            except RuntimeError:
                L = np.inf
                break
            dx = x[:, t] - self.x_nom
            L += dx @ self.Q @ dx + u[:, t] @ self.R @ u[:, t]
            sdv += self.dV[t]
        dx = x[:, -1] - self.x_nom
        L += dx @ self.Qf @ dx
        return x, u, L, -(eps * sdv - 0.5 * eps * eps * self.S2)

    def backward(self):
        Q2, R2 = 2 * self.Q, 2 * self.R
        xT = self.x_bar[:, -1]
        Vx = 2 * self.Qf @ xT - 2 * self.x_nom @ self.Qf
        Vxx = 2 * self.Qf
        S2 = 0.0
        ok = True
        for t in range(self.N - 2, -1, -1):
            x, u = self.x_bar[:, t], self.u_bar[:, t]
            fx, fu = self.fx[:, :, t], self.fu[:, :, t]
            lx = Q2 @ x - 2 * self.x_nom @ self.Q
            lu = R2 @ u
            Qx = lx + fx.T @ Vx
            Qu = lu + fu.T @ Vx
            Qxx = Q2 + fx.T @ Vxx @ fx
            Quu = R2 + fu.T @ Vxx @ fu
            Qux = fu.T @ Vxx @ fx
            d, cl, pd = box_qp(Quu, Qu, self.u_min - u, self.u_max - u)
            ok = ok and pd
            kap = -d
            S2 += kap @ Quu @ kap
            self.clamped[:, t] = cl
            if not any(cl):
                Qi = _inv(Quu)
                self.kappa[:, t] = Qi @ Qu
                self.K[:, :, t] = Qi @ Qux
                self.dV[t] = Qu @ Qi @ Qu
                Vx = Qx - Qu @ Qi @ Qux
                Vxx = Qxx - Qux.T @ Qi @ Qux
                continue
            K = np.zeros((self.m, self.n))
            for a in range(self.m):
                if not cl[a]:
                    K[a] = Qux[a] / Quu[a, a]
            self.kappa[:, t] = kap
            self.K[:, :, t] = K
            self.dV[t] = kap @ Qu
            Vx = Qx - K.T @ Qu - Qux.T @ kap + K.T @ Quu @ kap
            Vxx = Qxx - K.T @ Qux - Qux.T @ K + K.T @ Quu @ K
        self.S2 = S2
        self.not_pd = not ok
        return ok

    def solve(self):
        """OracleILQR.solve with the stop at a Quu that is not positive definite (self.not_pd)."""
        L = math.inf
        improvement = math.inf
        hist = []
        while improvement > self.delta and len(hist) < self.max_iters:
            L_new, eps, trials = self.forward(L)
            ok = self.backward()
            hist.append((L_new, eps, trials, self.percentage_derivs))
            improvement = L - L_new
            L = L_new
            if not ok:
                break
        return self.x_bar, self.u_bar, L, hist
