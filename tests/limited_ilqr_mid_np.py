"""ORACLE of control-limited iLQR for any m (test infrastructure): tests/limited_ilqr_np.py's LimitedOracleILQR with the box QP of
the mid-size workgroup kernels (ilqr_large.hpp: box_qp_wave, mid_backward_limited), restated in NumPy.

Same semantics (include/mi_ilqr.h: mi_ilqr_set_control_limits); only the box QP generalises: projected Newton (Bertsekas 1982, the
"boxQP" of Tassa, Mansard & Todorov 2014) from clip(0, lo, hi), Cholesky factors of the free block, Armijo backtracking along the
projected path, a fixed iteration cap, then one exact solve on the final free set.  Quu is strictly convex, so the minimiser is
unique: for m <= 2 the result is tests/limited_ilqr_np.py's box_qp up to rounding.  The free rows of K are Quu_ff^-1 Qux_f.
"""
import numpy as np

try:
    from tests.limited_ilqr_np import LimitedOracleILQR, LinesearchFailed  # noqa: F401
except ImportError:                               # (tests/ itself on sys.path: the GPU tests)
    from limited_ilqr_np import LimitedOracleILQR, LinesearchFailed  # noqa: F401

BOX_ITERS, BOX_LS = 32, 40          # the kernels' kBoxIters, kBoxLs


def _chol(A):
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    return L if np.all(np.isfinite(L)) else None


def _free_solve(H, r, free):
    """y with y_f = H_ff^-1 r_f, y_c = 0."""
    y = np.zeros(len(r))
    if free.any():
        y[free] = np.linalg.solve(H[np.ix_(free, free)], r[free])
    return y


def box_qp(Quu, Qu, lo, hi):
    """argmin 1/2 d^T Quu d + Qu^T d on lo <= d <= hi for any m -> (d, clamped flags, pd)."""
    H = np.asarray(Quu, float)
    g0 = np.asarray(Qu, float)
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    m = len(g0)
    if not np.all(np.isfinite(H)) or _chol(H) is None:
        return np.zeros(m), [False] * m, False

    def clamped(x, g):
        return (lo == hi) | ((x <= lo) & (g > 0)) | ((x >= hi) & (g < 0))

    def newton(x, free):
        xn = x.copy()
        r = -(g0 + H[:, ~free] @ x[~free])
        xn[free] = _free_solve(H, r, free)[free]
        return xn

    def f(x):
        return x @ (0.5 * (H @ x) + g0)

    x = np.clip(0.0, lo, hi) * np.ones(m)
    prev, full = None, False
    for _ in range(BOX_ITERS):
        g = g0 + H @ x
        C = clamped(x, g)
        if (full and prev is not None and np.array_equal(C, prev)) or C.all():
            break
        xn = newton(x, ~C)
        prev = C
        if not (np.any(xn < lo) or np.any(xn > hi)):
            x, full = xn, True
            continue
        full = False
        d = xn - x
        f0, gd = f(x), g @ d
        step, found = 1.0, False
        for _ in range(BOX_LS):
            xt = np.clip(x + step * d, lo, hi)
            if f(xt) - f0 <= 0.1 * step * gd:
                found = True
                break
            step *= 0.6
        if not found:
            break
        x = xt
    g = g0 + H @ x
    C = clamped(x, g)
    x = newton(x, ~C)
    return x, [bool(c) for c in C], True


class LimitedMidOracleILQR(LimitedOracleILQR):
    """LimitedOracleILQR with the general box QP (any m) and K_f = Quu_ff^-1 Qux_f.  With nothing clamped the step is the
    reference's (OracleILQR.backward: np.linalg.inv)."""

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
            cl = np.array(cl)
            self.clamped[:, t] = cl
            if not cl.any():
                Qi = np.linalg.inv(Quu)
                self.kappa[:, t] = Qi @ Qu
                self.K[:, :, t] = Qi @ Qux
                self.dV[t] = Qu @ Qi @ Qu
                Vx = Qx - Qu @ Qi @ Qux
                Vxx = Qxx - Qux.T @ Qi @ Qux
                continue
            K = np.zeros((self.m, self.n))
            free = ~cl
            if free.any():
                K[free] = np.linalg.solve(Quu[np.ix_(free, free)], Qux[free])
            self.kappa[:, t] = kap
            self.K[:, :, t] = K
            self.dV[t] = kap @ Qu
            Vx = Qx - K.T @ Qu - Qux.T @ kap + K.T @ Quu @ kap
            Vxx = Qxx - K.T @ Qux - Qux.T @ K + K.T @ Quu @ K
        self.S2 = S2
        self.not_pd = not ok
        return ok
