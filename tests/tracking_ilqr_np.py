"""ORACLE for reference trajectories: oracle/ilqr_np.py's OracleILQR with a time-varying target (test infrastructure).

TrackingOracleILQR overrides the two stages that read x_nom - rollout and backward - and nothing else: where OracleILQR uses
x_nom at time index t (t = 0 .. N-1, the terminal term included), this one uses r(t) = ref[min(clock + t, T - 1)], the reference
holding its last row past its end.  With a one-row reference every expression is OracleILQR's own, in its order: the results are
bitwise the same (tests/test_tracking_oracle.py).
"""
import numpy as np

from oracle.ilqr_np import OracleILQR


class TrackingOracleILQR(OracleILQR):
    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.ref = None          # (T, n), or None: the constant target x_nom
        self.clock = 0

    def set_reference(self, ref, clock=0):
        self.ref = None if ref is None else np.array(ref, float).reshape(-1, self.n)
        self.clock = int(clock)

    def r(self, t):
        if self.ref is None:
            return self.x_nom
        return self.ref[min(self.clock + t, len(self.ref) - 1)]

    def rollout(self, eps):
        """OracleILQR.rollout with x_nom -> r(t) (oracle/ilqr_np.py: the stage cost and the terminal term)."""
        n, m, N = self.n, self.m, self.N
        x = np.zeros((n, N))
        u = np.zeros((m, N - 1))
        x[:, 0] = self.x0
        L = 0.0
        expected = 0.0
        for t in range(N - 1):
            u[:, t] = self.u_bar[:, t] - eps * self.kappa[:, t] - self.K[:, :, t] @ (x[:, t] - self.x_bar[:, t])
            try:
                x[:, t + 1] = self.model.step(x[:, t], u[:, t])
            except RuntimeError:
                L = np.inf
                break
            dx = x[:, t] - self.r(t)
            L += dx @ self.Q @ dx + u[:, t] @ self.R @ u[:, t]
            expected += -eps * (1 - eps / 2) * self.dV[t]
        dx = x[:, -1] - self.r(N - 1)
        L += dx @ self.Qf @ dx
        return x, u, L, expected

    def backward(self):
        """OracleILQR.backward with x_nom -> r(t) (oracle/ilqr_np.py: the terminal Vx and lx_t)."""
        Q2, R2 = 2 * self.Q, 2 * self.R
        xT = self.x_bar[:, -1]
        Vx = 2 * self.Qf @ xT - 2 * self.r(self.N - 1) @ self.Qf
        Vxx = 2 * self.Qf
        for t in range(self.N - 2, -1, -1):
            x, u = self.x_bar[:, t], self.u_bar[:, t]
            fx, fu = self.fx[:, :, t], self.fu[:, :, t]
            lx = Q2 @ x - 2 * self.r(t) @ self.Q
            lu = R2 @ u
            Qx = lx + fx.T @ Vx
            Qu = lu + fu.T @ Vx
            Qxx = Q2 + fx.T @ Vxx @ fx
            Quu = R2 + fu.T @ Vxx @ fu
            Qux = fu.T @ Vxx @ fx
            Quu_inv = np.linalg.inv(Quu)
            self.kappa[:, t] = Quu_inv @ Qu
            self.K[:, :, t] = Quu_inv @ Qux
            self.dV[t] = Qu @ Quu_inv @ Qu
            Vx = Qx - Qu @ Quu_inv @ Qux
            Vxx = Qxx - Qux.T @ Quu_inv @ Qux
