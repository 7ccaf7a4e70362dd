// What the wave-per-problem and the lane-per-problem kernels share about the cost and the small dense algebra: the cost constants
// of a problem in registers (Consts, with a Limited<M> model's bounds: LimitRegs), the stage and terminal cost, the m <= 2 inverse
// and the box-QP backward step.
#pragma once
#include <hip/hip_runtime.h>

#include "fastmath.hpp"       // fast_rcp
#include "model_traits.hpp"   // UsesLimits

namespace mi {

// The bounds of one problem, in registers for the whole launch (Limited<M> kernels; empty otherwise).
template <class M, bool = UsesLimits<M>::value>
struct LimitRegs {};
template <class M>
struct LimitRegs<M, true> {
  double umin[M::m], umax[M::m];
  __device__ inline void load_limits(const double* p) {      // p: this problem's (2, m) record
#pragma unroll
    for (int k = 0; k < M::m; ++k) { umin[k] = p[k]; umax[k] = p[M::m + k]; }
  }
  // clip(v, u_min, u_max) by comparisons: a NaN stays NaN (its trial is rejected as without limits)
  __device__ __forceinline__ double clamp(int k, double v) const {
    v = v < umin[k] ? umin[k] : v;
    return v > umax[k] ? umax[k] : v;
  }
};

template <class M>
struct Consts : LimitRegs<M> {
  static constexpr int n = M::n, m = M::m;
  double Q[n][n], R[m][m], Qf[n][n], xnom[n];
  double qn[n];    // 2*x_nom^T Q    (ilqr.py:180)
  double qfn[n];   // 2*x_nom^T Qf   (ilqr.py:203)
  __device__ inline void load(const double* cm) { load(cm, cm + 2 * n * n + m * m); }
  // xn: this problem's target (x_nom_of); qn / qfn come from the same loop whichever array it is
  __device__ inline void load(const double* cm, const double* xn) {
    load_from([cm](int e) __attribute__((always_inline)) { return cm[e]; }, xn);
  }
  // at(e): entry e of Q | R | Qf wherever the matrices live (dense: cm[e]; the lane-per-problem kernels' per-problem matrices:
  // KArgs::cost_cols, batch-minor) - ONE loop builds the constants whichever array they came from
  template <class At>
  __device__ inline void load_from(At at, const double* xn) {
#pragma unroll
    for (int i = 0; i < n; ++i)
#pragma unroll
      for (int j = 0; j < n; ++j) { Q[i][j] = at(i * n + j); Qf[i][j] = at(n * n + m * m + i * n + j); }
#pragma unroll
    for (int i = 0; i < m; ++i)
#pragma unroll
      for (int j = 0; j < m; ++j) R[i][j] = at(n * n + i * m + j);
#pragma unroll
    for (int i = 0; i < n; ++i) xnom[i] = xn[i];
#pragma unroll
    for (int j = 0; j < n; ++j) {
      double s = 0.0, sf = 0.0;
#pragma unroll
      for (int i = 0; i < n; ++i) { s += (2.0 * xnom[i]) * Q[i][j]; sf += (2.0 * xnom[i]) * Qf[i][j]; }
      qn[j] = s; qfn[j] = sf;
    }
  }
  // Qf alone, read again (the lane-per-problem kernels' per-problem matrices: Qf is used twice per iteration, and re-reading it
  // there keeps n^2 values per lane out of the registers in between)
  template <class At>
  __device__ __forceinline__ void reload_Qf(At at) {
#pragma unroll
    for (int i = 0; i < n; ++i)
#pragma unroll
      for (int j = 0; j < n; ++j) Qf[i][j] = at(n * n + m * m + i * n + j);
  }
  // LDS image: Q | Qf | R | xnom | qn | qfn
  __device__ inline void to_lds(double* d) const {
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int i = 0; i < n; ++i)
#pragma unroll
        for (int j = 0; j < n; ++j) { d[i * n + j] = Q[i][j]; d[n * n + i * n + j] = Qf[i][j]; }
#pragma unroll
      for (int i = 0; i < m; ++i)
#pragma unroll
        for (int j = 0; j < m; ++j) d[2 * n * n + i * m + j] = R[i][j];
#pragma unroll
      for (int i = 0; i < n; ++i) { d[2 * n * n + m * m + i] = xnom[i]; d[2 * n * n + m * m + n + i] = qn[i]; d[2 * n * n + m * m + 2 * n + i] = qfn[i]; }
    }
  }
  __device__ inline void from_lds(const double* d) {
#pragma unroll
    for (int i = 0; i < n; ++i)
#pragma unroll
      for (int j = 0; j < n; ++j) { Q[i][j] = d[i * n + j]; Qf[i][j] = d[n * n + i * n + j]; }
#pragma unroll
    for (int i = 0; i < m; ++i)
#pragma unroll
      for (int j = 0; j < m; ++j) R[i][j] = d[2 * n * n + i * m + j];
#pragma unroll
    for (int i = 0; i < n; ++i) { xnom[i] = d[2 * n * n + m * m + i]; qn[i] = d[2 * n * n + m * m + n + i]; qfn[i] = d[2 * n * n + m * m + 2 * n + i]; }
  }
};

// The full row sums, also where Q is diagonal.  A wave-uniform branch that leaves out the products with Q's zeros (on a flag the
// host set for such a Q) gives the same bits and saves 12 of the 146 instructions of a cart-pole + wall rollout step, but MEASURED
// in the fused kernel (round 6, profiles/r06_c4_ab.txt) the line search got 26 % LONGER (178.6 k -> 224.9 k cycles per iteration):
// the second arm of the branch lives in the same loop, and its registers push the loop's values into the accumulation file.  The
// flag and its detection in mi_ilqr_set_cost left the sources with this finding.
template <class M>
__device__ __forceinline__ double stage_cost(const Consts<M>& c, const double (&x)[M::n], const double (&u)[M::m]) {
  constexpr int n = M::n, m = M::m;
  double dx[n];
#pragma unroll
  for (int i = 0; i < n; ++i) dx[i] = x[i] - c.xnom[i];
  double q = 0.0;
#pragma unroll
  for (int i = 0; i < n; ++i) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < n; ++j) s += c.Q[i][j] * dx[j];
    q += dx[i] * s;
  }
  double ru = 0.0;
#pragma unroll
  for (int i = 0; i < m; ++i) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < m; ++j) s += c.R[i][j] * u[j];
    ru += u[i] * s;
  }
  return q + ru;
}

template <class M>
__device__ __forceinline__ double terminal_cost(const Consts<M>& c, const double (&x)[M::n]) {
  constexpr int n = M::n;
  double dx[n];
#pragma unroll
  for (int i = 0; i < n; ++i) dx[i] = x[i] - c.xnom[i];
  double q = 0.0;
#pragma unroll
  for (int i = 0; i < n; ++i) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < n; ++j) s += c.Qf[i][j] * dx[j];
    q += dx[i] * s;
  }
  return q;
}

template <int m>
__device__ __forceinline__ void invert_small(const double (&A)[m][m], double (&Ai)[m][m]) {
  static_assert(m >= 1 && m <= 2, "wave-per-problem path covers m <= 2");
  if constexpr (m == 1) {
    Ai[0][0] = fast_rcp(A[0][0]);
  } else {
    const double id = fast_rcp(A[0][0] * A[1][1] - A[0][1] * A[1][0]);
    Ai[0][0] = A[1][1] * id; Ai[0][1] = -A[0][1] * id;
    Ai[1][0] = -A[1][0] * id; Ai[1][1] = A[0][0] * id;
  }
}

// ---------------------------------------------------------------------------
// Backward step with box control limits (Limited<M> kernels, m <= 2): given the expansion Qx, Qu, Qxx, Quu, Qux of
// step t (ilqr.py:651-656), solve  du* = argmin 1/2 du^T Quu du + Qu^T du  subject to  lo <= du <= hi
// (lo = u_min - u_bar_t, hi = u_max - u_bar_t) and set kappa = -du*.
//   m = 1: the clamp of -Qu / Quu.
//   m = 2: the unconstrained minimiser when it lies in the box; otherwise the best of the four edges u0 = lo0, u0 = hi0,
//          u1 = lo1, u1 = hi1 (infinite edges skipped), each with the free component's clamped 1-D minimiser (the row of
//          Quu du + Qu = 0 it solves); the smallest objective wins, a tie goes to the earlier edge.
// The clamped components are those the chosen candidate put on a bound - decided by that construction, never by
// comparing floats afterwards.  Their rows of K are 0; the free rows are Quu_ff^-1 Qux_f.  With nothing clamped every
// output is the reference's arithmetic (backward_step); otherwise dV = kappa^T Qu and the value update takes its general
// form Vx = Qx - K^T Qu - Qux^T kappa + K^T Quu kappa, Vxx = Qxx - K^T Qux - Qux^T K + K^T Quu K.
// s2 accumulates kappa^T Quu kappa.  Returns false when Quu is not positive definite (no minimiser; the problem stops
// with MI_STATUS_NOT_PD).  Shared by the wave- and lane-per-problem kernels.
// ---------------------------------------------------------------------------
template <int n, int m>
__device__ __forceinline__ bool box_qp_step(const double (&Qx)[n], const double (&Qu)[m], const double (&Qxx)[n][n],
                                            const double (&Quu)[m][m], const double (&Qux)[m][n], const double (&lo)[m],
                                            const double (&hi)[m], double (&kap)[m], double (&Kg)[m][n], double& dv,
                                            double& s2, double (&Vx)[n], double (&Vxx)[n][n]) {
  static_assert(m >= 1 && m <= 2, "box QP of the m <= 2 kernels");
  bool pd;
  if constexpr (m == 1) pd = Quu[0][0] > 0.0 && __builtin_isfinite(Quu[0][0]);
  else {
    const double det = Quu[0][0] * Quu[1][1] - Quu[0][1] * Quu[1][0];
    pd = Quu[0][0] > 0.0 && det > 0.0 && __builtin_isfinite(det) && __builtin_isfinite(Quu[0][0]) && __builtin_isfinite(Quu[1][1]) &&
         __builtin_isfinite(Quu[0][1]) && __builtin_isfinite(Quu[1][0]);
  }
  double Qi[m][m];
  invert_small<m>(Quu, Qi);
  double d[m];                                              // du*, the minimiser
  bool cl[m];                                               // component on a bound
#pragma unroll
  for (int a_ = 0; a_ < m; ++a_) {
    double s = 0.0;
#pragma unroll
    for (int b_ = 0; b_ < m; ++b_) s += Qi[a_][b_] * Qu[b_];
    d[a_] = -s;
    cl[a_] = false;
  }
  if constexpr (m == 1) {
    if (d[0] < lo[0]) { d[0] = lo[0]; cl[0] = true; }
    else if (d[0] > hi[0]) { d[0] = hi[0]; cl[0] = true; }
  } else {
    const bool inside = !(d[0] < lo[0]) && !(d[0] > hi[0]) && !(d[1] < lo[1]) && !(d[1] > hi[1]);
    if (!inside) {
      double best = __builtin_inf();
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int fx_ = e >> 1, fr = 1 - fx_;                // the component on the edge, the free one
        const double v = (e & 1) ? hi[fx_] : lo[fx_];
        if (!__builtin_isfinite(v)) continue;
        double f = -(Qu[fr] + Quu[fr][fx_] * v) / Quu[fr][fr];
        bool cf = false;
        if (f < lo[fr]) { f = lo[fr]; cf = true; }
        else if (f > hi[fr]) { f = hi[fr]; cf = true; }
        double c2[2];
        c2[fx_] = v; c2[fr] = f;
        const double obj = 0.5 * (c2[0] * (Quu[0][0] * c2[0] + Quu[0][1] * c2[1]) + c2[1] * (Quu[1][0] * c2[0] + Quu[1][1] * c2[1])) +
                           (Qu[0] * c2[0] + Qu[1] * c2[1]);
        if (obj < best) {
          best = obj;
          d[0] = c2[0]; d[1] = c2[1];
          cl[fx_] = true; cl[fr] = cf;
        }
      }
    }
  }
  bool any = false;
#pragma unroll
  for (int a_ = 0; a_ < m; ++a_) { kap[a_] = -d[a_]; any = any || cl[a_]; }
  double Qk[m];                                             // Quu kappa
#pragma unroll
  for (int a_ = 0; a_ < m; ++a_) {
    double s = 0.0;
#pragma unroll
    for (int b_ = 0; b_ < m; ++b_) s += Quu[a_][b_] * kap[b_];
    Qk[a_] = s;
  }
  double kqk = 0.0;
#pragma unroll
  for (int a_ = 0; a_ < m; ++a_) kqk += kap[a_] * Qk[a_];
  s2 += kqk;
  if (!any) {
    // the reference's step (ilqr.py:659-667; backward_step)
    double QuQi[m];
#pragma unroll
    for (int a_ = 0; a_ < m; ++a_) {
      double s = 0.0, q = 0.0;
#pragma unroll
      for (int b_ = 0; b_ < m; ++b_) { s += Qi[a_][b_] * Qu[b_]; q += Qu[b_] * Qi[b_][a_]; }
      kap[a_] = s;
      QuQi[a_] = q;
#pragma unroll
      for (int j = 0; j < n; ++j) {
        double g = 0.0;
#pragma unroll
        for (int b_ = 0; b_ < m; ++b_) g += Qi[a_][b_] * Qux[b_][j];
        Kg[a_][j] = g;
      }
    }
    dv = 0.0;
#pragma unroll
    for (int a_ = 0; a_ < m; ++a_) dv += QuQi[a_] * Qu[a_];
#pragma unroll
    for (int j = 0; j < n; ++j) {
      double s = Qx[j];
#pragma unroll
      for (int a_ = 0; a_ < m; ++a_) s -= QuQi[a_] * Qux[a_][j];
      Vx[j] = s;
    }
    double QuxTQi[n][m];
#pragma unroll
    for (int i = 0; i < n; ++i)
#pragma unroll
      for (int b_ = 0; b_ < m; ++b_) {
        double s = 0.0;
#pragma unroll
        for (int a_ = 0; a_ < m; ++a_) s += Qux[a_][i] * Qi[a_][b_];
        QuxTQi[i][b_] = s;
      }
#pragma unroll
    for (int i = 0; i < n; ++i)
#pragma unroll
      for (int j = 0; j < n; ++j) {
        double s = Qxx[i][j];
#pragma unroll
        for (int b_ = 0; b_ < m; ++b_) s -= QuxTQi[i][b_] * Qux[b_][j];
        Vxx[i][j] = s;
      }
    return pd;
  }
  // K: clamped rows 0, free rows Quu_ff^-1 Qux_f (at most one free component here)
#pragma unroll
  for (int a_ = 0; a_ < m; ++a_)
#pragma unroll
    for (int j = 0; j < n; ++j) Kg[a_][j] = cl[a_] ? 0.0 : Qux[a_][j] / Quu[a_][a_];
  dv = 0.0;
#pragma unroll
  for (int a_ = 0; a_ < m; ++a_) dv += kap[a_] * Qu[a_];
  double QK[m][n];                                          // Quu K
#pragma unroll
  for (int a_ = 0; a_ < m; ++a_)
#pragma unroll
    for (int j = 0; j < n; ++j) {
      double s = 0.0;
#pragma unroll
      for (int b_ = 0; b_ < m; ++b_) s += Quu[a_][b_] * Kg[b_][j];
      QK[a_][j] = s;
    }
#pragma unroll
  for (int j = 0; j < n; ++j) {
    double s = Qx[j];
#pragma unroll
    for (int a_ = 0; a_ < m; ++a_) s += -Kg[a_][j] * Qu[a_] - Qux[a_][j] * kap[a_] + Kg[a_][j] * Qk[a_];
    Vx[j] = s;
  }
#pragma unroll
  for (int i = 0; i < n; ++i)
#pragma unroll
    for (int j = 0; j < n; ++j) {
      double s = Qxx[i][j];
#pragma unroll
      for (int a_ = 0; a_ < m; ++a_) s += -Kg[a_][i] * Qux[a_][j] - Qux[a_][i] * Kg[a_][j] + Kg[a_][i] * QK[a_][j];
      Vxx[i][j] = s;
    }
  return pd;
}

}  // namespace mi
