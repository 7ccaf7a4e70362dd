// The parameter-identification kernels.  fit.hpp holds what a model's unit needs - fit_normal_kernel<M>, one lane per
// (transition, finite-difference slot) - and this unit instantiates it for every built-in model.  fit_update_kernel, WITHOUT a
// model, and its launcher (declared in host.hpp) are defined here and nowhere else, so a plugin unit, which includes fit.hpp for
// its model's kernel, compiles and carries none of it.
#include "fit.hpp"

namespace mi {

__device__ __forceinline__ bool fit_finite(double v) { return v - v == 0.0; }      // (false for NaN and +-inf)

// ONE WAVE PER PROBLEM.  Lane e folds entry e of the problem's partial rows left to right in wave order - an order that is a
// function of T and P alone - and lane 0 decides: the first rows become the kept normal equations (a cost that is not finite:
// MI_FIT_BAD_DATA); later rows are a trial's - accepted when its factorisation had succeeded and its cost is finite and below the
// kept one (theta, the kept equations and mu move; MI_FIT_CONVERGED by ftol or a zero cost), else rejected (mu at its ceiling
// already: MI_FIT_STALLED).  A problem still running then gets MI_FIT_MAX_ITERS at the closing decision, or its next trial row:
// (H + mu D) delta = g by Cholesky, D_ii = H_ii where that is positive, else 1, theta + delta clipped into the bounds by
// comparisons on the free entries.  A pivot that is not positive or not finite: the trial row is theta and is marked failed - the
// next launch evaluates it all the same and the decision after it rejects.
__global__ void __launch_bounds__(64) fit_update_kernel(mi_host::FitUpdateArgs a) {
  using namespace mi_host;
  __shared__ double s_row[64];
  const int b = (int)blockIdx.x, lane = (int)threadIdx.x, P = a.P, L = fit_row_len(P), np = a.n_params;
  double* st = a.state + (size_t)b * kFitStride;
  if (st[kFitStatus] != kFitRunning) return;                        // (wave-uniform: a finished problem is frozen)
  const double* pr = a.partial + (size_t)b * a.waves * L;
  const int e = lane < L ? lane : 0;
  double acc = pr[e];
  for (int w = 1; w < a.waves; ++w) acc += pr[(size_t)w * L + e];
  s_row[lane] = acc;
  wave_sync();
  if (lane == 0) {
    const double cn = s_row[0];
    double mu = st[kFitMu];
    bool running = true;
    if (a.first) {
      st[kFitC] = cn;
      st[kFitCost0] = cn;
      for (int q = 1; q < L; ++q) st[kFitC + q] = s_row[q];         // (g and the triangle follow c in the record as in the row)
      if (!fit_finite(cn)) { st[kFitStatus] = (double)MI_FIT_BAD_DATA; running = false; }
    } else {
      const double c = st[kFitC];
      st[kFitIters] = st[kFitIters] + 1.0;
      if (st[kFitTrialOk] != 0.0 && fit_finite(cn) && cn < c) {
        for (int i = 0; i < np; ++i) st[kFitTheta + i] = st[kFitTrial + i];
        for (int q = 0; q < L; ++q) st[kFitC + q] = s_row[q];
        mu = mu / 10.0;
        mu = mu < kFitMuMin ? kFitMuMin : mu;
        st[kFitAccepted] = st[kFitAccepted] + 1.0;
        if (c - cn <= a.ftol * c || cn == 0.0) { st[kFitStatus] = (double)MI_FIT_CONVERGED; running = false; }
      } else if (mu >= kFitMuMax) {
        st[kFitStatus] = (double)MI_FIT_STALLED;
        running = false;
      } else {
        mu = 10.0 * mu;
        mu = mu > kFitMuMax ? kFitMuMax : mu;
      }
      st[kFitMu] = mu;
    }
    if (running && a.last) { st[kFitStatus] = (double)MI_FIT_MAX_ITERS; running = false; }
    if (running) {
      // the next trial from the kept H, g
      const double* g = st + kFitC + 1;
      const double* Hu = g + P;
      double A[kFitMaxFree][kFitMaxFree], y[kFitMaxFree];
      for (int i = 0; i < P; ++i)
        for (int j = i; j < P; ++j) A[i][j] = A[j][i] = Hu[fit_tri(P, i, j)];
      for (int i = 0; i < P; ++i) { const double hd = A[i][i]; A[i][i] = hd + mu * (hd > 0.0 ? hd : 1.0); }
      bool ok = true;
      for (int j = 0; j < P && ok; ++j) {                           // A = L L', L in the lower triangle
        double s = A[j][j];
        for (int q = 0; q < j; ++q) s -= A[j][q] * A[j][q];
        if (!(s > 0.0) || !fit_finite(s)) { ok = false; break; }
        const double ljj = sqrt(s);
        A[j][j] = ljj;
        for (int i = j + 1; i < P; ++i) {
          double t = A[i][j];
          for (int q = 0; q < j; ++q) t -= A[i][q] * A[j][q];
          A[i][j] = t / ljj;
        }
      }
      if (ok) {
        for (int i = 0; i < P; ++i) {
          double t = g[i];
          for (int q = 0; q < i; ++q) t -= A[i][q] * y[q];
          y[i] = t / A[i][i];
        }
        for (int i = P - 1; i >= 0; --i) {
          double t = y[i];
          for (int q = i + 1; q < P; ++q) t -= A[q][i] * y[q];
          y[i] = t / A[i][i];
        }
      }
      for (int i = 0; i < np; ++i) st[kFitTrial + i] = st[kFitTheta + i];
      if (ok) {
        for (int i = 0; i < P; ++i) {
          const int k = a.free_idx[i];
          const double lo = a.bounds[k], hi = a.bounds[np + k];
          double v = st[kFitTheta + k] + y[i];
          v = v < lo ? lo : (v > hi ? hi : v);
          st[kFitTrial + k] = v;
        }
      }
      st[kFitTrialOk] = ok ? 1.0 : 0.0;
    }
  }
}

}  // namespace mi

namespace mi_host {

int launch_fit_update(mi_ilqr* h, const FitUpdateArgs& a) {
  if (a.B < 1 || a.P < 1 || a.P > kFitMaxFree || a.n_params < 1 || a.n_params > MI_ILQR_MAX_PARAMS || a.waves < 1 || !a.state || !a.partial || !a.bounds)
    return MI_ILQR_E_BAD_ARG;
  for (int i = 0; i < a.P; ++i)
    if (a.free_idx[i] < 0 || a.free_idx[i] >= a.n_params) return MI_ILQR_E_BAD_ARG;
  FitUpdateArgs args = a;
  void* argv[] = {&args};
  HIPCHK(hipExtLaunchKernel(reinterpret_cast<const void*>(mi::fit_update_kernel), dim3((unsigned)a.B), dim3(64), argv, 0, h->stream, a.ev0, a.ev1, 0));
  return MI_ILQR_OK;
}

}  // namespace mi_host

template int mi_host::launch_fit_normal<mi::Pendulum>(mi_ilqr*, const mi_host::FitArgs&);
template int mi_host::launch_fit_normal<mi::Acrobot>(mi_ilqr*, const mi_host::FitArgs&);
template int mi_host::launch_fit_normal<mi::CartPole>(mi_ilqr*, const mi_host::FitArgs&);
template int mi_host::launch_fit_normal<mi::CartPoleWall>(mi_ilqr*, const mi_host::FitArgs&);
template int mi_host::launch_fit_normal<mi::Synth36>(mi_ilqr*, const mi_host::FitArgs&);
template int mi_host::launch_fit_normal<mi::PlanarQuad>(mi_ilqr*, const mi_host::FitArgs&);
template int mi_host::launch_fit_normal<mi::Quad3D>(mi_ilqr*, const mi_host::FitArgs&);
template int mi_host::launch_fit_normal<mi::Arm27>(mi_ilqr*, const mi_host::FitArgs&);
template int mi_host::launch_fit_normal<mi::Arm27C>(mi_ilqr*, const mi_host::FitArgs&);
