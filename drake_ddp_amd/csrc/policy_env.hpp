// What an on-device Monte-Carlo run OBSERVES beside the cost (include/mi_ilqr.h, "Envelopes and a safety box"): per-step
// statistics of the states and controls over the samples, and the count of samples that stay inside a box.  policy_mc_kernel
// leaves a window's trajectories in the handle's scratch, sample-minor -
//     X[((b N + t) n + i) win + s]      U[((b (N-1) + t) m + k) win + s]      (NaN from the step at which a sample ended)
// - and the two kernels below reduce that buffer before the next window overwrites it.  No model templates: rows, pitches and
// dimensions are run-time values, one unit (k_policy_env.hip) serves every model, plugins included.
//
// policy_env_kernel: a ROW is one (t, i) of one problem, `win` doubles long.  Per row eight doubles persist across the windows,
//     count | K | s1 | s2 | min | max | argmin | argmax
// and the contract is a LEFT FOLD in global sample order (windows in order, s ascending): a non-finite v is skipped; the first finite
// v sets K = v; then d = v - K, s1 += d, s2 += d d (a rounded product, then a rounded sum: never an FMA, see the kernel),
// count += 1; v < min and v > max, strict, so a tie keeps the lower sample number; argmin / argmax are global sample numbers held in
// doubles.  Empty: 0 | 0 | 0 | 0 | +inf | -inf | -1 | -1.  A fixed order and no contraction: the result does not depend on the
// window, bit for bit, and a NumPy loop reproduces it (tests/policy_env_np.py).
// Shape: one wave per tile of 64 rows; the window's samples in tiles of 64 inside the wave, so the order needs no inter-wave step.
// Per tile 64 coalesced 512-byte row loads go into an LDS image of pitch 65 doubles, then lane r walks row r: with the odd pitch the
// 32 lanes of a ds_read_b64 half hit 32 distinct bank pairs (address / 4 mod 64), the row-wise ds_write_b64 is contiguous.  The image
// takes 64 x 65 x 8 = 33 280 bytes: 4 workgroups per CU.  A masked element (row >= R, sample >= win) enters the image as NaN - the
// fold skips it like a sample that has ended - and no lane reads outside the buffer.
//
// policy_box_kernel: one lane per sample, one wave = 64 consecutive samples of one problem, coalesced along s; per problem a row
// lo | hi (2 n doubles, +-inf: unbounded), wave-uniform.  ran: all N states finite.  OUTSIDE at t: x < lo or x > hi for some i
// (comparisons: a NaN is never outside).  exit: the first such t.  safe = ran and never outside; safe_success = safe and
// |x_{N-1,i} - x_nom_b,i| <= goal_b,i for all i.  Counters per problem, 64-bit integers: ran | safe | safe_success | exits[0 .. N-1]
// - wave ballot, popcount, one vector atomicAdd per wave and non-zero counter: integer addition is order-free.
#pragma once
#include "host.hpp"

namespace mi {

constexpr int kEnvFields = 8;
constexpr int kEnvTile = 64, kEnvPitch = 65;

#if defined(__HIPCC__)
__global__ void __launch_bounds__(64) policy_env_kernel(const double* __restrict__ buf, double* __restrict__ acc, int R, size_t win,
                                                        double first_global, int first) {
  // s2 += d d must be a rounded product and a rounded sum.  The build's -ffp-contract=fast lets the BACKEND fuse a multiply into the
  // add behind it whatever the source says - `#pragma clang fp contract(off)` here still gave v_fmac_f64 - so the product passes
  // through an empty asm on its register, which the compiler cannot look through (the idiom of policy_mc_kernel's drawn state).
  __shared__ double img[kEnvTile * kEnvPitch];
  const int tiles = (R + kEnvTile - 1) / kEnvTile;
  const int b = (int)(blockIdx.x / (unsigned)tiles);
  const int r0 = ((int)blockIdx.x - b * tiles) * kEnvTile;
  const int lane = (int)threadIdx.x;
  const int rows = R - r0 < kEnvTile ? R - r0 : kEnvTile;        // rows of this tile (>= 1)
  const bool mine = lane < rows;
  const double* base = buf + ((size_t)b * R + r0) * win;
  double* out = acc + ((size_t)b * R + r0 + lane) * kEnvFields;
  const double nan = __builtin_nan("");

  double cnt = 0.0, K = 0.0, s1 = 0.0, s2 = 0.0, mn = INFINITY, mx = -INFINITY, amin = -1.0, amax = -1.0;
  if (!first && mine) {
    cnt = out[0]; K = out[1]; s1 = out[2]; s2 = out[3]; mn = out[4]; mx = out[5]; amin = out[6]; amax = out[7];
  }
  for (size_t c0 = 0; c0 < win; c0 += kEnvTile) {
    // all 64 row loads of the tile are in flight before the first is used (in batches of 8 the tile took eight HBM latencies: 4.2i).
    // A masked element loads a clamped, valid address - the loads are unconditional - and enters the image as NaN.
    const bool in_s = c0 + lane < win;
    const size_t col = in_s ? c0 + lane : win - 1;
    double v[kEnvTile];
#pragma unroll
    for (int rr = 0; rr < kEnvTile; ++rr) v[rr] = base[(size_t)(rr < rows ? rr : rows - 1) * win + col];
#pragma unroll
    for (int rr = 0; rr < kEnvTile; ++rr) img[rr * kEnvPitch + lane] = (rr < rows && in_s) ? v[rr] : nan;
    __syncthreads();
    const double g0 = first_global + (double)c0;
#pragma unroll 8
    for (int s = 0; s < kEnvTile; ++s) {
      const double v = img[lane * kEnvPitch + s];
      if (fabs(v) < INFINITY) {                                  // finite; a NaN compares false
        const double g = g0 + (double)s;
        if (cnt == 0.0) K = v;
        const double d = v - K;
        s1 = s1 + d;
        double dd = d * d;
        asm volatile("" : "+v"(dd));                             // the product is rounded before it is added: see above
        s2 = s2 + dd;
        cnt = cnt + 1.0;
        if (v < mn) { mn = v; amin = g; }
        if (v > mx) { mx = v; amax = g; }
      }
    }
    __syncthreads();
  }
  if (mine) {
    out[0] = cnt; out[1] = K; out[2] = s1; out[3] = s2; out[4] = mn; out[5] = mx; out[6] = amin; out[7] = amax;
  }
}

// box: (B, 2 n) lo | hi;  x_nom + b x_nom_stride: the problem's target;  goal + b goal_stride: its goal row;  counters: (B, 3 + N)
__global__ void __launch_bounds__(64) policy_box_kernel(const double* __restrict__ X, const double* __restrict__ box,
                                                        const double* __restrict__ x_nom, size_t x_nom_stride,
                                                        const double* __restrict__ goal, size_t goal_stride,
                                                        unsigned long long* __restrict__ counters, int n, int N, size_t win) {
  const unsigned tiles = (unsigned)((win + 63) / 64);
  const int b = (int)(blockIdx.x / tiles);
  const size_t s = (size_t)(blockIdx.x - (unsigned)b * tiles) * 64 + threadIdx.x;
  const bool live = s < win;
  const size_t sl = live ? s : win - 1;                          // lanes past a ragged tail shadow the last sample and count for nothing
  const double* lo = box + (size_t)b * 2 * n;
  const double* hi = lo + n;
  const double* xt = x_nom + (size_t)b * x_nom_stride;
  const double* gl = goal + (size_t)b * goal_stride;
  unsigned long long* cnt = counters + (size_t)b * (3 + N);
  const double* x = X + (size_t)b * N * n * win + sl;
  bool fin = true, exited = false, goal_ok = true;
  for (int t = 0; t < N; ++t) {
    bool outside = false;
    for (int i = 0; i < n; ++i) {
      const double v = x[((size_t)t * n + i) * win];
      fin = fin && fabs(v) < INFINITY;
      outside = outside || v < lo[i] || v > hi[i];
      if (t == N - 1) goal_ok = goal_ok && fabs(v - xt[i]) <= gl[i];
    }
    const unsigned long long first_out = __ballot(live && outside && !exited);
    exited = exited || outside;
    if (first_out != 0ull && threadIdx.x == 0) atomicAdd(cnt + 3 + t, (unsigned long long)__popcll(first_out));
  }
  const bool ran = live && fin, safe = ran && !exited, succ = safe && goal_ok;
  const unsigned long long m_ran = __ballot(ran), m_safe = __ballot(safe), m_succ = __ballot(succ);
  if (threadIdx.x == 0) {
    if (m_ran) atomicAdd(cnt + 0, (unsigned long long)__popcll(m_ran));
    if (m_safe) atomicAdd(cnt + 1, (unsigned long long)__popcll(m_safe));
    if (m_succ) atomicAdd(cnt + 2, (unsigned long long)__popcll(m_succ));
  }
}
#endif

}  // namespace mi

#if defined(__HIPCC__)
namespace mi_host {

int launch_policy_env(mi_ilqr* h, const double* buf, double* acc, size_t B, size_t R, size_t win, double first_global, int first) {
  const unsigned long long blocks = (unsigned long long)B * ((R + kEnvTile - 1) / kEnvTile);
  if (blocks == 0 || blocks > 0x7fffffffull || R > 0x7fffffffull) return MI_ILQR_E_UNSUPPORTED;
  hipLaunchKernelGGL(policy_env_kernel, dim3((unsigned)blocks), dim3(64), 0, h->stream, buf, acc, (int)R, win, first_global, first);
  HIPCHK(hipGetLastError());
  return MI_ILQR_OK;
}

int launch_policy_box(mi_ilqr* h, const double* X, const double* box, const double* x_nom, size_t x_nom_stride, const double* goal,
                      size_t goal_stride, unsigned long long* counters, size_t B, int n, int N, size_t win) {
  const unsigned long long blocks = (unsigned long long)B * ((win + 63) / 64);
  if (blocks == 0 || blocks > 0x7fffffffull) return MI_ILQR_E_UNSUPPORTED;
  hipLaunchKernelGGL(policy_box_kernel, dim3((unsigned)blocks), dim3(64), 0, h->stream, X, box, x_nom, x_nom_stride, goal, goal_stride,
                     counters, n, N, win);
  HIPCHK(hipGetLastError());
  return MI_ILQR_OK;
}

}  // namespace mi_host
#endif
