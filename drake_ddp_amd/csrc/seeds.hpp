// Multi-start on the device (include/mi_ilqr.h, "Multi-start"): a handle of B problems read as G = B / K groups of K
// consecutive problems - the same problem under K initial guesses - and the step that joins the seeds of a group: draw the guesses
// where they are used, pick the best member, rebuild the guesses around it, hand the winners out.  No model templates: rows,
// layouts and dimensions are run-time values, one unit (k_seeds.hip) serves every model, plugins included.  No solve kernel and no
// KArgs is touched: the kernel reads cost / status / x_bar / u_bar as a solve left them and writes u_guess, the (G, 3) rows and the
// gather's staging arrays.
//
// seeds_kernel, ONE WORKGROUP PER GROUP (256 threads), nothing synchronises across workgroups:
//   SELECT.  Member k of group g is problem b = g K + k; it is eligible iff its status with MI_STATUS_FLAG_INDEFINITE masked off
//   is CONVERGED or MAX_ITERS and its cost is finite.  The threads stride over the members and keep a (cost, index) pair; the pairs
//   are reduced inside the wave by a butterfly of DPP row moves (wave_ops.hpp: row_xor over lane distance 1, 2, 4, 8) and v_readlane
//   of the four row results, across the four waves through LDS.  The combination - the smaller cost, of equal costs the smaller
//   index - is commutative and associative, so the result does not depend on the order it is applied in: the eligible member of
//   least cost, ties to the lowest index.  The count of eligible members is an integer sum.  No winner: -1 | +inf | 0.
//   WRITE (perturb, reseed).  u_guess[b, j, t] = base[sb, j, t] + sigma_u[b, j] z(seed, round, b, t div hold, j): sb = b for perturb,
//   the winner's problem for reseed; the ELITE slot - member 0 for perturb, the winner for reseed - gets its base unchanged, and so
//   does every element with sigma = 0 and every padding control (j >= m_user), bit for bit (no `+ 0 z`).  A group without a winner
//   falls back to perturb with non-finite entries of the base read as 0.  z: Philox4x32-10 under the key (seed lo, seed hi) at counter
//   (round, t div hold, b, 768 + j / 4), Box-Muller normal j mod 4 of the block (philox.hpp; blocks 0.. are the states', 256.. the
//   controls', 512.. the Monte-Carlo draws') - a function of (seed, round, b, t div hold, j) and of nothing else.  sigma z is a
//   rounded product and the sum a rounded sum, never an FMA (the idiom of policy_env_kernel), so the NumPy statement
//   (tests/seeds_np.py) differs by what the normals differ by.  The group's elements are walked in the order of the handle's
//   layout, so consecutive lanes write consecutive addresses: time fastest for [b][row][t], row fastest for [b][t][row] - the
//   group's K problems are one contiguous block in both - and member fastest for [t][row][b], runs of K.
//   ALIASING.  The base may BE the destination (a pending guess is perturbed in place).  The kernel is element-wise safe: perturb
//   and the fallback read only the element they write; reseed with a winner reads the winner's slot from every member, and that slot
//   is then not written at all (its value would be its own).
//   GATHER.  The winner's x_bar (n, N) and u_bar (m, N-1), time last, and its cost; no winner: NaN rows and +inf.
#pragma once
#include "host.hpp"
#include "philox.hpp"
#include "wave_ops.hpp"

namespace mi {

constexpr int kSeedsThreads = 256;
constexpr uint32_t kSeedsBlock = 768;      // the perturbation's first Philox block

#if defined(__HIPCC__)
using mi_host::SeedsArgs;
using mi_host::SEEDS_PERTURB;
using mi_host::SEEDS_SELECT;
using mi_host::SEEDS_RESEED;
using mi_host::SEEDS_GATHER;

// (cost, index): a is replaced by b when b is the better pair.  Total order, so min over any tree of combinations is the same pair.
__device__ __forceinline__ void seeds_better(double& c, int& i, double oc, int oi) {
  const bool take = oc < c || (oc == c && oi < i);
  c = take ? oc : c;
  i = take ? oi : i;
}

// element (b, row, t) of a (B, rows, len) trajectory array in the handle's layout
__device__ __forceinline__ size_t seeds_at(int layout, int B, int rows, int len, int b, int r, int t) {
  if (layout == 0) return ((size_t)b * rows + r) * len + t;
  if (layout == 1) return ((size_t)b * len + t) * rows + r;
  return ((size_t)t * rows + r) * B + b;
}

__global__ void __launch_bounds__(kSeedsThreads) seeds_kernel(SeedsArgs a) {
  __shared__ double s_cost[kSeedsThreads / 64];
  __shared__ int s_idx[kSeedsThreads / 64], s_cnt[kSeedsThreads / 64];
  const int g = (int)blockIdx.x, tid = (int)threadIdx.x, K = a.K, B = a.B;
  const int b0 = g * K;                                          // (g < G = B / K: every member is a problem of the handle)
  int winner = -1, eligible = 0;
  double win_cost = INFINITY;

  if (a.op != SEEDS_PERTURB) {
    double c = INFINITY;
    int i = 0x7fffffff, cnt = 0;
    for (int k = tid; k < K; k += kSeedsThreads) {
      const double ck = a.cost[b0 + k];
      const int st = a.status[b0 + k] & ~MI_STATUS_FLAG_INDEFINITE;
      if ((st == MI_STATUS_CONVERGED || st == MI_STATUS_MAX_ITERS) && fabs(ck) < INFINITY) {      // (a NaN compares false)
        ++cnt;
        seeds_better(c, i, ck, k);
      }
    }
    // all 256 threads are here: the DPP moves below read every lane
    seeds_better(c, i, row_xor_f64<1>(c), row_xor_i32<1>(i)); cnt += row_xor_i32<1>(cnt);
    seeds_better(c, i, row_xor_f64<2>(c), row_xor_i32<2>(i)); cnt += row_xor_i32<2>(cnt);
    seeds_better(c, i, row_xor_f64<4>(c), row_xor_i32<4>(i)); cnt += row_xor_i32<4>(cnt);
    seeds_better(c, i, row_xor_f64<8>(c), row_xor_i32<8>(i)); cnt += row_xor_i32<8>(cnt);
    double wc = readlane_f64(c, 0);
    int wi = __builtin_amdgcn_readlane(i, 0), wn = __builtin_amdgcn_readlane(cnt, 0);
#pragma unroll
    for (int row = 16; row < 64; row += 16) {
      seeds_better(wc, wi, readlane_f64(c, row), __builtin_amdgcn_readlane(i, row));
      wn += __builtin_amdgcn_readlane(cnt, row);
    }
    if ((tid & 63) == 0) { s_cost[tid >> 6] = wc; s_idx[tid >> 6] = wi; s_cnt[tid >> 6] = wn; }
    __syncthreads();
    wc = s_cost[0]; wi = s_idx[0]; wn = s_cnt[0];
#pragma unroll
    for (int w = 1; w < kSeedsThreads / 64; ++w) {
      seeds_better(wc, wi, s_cost[w], s_idx[w]);
      wn += s_cnt[w];
    }
    eligible = wn;
    if (wn > 0) { winner = wi; win_cost = wc; }
    if (tid == 0) {
      a.best[(size_t)g * 3 + 0] = (double)winner;
      a.best[(size_t)g * 3 + 1] = win_cost;
      a.best[(size_t)g * 3 + 2] = (double)eligible;
    }
    if (a.op == SEEDS_SELECT) return;
  }

  const int m = a.m, M1 = a.N - 1;
  if (a.op == SEEDS_GATHER) {
    const int n = a.n, N = a.N;
    const double nan = __builtin_nan("");
    const int wb = b0 + (winner < 0 ? 0 : winner);
    double* gx = a.gx + (size_t)g * n * N;
    for (int e = tid; e < n * N; e += kSeedsThreads) {           // time fastest on the way out
      const int r = e / N, t = e - r * N;
      gx[e] = winner < 0 ? nan : (a.x_bar ? a.x_bar[seeds_at(a.layout, B, n, N, wb, r, t)] : 0.0);
    }
    double* gu = a.gu + (size_t)g * m * M1;
    for (int e = tid; e < m * M1; e += kSeedsThreads) {
      const int r = e / M1, t = e - r * M1;
      gu[e] = winner < 0 ? nan : (a.u_src ? a.u_src[seeds_at(a.layout, B, m, M1, wb, r, t)] : 0.0);
    }
    if (tid == 0) a.gc[g] = winner < 0 ? INFINITY : a.cost[wb];
    return;
  }

  // perturb / reseed: the group's K m (N-1) elements in the layout's own order
  const bool from_winner = a.op == SEEDS_RESEED && winner >= 0, fallback = a.op == SEEDS_RESEED && winner < 0;
  const int elite = from_winner ? winner : 0;
  const bool aliased = a.u_src == a.u_dst;
  const uint32_t k0 = (uint32_t)(a.seed & 0xffffffffull), k1 = (uint32_t)(a.seed >> 32);
  const size_t per = (size_t)m * M1, total = (size_t)K * per;
  for (size_t e = tid; e < total; e += kSeedsThreads) {
    int k, j, t;
    if (a.layout == 2) { k = (int)(e % K); const size_t r = e / K; t = (int)(r / m); j = (int)(r - (size_t)t * m); }
    else {
      k = (int)(e / per);
      const size_t r = e - (size_t)k * per;
      if (a.layout == 0) { j = (int)(r / M1); t = (int)(r - (size_t)j * M1); }
      else { t = (int)(r / m); j = (int)(r - (size_t)t * m); }
    }
    const int b = b0 + k;
    if (from_winner && aliased && k == elite) continue;          // the slot every member reads, and its value is its own
    double v = a.u_src ? a.u_src[seeds_at(a.layout, B, m, M1, from_winner ? b0 + elite : b, j, t)] : 0.0;
    if (fallback && !(fabs(v) < INFINITY)) v = 0.0;
    const double s = (a.sigma && k != elite && j < a.m_user) ? a.sigma[(size_t)b * m + j] : 0.0;
    if (s != 0.0) {
      uint32_t c[4] = {a.round, (uint32_t)(t / a.hold), (uint32_t)b, kSeedsBlock + (uint32_t)(j >> 2)};
      philox4x32_10(k0, k1, c);
      double z0, z1;
      box_muller((j & 2) ? c[2] : c[0], (j & 2) ? c[3] : c[1], z0, z1);
      double sz = s * ((j & 1) ? z1 : z0);
      asm volatile("" : "+v"(sz));                               // the product is rounded before it is added (no FMA)
      v = v + sz;
    }
    a.u_dst[seeds_at(a.layout, B, m, M1, b, j, t)] = v;
  }
}
#endif

}  // namespace mi

#if defined(__HIPCC__)
namespace mi_host {

int launch_seeds(mi_ilqr* h, const SeedsArgs& a) {
  if (a.K < 1 || a.B % a.K != 0) return MI_ILQR_E_BAD_ARG;
  SeedsArgs args = a;
  void* argv[] = {&args};
  HIPCHK(hipExtLaunchKernel(reinterpret_cast<const void*>(seeds_kernel), dim3((unsigned)(a.B / a.K)), dim3(kSeedsThreads), argv, 0,
                            h->stream, a.ev0, a.ev1, 0));
  return MI_ILQR_OK;
}

}  // namespace mi_host
#endif
