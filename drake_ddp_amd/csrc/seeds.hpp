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
using mi_host::SeedsJoinArgs;
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

// SELECT of group b0 .. b0 + K - 1 by one workgroup of kSeedsThreads: every thread returns the winner (-1: none), its cost (+inf) and the
// number of eligible members.  All threads call it (the DPP moves read every lane, and there is one barrier inside).
__device__ __forceinline__ void seeds_select(const double* cost, const int32_t* status, int b0, int K, int tid, double* s_cost, int* s_idx,
                                             int* s_cnt, int& winner, double& win_cost, int& eligible) {
  double c = INFINITY;
  int i = 0x7fffffff, cnt = 0;
  for (int k = tid; k < K; k += kSeedsThreads) {
    const double ck = cost[b0 + k];
    const int st = status[b0 + k] & ~MI_STATUS_FLAG_INDEFINITE;
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
  winner = -1; win_cost = INFINITY;
  if (wn > 0) { winner = wi; win_cost = wc; }
}

__global__ void __launch_bounds__(kSeedsThreads) seeds_kernel(SeedsArgs a) {
  __shared__ double s_cost[kSeedsThreads / 64];
  __shared__ int s_idx[kSeedsThreads / 64], s_cnt[kSeedsThreads / 64];
  const int g = (int)blockIdx.x, tid = (int)threadIdx.x, K = a.K, B = a.B;
  const int b0 = g * K;                                          // (g < G = B / K: every member is a problem of the handle)
  int winner = -1, eligible = 0;
  double win_cost = INFINITY;

  if (a.op != SEEDS_PERTURB) {
    seeds_select(a.cost, a.status, b0, K, tid, s_cost, s_idx, s_cnt, winner, win_cost, eligible);
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

// seeds_mpc_join_kernel: the join between two re-solves of the receding-horizon loop (include/mi_ilqr.h, "Multi-start in the
// receding-horizon loop"), ONE WORKGROUP PER GROUP like seeds_kernel.  SELECT as above, then for a group with winner w
// every member gets x0 <- x_bar[w][:, replan] and u_guess[.., t] <- u_bar[w][.., min(t + replan, N - 2)] (+ sigma z for the members
// that are not w): mpc_shift's shift and seeds_kernel's reseed in one pass, the winner's plan read once per element.  No winner: each
// member's own shifted plan with non-finite entries read as 0, member 0 unperturbed, each member's own x_bar[:, replan].
// NOISE ONCE PER BLOCK.  An ITEM is (member k, control block jb = j div 4, window w = t div hold): one Philox block, whose four
// normals serve the block's up to four controls over the window's `hold` steps.  The group's K JB W items are numbered in the
// layout's order - [b][row][t]: (k, jb, w), window fastest; [b][t][row]: (k, w, jb), block fastest; [t][row][b]: (w, jb, k), member
// fastest - and taken 256 at a time: thread i of a TILE draws item i's normals (only the Box-Muller pairs whose live controls have
// sigma != 0; none for the winner's slot) into LDS, held per normal (s_z[jj][i]: consecutive threads, consecutive doubles), and
// after a barrier the tile's elements - item x control of the block x step of the window - are written with the time-last layout
// walking (control, item, step), the time-major one (step, item, control) and the batch-minor one (step, control, item): in each the
// fastest index of the walk is the fastest index of the layout, so consecutive lanes store consecutive addresses - runs of a whole
// row, of m controls and of K members - whatever `hold` is.  (A thread that kept its item's run of `hold` steps to itself would
// store at a stride of `hold` doubles in the time-last layout.)  With hold = 1 and m = 1 an item is one element and nothing is
// shared: the thread that draws the normal stores the element, without LDS and barriers.  The normals are those of seeds_kernel bit
// for bit: the same counter, the same Box-Muller call on the same word pair, the same rounded product and rounded sum.
constexpr int kSeedsJoinSteps = 1024;      // steps of a window taken per pass over a tile: the tile's element count stays below 2^20

__device__ __forceinline__ void seeds_mixed3(size_t i, uint32_t r0, uint32_t r1, uint32_t& d0, uint32_t& d1, uint32_t& d2) {
  d0 = (uint32_t)(i % r0);
  const size_t q = i / r0;
  d1 = (uint32_t)(q % r1);
  d2 = (uint32_t)(q / r1);
}

// item `il` of a tile whose first item has the digits (t0, t1, t2) under the radices (r0, r1), fastest first - two 32-bit divisions
// (t0 + il < 2^31 + 256) - and which digit is what: [b][row][t] w | jb | k, [b][t][row] jb | w | k, [t][row][b] k | jb | w
__device__ __forceinline__ void seeds_item(int layout, uint32_t il, uint32_t t0, uint32_t t1, uint32_t t2, uint32_t r0, uint32_t r1, int& k,
                                           uint32_t& jb, uint32_t& w) {
  const uint32_t x0 = t0 + il, c0 = x0 / r0, d0 = x0 - c0 * r0, x1 = t1 + c0, c1 = x1 / r1, d1 = x1 - c1 * r1, d2 = t2 + c1;
  if (layout == 0) { w = d0; jb = d1; k = (int)d2; }
  else if (layout == 1) { jb = d0; w = d1; k = (int)d2; }
  else { k = (int)d0; jb = d1; w = d2; }
}

// What the two write paths of seeds_mpc_join_kernel share, per element (member k = b - b0, control j, step t): the shifted plan of
// the source problem - the winner's, or the member's own with non-finite entries read as 0 where the group has none -, the
// member's sigma (0 for the elite slot and the padding controls), and base + sigma z as a rounded product and a rounded sum.
__device__ __forceinline__ double seeds_join_base(const SeedsJoinArgs& a, int M1, int src_b, int j, int t, bool from_winner) {
  const int ts = t + a.replan < M1 ? t + a.replan : M1 - 1;
  double v = a.u_bar[seeds_at(a.layout, a.B, a.m, M1, src_b, j, ts)];
  if (!from_winner && !(fabs(v) < INFINITY)) v = 0.0;
  return v;
}
__device__ __forceinline__ double seeds_join_sigma(const SeedsJoinArgs& a, int b, int j, bool elite) {
  return (a.sigma && !elite && j < a.m_user) ? a.sigma[(size_t)b * a.m + j] : 0.0;
}
__device__ __forceinline__ double seeds_rounded_add(double v, double sg, double z) {
  double sz = sg * z;
  asm volatile("" : "+v"(sz));                                   // the product is rounded before it is added (no FMA)
  return v + sz;
}

__global__ void __launch_bounds__(kSeedsThreads) seeds_mpc_join_kernel(SeedsJoinArgs a) {
  __shared__ double s_cost[kSeedsThreads / 64];
  __shared__ int s_idx[kSeedsThreads / 64], s_cnt[kSeedsThreads / 64];
  __shared__ double s_z[4][kSeedsThreads];
  const int g = (int)blockIdx.x, tid = (int)threadIdx.x, K = a.K, B = a.B;
  const int b0 = g * K;
  int winner, eligible;
  double win_cost;
  seeds_select(a.cost, a.status, b0, K, tid, s_cost, s_idx, s_cnt, winner, win_cost, eligible);
  if (tid == 0) {
    a.best[(size_t)g * 3 + 0] = (double)winner;
    a.best[(size_t)g * 3 + 1] = win_cost;
    a.best[(size_t)g * 3 + 2] = (double)eligible;
  }
  const bool from_winner = winner >= 0;
  const int elite = from_winner ? winner : 0;
  const int n = a.n, N = a.N, m = a.m, M1 = N - 1, rp = a.replan, layout = a.layout;

  // the K initial states (x0 is (B, n) in every layout) - with a plant the group's plant state, which every member's plant row
  // gets too -, and the log's flags: a failed seed replaced by the winner logs again, the members of a group whose plant has ended
  // do not
  for (size_t e = tid; e < (size_t)K * n; e += kSeedsThreads) {
    const int k = (int)(e / n), i = (int)(e - (size_t)k * n);
    const double v = a.plant_x ? a.plant_x[(size_t)g * n + i] : a.x_bar[seeds_at(layout, B, n, N, b0 + (from_winner ? winner : k), i, rp)];
    a.x0[(size_t)(b0 + k) * n + i] = v;
    if (a.plant_x) a.plant_rows[(size_t)(b0 + k) * n + i] = v;
  }
  const bool ended = a.plant_x && a.plant_ended[g] != 0.0;
  for (int k = tid; k < K; k += kSeedsThreads) {
    if (a.mpc_dead && (from_winner || ended)) a.mpc_dead[b0 + k] = ended ? 1.0 : 0.0;
    if (a.plant_x) a.plant_dead[b0 + k] = ended ? 1.0 : 0.0;
  }

  const uint32_t hold = (uint32_t)a.hold, W = (uint32_t)(((unsigned long long)M1 + hold - 1) / hold), JB = (uint32_t)(m + 3) >> 2;
  const uint32_t JJ = m < 4 ? (uint32_t)m : 4u, run = hold < (uint32_t)M1 ? hold : (uint32_t)M1;
  // the radices of an item's number, fastest first (seeds_item)
  const uint32_t r0 = layout == 0 ? W : (layout == 1 ? JB : (uint32_t)K), r1 = layout == 1 ? W : JB;
  const uint32_t k0 = (uint32_t)(a.seed & 0xffffffffull), k1 = (uint32_t)(a.seed >> 32);
  const size_t items = (size_t)K * JB * W;
  for (size_t tile0 = 0; tile0 < items; tile0 += kSeedsThreads) {
    const uint32_t IT = (uint32_t)(items - tile0 < (size_t)kSeedsThreads ? items - tile0 : (size_t)kSeedsThreads);
    uint32_t t0, t1, t2;                                         // the digits of the tile's first item (the same in every thread)
    seeds_mixed3(tile0, r0, r1, t0, t1, t2);
    if (run == 1 && JJ == 1) {
      // hold = 1 and m = 1: an item IS an element and there is nothing to share - the thread that draws the normal stores the
      // element, no LDS and no barrier (the condition is the same in every thread); items are numbered in address order
      if ((uint32_t)tid < IT) {
        int k; uint32_t jb, w;
        seeds_item(layout, (uint32_t)tid, t0, t1, t2, r0, r1, k, jb, w);
        const int t = (int)w, b = b0 + k;
        double v = seeds_join_base(a, M1, from_winner ? b0 + winner : b, 0, t, from_winner);
        const double sg = seeds_join_sigma(a, b, 0, k == elite);
        if (sg != 0.0) {
          uint32_t c[4] = {a.round, w, (uint32_t)b, kSeedsBlock};
          philox4x32_10(k0, k1, c);
          double z0, z1;
          box_muller(c[0], c[1], z0, z1);
          v = seeds_rounded_add(v, sg, z0);
        }
        a.u_guess[seeds_at(layout, B, m, M1, b, 0, t)] = v;
      }
      continue;
    }
    __syncthreads();                                             // (the previous tile's normals have been read)
    if ((uint32_t)tid < IT) {
      int k; uint32_t jb, w;
      seeds_item(layout, (uint32_t)tid, t0, t1, t2, r0, r1, k, jb, w);
      bool pair0 = false, pair1 = false;
      if (a.sigma && k != elite) {
        const double* sg = a.sigma + (size_t)(b0 + k) * m;
        const int j0 = (int)(jb << 2);
        pair0 = (j0 < a.m_user && sg[j0] != 0.0) || (j0 + 1 < a.m_user && sg[j0 + 1] != 0.0);
        pair1 = (j0 + 2 < a.m_user && sg[j0 + 2] != 0.0) || (j0 + 3 < a.m_user && sg[j0 + 3] != 0.0);
      }
      if (pair0 || pair1) {
        uint32_t c[4] = {a.round, w, (uint32_t)(b0 + k), kSeedsBlock + jb};
        philox4x32_10(k0, k1, c);
        if (pair0) { double z0, z1; box_muller(c[0], c[1], z0, z1); s_z[0][tid] = z0; s_z[1][tid] = z1; }
        if (pair1) { double z2, z3; box_muller(c[2], c[3], z2, z3); s_z[2][tid] = z2; s_z[3][tid] = z3; }
      }
    }
    __syncthreads();
    for (uint32_t s0 = 0; s0 < run; s0 += kSeedsJoinSteps) {
      const uint32_t S = run - s0 < (uint32_t)kSeedsJoinSteps ? run - s0 : (uint32_t)kSeedsJoinSteps, slots = IT * JJ * S;
      for (uint32_t q = tid; q < slots; q += kSeedsThreads) {
        uint32_t il, jj, s;
        if (layout == 0) { const uint32_t r = q / S; s = q - r * S; jj = r / IT; il = r - jj * IT; }
        else if (layout == 1) { const uint32_t r = q / JJ; jj = q - r * JJ; s = r / IT; il = r - s * IT; }
        else { const uint32_t r = q / IT; il = q - r * IT; s = r / JJ; jj = r - s * JJ; }
        int k; uint32_t jb, w;
        seeds_item(layout, il, t0, t1, t2, r0, r1, k, jb, w);
        const unsigned long long tt = (unsigned long long)w * hold + s0 + s;
        const int j = (int)((jb << 2) + jj);
        if (tt >= (unsigned long long)M1 || j >= m) continue;    // (the last window's tail, the last block's)
        const int t = (int)tt, b = b0 + k;
        double v = seeds_join_base(a, M1, from_winner ? b0 + winner : b, j, t, from_winner);
        const double sg = seeds_join_sigma(a, b, j, k == elite);
        if (sg != 0.0) v = seeds_rounded_add(v, sg, s_z[jj][il]);
        a.u_guess[seeds_at(layout, B, m, M1, b, j, t)] = v;
      }
    }
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

int launch_seeds_mpc_join(mi_ilqr* h, const SeedsJoinArgs& a) {
  if (a.K < 1 || a.B % a.K != 0 || a.hold < 1 || a.replan < 1 || a.replan >= a.N - 1 || a.layout < 0 || a.layout > 2) return MI_ILQR_E_BAD_ARG;
  if (!a.u_bar || !a.x_bar || !a.u_guess || !a.x0 || !a.cost || !a.status || !a.best) return MI_ILQR_E_BAD_ARG;
  if (a.plant_x && (!a.plant_ended || !a.plant_rows || !a.plant_dead)) return MI_ILQR_E_BAD_ARG;
  SeedsJoinArgs args = a;
  void* argv[] = {&args};
  HIPCHK(hipExtLaunchKernel(reinterpret_cast<const void*>(seeds_mpc_join_kernel), dim3((unsigned)(a.B / a.K)), dim3(kSeedsThreads), argv, 0,
                            h->stream, a.ev0, a.ev1, 0));
  return MI_ILQR_OK;
}

}  // namespace mi_host
#endif
