// The LDS layouts of the wave-per-problem kernels (Lay, WS, carve) and of the workgroup-per-problem kernels (LLay), with the byte
// counts the host asks for (ws_bytes, large_lds_bytes, large_lds_bytes_hbm) next to the code that carves them.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace mi {

// ---------------------------------------------------------------------------
// LDS layout: array-of-records, ONE record per time step, so that everything a
// sequential step touches is reachable from a single per-step pointer with
// compile-time (immediate) offsets — no per-access address arithmetic in the
// latency-critical loops, and adjacent fields fuse into ds_read2/ds_read_b128.
//   G_t  nominal trajectory + gains : x_bar[n] | K[m][n] | u_bar[m] | kappa[m], dV
//   T_t  trial trajectory           : x[n] | u[m]
//   J_t  dynamics partials          : fx[n][n] | fu[n][m]
// (HBM keeps the reference's time-last layout; the staging copy transposes.)
// Each array has one pad record before index 0 and after the last index so the
// one-step-ahead software prefetch never needs a clamp.
// ---------------------------------------------------------------------------
template <int n, int m>
struct Lay {
  static constexpr int even(int v) { return (v + 1) & ~1; }
  static constexpr int XB = 0;
  static constexpr int KK = even(n);
  static constexpr int UB = KK + even(m * n);
  static constexpr int KAP = UB + even(m);
  static constexpr int DV = KAP + m;
  // n = 2 (the passes over time are lane-chunked there: Riccati scan, Newton rollout): record strides
  // are ODD numbers of doubles, so lanes reading consecutive records hit 32 different bank pairs and
  // lanes owning chunks of 2..4 consecutive records conflict at most 4-way instead of 32-way.  Larger
  // n keeps 16-byte aligned records (b128 loads in the wave-uniform sweeps matter more there).
  static constexpr int pad(int v) { return n <= 2 ? (v | 1) : even(v); }
  static constexpr int GS = pad(DV + 1);
  static constexpr int XN = 0, UN = even(n), TS = pad(UN + m);
  static constexpr int FX = 0, FU = even(n * n), JS = pad(FU + n * m);
  static constexpr int DUMP_DOUBLES = 64 * 2 + (GS > JS ? GS : JS);   // 16 B per lane + one record of slack
  // copy of the cost constants (Consts<M>) for code that runs outside the kernel function (outlined passes)
  static constexpr int CST_DOUBLES = (n >= 3) ? even(2 * n * n + m * m + 3 * n) : 0;
};

struct WS {
  double *G, *T, *J;       // point at record index 0 (pad record lives at index -1)
  double* dump;            // per-lane sink for predicated-off stores (lane*16 B)
  double* cst;             // Consts<M> image (n >= 3)
  int *kp, *aux, *need, *binA, *binB;
  int N;
  int n_store, t_stride;   // T holds n_store trajectories, t_stride doubles apart
};

template <int n, int m>
__host__ __device__ constexpr size_t ws_bytes(int N, int n_store = 1) {
  using L = Lay<n, m>;
  return ((size_t)(N + 2) * L::GS + (size_t)n_store * (N + 2) * L::TS + (size_t)(N + 2) * L::JS + L::DUMP_DOUBLES + L::CST_DOUBLES) * 8 +
         (size_t)7 * N * 4 + 16;
}

template <int n, int m>
__device__ inline WS carve(char* base, int N, int n_store) {
  using L = Lay<n, m>;
  WS w;
  w.N = N;
  double* p = reinterpret_cast<double*>(base);
  w.G = p + L::GS; p += (size_t)(N + 2) * L::GS;
  w.T = p + L::TS; p += (size_t)n_store * (N + 2) * L::TS;
  w.n_store = n_store; w.t_stride = (N + 2) * L::TS;
  w.J = p + L::JS; p += (size_t)(N + 2) * L::JS;
  w.dump = p; p += L::DUMP_DOUBLES;
  w.cst = p; p += L::CST_DOUBLES;
  int* q = reinterpret_cast<int*>(p);
  w.kp = q; q += N;
  w.aux = q; q += N;
  w.need = q; q += N;
  w.binA = q; q += 2 * N;
  w.binB = q;
  return w;
}

// ---------------------------------------------------------------------------
// Workgroup-per-problem kernels (ilqr_large.hpp): one fixed block of doubles per workgroup (LLay), the per-step cost
// gradients behind it, then the integer scratch of the key-point code.
// ---------------------------------------------------------------------------
constexpr int kLargeThreads = 256;
constexpr int kPdFlag = 8;          // slot of the reduction scratch (LLay::oRed) where a backward pass leaves "a Quu was not positive definite"
// Control limits (Limited<M> kernels of the mid-size family, mi_ilqr_set_control_limits): further slots of the reduction scratch
// (block_sum uses 0..3) - S2 = sum_t kappa_t^T Quu_t kappa_t of the last backward pass, and the problem's bounds u_min | u_max,
// read once per launch.  The LDS layout and large_lds_bytes stay what they are.
constexpr int kS2Slot = 9, kLimSlot = 16;

template <int n, int m>
struct LLay {
  static constexpr int nm = n + m;
  // doubles
  static constexpr int QC = m * (m + 1) / 2;               // packed lower triangle of Quu
  static constexpr int T16 = 16;                           // MFMA tile edge
  static constexpr int NP = ((n + 15) / 16) * 16;          // n padded to whole tiles (rows of Vxx)
  static constexpr int KN = (n + 3) / 4, NK = 4 * KN;      // MFMA k-steps over a contraction of length n, n padded to them
  // Columns of the augmented matrices F = [fx | fu], T1, H.  COMPACT: u follows x directly and the last column tile
  // holds the tail of x together with all of u (n = 36, m = 12: three tiles).  SPLIT (that tile would not start inside
  // x, or n is not a multiple of 4: n = 37): x is padded to whole tiles and u gets a tile of its own - the pad
  // rows / columns are zero and never stored, so Quu still sits at the corner of the last diagonal tile.
  // MID (n <= 32: one or two row tiles, any m <= 16 - mid_backward): always split, and always 48 columns - a row stride
  // of 48 doubles keeps the four rows of a k-step on disjoint banks for the 64-bit reads (32 would put them on the same).
  static constexpr bool kMid = n <= 32;
  static constexpr int NMPc = ((nm + 15) / 16) * 16;
  // (COMPACT only when x's tail and u fill the last tile exactly - (36, 12), (40, 8): with pad columns behind u, Quu would not
  //  end at the tile's corner, which the solver wave's row mapping relies on; (36, 4), (36, 8), (40, 4) take the split layout)
  static constexpr bool kSplit = kMid || !(NMPc - 16 <= n && n % 4 == 0 && nm == NMPc);
  static constexpr int UC = kSplit ? NP : n;               // column of u_0
  static constexpr int NMP = kMid ? 48 : (kSplit ? NP + ((m + 15) / 16) * 16 : NMPc);
  static constexpr int TS = NMP + 4;                       // row stride of T1 / H: whole tiles + the Vx/first-order column
  static constexpr int VS = NK | 1;                        // odd row stride of Vxx: conflict-free column-of-tile reads
  static constexpr int oQ = 0, oQf = oQ + n * n, oR = oQf + n * n, oXnom = oR + m * m, oQn = oXnom + n,
                       oQfn = oQn + n, oVxx = oQfn + n, oVx = oVxx + NP * VS, oF = oVx + NK + (NK & 1),
                       oT1 = oF + NK * NMP, oH = oT1 + NK * TS, oXs = oH + NMP * TS, oUs = oXs + n,
                       oRed = oUs + m, oXb = oRed + kLargeThreads, oQc = oXb + n + m + ((n + m) & 1),
                       oQT = oQc + m * m + m + (m & 1), oS = oQT + (kSplit ? 0 : n * n + ((n * n) & 1)),
                       oEnd = oS + 16 * 17 + 1;                // 16x16 tile, odd row stride
  static constexpr size_t doubles = oEnd + 8;
};

// Integer scratch of the key-point code: five arrays of N (or 2 N) ints - and, while every step is a key-point, the home of the
// cluster hand-shake's state (aux[0..3], the leader's six counters / a helper's last round in `need`): each array is therefore
// at least kIntRowMin ints long.  (Round 5's last session moved that state from registers into these arrays; with N = 3 aux[3]
// WAS need[0] - the leader's round counter - and every clustered solve of a three-step horizon ended with MI_STATUS_INTERNAL.  Found
// in round 6 by running the GPU suite with clusters forced: test_shortest_horizons_vs_c_oracle swallowed the RuntimeError.)
constexpr int kIntRowMin = 8;
__host__ __device__ constexpr int int_row(int N) { return N > kIntRowMin ? N : kIntRowMin; }
template <int n, int m>
__host__ __device__ constexpr size_t large_lds_bytes(int N) {
  // fixed block + per-step cost gradients [N][n+m] + integer scratch of the key-point code
  return (LLay<n, m>::doubles + (size_t)N * (n + m)) * 8 + (size_t)7 * int_row(N) * 4 + 16;
}

// Horizons whose cost gradients do not fit next to the fixed block any more (N > 148 for (36, 12), > 319 for (27, 7)): the
// gradients go to HBM (KArgs::lxu) and LDS keeps the fixed block + the key-point scratch - a slower backward step (one L2 read
// of lx_t | lu_t per step on the wave that forms the first-order column), but no horizon limit short of 160 KB of integers.
template <int n, int m>
__host__ __device__ constexpr size_t large_lds_bytes_hbm(int N) {
  return (size_t)LLay<n, m>::doubles * 8 + (size_t)7 * int_row(N) * 4 + 16;
}

}  // namespace mi
