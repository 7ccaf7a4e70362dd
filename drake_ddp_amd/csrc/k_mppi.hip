// The sampling-based MPC kernels.  mppi.hpp holds what a model's unit needs - the sampled rollout, one lane per sample,
// and the two functions that form a sample's applied control - and this unit instantiates it for every built-in model.  The kernels
// WITHOUT a model - the update, the staging copy, the hand-over - and their launchers (declared in host.hpp) are defined here and
// nowhere else, so a plugin unit, which includes mppi.hpp for its model's rollout, compiles and carries none of them.
#include "mppi.hpp"

namespace mi {

// (cost, sample): a is replaced by b when b is the better pair - a total order
__device__ __forceinline__ void mppi_better(double& c, int& i, double oc, int oi) {
  const bool take = oc < c || (oc == c && oi < i);
  c = take ? oc : c;
  i = take ? oi : i;
}

__global__ void __launch_bounds__(kMppiThreads) mppi_update_kernel(mi_host::MppiUpdateArgs a) {
  __shared__ double s_w[kMppiTile];
  __shared__ double s_cost[kMppiThreads / 64];
  __shared__ int s_idx[kMppiThreads / 64], s_cnt[kMppiThreads / 64];
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, S = a.S, m = a.m, M1 = a.N - 1;
  const double* L = a.cost + (size_t)b * S;

  // 1. the least finite cost, its sample, the finite count
  double c = INFINITY;
  int ci = 0x7fffffff, cnt = 0;
  for (int s = tid; s < S; s += kMppiThreads) {
    const double ck = L[s];
    if (fabs(ck) < INFINITY) {                                      // (a NaN compares false)
      ++cnt;
      mppi_better(c, ci, ck, s);
    }
  }
  // all 256 threads are here: the DPP moves below read every lane
  mppi_better(c, ci, row_xor_f64<1>(c), row_xor_i32<1>(ci)); cnt += row_xor_i32<1>(cnt);
  mppi_better(c, ci, row_xor_f64<2>(c), row_xor_i32<2>(ci)); cnt += row_xor_i32<2>(cnt);
  mppi_better(c, ci, row_xor_f64<4>(c), row_xor_i32<4>(ci)); cnt += row_xor_i32<4>(cnt);
  mppi_better(c, ci, row_xor_f64<8>(c), row_xor_i32<8>(ci)); cnt += row_xor_i32<8>(cnt);
  double Lmin = readlane_f64(c, 0);
  int best = __builtin_amdgcn_readlane(ci, 0), nfin = __builtin_amdgcn_readlane(cnt, 0);
#pragma unroll
  for (int r = 16; r < 64; r += 16) {
    mppi_better(Lmin, best, readlane_f64(c, r), __builtin_amdgcn_readlane(ci, r));
    nfin += __builtin_amdgcn_readlane(cnt, r);
  }
  if ((tid & 63) == 0) { s_cost[tid >> 6] = Lmin; s_idx[tid >> 6] = best; s_cnt[tid >> 6] = nfin; }
  __syncthreads();
  Lmin = s_cost[0]; best = s_idx[0]; nfin = s_cnt[0];
#pragma unroll
  for (int wv = 1; wv < kMppiThreads / 64; ++wv) {
    mppi_better(Lmin, best, s_cost[wv], s_idx[wv]);
    nfin += s_cnt[wv];
  }

  // 2. the weights, tile by tile: s_w[s - tile0] = e_s (Z == 0) or e_s / Z; -1 marks a non-finite sample
  const double T = a.temperature;
  int resident = -1;                                                // the tile whose NORMALISED weights are in LDS
  auto fill = [&](int tile0, double Z) {
    __syncthreads();                                                // (the previous contents have been read)
    const int end = S - tile0 < kMppiTile ? S - tile0 : kMppiTile;
    for (int q = tid; q < end; q += kMppiThreads) {
      const int s = tile0 + q;
      const double Ls = L[s];
      double e = -1.0;
      if (fabs(Ls) < INFINITY) {
        e = T == 0.0 ? (s == best ? 1.0 : 0.0) : exp(-(Ls - Lmin) / T);
        if (Z != 0.0) e = e / Z;
      }
      s_w[q] = e;
    }
    __syncthreads();
    return end;
  };
  double Z = 0.0, Q = 0.0;
  if (nfin > 0) {                                                   // (the same in every thread)
    for (int tile0 = 0; tile0 < S; tile0 += kMppiTile) {
      const int end = fill(tile0, 0.0);
      for (int q = 0; q < end; ++q) { const double e = s_w[q]; if (e >= 0.0) Z += e; }
    }
    for (int tile0 = 0; tile0 < S; tile0 += kMppiTile) {
      const int end = fill(tile0, Z);
      resident = tile0;
      for (int q = 0; q < end; ++q) { const double wq = s_w[q]; if (wq >= 0.0) Q += wq * wq; }
    }
  }

  // 3. the log rows
  if (tid == 0) {
    a.best[(size_t)b * 3 + 0] = nfin > 0 ? (double)best : -1.0;
    a.best[(size_t)b * 3 + 1] = nfin > 0 ? Lmin : INFINITY;
    a.best[(size_t)b * 3 + 2] = (double)nfin;
    a.costlog[(size_t)b * 2 + 0] = L[0];
    a.costlog[(size_t)b * 2 + 1] = nfin > 0 ? 1.0 / Q : __builtin_nan("");
  }

  // 4. the blend
  const int JB = (m + 3) >> 2, items = M1 * JB;
  const uint32_t k0 = (uint32_t)(a.seed & 0xffffffffull), k1 = (uint32_t)(a.seed >> 32);
  const double* lim = a.ulim ? a.ulim + (size_t)b * 2 * m : nullptr;
  const double* uin = a.nom_in + (size_t)b * M1 * m;
  double* uout = a.nom_out + (size_t)b * M1 * m;
  for (int item0 = 0; item0 < items; item0 += kMppiThreads) {
    const int item = item0 + tid;
    const bool valid = item < items;
    const int t = valid ? item / JB : 0, jb = valid ? item - t * JB : 0;
    double u[4], sg[4], acc[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int k = 4 * jb + jj;
      u[jj] = (valid && k < m) ? uin[(size_t)t * m + k] : 0.0;
      sg[jj] = (valid && a.sigma && k < a.m_user && k < m) ? a.sigma[(size_t)b * m + k] : 0.0;
      acc[jj] = 0.0;
    }
    const bool pair0 = sg[0] != 0.0 || sg[1] != 0.0, pair1 = sg[2] != 0.0 || sg[3] != 0.0;
    const uint32_t w = (uint32_t)(t / a.hold);
    bool first = true;
    if (nfin > 0) {
      for (int tile0 = 0; tile0 < S; tile0 += kMppiTile) {
        int end = S - tile0 < kMppiTile ? S - tile0 : kMppiTile;
        if (resident != tile0) { end = fill(tile0, Z); resident = tile0; }
        if (!valid) continue;
        for (int q = 0; q < end; ++q) {
          const double wq = s_w[q];
          if (!(wq >= 0.0)) continue;                               // a non-finite sample: skipped
          const int s = tile0 + q;
          double z[4] = {0.0, 0.0, 0.0, 0.0};
          if (s != 0 && (pair0 || pair1)) mppi_block_normals(k0, k1, a.sample0 + (uint32_t)s, w, (uint32_t)b, (uint32_t)jb, pair0, pair1, z);
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            const int k = 4 * jb + jj;
            if (k < m) {
              const double v = mppi_applied(u[jj], s == 0 ? 0.0 : sg[jj], z[jj], lim, m, k);
              double pr = wq * v;
              asm volatile("" : "+v"(pr));                          // a rounded product, then a rounded sum
              acc[jj] = first ? pr : acc[jj] + pr;
            }
          }
          first = false;
        }
      }
    }
    if (valid) {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int k = 4 * jb + jj;
        if (k < m) {
          double r = u[jj];                                         // a problem without a finite sample keeps u
          if (nfin > 0) {
            r = acc[jj];
            if (lim) { const double lo = lim[k], hi = lim[m + k]; r = r < lo ? lo : (r > hi ? hi : r); }
          }
          uout[(size_t)t * m + k] = r;
        }
      }
    }
  }
}

// element (b, row, t) of a (B, rows, len) trajectory array in the handle's layout (0 [b][row][t], 1 [b][t][row], 2 [t][row][b])
__device__ __forceinline__ size_t mppi_at(int layout, int B, int rows, int len, int b, int r, int t) {
  if (layout == 0) return ((size_t)b * rows + r) * len + t;
  if (layout == 1) return ((size_t)b * len + t) * rows + r;
  return ((size_t)t * rows + r) * B + b;
}
// ... and the (b, row, t) of element e of that array
__device__ __forceinline__ void mppi_from(int layout, int B, int rows, int len, size_t e, int& b, int& r, int& t) {
  if (layout == 0) { t = (int)(e % len); const size_t q = e / len; r = (int)(q % rows); b = (int)(q / rows); }
  else if (layout == 1) { r = (int)(e % rows); const size_t q = e / rows; t = (int)(q % len); b = (int)(q / len); }
  else { b = (int)(e % B); const size_t q = e / B; r = (int)(q % rows); t = (int)(q / rows); }
}

// the nominal from the handle's layout (src == nullptr: zeros) into the time-major staging copy (B, N-1, m)
__global__ void __launch_bounds__(256) mppi_stage_kernel(const double* __restrict__ src, double* __restrict__ nom, int B, int m, int M1, int layout) {
  const size_t total = (size_t)B * m * M1;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    int b, r, t;
    mppi_from(1, B, m, M1, e, b, r, t);
    nom[e] = src ? src[mppi_at(layout, B, m, M1, b, r, t)] : 0.0;
  }
}

// the final nominal -> u_guess in the handle's layout, shifted (walked in the layout's order: element e is address e), the
// time-last copy, and the closing row of the cost log: the closing rollout's cost | NaN
__global__ void __launch_bounds__(256) mppi_handover_kernel(const double* __restrict__ nom, double* __restrict__ u_guess, double* __restrict__ tl,
                                                              const double* __restrict__ cost1, double* __restrict__ costlog, int B, int m,
                                                              int M1, int layout, int shift) {
  const size_t total = (size_t)B * m * M1, first = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  for (size_t e = first; e < total; e += stride) {
    int b, r, t;
    mppi_from(layout, B, m, M1, e, b, r, t);
    const int ts = t + shift < M1 ? t + shift : M1 - 1;
    u_guess[e] = nom[mppi_at(1, B, m, M1, b, r, ts)];
  }
  for (size_t e = first; e < total; e += stride) {
    int b, r, t;
    mppi_from(0, B, m, M1, e, b, r, t);
    tl[e] = nom[mppi_at(1, B, m, M1, b, r, t)];
  }
  for (size_t e = first; e < (size_t)B; e += stride) {
    costlog[e * 2 + 0] = cost1[e];
    costlog[e * 2 + 1] = __builtin_nan("");
  }
}

}  // namespace mi

namespace mi_host {

int launch_mppi_update(mi_ilqr* h, const MppiUpdateArgs& a) {
  if (a.B < 1 || a.S < 1 || a.m < 1 || a.N < 2 || a.hold < 1 || !a.nom_in || !a.nom_out || a.nom_in == a.nom_out || !a.cost || !a.best || !a.costlog)
    return MI_ILQR_E_BAD_ARG;
  MppiUpdateArgs args = a;
  void* argv[] = {&args};
  HIPCHK(hipExtLaunchKernel(reinterpret_cast<const void*>(mi::mppi_update_kernel), dim3((unsigned)a.B), dim3(mi::kMppiThreads), argv, 0, h->stream,
                            a.ev0, a.ev1, 0));
  return MI_ILQR_OK;
}

static unsigned mppi_blocks(size_t total) { const size_t bl = (total + 255) / 256; return (unsigned)(bl < 8192 ? (bl ? bl : 1) : 8192); }

int launch_mppi_stage(mi_ilqr* h, const double* src, double* nom, int B, int m, int N, int layout, hipEvent_t ev0) {
  if (!nom || B < 1 || m < 1 || N < 2 || layout < 0 || layout > 2) return MI_ILQR_E_BAD_ARG;
  int M1 = N - 1;
  void* argv[] = {&src, &nom, &B, &m, &M1, &layout};
  HIPCHK(hipExtLaunchKernel(reinterpret_cast<const void*>(mi::mppi_stage_kernel), dim3(mppi_blocks((size_t)B * m * M1)), dim3(256), argv, 0,
                            h->stream, ev0, nullptr, 0));
  return MI_ILQR_OK;
}

int launch_mppi_handover(mi_ilqr* h, const double* nom, double* u_guess, double* tl, const double* cost1, double* costlog, int B, int m, int N,
                         int layout, int shift, hipEvent_t ev1) {
  if (!nom || !u_guess || !tl || !cost1 || !costlog || B < 1 || m < 1 || N < 2 || layout < 0 || layout > 2 || shift < 0 || shift > N - 2)
    return MI_ILQR_E_BAD_ARG;
  int M1 = N - 1;
  void* argv[] = {&nom, &u_guess, &tl, &cost1, &costlog, &B, &m, &M1, &layout, &shift};
  HIPCHK(hipExtLaunchKernel(reinterpret_cast<const void*>(mi::mppi_handover_kernel), dim3(mppi_blocks((size_t)B * m * M1)), dim3(256), argv, 0,
                            h->stream, nullptr, ev1, 0));
  return MI_ILQR_OK;
}

}  // namespace mi_host

template int mi_host::launch_mppi_rollout<mi::Pendulum>(mi_ilqr*, const mi_host::MppiArgs&);
template int mi_host::launch_mppi_rollout<mi::Acrobot>(mi_ilqr*, const mi_host::MppiArgs&);
template int mi_host::launch_mppi_rollout<mi::CartPole>(mi_ilqr*, const mi_host::MppiArgs&);
template int mi_host::launch_mppi_rollout<mi::CartPoleWall>(mi_ilqr*, const mi_host::MppiArgs&);
template int mi_host::launch_mppi_rollout<mi::Synth36>(mi_ilqr*, const mi_host::MppiArgs&);
template int mi_host::launch_mppi_rollout<mi::PlanarQuad>(mi_ilqr*, const mi_host::MppiArgs&);
template int mi_host::launch_mppi_rollout<mi::Quad3D>(mi_ilqr*, const mi_host::MppiArgs&);
template int mi_host::launch_mppi_rollout<mi::Arm27>(mi_ilqr*, const mi_host::MppiArgs&);
template int mi_host::launch_mppi_rollout<mi::Arm27C>(mi_ilqr*, const mi_host::MppiArgs&);
