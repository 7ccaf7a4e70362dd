// libmi_ilqr.so, host side - memory and layout: the owner of the handle's device memory, the staged host -> device copy, the layout
// conversions between the kernels' layouts and the boundary's (host_internal.hpp: LAYOUT_*), and the protocol of the per-problem
// arrays (host.hpp: RowStore).  Calls nothing of the other host units.
#include <algorithm>
#include <cstring>
#include <vector>

#include "host_internal.hpp"

using namespace mi_host;

namespace {     // the kernels: global, as ever - their names do not change with the unit

// TL <-> TM: a per-problem (rows x len) transpose; both sides of a problem fit the caches, a gather is enough.
__global__ void __launch_bounds__(256) relayout_tm_kernel(const double* __restrict__ src, double* __restrict__ dst,
                                                            int rows, int len, int to_tm) {
  const size_t base = (size_t)blockIdx.x * rows * len;
  for (int e = threadIdx.x; e < rows * len; e += 256) {
    int r, t;
    if (to_tm) { t = e / rows; r = e - t * rows; dst[base + e] = src[base + (size_t)r * len + t]; }
    else { r = e / len; t = e - r * len; dst[base + e] = src[base + (size_t)t * rows + r]; }
  }
}

// TL <-> BM: for every row r a (B x len) <-> (len x B) transpose with pitches; 32 x 32 tiles through LDS
// so that both the reads and the writes are coalesced.  grid = (ceil(len/32), ceil(B/32), rows).
__global__ void __launch_bounds__(256) relayout_bm_kernel(const double* __restrict__ src, double* __restrict__ dst,
                                                            int B, int rows, int len, int to_bm) {
  __shared__ double tile[32][33];
  const int r = blockIdx.z, t0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;          // 32 x 8 threads
  if (to_bm) {
    for (int j = ty; j < 32; j += 8) {                             // read TL: t fastest
      const int b = b0 + j, t = t0 + tx;
      if (b < B && t < len) tile[j][tx] = src[((size_t)b * rows + r) * len + t];
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {                             // write BM: b fastest
      const int t = t0 + j, b = b0 + tx;
      if (b < B && t < len) dst[((size_t)t * rows + r) * B + b] = tile[tx][j];
    }
  } else {
    for (int j = ty; j < 32; j += 8) {                             // read BM: b fastest
      const int t = t0 + j, b = b0 + tx;
      if (b < B && t < len) tile[j][tx] = src[((size_t)t * rows + r) * B + b];
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {                             // write TL: t fastest
      const int b = b0 + j, t = t0 + tx;
      if (b < B && t < len) dst[((size_t)b * rows + r) * len + t] = tile[tx][j];
    }
  }
}

// One control sequence (m, len), time last, written for every problem in the handle's layout:
// layout 0 = [b][k][t] (wave-per-problem), 1 = [b][t][k] (workgroup-per-problem), 2 = [t][k][b] (lane-per-problem).
__global__ void __launch_bounds__(256) broadcast_u_kernel(const double* __restrict__ src, double* __restrict__ dst,
                                                            int B, int m, int len, int layout) {
  const size_t total = (size_t)B * m * len;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    int k, t;
    if (layout == 0) { const size_t r = e % ((size_t)m * len); k = (int)(r / len); t = (int)(r - (size_t)k * len); }
    else if (layout == 1) { const size_t r = e % ((size_t)m * len); t = (int)(r / m); k = (int)(r - (size_t)t * m); }
    else { const size_t r = e / B; t = (int)(r / m); k = (int)(r - (size_t)t * m); }
    dst[e] = src[(size_t)k * len + t];
  }
}

// Batched (R x C) -> (C x R) transposes with pitches, 32 x 32 tiles through LDS so that reads and writes are both coalesced: matrix
// z = (o, i), i < inner; element (r, c) is read at src[o src_outer + i src_inner + r src_r + c], written at dst[o dst_outer +
// i dst_inner + c dst_c + r].  The sample-minor <-> boundary conversions of mi_ilqr_policy_rollout.  grid = (ceil(C/32), ceil(R/32), <= Z).
__global__ void __launch_bounds__(256) transpose_tiles_kernel(const double* __restrict__ src, double* __restrict__ dst, int R, int C,
                                                                int Z, int inner, size_t src_outer, size_t src_inner, size_t src_r,
                                                                size_t dst_outer, size_t dst_inner, size_t dst_c) {
  __shared__ double tile[32][33];
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;          // 32 x 8 threads
  for (int z = blockIdx.z; z < Z; z += gridDim.z) {
    const int o = z / inner, i = z - o * inner;
    const double* s_ = src + (size_t)o * src_outer + (size_t)i * src_inner;
    double* d_ = dst + (size_t)o * dst_outer + (size_t)i * dst_inner;
    for (int j = ty; j < 32; j += 8) {
      const int r = r0 + j, c = c0 + tx;
      if (r < R && c < C) tile[j][tx] = s_[(size_t)r * src_r + c];
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
      const int c = c0 + j, r = r0 + tx;
      if (r < R && c < C) d_[(size_t)c * dst_c + r] = tile[tx][j];
    }
    __syncthreads();
  }
}

}  // namespace

namespace mi_host {

namespace {

// rows of the (rows,len) time-last view of a double field; 0 = not a trajectory array
int traj_rows(const mi_ilqr* h, int which, int* len) {
  const int n = h->n, m = h->m, N = h->N;
  switch (which) {
    case MI_F_X_BAR: case MI_F_X_TRIAL: *len = N; return n;
    case MI_F_U_BAR: case MI_F_U_TRIAL: case MI_F_KAPPA: *len = N - 1; return m;
    case MI_F_K: *len = N - 1; return m * n;
    case MI_F_FX: *len = N - 1; return n * n;
    case MI_F_FU: *len = N - 1; return n * m;
    case MI_F_DV: *len = N - 1; return 1;
  }
  *len = 0;
  return 0;
}

}  // namespace

int dev_alloc_bytes(mi_ilqr* h, void** p, size_t bytes, bool zero) {
  void* q = nullptr;
  HIPCHK(hipMalloc(&q, bytes));
  h->owned.push_back(q);
  if (zero) HIPCHK(hipMemset(q, 0, bytes));
  *p = q;
  return MI_ILQR_OK;
}
int dev_free_ptr(mi_ilqr* h, void* q) {
  if (!q) return MI_ILQR_OK;
  const auto it = std::find(h->owned.begin(), h->owned.end(), q);
  if (it != h->owned.end()) h->owned.erase(it);
  HIPCHK(hipFree(q));
  return MI_ILQR_OK;
}

int ensure_scratch(mi_ilqr* h, size_t bytes) {
  if (h->scratch_bytes >= bytes) return MI_ILQR_OK;
  HIPCHK(hipStreamSynchronize(h->stream));
  h->scratch_bytes = 0;
  int rc = dev_free(h, h->scratch);
  if (rc == MI_ILQR_OK) rc = dev_alloc(h, h->scratch, (bytes + 7) / 8);
  if (rc == MI_ILQR_OK) h->scratch_bytes = bytes;
  return rc;
}

// Convert between the handle's kernel layout and time-last, on the handle's stream.
int relayout(mi_ilqr* h, const double* src, double* dst, int rows, int len, bool to_kernel_layout) {
  if (layout_of(h) == LAYOUT_BM) {
    const dim3 grid((len + 31) / 32, (h->B + 31) / 32, rows);
    hipLaunchKernelGGL(relayout_bm_kernel, grid, dim3(256), 0, h->stream, src, dst, h->B, rows, len, to_kernel_layout ? 1 : 0);
  } else {
    hipLaunchKernelGGL(relayout_tm_kernel, dim3(h->B), dim3(256), 0, h->stream, src, dst, rows, len, to_kernel_layout ? 1 : 0);
  }
  HIPCHK(hipGetLastError());
  return MI_ILQR_OK;
}

// ... and one (m, N-1) control sequence for every problem, in the handle's layout
int broadcast_u(mi_ilqr* h, const double* one, double* dst) {
  const size_t total = (size_t)h->m * (h->N - 1) * h->B;
  const int blocks = (int)std::min<size_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(broadcast_u_kernel, dim3(blocks), dim3(256), 0, h->stream, one, dst, h->B, h->m, h->N - 1, layout_of(h));
  HIPCHK(hipGetLastError());
  return MI_ILQR_OK;
}

int transpose_tiles(mi_ilqr* h, const double* src, double* dst, int R, int C, size_t outer, int inner, size_t src_outer, size_t src_inner,
                    size_t src_r, size_t dst_outer, size_t dst_inner, size_t dst_c) {
  const size_t Z = outer * (size_t)inner;
  if (Z > 0x7fffffffull) return MI_ILQR_E_UNSUPPORTED;
  const dim3 grid((C + 31) / 32, (R + 31) / 32, (unsigned)std::min<size_t>(Z, 65535));
  if (grid.y > 65535) return MI_ILQR_E_UNSUPPORTED;
  hipLaunchKernelGGL(transpose_tiles_kernel, grid, dim3(256), 0, h->stream, src, dst, R, C, (int)Z, inner, src_outer, src_inner, src_r,
                     dst_outer, dst_inner, dst_c);
  HIPCHK(hipGetLastError());
  return MI_ILQR_OK;
}

// Does this double field cross the boundary through a layout conversion (relayout), and with which rows and length?  The
// trajectory arrays of the handles whose kernel layout is not time-last - except single-row ones in the time-major layout, which
// are the same bytes either way.  A control sequence handed to mi_ilqr_set_initial has MI_F_U_BAR's shape.
bool needs_relayout(const mi_ilqr* h, int which, int* rows, int* len) {
  const int layout = layout_of(h);
  *rows = layout == LAYOUT_TL ? 0 : traj_rows(h, which, len);
  return *rows > 1 || (layout == LAYOUT_BM && *rows == 1);
}

// Host -> device copy of a caller's (pageable) buffer, ordered on the handle's stream.  Small inputs go through
// the handle's page-locked staging block and an ASYNCHRONOUS copy: the call returns after a host memcpy, the
// kernels that follow on the stream see the data (a blocking hipMemcpy costs ~15-20 us each whatever its size).
// Large ones keep the runtime's own pipelined staging.
int stage_h2d(mi_ilqr* h, void* dst, const void* src, size_t bytes) {
  constexpr size_t kSmall = 256 * 1024;
  if (bytes > kSmall) {
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return MI_ILQR_OK;
  }
  if (!h->pin_in) {
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h->pin_in), 4 * kSmall, hipHostMallocDefault));
    for (hipEvent_t& e : h->pin_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    h->pin_off = 0;
  }
  if (h->pin_off + bytes > 4 * kSmall) {          // the block is used as a ring; wrap once the copies in flight are done
    for (hipEvent_t e : h->pin_ev) HIPCHK(hipEventSynchronize(e));      // (on either solve slot's stream; never recorded: done)
    h->pin_off = 0;
  }
  char* stage = h->pin_in + h->pin_off;
  std::memcpy(stage, src, bytes);
  HIPCHK(hipMemcpyAsync(dst, stage, bytes, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipEventRecord(h->pin_ev[h->stream == h->slots[1].stream ? 1 : 0], h->stream));
  h->pin_off += (bytes + 255) & ~(size_t)255;
  return MI_ILQR_OK;
}

// The protocol of a per-problem array (host.hpp: RowStore).  store_upload: (B, width) rows from the host become the array's contents
// and the handle enters its per-problem mode.  Rows that equal what the device already holds are not sent.  Kernels already enqueued
// (mi_ilqr_solve_async) read the previous rows: stage_h2d copies on the handle's stream, behind them.  The mirror is committed only
// once every copy is enqueued; a failed allocation or copy leaves the mode - the device copies are undefined then, and the handle
// falls back to what it can vouch for - and returns the error.
void store_drop(RowStore& s) {
  s.synced = false;
  s.mirror.clear();
}

int store_upload(mi_ilqr* h, RowStore& s, const double* src) {
  const size_t B = h->B, cnt = B * s.width;
  if (s.synced && std::memcmp(s.mirror.data(), src, cnt * 8) == 0) return MI_ILQR_OK;
  store_drop(s);
  HIPCHK(hipSetDevice(h->d.device_id));
  int rc = MI_ILQR_OK;
  if (!s.rows) rc = dev_alloc(h, s.rows, cnt);
  if (rc == MI_ILQR_OK && s.batch_minor_copy && !s.cols) rc = dev_alloc(h, s.cols, cnt);
  if (rc == MI_ILQR_OK) rc = stage_h2d(h, s.rows, src, cnt * 8);
  if (rc == MI_ILQR_OK && s.batch_minor_copy) {
    std::vector<double> cols(cnt);
    for (size_t b = 0; b < B; ++b)
      for (size_t k = 0; k < s.width; ++k) cols[k * B + b] = src[b * s.width + k];
    rc = stage_h2d(h, s.cols, cols.data(), cnt * 8);
  }
  if (rc != MI_ILQR_OK) return rc;
  s.mirror.assign(src, src + cnt);
  s.synced = true;
  return MI_ILQR_OK;
}

// ... and the same with ONE row for every problem
int store_upload_broadcast(mi_ilqr* h, RowStore& s, const double* row) {
  std::vector<double> rows((size_t)h->B * s.width);
  for (size_t b = 0; b < (size_t)h->B; ++b) std::memcpy(rows.data() + b * s.width, row, s.width * 8);
  return store_upload(h, s, rows.data());
}

// mi_ilqr_get of a per-problem array: the mirror; in shared mode `shared_row` for every problem, or zeros (nullptr)
int store_read(const mi_ilqr* h, const RowStore& s, const double* shared_row, double* dst, size_t bytes) {
  if (s.width == 0) return MI_ILQR_E_UNSUPPORTED;
  if (bytes != (size_t)h->B * s.width * 8) return MI_ILQR_E_BAD_SHAPE;
  if (s.synced) std::memcpy(dst, s.mirror.data(), bytes);
  else if (!shared_row) std::memset(dst, 0, bytes);
  else for (size_t b = 0; b < (size_t)h->B; ++b) std::memcpy(dst + b * s.width, shared_row, s.width * 8);
  return MI_ILQR_OK;
}

RowField row_field(mi_ilqr* h, int which) {
  switch (which) {
    case MI_F_X_NOM: return {&h->targets, shared_x_nom(h)};
    case MI_F_TARGET_STEP: return {&h->target_steps, nullptr};
    case MI_F_MODEL_PARAMS: return {&h->params, h->d.model_params};
    case MI_F_COST_MATRICES: return {&h->costs, h->h_costmat.data()};
    case MI_F_POLICY_NOISE: return {&h->policy_noise, nullptr};        // (not set: no noise, zeros)
    case MI_F_PLANT_STATE: return {&h->plant_state, nullptr};          // (mi_ilqr_get refuses it while the handle holds no plant)
    case MI_F_PLANT_PARAMS: return {&h->plant_params, h->d.model_params};   // (not set: the problem's model row, get_plant_field)
    case MI_F_PLANT_NOISE: return {&h->plant_noise, nullptr};
    case MI_F_POLICY_MC_DIST: return {&h->policy_mc_dist, nullptr};    // (not set: zeros)
    case MI_F_POLICY_MC_BOX: return {&h->mc_box, nullptr};             // (the same)
    case MI_F_SEEDS_SIGMA: return {&h->seeds_sigma, nullptr};          // (the same)
  }
  return {nullptr, nullptr};
}

// The lane-per-problem kernels' per-problem-cost instantiations on a handle with ONE target: its x_nom as (B, n) rows.
int refresh_lane_target_rows(mi_ilqr* h) {
  RowStore& s = h->lane_targets;      // (only ever one row repeated: the first says what all of them are, on every launch)
  if (s.synced && std::memcmp(s.mirror.data(), shared_x_nom(h), s.width * 8) == 0) return MI_ILQR_OK;
  return store_upload_broadcast(h, s, shared_x_nom(h));
}

// Per-problem targets (MI_F_X_NOM / MI_F_TARGET_STEP): the two arrays enter and leave their mode together.
void drop_per_problem_targets(mi_ilqr* h) {
  store_drop(h->targets);
  store_drop(h->target_steps);
  h->target_steps_moving = false;
}

int upload_target_rows(mi_ilqr* h, RowStore& s, const double* src) {
  const int rc = store_upload(h, s, src);
  if (rc != MI_ILQR_OK) drop_per_problem_targets(h);
  return rc;
}

}  // namespace mi_host
