// Lane and wave primitives that more than one kernel family uses: opaque lane index, lane-0 broadcast, wave / team rendezvous,
// the write-through result store, DPP row moves and the fixed-order wave sum.  Each is defined before its first use.
#pragma once
#include <hip/hip_runtime.h>

namespace mi {

// threadIdx.x behind an empty asm, for the STAGES of a solve kernel (a rollout, a linearization, a backward pass): what a stage
// derives from its lane index is loop-invariant for the solve loop around the stages, the compiler hoists it out of that loop,
// and the hoisted values - dozens of lane-dependent addresses per stage - then live across every other stage and get spilled in
// whichever inner loop is tightest.  Opaque per call, they are formed at the top of the stage and die with it (measured on the
// workgroup-per-problem kernels, round 5: backward pass of the arm 6.2 k -> 5.5 k cycles per step, of the coupled arm 7.4 k -> 5.5 k;
// on the wave-per-problem kernels of ilqr_small.hpp it changes nothing - C2 43.19 M it/s either way - and they keep threadIdx.x).
__device__ __forceinline__ int stage_lane() {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

__device__ __forceinline__ double bcast_lane0(double v) {
  union { double d; int i[2]; } u;
  u.d = v;
  u.i[0] = __builtin_amdgcn_readfirstlane(u.i[0]);
  u.i[1] = __builtin_amdgcn_readfirstlane(u.i[1]);
  return u.d;
}

// One wavefront owns a problem's LDS outside the linearization: ordering its own LDS traffic needs
// no s_barrier (LDS executes a wave's operations in order), only that the compiler keeps the order
// and waits for completion.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// Rendezvous of the main wave with its helper waves (LDS traffic only).
__device__ __forceinline__ void team_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Result write-back store that goes THROUGH the L2 (device-scope relaxed store = sc1): most waves of a launch
// finish long before its slowest problem, and lines they leave dirty would all be written back by the
// end-of-kernel release, i.e. inside the gap before the next dispatch.
__device__ __forceinline__ void wt_store(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Sum over each 16-lane row, result in every lane of the row: four DPP row rotations (8, 4, 2, 1)
// instead of four ds_bpermute round trips through the LDS crossbar.
template <int ROT>
__device__ __forceinline__ double row_ror_f64(double v) {
  union { double d; int i[2]; } u, r;
  u.d = v;
  r.i[0] = __builtin_amdgcn_mov_dpp(u.i[0], 0x120 + ROT, 0xF, 0xF, true);
  r.i[1] = __builtin_amdgcn_mov_dpp(u.i[1], 0x120 + ROT, 0xF, 0xF, true);
  return r.d;
}
__device__ __forceinline__ double row16_sum(double p) {
  p += row_ror_f64<8>(p);
  p += row_ror_f64<4>(p);
  p += row_ror_f64<2>(p);
  p += row_ror_f64<1>(p);
  return p;
}

// value of lane (this lane ^ D) of this lane's 16-lane row, D = 1, 2, 4, 8 - the partner of a butterfly level: quad permutations
// for 1 and 2, the half-row mirror (^ 7) followed by the reversed quad (^ 3) for 4, the rotation by 8 for 8.  DPP moves only.
template <int D>
__device__ __forceinline__ int row_xor_i32(int v) {
  static_assert(D == 1 || D == 2 || D == 4 || D == 8, "a lane distance inside a 16-lane row");
  if constexpr (D == 1) return __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true);                    // quad_perm:[1,0,3,2]
  else if constexpr (D == 2) return __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, true);               // quad_perm:[2,3,0,1]
  else if constexpr (D == 4)
    return __builtin_amdgcn_mov_dpp(__builtin_amdgcn_mov_dpp(v, 0x141, 0xF, 0xF, true), 0x1B, 0xF, 0xF, true);   // row_half_mirror, quad_perm:[3,2,1,0]
  else return __builtin_amdgcn_mov_dpp(v, 0x128, 0xF, 0xF, true);                                    // row_ror:8
}
template <int D>
__device__ __forceinline__ double row_xor_f64(double v) {
  union { double d; int i[2]; } u, r;
  u.d = v;
  r.i[0] = row_xor_i32<D>(u.i[0]);
  r.i[1] = row_xor_i32<D>(u.i[1]);
  return r.d;
}

// value of lane LANE of this lane's 16-lane row, for a double: one v_mov_b64_dpp row_newbcast
// (gfx90a+ DPP64).  bound_ctrl with full row/bank masks: every lane is written.
template <int LANE>
__device__ __forceinline__ double row_share(double v) {
  return __builtin_amdgcn_update_dpp(v, v, 0x150 + LANE, 0xF, 0xF, true);
}

// value of `v` in lane `srclane` (wave-uniform index), through v_readlane
__device__ __forceinline__ double readlane_f64(double v, int srclane) {
  union { double d; int i[2]; } u;
  u.d = v;
  u.i[0] = __builtin_amdgcn_readlane(u.i[0], srclane);
  u.i[1] = __builtin_amdgcn_readlane(u.i[1], srclane);
  return u.d;
}

// Sum over the wave, result in every lane, fixed order: DPP row sums, then the four row totals
// through v_readlane (SGPRs) - no ds_bpermute round trips.
__device__ __forceinline__ double wave_sum(double v) {
  v = row16_sum(v);
  return (readlane_f64(v, 0) + readlane_f64(v, 16)) + (readlane_f64(v, 32) + readlane_f64(v, 48));
}

// value of `v` in lane `src` (any lane; out-of-range callers mask the result)
__device__ __forceinline__ double lane_read_f64(double v, int src) {
  union { double d; int i[2]; } u, r;
  u.d = v;
  r.i[0] = __builtin_amdgcn_ds_bpermute(src << 2, u.i[0]);
  r.i[1] = __builtin_amdgcn_ds_bpermute(src << 2, u.i[1]);
  return r.d;
}

// A DPP move of a double that delivers 0 where there is no source lane (CTRL: the DPP control, ROWS: the row mask)
template <int CTRL, int ROWS>
__device__ __forceinline__ double dpp_f64_or_zero(double v) {
  union { double d; int i[2]; } u, r;
  u.d = v;
  if constexpr (ROWS == 0xF) {                                              // no source lane: 0 (bound_ctrl)
    r.i[0] = __builtin_amdgcn_mov_dpp(u.i[0], CTRL, 0xF, 0xF, true);
    r.i[1] = __builtin_amdgcn_mov_dpp(u.i[1], CTRL, 0xF, 0xF, true);
  } else {                                                                  // row not selected: 0 (old value)
    r.i[0] = __builtin_amdgcn_update_dpp(0, u.i[0], CTRL, ROWS, 0xF, true);
    r.i[1] = __builtin_amdgcn_update_dpp(0, u.i[1], CTRL, ROWS, 0xF, true);
  }
  return r.d;
}

}  // namespace mi
