// Counter-based random numbers for the noisy policy rollouts (policy_rollout.hpp, NZ = true): Philox4x32-10 (Salmon, Moraes, Dror,
// Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11 - the Random123 library's known-answer vectors are in
// tests/test_policy_noise_oracle.py) and the Box-Muller transform of its words into standard normals.  A leaf header: a block of
// four words is a pure function of (key, counter), so a normal depends on nothing but what the caller puts into them - no state,
// no memory, no dependence on the launch geometry.  tests/policy_noise_np.py is the NumPy statement of the same thing.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MI_PHILOX_HD __host__ __device__
#else
#define MI_PHILOX_HD
#endif

namespace mi {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;      // round multipliers
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;      // Weyl increments of the key

MI_PHILOX_HD inline uint32_t philox_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

// c[0..3] <- Philox4x32-10 of the counter c under the key (k0, k1)
MI_PHILOX_HD inline void philox4x32_10(uint32_t k0, uint32_t k1, uint32_t (&c)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = philox_mulhi(kPhiloxM0, c[0]), lo0 = kPhiloxM0 * c[0];
    const uint32_t hi1 = philox_mulhi(kPhiloxM1, c[2]), lo1 = kPhiloxM1 * c[2];
    c[0] = hi1 ^ c[1] ^ k0;
    c[1] = lo1;
    c[2] = hi0 ^ c[3] ^ k1;
    c[3] = lo0;
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
}

#if defined(__HIPCC__)
// Two words -> two independent standard normals: u_a = (wa + 1/2) 2^-32 and u_b = (wb + 1/2) 2^-32 are exact in fp64 and lie in
// (0, 1); z0 = r cos(2 pi u_b), z1 = r sin(2 pi u_b), r = sqrt(-2 ln u_a).  |z| <= sqrt(66 ln 2) = 6.77.  The accurate library
// log / sqrt / sincospi (2 u_b is exact, 2 pi u_b would not be): a normal agrees with its extended-precision value to a few ulp.
__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, double& z0, double& z1) {
  const double ua = ((double)wa + 0.5) * 0x1p-32, ub2 = ((double)wb + 0.5) * 0x1p-31;
  const double r = sqrt(-2.0 * log(ua));
  double s, c;
  sincospi(ub2, &s, &c);
  z0 = r * c;
  z1 = r * s;
}

// The normals of one block: z[0], z[1] from words (0, 1) and - `both` - z[2], z[3] from words (2, 3).  The callers unroll their
// loops over the blocks, so `both` is a constant where this is inlined and the pair nobody reads is not computed.
__device__ __forceinline__ void philox_normals(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, bool both,
                                               double (&z)[4]) {
  uint32_t c[4] = {c0, c1, c2, c3};
  philox4x32_10(k0, k1, c);
  box_muller(c[0], c[1], z[0], z[1]);
  z[2] = z[3] = 0.0;
  if (both) box_muller(c[2], c[3], z[2], z[3]);
}
#endif

}  // namespace mi
