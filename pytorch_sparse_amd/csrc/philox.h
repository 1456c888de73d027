// Philox4x32-10 counter-based generator, shared by the samplers (sample.hip, hgt_sample.hip) and the dropout mask of the
// fused attention (attention.hip).  philox compiles for the host too -- the mask query of attention.hip is host
// arithmetic through the kernels' own rule; the device pass keeps __umulhi.
#pragma once

#include "common.h"

namespace tsamd {

// ---- Philox4x32-10 (Salmon et al., SC'11) --------------------------------------------------------
struct U4 {
  uint32_t x, y, z, w;
};

__host__ __device__ inline uint32_t philox_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

__host__ __device__ inline U4 philox(uint64_t seed, uint64_t c_lo, uint32_t c2, uint32_t c3) {
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  U4 c = {(uint32_t)c_lo, (uint32_t)(c_lo >> 32), c2, c3};
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = philox_mulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const uint32_t hi1 = philox_mulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = {hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

__device__ inline uint64_t u64(uint32_t lo, uint32_t hi) { return (uint64_t)lo | ((uint64_t)hi << 32); }

}  // namespace tsamd
