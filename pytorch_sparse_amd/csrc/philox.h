// Philox4x32-10 counter-based generator, shared by the samplers (sample.hip, hgt_sample.hip).
#pragma once

#include "common.h"

namespace tsamd {

// ---- Philox4x32-10 (Salmon et al., SC'11) --------------------------------------------------------
struct U4 {
  uint32_t x, y, z, w;
};

__device__ inline U4 philox(uint64_t seed, uint64_t c_lo, uint32_t c2, uint32_t c3) {
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  U4 c = {(uint32_t)c_lo, (uint32_t)(c_lo >> 32), c2, c3};
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = {hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

__device__ inline uint64_t u64(uint32_t lo, uint32_t hi) { return (uint64_t)lo | ((uint64_t)hi << 32); }

}  // namespace tsamd
