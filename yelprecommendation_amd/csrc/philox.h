// Counter-based random numbers for the device side: Philox4x32 (Salmon et al., SC'11) and the uint32 -> [0, 1)
// map.  Every sampler and dropout mask of the engine is a pure function of (seed, position) through these two,
// and the tests pin their words bit for bit against oracle/ — one definition, so that no file can drift alone.
#pragma once
#include "common.h"

namespace yr {

// one round: the counter under this round's key (the loops below step the key)
__device__ __forceinline__ uint4 philox_round(uint4 ctr, uint2 key) {
  const uint32_t hi0 = __umulhi(0xD2511F53u, ctr.x), lo0 = 0xD2511F53u * ctr.x;
  const uint32_t hi1 = __umulhi(0xCD9E8D57u, ctr.z), lo1 = 0xCD9E8D57u * ctr.z;
  return make_uint4(hi1 ^ ctr.y ^ key.x, lo1, hi0 ^ ctr.w ^ key.y, lo0);
}

// ROUNDS = 10 is the standard generator (dropout masks); 7 is the shortest variant that passes BigCrush
// (sampling keys, where the word count per element is the cost).
template <int ROUNDS>
__device__ __forceinline__ uint4 philox4x32(uint4 ctr, uint2 key) {
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    ctr = philox_round(ctr, key);
    key.x += 0x9E3779B9u;
    key.y += 0xBB67AE85u;
  }
  return ctr;
}

// The same words from a loop that the compiler is not told to unroll, for cdae_train_lists_kernel, which is slower
// with the unrolled form: 85 instead of 61 us per 4,096 rows (profiles/helpers_refactor_cdae_lists_ms.txt).
__device__ __forceinline__ uint4 philox4x32_rolled(uint4 ctr, uint2 key, int rounds) {
  for (int r = 0; r < rounds; ++r) {
    ctr = philox_round(ctr, key);
    key.x += 0x9E3779B9u;
    key.y += 0xBB67AE85u;
  }
  return ctr;
}

// the top 24 bits as a float in [0, 1): exact, and u01(x) >= p keeps an element with probability 1 - p
__device__ __forceinline__ float u01(uint32_t x) { return (float)(x >> 8) * (1.0f / 16777216.0f); }

}  // namespace yr
