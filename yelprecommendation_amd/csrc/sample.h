// The two pieces every device-side negative sampler of the engine is made of: an unbiased integer below n from one
// Philox4x32-7 block keyed by (seed, epoch), and membership in an ascending id list.  One copy, used by
// csrc/triplets.hip and csrc/s3rec_batches.hip; oracle/triplet_sampler.py (keys, _draw) states the same words on the
// CPU and the tests pin them bit for bit.
#pragma once
#include "common.h"
#include "philox.h"

namespace yr {

constexpr int kMaxDraws = 4096;   // rejected draws per element before a sampler stops drawing and walks the catalogue

// the Philox key of the draws of one (seed, epoch)
__device__ __forceinline__ uint2 sample_key(uint64_t seed, uint64_t epoch) {
  return make_uint2((uint32_t)seed ^ (uint32_t)(epoch * 0x9E3779B97F4A7C15ull >> 32),
                    (uint32_t)(seed >> 32) ^ (uint32_t)epoch);
}

// draw d of element t: floor(u32 * n32 / 2^32), Lemire's multiply-shift with rejection of the short first
// interval (the block's three other words are the redraws) — uniform over [0, n32)
__device__ __forceinline__ uint32_t sample_draw(uint64_t t, uint32_t d, uint32_t n32, uint2 key) {
  const uint4 w = philox4x32<7>(make_uint4((uint32_t)t, (uint32_t)(t >> 32), d, 0u), key);
  uint64_t m = (uint64_t)w.x * n32;
  if ((uint32_t)m < n32) {
    const uint32_t thr = (0u - n32) % n32;
    const uint32_t alt[3] = {w.y, w.z, w.w};
    int a = 0;
    while ((uint32_t)m < thr && a < 3) m = (uint64_t)alt[a++] * n32;
  }
  return (uint32_t)(m >> 32);
}

// is v one of idx[lo, hi), ascending?  (binary search)
__device__ __forceinline__ bool sorted_contains(const int64_t* __restrict__ idx, int64_t lo, int64_t hi, int64_t v) {
  const int64_t end = hi;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (idx[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo < end && idx[lo] == v;
}

}  // namespace yr
