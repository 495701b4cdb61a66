// The pieces the two S3Rec catalogue sweeps share (csrc/s3rec_pretrain.hip: the catalogue BCE; csrc/s3rec_rank.hip:
// the catalogue rank): the tile geometry of the form that owns 32 rows and sweeps a table on v_mfma_f32_32x32x2_f32,
// the accumulator layout, and the cursor over a row's ascending column list.
#pragma once
#include "common.h"

namespace yr {

// The geometry both files run on.  csrc/s3rec_pretrain.hip keeps its own named constants (kCb*: its tests read them
// from its text) and ties them to these with static_assert.
constexpr int kSweepTile = 32;              // rows and columns of a tile: the 32 x 32 x 2 f32 matrix instruction
constexpr int kSweepTilesPerWave = 16;      // column tiles a wave sweeps in the form that owns rows
constexpr int kSweepColChunk = kWavesPerBlock * kSweepTilesPerWave * kSweepTile;   // 2,048 columns per workgroup
constexpr int kSweepGridMax = 2048;         // workgroups per launch; the kernels' own loops go on from there

__device__ __forceinline__ int cb_acc_row(int q, int lane) { return (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5); }

// first k in [lo, hi) with idx[k] >= v
__device__ __forceinline__ int64_t cb_lower_bound(const int64_t* __restrict__ idx, int64_t lo, int64_t hi, int64_t v) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (idx[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// bit c of the result: column c0 + c is on the list (a target of the key; an excluded column of the row).  `cur`
// walks the ascending list and stays at the first entry not below c0 + 32
__device__ __forceinline__ uint32_t cb_mask(const int64_t* __restrict__ idx, int64_t& cur, int64_t end, int64_t c0) {
  uint32_t m = 0;
  while (cur < end) {
    const int64_t v = idx[cur];
    if (v >= c0 + kSweepTile) break;
    if (v >= c0) m |= 1u << (int)(v - c0);
    ++cur;
  }
  return m;
}

}  // namespace yr
