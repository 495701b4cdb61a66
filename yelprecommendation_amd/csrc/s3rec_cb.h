// The pieces the catalogue sweeps share (csrc/s3rec_pretrain.hip: the catalogue BCE; csrc/s3rec_rank.hip: the rank of
// one held-out item per sequence; csrc/catalogue_rank.hip: the ranks of every held-out item of MF and NGCF): the tile
// geometry of the form that owns 32 rows and sweeps a table on v_mfma_f32_32x32x2_f32, the tile's arithmetic and
// accumulator layout, and the cursor over a row's ascending column list.
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

// ---- the rank sweeps' tile (csrc/s3rec_rank.hip, csrc/catalogue_rank.hip) ----
// The lane's half of its owned row, k = 8 c + 4 hh + t at own[4 c + t] (hh = lane >> 5): the order of the swept rows'
// 16-byte loads.  `row` points at element 4 hh of the row.
template <int E>
__device__ __forceinline__ void rank_own(float (&own)[E / 2], const float* __restrict__ row, bool ok) {
#pragma unroll
  for (int c = 0; c < E / 8; ++c) {
    const float4 v = ok ? ld4(row + 8 * c) : zero4();
    own[4 * c + 0] = v.x;
    own[4 * c + 1] = v.y;
    own[4 * c + 2] = v.z;
    own[4 * c + 3] = v.w;
  }
}

// acc[q] in lane j += <swept row cb_acc_row(q, lane), owned row j> over the E dims of one table, k ascending; `w` is
// the lane's swept row + 4 (lane >> 5)
template <int E>
__device__ __forceinline__ f32x16 rank_tile_add(f32x16 acc, const float* __restrict__ w, bool ok,
                                                const float (&own)[E / 2]) {
#pragma unroll
  for (int c = 0; c < E / 8; ++c) {
    float4 wv = ld4(w + 8 * c);
    if (!ok) wv = zero4();
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.x, own[4 * c + 0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.y, own[4 * c + 1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.z, own[4 * c + 2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.w, own[4 * c + 3], acc, 0, 0, 0);
  }
  return acc;
}

// one table: the accumulator starts at 0
template <int E>
__device__ __forceinline__ f32x16 rank_tile(const float* __restrict__ w, bool ok, const float (&own)[E / 2]) {
  return rank_tile_add<E>(zero16(), w, ok, own);
}

// The diagonal of a tile whose swept row in lane r is a row chosen FOR owned row r (its target): the element of owned
// row r = lane & 31 against swept row r sits in the half hh = (r >> 2) & 1 at q = (r & 3) + 4 (r >> 3).  Every lane
// of the wave gets the value of its owned row.
__device__ __forceinline__ float rank_diagonal(const f32x16& acc, int lane) {
  const int r = lane & 31;
  float ts = 0.0f;
#pragma unroll
  for (int q = 0; q < 16; ++q) ts = cb_acc_row(q, lane) == r ? acc[q] : ts;
  return __shfl(ts, r + 32 * ((r >> 2) & 1), kWave);
}

__device__ __forceinline__ uint32_t low_bits(int n) { return n >= 32 ? ~0u : (1u << n) - 1u; }   // n in [0, 32]

}  // namespace yr
