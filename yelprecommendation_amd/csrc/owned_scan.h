// The tiled integer scan of the owner passes (csrc/cdae_owned.hip, csrc/ngcf_owned.hip): counts per destination ->
// where each destination's segment starts, or (COMPACT) int32 flags -> the ascending list of the flagged indices.
// Integer sums only: the result does not depend on any order of execution.
#pragma once
#include "common.h"

namespace yr {

constexpr int kScanPerThread = 4;
constexpr int kScanTile = kScanPerThread * kBlock;
static_assert(kScanPerThread == 4, "the counts before a tile are read as int4");

// start[c] = entries of the columns before c, start[I] = all of them.  A workgroup per tile of kScanTile columns: it
// sums the counts of every column before its tile itself (coalesced, at most 4 I bytes out of L2 — one launch, no
// hand-off between workgroups; a single workgroup walking all of I = 38,048 took 85 us) and scans its own tile.
// COMPACT: cnt holds flags (0 / non-zero, counted as 1); instead of start[], out[k] = the k-th flagged index in
// ascending order and *total = their number (out needs room for every flagged index, nothing past them is written).
// cnt must be 16-byte aligned; launch with (I + kScanTile - 1) / kScanTile workgroups of kBlock threads.
template <bool COMPACT>
__global__ __launch_bounds__(kBlock) void owned_scan_kernel(const int32_t* __restrict__ cnt, int64_t I,
                                                            int32_t* __restrict__ out, int32_t* __restrict__ total) {
  __shared__ int s_before[kWavesPerBlock];
  __shared__ int s_incl[kWavesPerBlock];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t lo = (int64_t)blockIdx.x * kScanTile;
  int before = 0;                                   // lo is a multiple of the tile; cnt is 16-byte aligned
#pragma unroll 4
  for (int64_t i = (int64_t)threadIdx.x * kScanPerThread; i < lo; i += kScanTile) {
    const int4 t = *reinterpret_cast<const int4*>(cnt + i);
    if (COMPACT) before += ((t.x != 0) + (t.y != 0)) + ((t.z != 0) + (t.w != 0));
    else before += (t.x + t.y) + (t.z + t.w);
  }
  const int64_t at = lo + (int64_t)threadIdx.x * kScanPerThread;
  int v[kScanPerThread], mine = 0;
#pragma unroll
  for (int k = 0; k < kScanPerThread; ++k) {
    v[k] = at + k < I ? cnt[at + k] : 0;
    if (COMPACT) v[k] = v[k] != 0;
    mine += v[k];
  }
  int incl = mine;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const int t = __shfl_up(incl, d, kWave);
    if (lane >= d) incl += t;
  }
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) before += __shfl_xor(before, d, kWave);
  if (lane == kWave - 1) s_incl[wave] = incl;
  if (lane == 0) s_before[wave] = before;
  __syncthreads();
  int run = incl - mine;
  for (int w = 0; w < kWavesPerBlock; ++w) run += s_before[w] + (w < wave ? s_incl[w] : 0);
#pragma unroll
  for (int k = 0; k < kScanPerThread; ++k) {
    if (COMPACT) {
      if (v[k]) out[run] = (int32_t)(at + k);       // v[k] != 0 implies at + k < I
    } else if (at + k < I) {
      out[at + k] = run;
    }
    run += v[k];
  }
  if (at < I && at + kScanPerThread >= I) {         // the thread that holds the last column
    if (COMPACT) total[0] = run;
    else out[I] = run;
  }
}

inline int owned_scan_grid(int64_t I) { return (int)((I + kScanTile - 1) / kScanTile); }

}  // namespace yr
