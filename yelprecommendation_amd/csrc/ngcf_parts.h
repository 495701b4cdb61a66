// Pieces of the NGCF kernels that csrc/ngcf.hip (float atomics, arrival order) and csrc/ngcf_owned.hip (owner
// passes, fixed order) both use: the layer-gradient pointer pack and the chunk walk + MFMA loop of the weight
// gradient, whose two forms differ in their last lines only.
#pragma once
#include "common.h"

namespace yr {

struct LayerGradPtrs { float* p[YR_NGCF_MAX_LAYERS]; };

constexpr float kSlope = 0.01f;   // nn.functional.leaky_relu default (models/ngcf.py:72)

// dW1[j, c] += sum_r dP[r, j] (Z+E)[r, c];  dW2[j, c] += sum_r dP[r, j] (E*Z)[r, c]
// One workgroup per chunk of WChunk<D>::ROWS rows: dP, A = Z+E and H = E*Z of the chunk are staged in LDS
// (pitch D+1: the column reads below are conflict-free) and every wave computes whole 32x32
// output tiles over K = ROWS with one ds_read_b32 per operand per MFMA.
template <int D>
struct WChunk {
  static constexpr int ROWS = 4096 / D;      // rows per workgroup: 3 staged tiles stay under 64 KiB of LDS
};

// The body of ngcf_dense_bwd_weight_kernel (csrc/ngcf.hip) and of ngcf_owned_dw_slots_kernel (csrc/ngcf_owned.hip).
// SLOTS = false: the workgroup's 2 D^2 partial sums are ADDED to dW1 / dW2 with float atomics.  SLOTS = true: they
// are plain-STORED to dW1 / dW2, which then point at the workgroup's own slot of a scratch array.  A workgroup's
// partial sums are the same bits in both forms: rows blockIdx.x * ROWS + k * gridDim.x * ROWS + [0, ROWS), chunk after
// chunk, every output element one k-ordered fmaf chain (v_mfma_f32_32x32x2_f32) over the two halves of a chunk.
template <int D, bool SUB, bool SLOTS>
__device__ __forceinline__ void ngcf_dense_bwd_weight_body(
    const float* __restrict__ dEout, const float* __restrict__ Eout, const float* __restrict__ E,
    const float* __restrict__ Z, int n_all, float* __restrict__ dW1, float* __restrict__ dW2,
    const int32_t* __restrict__ rows, const int32_t* __restrict__ count) {
  const int n = SUB ? *count : n_all;         // rows to sum over: the list's length in the row-list form
  // pitch D: an MFMA operand read is 32 consecutive floats of one staged row per half-wave, which is
  // conflict-free at any pitch, and a multiple of 4 keeps the staging stores 16 bytes wide
  constexpr int PITCH = D;
  constexpr int kWRows = WChunk<D>::ROWS;
  constexpr int RT = (D + 31) / 32;          // tiles along j (rows of dW) and along c (per matrix)
  constexpr int NT = RT * RT * 2;            // output tiles: RT x RT for dW1, same for dW2
  constexpr int NV = kWRows * D / 4 / kBlock;   // float4 per thread per operand and chunk (= 4)
  if (SUB && (int64_t)blockIdx.x * kWRows >= n) return;   // row-list form: the grid is sized for an upper bound
  __shared__ __attribute__((aligned(16))) float s_dp[kWRows * PITCH];
  __shared__ __attribute__((aligned(16))) float s_a[kWRows * PITCH];
  __shared__ __attribute__((aligned(16))) float s_h[kWRows * PITCH];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int i = lane & 31, h = lane >> 5;
  constexpr int TPW = (NT + kWavesPerBlock - 1) / kWavesPerBlock;   // output tiles per wave
  f32x16 acc[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) acc[t] = zero16();
  // the next chunk's rows travel in registers while the MFMAs of the current chunk run
  float4 pg[NV], po[NV], pe[NV], pz[NV];
  auto fetch = [&](int64_t row0) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int q = threadIdx.x + v * kBlock;
      const int64_t r = row0 + q / (D / 4);
      const int c4 = (q % (D / 4)) * 4;
      pg[v] = po[v] = pe[v] = pz[v] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < n) {
        const int64_t o = (SUB ? (int64_t)rows[r] : r) * D + c4;
        pg[v] = ld4(dEout + o); po[v] = ld4(Eout + o); pe[v] = ld4(E + o); pz[v] = ld4(Z + o);
      }
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int q = threadIdx.x + v * kBlock;
      const int at = (q / (D / 4)) * PITCH + (q % (D / 4)) * 4;
      const float4 g = pg[v], o = po[v], e = pe[v], z = pz[v];
      *reinterpret_cast<float4*>(s_dp + at) = make_float4(o.x > 0.0f ? g.x : kSlope * g.x, o.y > 0.0f ? g.y : kSlope * g.y,
                                                          o.z > 0.0f ? g.z : kSlope * g.z, o.w > 0.0f ? g.w : kSlope * g.w);
      *reinterpret_cast<float4*>(s_a + at) = make_float4(z.x + e.x, z.y + e.y, z.z + e.z, z.w + e.w);
      *reinterpret_cast<float4*>(s_h + at) = make_float4(e.x * z.x, e.y * z.y, e.z * z.z, e.w * z.w);
    }
  };
  // persistent over row chunks: the 2 D^2 partial sums stay in registers until the end, so the
  // float atomics on dW scale with the grid, not with n
  const int64_t stride = (int64_t)gridDim.x * kWRows;
  int64_t row0 = (int64_t)blockIdx.x * kWRows;
  if (row0 < n) fetch(row0);
  for (; row0 < n; row0 += stride) {
    __syncthreads();                                 // the previous chunk's MFMAs are done with the LDS tiles
    stash();
    __syncthreads();
    if (row0 + stride < n) fetch(row0 + stride);
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int tile = wave + t * kWavesPerBlock;
      if (tile < NT) {
        const int which = tile / (RT * RT);      // 0: dW1 (A), 1: dW2 (H)
        const int tj = (tile % (RT * RT)) / RT, tc = tile % RT;
        const float* s_b = which ? s_h : s_a;
        const int j = tj * 32 + i, c = tc * 32 + i;
#pragma unroll 8
        for (int s = 0; s < kWRows / 2; ++s) {
          const int r = h * (kWRows / 2) + s;
          const float av = j < D ? s_dp[r * PITCH + j] : 0.0f;
          const float bv = c < D ? s_b[r * PITCH + c] : 0.0f;
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int tile = wave + t * kWavesPerBlock;
    if (tile < NT) {
      const int which = tile / (RT * RT);
      const int tj = (tile % (RT * RT)) / RT, tc = tile % RT;
      const int c = tc * 32 + i;
      float* out = which ? dW2 : dW1;
      if (c < D) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int jj = tj * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
          if (jj < D) {
            if (SLOTS) out[jj * D + c] = acc[t][reg];
            else atomicAdd(out + jj * D + c, acc[t][reg]);
          }
        }
      }
    }
  }
}

}  // namespace yr
