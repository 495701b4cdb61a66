// S3Rec pre-training for gfx950 (MI355X): the "catalogue BCE" of reference trainers/s3rec_trainer.py:137-152 over
// models/s3rec.py:137-164 — binary cross-entropy with logits between every projected encoder row F[n] and every row
// T[r] of a whole table (item_embedding: MIP; attribute_embedding: AAP, MAP), with its mean over all N R elements.
// The reference builds the [B, L, R] logits and a dense [B, L, R] target array; here no [N, R] array exists in any
// pass: the targets are a list per key (or the key itself), the loss is taken in the epilogue of the matrix sweep
// and the logits are computed again where the second gradient needs them (as the backward recomputes P).
//
//   z[n, r] = zscale[n] <F[n], T[r]>           y[n, r] = yscale[n] [r in targets(key[n])]
//   term    = max(z, 0) - z y + log1p(exp(-|z|))              row_loss[n] = sum_r term,  loss = sum / (N R)
//   g[n, r] = zscale[n] (sigmoid(z) - y) / (N R)              dF = g T,  dT = g^T F
//
// One kernel text, s3rec_cbce_kernel<E, ROWS>, sweeps 32 x 32 tiles of z on v_mfma_f32_32x32x2_f32.  A wave OWNS 32
// rows of one matrix — their E floats stay in its registers as the B operand, so a lane is an owned row — and SWEEPS
// 32-row tiles of the other, read 16 bytes per lane straight from global memory (L2 / L1) as the A operand.  The
// accumulators then hold, in lane j, the logits of owned row j against the swept rows acc_row(q, lane): exactly the
// A operand of the second product dO[j] += sum_i g[i, j] W[i], whose k-th step reads swept row acc_row(k, lane) —
// g goes from the epilogue into the next matrix instruction without leaving the registers.
//   ROWS = true   owns kCbTile rows of F, sweeps T: the loss terms and dF.  A workgroup is (row tile, column chunk of
//                 kCbColChunk columns), its four waves take kCbTilesPerWave column tiles each and are added in wave
//                 order in LDS; the chunks' partial sums go to the workspace and are added chunk after chunk by
//                 s3rec_cbce_reduce_kernel.  The chunk is a constant, so a row's sums do not depend on N.
//   ROWS = false  owns kCbTile rows of T, sweeps F: dT.  A workgroup is a column tile, wave w takes the row tiles
//                 w, w + 4, ..., and the four are added in wave order in LDS: dT is written once, no partials.
// No float atomics anywhere: every sum has one order, two calls give one answer bit for bit.
#include <math.h>

#include <algorithm>

#include "s3rec_cb.h"     // the tile geometry, cb_acc_row, cb_lower_bound, cb_mask: shared with csrc/s3rec_rank.hip

namespace yr {

constexpr int kCbTile = 32;                 // rows and columns of a tile: the 32 x 32 x 2 f32 matrix instruction
constexpr int kCbTilesPerWave = 16;         // column tiles a wave sweeps in the ROWS form
constexpr int kCbColChunk = kWavesPerBlock * kCbTilesPerWave * kCbTile;   // 2,048 columns per workgroup
constexpr int kCbGridMax = 2048;            // workgroups per launch; the kernels' own loops go on from there
constexpr int kCbLossBlock = 256;           // threads of the single workgroup that adds row_loss up

static_assert(kCbTile == kSweepTile && kCbTilesPerWave == kSweepTilesPerWave && kCbColChunk == kSweepColChunk &&
                  kCbGridMax == kSweepGridMax, "one geometry for the catalogue sweeps (s3rec_cb.h)");

struct Cbce {
  const float* F;             // [N][E]
  const float* T;             // [R][E]
  const float *zscale, *yscale;
  const int64_t* key;         // [N]
  const int64_t *tgt_ptr, *tgt_idx;   // CSR over K keys, or null: the key is the one target column
  int64_t N, R, K;
  float inv;                  // 1 / (N R)
  float* part_loss;           // [chunks][N]
  float* part_dF;             // [chunks][N][E], null: no dF
  float* dT;                  // [R][E] (ROWS = false)
  int64_t chunks;
  int32_t* err_flag;
};

template <int E, bool ROWS>
__global__ __launch_bounds__(kBlock, E <= 64 ? 2 : 1) void s3rec_cbce_kernel(Cbce p) {
  constexpr int NT = E >= 32 ? E / 32 : 1;            // column tiles of the owned rows' gradient
  __shared__ float sO[kCbTile * E];
  __shared__ float sL[kCbTile];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int r = lane & 31, hh = lane >> 5;
  const float* own_mat = ROWS ? p.F : p.T;
  const float* swp_mat = ROWS ? p.T : p.F;
  const int64_t own_n = ROWS ? p.N : p.R, swp_n = ROWS ? p.R : p.N;
  const int64_t own_tiles = (own_n + kCbTile - 1) / kCbTile;
  const int64_t units = ROWS ? own_tiles * p.chunks : own_tiles;
  const bool grad = ROWS ? p.part_dF != nullptr : true;
  int flag = 0;

  for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int64_t ot = ROWS ? unit / p.chunks : unit;
    const int64_t chunk = ROWS ? unit - ot * p.chunks : 0;
    const int64_t j0 = ot * kCbTile, j = j0 + r;      // the lane's owned row
    const bool own_ok = j < own_n;

    // the owned rows, k = 8 c + 4 hh + t at own[4 c + t]: the order of the swept rows' 16-byte loads
    float own[E / 2];
#pragma unroll
    for (int c = 0; c < E / 8; ++c) {
      const float4 v = own_ok ? ld4(own_mat + j * E + 8 * c + 4 * hh) : zero4();
      own[4 * c + 0] = v.x;
      own[4 * c + 1] = v.y;
      own[4 * c + 2] = v.z;
      own[4 * c + 3] = v.w;
    }

    // what the epilogue needs of a row n of F: its two factors and its targets (ROWS: the lane's own row)
    float zs = 0.0f, ys = 0.0f;
    int64_t cur = 0, end = 0, mip_key = -1;
    auto row_meta = [&](int64_t n, int64_t c_first) {
      zs = ys = 0.0f;
      cur = end = 0;
      mip_key = -1;
      if (n < p.N) {
        zs = p.zscale[n];
        ys = p.yscale[n];
        const int64_t k = p.key[n];
        if (k < 0 || k >= p.K) {
          flag = YR_FLAG_BAD_ITEM;
        } else if (p.tgt_ptr) {
          end = p.tgt_ptr[k + 1];
          cur = cb_lower_bound(p.tgt_idx, p.tgt_ptr[k], end, c_first);
        } else {
          mip_key = k;
        }
      }
    };

    // the swept tiles of this wave: [t_begin, t_end) step t_step, tile t covers swept rows 32 t ..
    int64_t t_begin, t_end, t_step;
    if (ROWS) {
      t_begin = chunk * (kCbColChunk / kCbTile) + (int64_t)wave * kCbTilesPerWave;
      t_end = std::min<int64_t>(t_begin + kCbTilesPerWave, (swp_n + kCbTile - 1) / kCbTile);
      t_step = 1;
      row_meta(j, t_begin * kCbTile);
    } else {
      t_begin = wave;
      t_end = (swp_n + kCbTile - 1) / kCbTile;
      t_step = kWavesPerBlock;
    }

    f32x16 dacc[NT];
#pragma unroll
    for (int u = 0; u < NT; ++u) dacc[u] = zero16();
    float lsum = 0.0f;

    for (int64_t t = t_begin; t < t_end; t += t_step) {
      const int64_t i0 = t * kCbTile, i = i0 + r;     // the lane's swept row
      const bool swp_ok = i < swp_n;
      uint32_t mask;
      if (ROWS) {
        mask = p.tgt_ptr ? cb_mask(p.tgt_idx, cur, end, i0)
                         : (mip_key >= i0 && mip_key < i0 + kCbTile ? 1u << (int)(mip_key - i0) : 0u);
      } else {
        row_meta(i, j0);                              // the lane's swept row of F against the owned columns
        mask = p.tgt_ptr ? cb_mask(p.tgt_idx, cur, end, j0)
                         : (mip_key >= j0 && mip_key < j0 + kCbTile ? 1u << (int)(mip_key - j0) : 0u);
      }

      // acc[q] in lane j = <swept row acc_row(q, lane), owned row j>
      f32x16 acc = zero16();
      const float* w = swp_mat + (swp_ok ? i : 0) * E + 4 * hh;
#pragma unroll
      for (int c = 0; c < E / 8; ++c) {
        float4 wv = ld4(w + 8 * c);
        if (!swp_ok) wv = zero4();
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.x, own[4 * c + 0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.y, own[4 * c + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.z, own[4 * c + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.w, own[4 * c + 3], acc, 0, 0, 0);
      }

      // the epilogue: the loss terms (ROWS) and g in place of the logits
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int ri = cb_acc_row(q, lane);           // the swept row of this element inside the tile
        float zsq, ysq;
        bool hit, ok;
        if (ROWS) {
          zsq = zs;
          ysq = ys;
          hit = (mask >> ri) & 1u;
          ok = own_ok && i0 + ri < swp_n;
        } else {
          zsq = __shfl(zs, ri, kWave);
          ysq = __shfl(ys, ri, kWave);
          hit = (__shfl(mask, ri, kWave) >> r) & 1u;
          ok = own_ok && i0 + ri < swp_n;
        }
        const float z = zsq * acc[q];
        const float y = hit ? ysq : 0.0f;
        const float ez = fast_exp(-fabsf(z));
        const float rc = fast_rcp(1.0f + ez);
        const float sig = z >= 0.0f ? rc : ez * rc;
        if (ROWS) {
          const float term = (fmaxf(z, 0.0f) - z * y) + fast_log(1.0f + ez);
          lsum += ok ? term : 0.0f;
        }
        acc[q] = ok ? zsq * ((sig - y) * p.inv) : 0.0f;
      }

      // dO[j] += sum_i g[i, j] W[i]: step q of the matrix instruction reads swept row acc_row(q, lane)
      if (grad) {
#pragma unroll
        for (int u = 0; u < NT; ++u) {
          const int e = u * 32 + r;
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int64_t iq = i0 + cb_acc_row(q, lane);
            const float b = (iq < swp_n && e < E) ? swp_mat[iq * E + e] : 0.0f;
            dacc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[q], b, dacc[u], 0, 0, 0);
          }
        }
      }
    }

    // the four waves in wave order: sO [32][E] of the owned rows' gradient, sL [32] of their loss
    if (ROWS) lsum += __shfl_xor(lsum, 32, kWave);
    for (int w = 0; w < kWavesPerBlock; ++w) {
      if (wave == w) {
        if (grad) {
#pragma unroll
          for (int u = 0; u < NT; ++u) {
            const int e = u * 32 + r;
            if (e < E) {
#pragma unroll
              for (int q = 0; q < 16; ++q) {
                float* s = sO + cb_acc_row(q, lane) * E + e;
                *s = w == 0 ? dacc[u][q] : *s + dacc[u][q];
              }
            }
          }
        }
        if (ROWS && hh == 0) sL[r] = w == 0 ? lsum : sL[r] + lsum;
      }
      __syncthreads();
    }
    if (grad) {
      float* out = ROWS ? p.part_dF + (chunk * p.N + j0) * E : p.dT + j0 * E;
      const int64_t rows = std::min<int64_t>(kCbTile, own_n - j0);
      for (int e = tid; e < rows * E; e += kBlock) out[e] = sO[e];
    }
    if (ROWS && tid < kCbTile && j0 + tid < p.N) p.part_loss[chunk * p.N + j0 + tid] = sL[tid];
    __syncthreads();                                  // the next unit overwrites sO and sL
  }
  if (flag && p.err_flag) atomicOr(p.err_flag, flag);
}

// row_sum[n] (and row_loss[n] where given) = the chunks' partial sums, chunk after chunk; dF likewise
__global__ __launch_bounds__(kBlock) void s3rec_cbce_reduce_kernel(const float* __restrict__ part_loss,
                                                                   const float* __restrict__ part_dF, int64_t chunks,
                                                                   int64_t N, int E, float* __restrict__ row_sum,
                                                                   float* __restrict__ row_loss,
                                                                   float* __restrict__ dF) {
  const int64_t NE = N * E, total = N + (part_dF ? NE : 0), stride = (int64_t)gridDim.x * kBlock;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += stride) {
    const bool is_loss = e < N;
    const float* src = is_loss ? part_loss + e : part_dF + (e - N);
    const int64_t step = is_loss ? N : NE;
    float s = src[0];
    for (int64_t c = 1; c < chunks; ++c) s += src[c * step];
    if (is_loss) {
      row_sum[e] = s;
      if (row_loss) row_loss[e] = s;
    } else {
      dF[e - N] = s;
    }
  }
}

// loss = (sum_n row_sum[n]) / (N R): one workgroup, a double per thread over its rows in order, then a fixed tree
__global__ __launch_bounds__(kCbLossBlock) void s3rec_cbce_loss_kernel(const float* __restrict__ row_sum, int64_t N,
                                                                       double inv, float* __restrict__ loss) {
  __shared__ double sd[kCbLossBlock];
  double s = 0.0;
  for (int64_t n = threadIdx.x; n < N; n += kCbLossBlock) s += (double)row_sum[n];
  sd[threadIdx.x] = s;
  __syncthreads();
  for (int m = kCbLossBlock / 2; m >= 1; m >>= 1) {
    if ((int)threadIdx.x < m) sd[threadIdx.x] += sd[threadIdx.x + m];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = (float)(sd[0] * inv);
}

}  // namespace yr

using namespace yr;

static bool cbce_width_ok(int E) { return E == 16 || E == 32 || E == 64 || E == 128; }   // s3rec_width_ok

static int64_t cbce_chunks(int64_t R) { return (R + kCbColChunk - 1) / kCbColChunk; }

template <bool ROWS>
static int cbce_launch(const Cbce& p, int E, int64_t units, hipStream_t stream) {
  const dim3 grid((unsigned)std::min<int64_t>(units, kCbGridMax)), block(kBlock);
  switch (E) {
    case 16: hipLaunchKernelGGL((s3rec_cbce_kernel<16, ROWS>), grid, block, 0, stream, p); break;
    case 32: hipLaunchKernelGGL((s3rec_cbce_kernel<32, ROWS>), grid, block, 0, stream, p); break;
    case 64: hipLaunchKernelGGL((s3rec_cbce_kernel<64, ROWS>), grid, block, 0, stream, p); break;
    default: hipLaunchKernelGGL((s3rec_cbce_kernel<128, ROWS>), grid, block, 0, stream, p); break;
  }
  return launch_status();
}

extern "C" int64_t yr_s3rec_catalogue_bce_workspace_floats(int64_t N, int64_t R, int E) {
  if (N < 0 || R < 0 || E <= 0) return YR_ERR_BADARG;
  if (!cbce_width_ok(E)) return YR_ERR_UNSUPPORTED;
  return N * (1 + cbce_chunks(R) * (1 + (int64_t)E));
}

extern "C" int yr_s3rec_catalogue_bce(const float* F, const float* T, const float* zscale, const float* yscale,
                                      const int64_t* key, const int64_t* tgt_ptr, const int64_t* tgt_idx, int64_t N,
                                      int64_t R, int64_t K, int E, float* loss, float* row_loss, float* dF, float* dT,
                                      float* workspace, int64_t workspace_floats, int32_t* err_flag, void* stream) {
  if (N < 0 || R < 0 || K < 0 || E <= 0 || workspace_floats < 0) return YR_ERR_BADARG;
  if (!cbce_width_ok(E)) return YR_ERR_UNSUPPORTED;
  if (N == 0 || R == 0) return 0;
  if (!F || !T || !zscale || !yscale || !key || !loss || !workspace) return YR_ERR_BADARG;
  if ((tgt_ptr == nullptr) != (tgt_idx == nullptr)) return YR_ERR_BADARG;
  if (((reinterpret_cast<uintptr_t>(F) | reinterpret_cast<uintptr_t>(T)) & 15) != 0) return YR_ERR_BADARG;
  const int64_t chunks = cbce_chunks(R);
  if (workspace_floats < N * (1 + chunks * (1 + (int64_t)E))) return YR_ERR_BADARG;
  float* row_sum = workspace;
  float* part_loss = row_sum + N;
  float* part_dF = part_loss + chunks * N;
  const double inv = 1.0 / ((double)N * (double)R);
  const Cbce p{F, T, zscale, yscale, key, tgt_ptr, tgt_idx, N, R, K, (float)inv, part_loss, dF ? part_dF : nullptr, dT,
               chunks, err_flag};
  hipStream_t st = (hipStream_t)stream;
  const int64_t row_tiles = (N + kCbTile - 1) / kCbTile, col_tiles = (R + kCbTile - 1) / kCbTile;
  if (const int s = cbce_launch<true>(p, E, row_tiles * chunks, st)) return s;
  hipLaunchKernelGGL(s3rec_cbce_reduce_kernel, dim3(grid_for(N * (dF ? 1 + (int64_t)E : 1), kBlock)), dim3(kBlock), 0,
                     st, part_loss, dF ? part_dF : nullptr, chunks, N, E, row_sum, row_loss, dF);
  if (const int s = launch_status()) return s;
  hipLaunchKernelGGL(s3rec_cbce_loss_kernel, dim3(1), dim3(kCbLossBlock), 0, st, row_sum, N, inv, loss);
  if (const int s = launch_status()) return s;
  if (dT) return cbce_launch<false>(p, E, col_tiles, st);
  return 0;
}
