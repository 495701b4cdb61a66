// CDAE without negative sampling for gfx950 (MI355X): the plain BCE of reference trainers/cdae_trainer.py:36-54 over
// models/cdae.py:46-52 and loss.py (nn.BCELoss, negative_sampling: false) — the mean over ALL B I positions of a batch
// of the BCE between the prediction act(z W_o^T + b_o) and the 0/1 row of the user's items.  The reference builds the
// [B, I] prediction and the dense [B, I] target; the dense decoder of this project (csrc/cdae.hip, EPI == 1) still
// writes a [B, I] gradient array G for two more products.  Here no [B, I] array exists in any pass: the targets are
// the ascending item list of the row's user (one CSR keyed by user[n]), the loss is taken in the epilogue of the
// matrix sweep, and the pre-activations are computed again where the second gradient needs them — the form of
// csrc/s3rec_pretrain.hip, whose geometry and helpers (s3rec_cb.h) this file runs on.  What differs from it:
//
//   pre[n, i] = b_o[i] + <z[n], W_o[i]>                       a bias per swept column (and its gradient db_o)
//   y         = act(pre)                                      sigmoid or identity
//   term      = -(t max(log y, -100) + (1 - t) max(log(1 - y), -100))      torch's BCELoss on the PREDICTION, as
//   g         = (y - t) / max((1 - y) y, 1e-12) act'(y) / (B I)            csrc/cdae.hip (EPI == 1) and bce_term of
//                                                                          csrc/cdae_sparse.hip state it
//   row_loss[n] = sum_i term           dz = g W_o           dW_o = g^T z           db_o = sum_n g
//
// The term is NOT BCE-with-logits: where f32 saturates the two differ (sigmoid, pre = 30, t = 0: y rounds to 1, the
// clamped logarithm gives 100 and the gradient is 0; with logits it would be 30 and 1), and this route says what the
// dense route says: the same operations in the same order on the prediction, with the hardware forms of exp, log and
// the reciprocal (fast_exp / fast_log / fast_rcp of common.h, about 1 ulp each) where the dense epilogue calls expf, logf
// and the IEEE division — those cost this sweep more than its matrix instructions (measured: DESIGN 4.6).  The hardware
// forms saturate exactly as the library's: exp of -30 vanishes beside 1, rcp(1) = 1, log(1) = 0, log(0) = -inf.
//
// One kernel text, cdae_cbce_kernel<H, ROWS>, sweeps 32 x 32 tiles of pre on v_mfma_f32_32x32x2_f32.  A wave OWNS 32
// rows of one matrix (their H floats stay in registers as the B operand: a lane is an owned row) and SWEEPS 32-row
// tiles of the other, read 16 bytes per lane from global memory as the A operand.  The accumulators hold, in lane j,
// the pre-activations of owned row j against swept rows cb_acc_row(q, lane): after the epilogue they hold g, which is
// the A operand of the second product without leaving the registers.
//   ROWS = true   owns 32 rows of z, sweeps W_o: row loss and dz.  A workgroup is (row tile, chunk of kSweepColChunk
//                 columns); its four waves take kSweepTilesPerWave column tiles each and are added in wave order in
//                 LDS; the chunks' partial sums go to the workspace and cdae_cbce_reduce_kernel adds them chunk after
//                 chunk.  The chunk is a constant, so a row's sums do not depend on B.  Without dz: the loss only.
//   ROWS = false  owns 32 rows of W_o, sweeps z: dW_o and db_o.  A workgroup is a column tile, wave w takes the row
//                 tiles w, w + 4, ..., the four are added in wave order in LDS: each is written exactly once.
// No float atomics: every sum has one order, two calls give one answer bit for bit.
#include <math.h>

#include <algorithm>

#include "s3rec_cb.h"     // the tile geometry, cb_acc_row, cb_lower_bound, cb_mask

namespace yr {

struct CdaeCbce {
  const float* z;             // [B][H]
  const float* Wo;            // [I][H]
  const float* bo;            // [I]
  const int64_t* user;        // [B]: the key of a row
  const int64_t *tgt_ptr, *tgt_idx;   // CSR over K users, item ids ascending
  int64_t B, I, K;
  int act;                    // 1: sigmoid, 0: identity
  float inv;                  // 1 / (B I)
  float* part_loss;           // [chunks][B]
  float* part_dz;             // [chunks][B][H], null: no dz
  float* dWo;                 // [I][H] (ROWS = false)
  float* dbo;                 // [I]    (ROWS = false)
  int64_t chunks;
  int32_t* err_flag;
};

// the BCE term of pre-activation `pre` against target t, and g = d term / d pre without 1 / (B I): the arithmetic of
// the dense decoder's epilogue (csrc/cdae.hip, EPI == 1), operation by operation, on the hardware's exp / log / rcp
__device__ __forceinline__ void cdae_bce_of_pre(float pre, float t, int act, float& term, float& g) {
  float y = pre;
  if (act == 1) y = fast_rcp(1.0f + fast_exp(-y));
  term = -(t * fmaxf(fast_log(y), -100.0f) + (1.0f - t) * fmaxf(fast_log(1.0f - y), -100.0f));
  g = (y - t) * fast_rcp(fmaxf((1.0f - y) * y, 1e-12f));
  if (act == 1) g *= y * (1.0f - y);
}

template <int H, bool ROWS>
__global__ __launch_bounds__(kBlock, H <= 64 ? 2 : 1) void cdae_cbce_kernel(CdaeCbce p) {
  constexpr int NT = H >= 32 ? H / 32 : 1;            // column tiles of the owned rows' gradient
  __shared__ float sO[kSweepTile * H];
  __shared__ float sL[kSweepTile];                    // ROWS: the rows' loss; else: the columns' db_o
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);    // uniform: the tile loop's counters stay scalar
  const int r = lane & 31, hh = lane >> 5;
  const float* own_mat = ROWS ? p.z : p.Wo;
  const float* swp_mat = ROWS ? p.Wo : p.z;
  const int64_t own_n = ROWS ? p.B : p.I, swp_n = ROWS ? p.I : p.B;
  const int64_t own_tiles = (own_n + kSweepTile - 1) / kSweepTile;
  const int64_t units = ROWS ? own_tiles * p.chunks : own_tiles;
  const bool grad = ROWS ? p.part_dz != nullptr : true;
  int flag = 0;

  for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int64_t ot = ROWS ? unit / p.chunks : unit;
    const int64_t chunk = ROWS ? unit - ot * p.chunks : 0;
    const int64_t j0 = ot * kSweepTile, j = j0 + r;   // the lane's owned row
    const bool own_ok = j < own_n;

    // the owned rows, k = 8 c + 4 hh + t at own[4 c + t]: the order of the swept rows' 16-byte loads
    float own[H / 2];
#pragma unroll
    for (int c = 0; c < H / 8; ++c) {
      const float4 v = own_ok ? ld4(own_mat + j * H + 8 * c + 4 * hh) : zero4();
      own[4 * c + 0] = v.x;
      own[4 * c + 1] = v.y;
      own[4 * c + 2] = v.z;
      own[4 * c + 3] = v.w;
    }
    const float own_bias = (!ROWS && own_ok) ? p.bo[j] : 0.0f;     // ROWS = false: the lane's column of W_o

    // the targets of a row n of z, from column c_first on (ROWS: the lane's own row)
    int64_t cur = 0, end = 0;
    auto row_meta = [&](int64_t n, int64_t c_first) {
      cur = end = 0;
      if (n < p.B) {
        const int64_t k = p.user[n];
        if (k < 0 || k >= p.K) {
          flag = YR_FLAG_BAD_ITEM;
        } else {
          end = p.tgt_ptr[k + 1];
          cur = cb_lower_bound(p.tgt_idx, p.tgt_ptr[k], end, c_first);
        }
      }
    };

    // the swept tiles of this wave: [t_begin, t_end) step t_step, tile t covers swept rows 32 t ..
    int64_t t_begin, t_end, t_step;
    if (ROWS) {
      t_begin = chunk * (kSweepColChunk / kSweepTile) + (int64_t)wave * kSweepTilesPerWave;
      t_end = std::min<int64_t>(t_begin + kSweepTilesPerWave, (swp_n + kSweepTile - 1) / kSweepTile);
      t_step = 1;
      row_meta(j, t_begin * kSweepTile);
    } else {
      t_begin = wave;
      t_end = (swp_n + kSweepTile - 1) / kSweepTile;
      t_step = kWavesPerBlock;
    }

    f32x16 dacc[NT];
#pragma unroll
    for (int u = 0; u < NT; ++u) dacc[u] = zero16();
    float lsum = 0.0f;                                // ROWS: the row's loss terms; else: the column's sum of g

    for (int64_t t = t_begin; t < t_end; t += t_step) {
      const int64_t i0 = t * kSweepTile, i = i0 + r;  // the lane's swept row
      const bool swp_ok = i < swp_n;
      uint32_t mask;
      float swp_bias = 0.0f;
      if (ROWS) {
        mask = cb_mask(p.tgt_idx, cur, end, i0);
        swp_bias = swp_ok ? p.bo[i] : 0.0f;           // the bias of swept column i0 + r, fetched by its lane
      } else {
        row_meta(i, j0);                              // the lane's swept row of z against the owned columns
        mask = cb_mask(p.tgt_idx, cur, end, j0);
      }

      // acc[q] in lane j = the bias of the element's column + <swept row acc_row(q, lane), owned row j>: the bias is
      // what the accumulator starts from, so it occupies no register of its own beside the tile
      f32x16 acc;
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[q] = ROWS ? __shfl(swp_bias, cb_acc_row(q, lane), kWave) : own_bias;
      const float* w = swp_mat + (swp_ok ? i : 0) * H + 4 * hh;
#pragma unroll
      for (int c = 0; c < H / 8; ++c) {
        float4 wv = ld4(w + 8 * c);
        if (!swp_ok) wv = zero4();
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.x, own[4 * c + 0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.y, own[4 * c + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.z, own[4 * c + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.w, own[4 * c + 3], acc, 0, 0, 0);
      }

      // the epilogue: the loss terms (ROWS) and g in place of the pre-activations
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int ri = cb_acc_row(q, lane);           // the swept row of this element inside the tile
        const bool ok = own_ok && i0 + ri < swp_n;
        const bool hit = ((ROWS ? mask >> ri : __shfl(mask, ri, kWave) >> r) & 1u) != 0;
        float term, g;
        cdae_bce_of_pre(acc[q], hit ? 1.0f : 0.0f, p.act, term, g);
        g = ok ? g * p.inv : 0.0f;
        lsum += ROWS ? (ok ? term : 0.0f) : g;
        acc[q] = g;
      }

      // dO[j] += sum_i g[i, j] W[i]: step q of the matrix instruction reads swept row acc_row(q, lane)
      if (grad) {
        const float* tile = swp_mat + i0 * H;         // 32-bit offsets inside the tile
        const int rows_in = (int)std::min<int64_t>(kSweepTile, swp_n - i0);
#pragma unroll
        for (int u = 0; u < NT; ++u) {
          const int e = u * 32 + r;
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int ri = cb_acc_row(q, lane);
            const float b = (ri < rows_in && e < H) ? tile[ri * H + e] : 0.0f;
            dacc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[q], b, dacc[u], 0, 0, 0);
          }
        }
      }
    }

    // the four waves in wave order: sO [32][H] of the owned rows' gradient, sL [32] of their loss / their db_o
    lsum += __shfl_xor(lsum, 32, kWave);
    for (int w = 0; w < kWavesPerBlock; ++w) {
      if (wave == w) {
        if (grad) {
#pragma unroll
          for (int u = 0; u < NT; ++u) {
            const int e = u * 32 + r;
            if (e < H) {
#pragma unroll
              for (int q = 0; q < 16; ++q) {
                float* s = sO + cb_acc_row(q, lane) * H + e;
                *s = w == 0 ? dacc[u][q] : *s + dacc[u][q];
              }
            }
          }
        }
        if (hh == 0) sL[r] = w == 0 ? lsum : sL[r] + lsum;
      }
      __syncthreads();
    }
    if (grad) {
      float* out = ROWS ? p.part_dz + (chunk * p.B + j0) * H : p.dWo + j0 * H;
      const int64_t rows = std::min<int64_t>(kSweepTile, own_n - j0);
      for (int e = tid; e < rows * H; e += kBlock) out[e] = sO[e];
    }
    if (tid < kSweepTile && j0 + tid < own_n) {
      if (ROWS) p.part_loss[chunk * p.B + j0 + tid] = sL[tid];
      else p.dbo[j0 + tid] = sL[tid];
    }
    __syncthreads();                                  // the next unit overwrites sO and sL
  }
  if (flag && p.err_flag) atomicOr(p.err_flag, flag);
}

// row_loss[n] = the chunks' partial sums, chunk after chunk; dz likewise
__global__ __launch_bounds__(kBlock) void cdae_cbce_reduce_kernel(const float* __restrict__ part_loss,
                                                                  const float* __restrict__ part_dz, int64_t chunks,
                                                                  int64_t B, int H, float* __restrict__ row_loss,
                                                                  float* __restrict__ dz) {
  const int64_t BH = B * H, total = B + (part_dz ? BH : 0), stride = (int64_t)gridDim.x * kBlock;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += stride) {
    const bool is_loss = e < B;
    const float* src = is_loss ? part_loss + e : part_dz + (e - B);
    const int64_t step = is_loss ? B : BH;
    float s = src[0];
    for (int64_t c = 1; c < chunks; ++c) s += src[c * step];
    if (is_loss) row_loss[e] = s;
    else dz[e - B] = s;
  }
}

}  // namespace yr

using namespace yr;

static bool cdae_cbce_width_ok(int H) { return H == 16 || H == 32 || H == 64 || H == 128; }

static int64_t cdae_cbce_chunks(int64_t I) { return (I + kSweepColChunk - 1) / kSweepColChunk; }

template <bool ROWS>
static int cdae_cbce_launch(const CdaeCbce& p, int H, int64_t units, hipStream_t stream) {
  const dim3 grid((unsigned)std::min<int64_t>(units, kSweepGridMax)), block(kBlock);
  switch (H) {
    case 16: hipLaunchKernelGGL((cdae_cbce_kernel<16, ROWS>), grid, block, 0, stream, p); break;
    case 32: hipLaunchKernelGGL((cdae_cbce_kernel<32, ROWS>), grid, block, 0, stream, p); break;
    case 64: hipLaunchKernelGGL((cdae_cbce_kernel<64, ROWS>), grid, block, 0, stream, p); break;
    default: hipLaunchKernelGGL((cdae_cbce_kernel<128, ROWS>), grid, block, 0, stream, p); break;
  }
  return launch_status();
}

extern "C" int64_t yr_cdae_catalogue_bce_workspace_floats(int64_t B, int64_t I, int H) {
  if (B < 0 || I < 0 || H <= 0) return YR_ERR_BADARG;
  if (!cdae_cbce_width_ok(H)) return YR_ERR_UNSUPPORTED;
  return B * cdae_cbce_chunks(I) * (1 + (int64_t)H);
}

extern "C" int yr_cdae_catalogue_bce(const float* z, const float* Wo, const float* bo, const int64_t* user,
                                     const int64_t* tgt_ptr, const int64_t* tgt_idx, int64_t B, int64_t I, int64_t K,
                                     int H, int act, float* row_loss, float* dz, float* dWo, float* dbo,
                                     float* workspace, int64_t workspace_floats, int32_t* err_flag, void* stream) {
  if (B < 0 || I < 0 || K < 0 || H <= 0 || workspace_floats < 0 || (act != 0 && act != 1)) return YR_ERR_BADARG;
  if (!cdae_cbce_width_ok(H)) return YR_ERR_UNSUPPORTED;
  if (B == 0 || I == 0) return 0;
  if (!z || !Wo || !bo || !user || !tgt_ptr || !tgt_idx || !row_loss || !workspace) return YR_ERR_BADARG;
  if ((dWo == nullptr) != (dbo == nullptr)) return YR_ERR_BADARG;
  if (((reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(Wo)) & 15) != 0) return YR_ERR_BADARG;
  const int64_t chunks = cdae_cbce_chunks(I);
  if (workspace_floats < B * chunks * (1 + (dz ? (int64_t)H : 0))) return YR_ERR_BADARG;
  float* part_loss = workspace;
  float* part_dz = part_loss + chunks * B;
  const double inv = 1.0 / ((double)B * (double)I);
  const CdaeCbce p{z, Wo, bo, user, tgt_ptr, tgt_idx, B, I, K, act, (float)inv, part_loss, dz ? part_dz : nullptr,
                   dWo, dbo, chunks, err_flag};
  hipStream_t st = (hipStream_t)stream;
  const int64_t row_tiles = (B + kSweepTile - 1) / kSweepTile, col_tiles = (I + kSweepTile - 1) / kSweepTile;
  if (const int s = cdae_cbce_launch<true>(p, H, row_tiles * chunks, st)) return s;
  hipLaunchKernelGGL(cdae_cbce_reduce_kernel, dim3(grid_for(B * (dz ? 1 + (int64_t)H : 1), kBlock)), dim3(kBlock), 0,
                     st, part_loss, dz ? part_dz : nullptr, chunks, B, H, row_loss, dz);
  if (const int s = launch_status()) return s;
  if (dWo) return cdae_cbce_launch<false>(p, H, col_tiles, st);
  return 0;
}
