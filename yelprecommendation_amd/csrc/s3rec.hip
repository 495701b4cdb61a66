// S3Rec scoring kernels for gfx950 (MI355X): the self-attention encoder of reference models/s3rec.py:53-71,184-214
// in eval() mode, fused from the embedding gather to the last LayerNorm, and the two score forms of
// models/s3rec.py:73-115 (finetune: every position; evaluate: the last position against a candidate list).
//
// Encoder: one workgroup (4 waves) per sequence.  The sequence's activations never leave the CU: five LDS tiles
//   sH [LP][E + 1]   h, the block's input (both residuals add it: models/s3rec.py:64,70), then the block's output
//   sQ [LP][E + 1]   Q of the head, then A_h = P V (Q is dead once S is formed), then relu(W_1 x1 + b_1)
//   sK [LP][E + 1]   K of the head (rows of REAL positions zeroed: the reference's quirk), then the two pre-LayerNorm sums
//   sV [LP][E + 1]   V of the head, then x1 = LayerNorm1(h + attn)
//   sS [LP][LP + 1]  Q K^T, then the softmax P
//   sPad [LP]        1.0 where X <= 0 (and in the tile's padding rows), else 0.0
// LP = 32 (L <= 32) or 64: the rows are padded to the 32 x 32 x 2 f32 matrix instruction.  Rows >= L start as zeros
// and stay finite; the causal exclusion (keys j > i get probability exactly 0) keeps them out of every row < L, and
// they are never stored.  The odd pitches make both the row-per-lane operand reads (lane = row, 32 rows of one k)
// and the column-per-lane reads and stores (lane = column) conflict-free on the 32-bank ds_read_b32 / ds_write_b32.
//
// Every product runs on v_mfma_f32_32x32x2_f32, a wave owning whole 32 x 32 output tiles:
//   Q, K, V, FFN, output projection: A = activations from LDS, B = the weight rows straight from global memory (L2),
//     16 bytes per lane and 8 k: lane half hh takes k = 8 c + 4 hh + t, the A reads follow the same order;
//   S = Q K^T and A_h = P V: both operands from LDS, k = 2 s + hh.  Tiles above the diagonal are skipped and P V
//     sums over the keys up to the tile's last row only.
// attn = sum_h A_h W_o[:, hE:(h+1)E]^T stays in the matrix accumulators across the heads (two tiles per wave at
// the most: 32 registers), so the concatenation is never built.
//
// Packed parameters (one f32 buffer per model, block after block; H = heads, all offsets multiples of 16 floats):
//   W_q [H][E][E] | W_k [H][E][E] | W_v [H][E][E] | W_o [E][H E] | b_o [E] | ln1.weight [E] | ln1.bias [E] |
//   W_1 [E][E] | b_1 [E] | W_2 [E][E] | b_2 [E] | ln2.weight [E] | ln2.bias [E]          = (4 H + 2) E^2 + 7 E floats
#include <math.h>

#include "common.h"

namespace yr {

constexpr int kS3MaxL = 64;
constexpr int kS3MaxHeads = 4;
constexpr int kS3MaxBlocks = 4;
constexpr float kS3LnEps = 1e-5f;

struct S3Enc {
  const float* item_emb;      // [num_items + 1][E]
  const float* pos;           // [L][E]
  const float* params;        // packed, see above
  const int64_t* X;           // [B][L]
  int64_t B, num_items;
  int L, heads, blocks, last_only;
  float* out;                 // [B][L][E], or [B][E] (last_only)
  int32_t* err_flag;
};

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) x = fmaxf(x, __shfl_xor(x, m, kWave));
  return x;
}

// acc += A (32 x K) . W^T for 32 rows of W: A[i][k] at A[i * pa + k] (LDS), W[n][k] at W[n * ldw + k] (global,
// 16-byte aligned rows); rows n >= nvalid of W do not exist and count as zeros
template <int K>
__device__ __forceinline__ f32x16 mma_weights(const float* A, int pa, const float* __restrict__ W, int64_t ldw,
                                              int nvalid, f32x16 acc, int lane) {
  const int r = lane & 31, hh = lane >> 5;
  const bool ok = r < nvalid;
  const float* a = A + r * pa + 4 * hh;
  const float* w = W + (ok ? r : 0) * ldw + 4 * hh;
#pragma unroll 4
  for (int c = 0; c < K; c += 8) {
    float4 wv = ld4(w + c);
    if (!ok) wv = zero4();
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c + 0], wv.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c + 1], wv.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c + 2], wv.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c + 3], wv.w, acc, 0, 0, 0);
  }
  return acc;
}

// acc += A (32 x K) . B (K x 32), both in LDS: A[i][k] at A[i * pa + k], B[k][n] at B[min(n, nvalid - 1) * sn + k * sk]
__device__ __forceinline__ f32x16 mma_lds(const float* A, int pa, const float* B, int sn, int sk, int nvalid, int K,
                                          f32x16 acc, int lane) {
  const int r = lane & 31, hh = lane >> 5;
  const float* a = A + r * pa + hh;
  const float* b = B + (r < nvalid ? r : nvalid - 1) * sn + hh * sk;
  for (int k = 0; k < K; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k], b[k * sk], acc, 0, 0, 0);
  return acc;
}

// element q of a lane's accumulators is (row, col) of the 32 x 32 tile
__device__ __forceinline__ int acc_row(int q, int lane) { return (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5); }

// dst[i][:] = LayerNorm(src[i][:]) (biased variance) for the rows of this wave
template <int E>
__device__ __forceinline__ void layernorm_rows(const float* src, float* dst, int P, int rows, const float* __restrict__ g,
                                               const float* __restrict__ b, int lane, int wave) {
  constexpr int EPL = E > kWave ? E / kWave : 1;
  for (int i = wave; i < rows; i += kWavesPerBlock) {
    float x[EPL], s = 0.0f;
#pragma unroll
    for (int t = 0; t < EPL; ++t) {
      const int e = lane + kWave * t;
      x[t] = e < E ? src[i * P + e] : 0.0f;
      s += x[t];
    }
    const float mean = wave_sum(s) / (float)E;
    float v = 0.0f;
#pragma unroll
    for (int t = 0; t < EPL; ++t) {
      const int e = lane + kWave * t;
      const float d = e < E ? x[t] - mean : 0.0f;
      v += d * d;
    }
    const float rstd = 1.0f / sqrtf(wave_sum(v) / (float)E + kS3LnEps);
#pragma unroll
    for (int t = 0; t < EPL; ++t) {
      const int e = lane + kWave * t;
      if (e < E) dst[i * P + e] = (x[t] - mean) * rstd * g[e] + b[e];
    }
  }
}

inline size_t s3rec_lds_bytes(int E, int L) {
  const int LP = L > 32 ? 64 : 32;
  return (size_t)(4 * LP * (E + 1) + LP * (LP + 1) + LP) * sizeof(float);
}

template <int E>
__global__ __launch_bounds__(kBlock) void s3rec_encode_kernel(S3Enc p) {
  extern __shared__ float s3_lds[];
  constexpr int P = E + 1;
  constexpr int NT = E >= 32 ? E / 32 : 1;          // column tiles of an [LP][E] result
  const int L = p.L, H = p.heads;
  const int LP = L > 32 ? 64 : 32, MT = LP / 32, PS = LP + 1;
  const int ntile = MT * NT;                         // <= 8: two per wave
  float* sH = s3_lds;
  float* sQ = sH + LP * P;
  float* sK = sQ + LP * P;
  float* sV = sK + LP * P;
  float* sS = sV + LP * P;
  float* sPad = sS + LP * PS;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int r = lane & 31;
  const float sqrtE = sqrtf((float)E);
  const int64_t EE = (int64_t)E * E;
  const int64_t block_stride = (4 * H + 2) * EE + 7 * E;

  for (int64_t seq = blockIdx.x; seq < p.B; seq += gridDim.x) {
    // h = item_embedding[X] + positional_encoding (the positional row at padded positions too)
    const int64_t* X = p.X + seq * L;
    int flag = 0;
    for (int e = tid; e < LP * E; e += kBlock) {
      const int i = e / E, d = e - i * E;
      float v = 0.0f;
      if (i < L) {
        const int64_t id = X[i];
        if (id >= 0 && id <= p.num_items) v = p.item_emb[id * E + d];
        else flag = YR_FLAG_BAD_ITEM;
        v += p.pos[i * E + d];
      }
      sH[i * P + d] = v;
    }
    if (tid < LP) sPad[tid] = (tid < L && X[tid] > 0) ? 0.0f : 1.0f;
    if (flag && p.err_flag) atomicOr(p.err_flag, flag);
    __syncthreads();

    for (int blk = 0; blk < p.blocks; ++blk) {
      const float* Wq = p.params + blk * block_stride;
      const float* Wo = Wq + 3 * H * EE;
      const float* bo = Wo + H * EE;
      const float *g1 = bo + E, *be1 = g1 + E;
      const float* W1 = be1 + E;
      const float* b1 = W1 + EE;
      const float* W2 = b1 + E;
      const float* b2 = W2 + EE;
      const float *g2 = b2 + E, *be2 = g2 + E;

      f32x16 oacc[2] = {zero16(), zero16()};          // attn tiles wave, wave + 4 across the heads
      for (int h = 0; h < H; ++h) {
        // Q, K, V of head h: 3 ntile tiles dealt to the waves
        for (int w = wave; w < 3 * ntile; w += kWavesPerBlock) {
          const int m = w / ntile, t = w - m * ntile, it = t / NT, jt = t - it * NT;
          const float* W = Wq + (m * H + h) * EE + (int64_t)jt * 32 * E;
          const f32x16 acc = mma_weights<E>(sH + it * 32 * P, P, W, E, E - jt * 32, zero16(), lane);
          float* dst = m == 0 ? sQ : m == 1 ? sK : sV;
          const int col = jt * 32 + r;
          if (col < E) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
              const int row = it * 32 + acc_row(q, lane);
              dst[row * P + col] = m == 1 ? acc[q] * sPad[row] : acc[q];
            }
          }
        }
        __syncthreads();
        // S = Q K^T on and below the diagonal tiles
        for (int w = wave; w < MT * (MT + 1) / 2; w += kWavesPerBlock) {
          const int it = w == 0 ? 0 : 1, jt = w == 2 ? 1 : 0;
          const f32x16 acc = mma_lds(sQ + it * 32 * P, P, sK + jt * 32 * P, P, 1, 32, E, zero16(), lane);
#pragma unroll
          for (int q = 0; q < 16; ++q) sS[(it * 32 + acc_row(q, lane)) * PS + jt * 32 + r] = acc[q];
        }
        __syncthreads();
        // P = softmax over the keys j <= i of S / sqrt(E); the keys j > i get exactly 0
        for (int i = wave; i < LP; i += kWavesPerBlock) {
          const bool on = lane <= i;
          const float v = on ? sS[i * PS + lane] / sqrtE : -INFINITY;
          const float mx = wave_max(v);
          const float ex = on ? expf(v - mx) : 0.0f;
          const float sum = wave_sum(ex);
          if (lane < LP) sS[i * PS + lane] = ex / sum;
        }
        __syncthreads();
        // A_h = P V into sQ
        for (int t = wave; t < ntile; t += kWavesPerBlock) {
          const int it = t / NT, jt = t - it * NT;
          const f32x16 acc = mma_lds(sS + it * 32 * PS, PS, sV + jt * 32, 1, P, E - jt * 32, (it + 1) * 32, zero16(), lane);
          const int col = jt * 32 + r;
          if (col < E) {
#pragma unroll
            for (int q = 0; q < 16; ++q) sQ[(it * 32 + acc_row(q, lane)) * P + col] = acc[q];
          }
        }
        __syncthreads();
        // attn += A_h W_o[:, hE:(h+1)E]^T
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int t = wave + kWavesPerBlock * u;
          if (t < ntile) {
            const int it = t / NT, jt = t - it * NT;
            oacc[u] = mma_weights<E>(sQ + it * 32 * P, P, Wo + (int64_t)jt * 32 * H * E + h * E, (int64_t)H * E,
                                     E - jt * 32, oacc[u], lane);
          }
        }
        __syncthreads();
      }
      // h + attn + b_o -> sK, x1 = LayerNorm1 -> sV
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int t = wave + kWavesPerBlock * u;
        const int it = t / NT, jt = t - it * NT, col = jt * 32 + r;
        if (t < ntile && col < E) {
          const float bias = bo[col];
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int row = it * 32 + acc_row(q, lane);
            sK[row * P + col] = sH[row * P + col] + (oacc[u][q] + bias);
          }
        }
      }
      __syncthreads();
      layernorm_rows<E>(sK, sV, P, LP, g1, be1, lane, wave);
      __syncthreads();
      // relu(W_1 x1 + b_1) -> sQ
      for (int t = wave; t < ntile; t += kWavesPerBlock) {
        const int it = t / NT, jt = t - it * NT, col = jt * 32 + r;
        const f32x16 acc = mma_weights<E>(sV + it * 32 * P, P, W1 + (int64_t)jt * 32 * E, E, E - jt * 32, zero16(), lane);
        if (col < E) {
          const float bias = b1[col];
#pragma unroll
          for (int q = 0; q < 16; ++q) sQ[(it * 32 + acc_row(q, lane)) * P + col] = fmaxf(acc[q] + bias, 0.0f);
        }
      }
      __syncthreads();
      // h + W_2 (.) + b_2 -> sK (the reference adds the block's INPUT here, not x1), LayerNorm2 -> sH
      for (int t = wave; t < ntile; t += kWavesPerBlock) {
        const int it = t / NT, jt = t - it * NT, col = jt * 32 + r;
        const f32x16 acc = mma_weights<E>(sQ + it * 32 * P, P, W2 + (int64_t)jt * 32 * E, E, E - jt * 32, zero16(), lane);
        if (col < E) {
          const float bias = b2[col];
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int row = it * 32 + acc_row(q, lane);
            sK[row * P + col] = sH[row * P + col] + (acc[q] + bias);
          }
        }
      }
      __syncthreads();
      layernorm_rows<E>(sK, sH, P, LP, g2, be2, lane, wave);
      __syncthreads();
    }

    if (p.last_only) {
      for (int d = tid; d < E; d += kBlock) p.out[seq * E + d] = sH[(L - 1) * P + d];
    } else {
      float* out = p.out + seq * L * E;
      for (int e = tid; e < L * E; e += kBlock) {
        const int i = e / E;
        out[e] = sH[i * P + (e - i * E)];
      }
    }
    __syncthreads();                                  // the next sequence overwrites sH
  }
}

// out_a[r] = <I[items_a[r]], h[r / per_a]> for r < rows_a and the same for list b: 16 lanes per row.  A bad id
// raises the flag and scores 0.
struct S3Scores {
  const float* item_emb;
  const float* h;
  const int64_t *items_a, *items_b;
  int64_t rows_a, rows_b, per_a, per_b, num_items;
  int E;
  float *out_a, *out_b;
  int32_t* err_flag;
};

__global__ __launch_bounds__(kBlock) void s3rec_scores_kernel(S3Scores p) {
  constexpr int LPR = 16;
  const int sub = threadIdx.x & (LPR - 1);
  const int64_t rows = p.rows_a + p.rows_b;
  const int64_t rounds = (rows + kBlock / LPR - 1) / (kBlock / LPR);
  int flag = 0;
  // whole rounds, so that the 16 lanes of a row stay together in the shuffles
  for (int64_t rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
    const int64_t row = rd * (kBlock / LPR) + threadIdx.x / LPR;
    float s = 0.0f;
    bool ok = false;
    const bool a = row < p.rows_a;
    const int64_t ra = a ? row : row - p.rows_a;
    if (row < rows) {
      const int64_t id = a ? p.items_a[ra] : p.items_b[ra];
      ok = id >= 0 && id <= p.num_items;
      if (ok) {
        const float* e = p.item_emb + id * p.E;
        const float* hr = p.h + (ra / (a ? p.per_a : p.per_b)) * p.E;
        for (int d = sub; d < p.E; d += LPR) s += e[d] * hr[d];
      } else {
        flag = YR_FLAG_BAD_ITEM;
      }
    }
    s = group_sum<LPR>(s);
    if (row < rows && sub == 0) (a ? p.out_a : p.out_b)[ra] = s;
  }
  if (flag && p.err_flag) atomicOr(p.err_flag, flag);
}

}  // namespace yr

using namespace yr;

static bool s3rec_width_ok(int E) { return E == 16 || E == 32 || E == 64 || E == 128; }

template <int E>
static int s3rec_launch(const S3Enc& p, hipStream_t stream) {
  const size_t lds = s3rec_lds_bytes(E, p.L);
  static bool raised = false;                        // more than the default 64 KB of dynamic LDS: once per process
  if (!raised && lds > 65536) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&s3rec_encode_kernel<E>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256);
    if (e != hipSuccess) return (int)e;
    raised = true;
  }
  const int grid = (int)std::min<int64_t>(p.B, 1 << 20);
  hipLaunchKernelGGL(s3rec_encode_kernel<E>, dim3(grid), dim3(kBlock), lds, stream, p);
  return launch_status();
}

extern "C" int yr_s3rec_encode(const float* item_emb, const float* pos_enc, const float* params, const int64_t* X,
                               int64_t B, int L, int E, int heads, int blocks, int64_t num_items, int last_only,
                               float* out, int32_t* err_flag, void* stream) {
  if (B < 0 || L <= 0 || E <= 0 || heads <= 0 || blocks <= 0 || num_items < 0) return YR_ERR_BADARG;
  if (!s3rec_width_ok(E) || L > kS3MaxL || heads > kS3MaxHeads || blocks > kS3MaxBlocks) return YR_ERR_UNSUPPORTED;
  if (B == 0) return 0;
  if (!item_emb || !pos_enc || !params || !X || !out) return YR_ERR_BADARG;
  if ((reinterpret_cast<uintptr_t>(params) & 15) != 0) return YR_ERR_BADARG;
  const S3Enc p{item_emb, pos_enc, params, X, B, num_items, L, heads, blocks, last_only != 0, out, err_flag};
  switch (E) {
    case 16: return s3rec_launch<16>(p, (hipStream_t)stream);
    case 32: return s3rec_launch<32>(p, (hipStream_t)stream);
    case 64: return s3rec_launch<64>(p, (hipStream_t)stream);
    default: return s3rec_launch<128>(p, (hipStream_t)stream);
  }
}

static int s3rec_scores(const S3Scores& p, hipStream_t stream) {
  const int64_t rows = p.rows_a + p.rows_b;
  hipLaunchKernelGGL(s3rec_scores_kernel, dim3(grid_for(rows, kBlock / 16)), dim3(kBlock), 0, stream, p);
  return launch_status();
}

extern "C" int yr_s3rec_seq_scores(const float* item_emb, const float* h, const int64_t* pos_items,
                                   const int64_t* neg_items, int64_t rows, int E, int64_t num_items, float* pos_preds,
                                   float* neg_preds, int32_t* err_flag, void* stream) {
  if (rows < 0 || E <= 0 || num_items < 0) return YR_ERR_BADARG;
  if (!s3rec_width_ok(E)) return YR_ERR_UNSUPPORTED;
  if (rows == 0) return 0;
  if (!item_emb || !h || !pos_items || !neg_items || !pos_preds || !neg_preds) return YR_ERR_BADARG;
  return s3rec_scores(S3Scores{item_emb, h, pos_items, neg_items, rows, rows, 1, 1, num_items, E, pos_preds, neg_preds,
                               err_flag},
                      (hipStream_t)stream);
}

extern "C" int yr_s3rec_candidate_scores(const float* item_emb, const float* h_last, const int64_t* pos_item,
                                         const int64_t* neg_items, int64_t B, int64_t C, int E, int64_t num_items,
                                         float* pos_pred, float* neg_preds, int32_t* err_flag, void* stream) {
  if (B < 0 || C <= 0 || E <= 0 || num_items < 0) return YR_ERR_BADARG;
  if (!s3rec_width_ok(E)) return YR_ERR_UNSUPPORTED;
  if (B == 0) return 0;
  if (!item_emb || !h_last || !pos_item || !neg_items || !pos_pred || !neg_preds) return YR_ERR_BADARG;
  return s3rec_scores(S3Scores{item_emb, h_last, pos_item, neg_items, B, B * C, 1, C, num_items, E, pos_pred, neg_preds,
                               err_flag},
                      (hipStream_t)stream);
}
