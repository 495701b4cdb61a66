// S3Rec kernels for gfx950 (MI355X): the self-attention encoder of reference models/s3rec.py:53-71,184-214, fused
// from the embedding gather to the last LayerNorm, in eval() mode (scoring) and in train() mode (dropout and a stash,
// see "what train() mode adds" below): one kernel text, s3rec_encode_kernel<E, TRAIN>; the two score forms of
// models/s3rec.py:73-115 (finetune: every position; evaluate: the last position against a candidate list); and, under
// "backward" below, the encoder's backward pass and the score and item gradients.
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
#include "philox.h"

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

// P = softmax over the keys j <= i of S / sqrt(E), in place, a wave per row; the keys j > i get exactly 0
__device__ __forceinline__ void softmax_causal_rows(float* sS, int PS, int LP, float sqrtE, int lane, int wave) {
  for (int i = wave; i < LP; i += kWavesPerBlock) {
    const bool on = lane <= i;
    const float v = on ? sS[i * PS + lane] / sqrtE : -INFINITY;
    const float mx = wave_max(v);
    const float ex = on ? expf(v - mx) : 0.0f;
    const float sum = wave_sum(ex);
    if (lane < LP) sS[i * PS + lane] = ex / sum;
  }
}

inline size_t s3rec_lds_bytes(int E, int L) {
  const int LP = L > 32 ? 64 : 32;
  return (size_t)(4 * LP * (E + 1) + LP * (LP + 1) + LP) * sizeof(float);
}

// ========================================================== the encoder (both modes) and what train() mode adds
// s3rec_encode_kernel<E, true> adds to the encoder dropout at the two sites of a block (reference
// models/s3rec.py:62,68: after W_o + b_o and after W_2 + b_2, before the residual) and a stash in global memory of
// what the backward consumes; the backward (s3rec_backward_kernel) walks the blocks in reverse, again one
// workgroup per sequence and nothing reduced across workgroups: it leaves, per block, the delta tensors whose
// transposed products with the stash are the weight gradients (yr_gemm_f32 transA = 1) and whose column sums are
// the bias / LayerNorm gradients (yr_colsum).
//
// Workspace, block after block, R = B L rows with row index b L + i, every array [R][width] row-major:
//   stash   h_in E | qkv 3 H E (Q[H] | K[H] | V[H], K masked: the order of the packed W_q | W_k | W_v) | A H E |
//           x1 E | xh1 E (LayerNorm1's normalised value) | relu E | xh2 E | rstd 4 (rstd1, rstd2, -, -)
//   deltas  g2 E (the gradient arriving at the block's output) | gx2 E = g2 * xh2 | d2m E = d_s2 * mask2 | dz1 E |
//           g1 E = d_x1 | gx1 E = g1 * xh1 | d1m E = d_s1 * mask1 | dqkv 3 H E | dA H E (staging only)
//   = (12 + 8 H) E + 4 floats per row and block.  P is recomputed from the stashed Q and K.
// The dropout mask is a pure function of (seed, site = 2 block + {0, 1}, flat index in [B, L, E]) in the law of
// yr_dropout_seeded: float4 group q draws philox4x32<10> at the counter (q lo, q hi, site, 0), word t belongs to
// element 4 q + t, kept where u01 >= p and scaled by 1 / (1 - p).  The backward draws it again.

struct S3Layout {
  int64_t h_in, qkv, A, x1, xh1, relu, xh2, rstd, g2, gx2, d2m, dz1, g1, gx1, d1m, dqkv, dA, block;
};

__host__ __device__ inline S3Layout s3_layout(int64_t R, int E, int H) {
  S3Layout o;
  const int64_t RE = R * E;
  int64_t at = 0;
  o.h_in = at; at += RE;
  o.qkv = at; at += 3 * H * RE;
  o.A = at; at += H * RE;
  o.x1 = at; at += RE;
  o.xh1 = at; at += RE;
  o.relu = at; at += RE;
  o.xh2 = at; at += RE;
  o.rstd = at; at += 4 * R;
  o.g2 = at; at += RE;
  o.gx2 = at; at += RE;
  o.d2m = at; at += RE;
  o.dz1 = at; at += RE;
  o.g1 = at; at += RE;
  o.gx1 = at; at += RE;
  o.d1m = at; at += RE;
  o.dqkv = at; at += 3 * H * RE;
  o.dA = at; at += H * RE;
  o.block = at;
  return o;
}

struct S3Train {
  S3Enc enc;                  // last_only unused; out [B][L][E] (forward) or d_emb [B][L][E] (backward)
  float* ws;
  const float* dh_out;        // backward only: [B][L][E]
  uint64_t seed;
  float p, scale;             // dropout probability and 1 / (1 - p)
};

// The dropout of one site over a sequence's [LP][E] tile, a thread per float4 group (E is a multiple of 4 and so
// is idx0, the flat index of the sequence's first element: a group never leaves its row):
//   tile[i][d] = (res ? res[i][d] : 0) + (kept ? tile[i][d] * scale : 0), rows >= L dropped whole;
// gout (may be null) receives the rows < L of the result.
template <int E>
__device__ __forceinline__ void dropout_tile(float* tile, const float* res, int P, int L, int LP, uint2 key,
                                             uint32_t site, int64_t idx0, float p, float scale, float* gout, int tid) {
  for (int g = tid; g < LP * (E / 4); g += kBlock) {
    const int i = g / (E / 4), d = 4 * (g - i * (E / 4));
    const int64_t q = (idx0 + (int64_t)i * E + d) >> 2;
    const uint4 w = philox4x32_rolled(make_uint4((uint32_t)q, (uint32_t)(q >> 32), site, 0u), key, 10);
    const uint32_t word[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float* x = tile + i * P + d + t;
      const float v = (i < L && u01(word[t]) >= p) ? *x * scale : 0.0f;
      *x = res ? res[i * P + d + t] + v : v;
      if (gout && i < L) gout[i * E + d + t] = *x;
    }
  }
}

// acc += A (32 x K, LDS) . W for 32 columns of a row-major global matrix: W(k, n) at W[k * ldw + n]; the columns
// n >= nvalid do not exist and count as zeros
template <int K>
__device__ __forceinline__ f32x16 mma_weights_n(const float* A, int pa, const float* __restrict__ W, int64_t ldw,
                                                int nvalid, f32x16 acc, int lane) {
  const int r = lane & 31, hh = lane >> 5;
  const bool ok = r < nvalid;
  const float* a = A + r * pa + hh;
  const float* w = W + (ok ? r : 0) + hh * ldw;
#pragma unroll 4
  for (int k = 0; k < K; k += 2) {
    const float wv = ok ? w[k * ldw] : 0.0f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k], wv, acc, 0, 0, 0);
  }
  return acc;
}

// acc += A (32 x [k0, k1)) . B ([k0, k1) x 32), both in LDS with free strides: A(i, k) at A[i * ai + k * ak],
// B(k, n) at B[min(n, nvalid - 1) * bn + k * bk]
__device__ __forceinline__ f32x16 mma_lds_s(const float* A, int ai, int ak, const float* B, int bn, int bk, int nvalid,
                                            int k0, int k1, f32x16 acc, int lane) {
  const int r = lane & 31, hh = lane >> 5;
  const float* a = A + r * ai + hh * ak;
  const float* b = B + (r < nvalid ? r : nvalid - 1) * bn + hh * bk;
  for (int k = k0; k < k1; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k * ak], b[k * bk], acc, 0, 0, 0);
  return acc;
}

// dst[i][:] = LayerNorm(src[i][:]) (biased variance) for the rows of this wave.  STASH: also stores the normalised
// value, rstd and (y_out given) the result for the rows < L of this sequence; otherwise the three pointers are unused
template <int E, bool STASH>
__device__ __forceinline__ void layernorm_rows(const float* src, float* dst, int P, int rows, int L,
                                               const float* __restrict__ g, const float* __restrict__ b, float* xh_out,
                                               float* rstd_out, float* y_out, int lane, int wave) {
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
    if (STASH && i < L && lane == 0) rstd_out[i * 4] = rstd;
#pragma unroll
    for (int t = 0; t < EPL; ++t) {
      const int e = lane + kWave * t;
      if (e < E) {
        const float xh = (x[t] - mean) * rstd;
        const float y = xh * g[e] + b[e];
        dst[i * P + e] = y;
        if (STASH && i < L) {
          xh_out[i * E + e] = xh;
          if (y_out) y_out[i * E + e] = y;
        }
      }
    }
  }
}

inline size_t s3rec_train_lds_bytes(int E, int L) {
  const int LP = L > 32 ? 64 : 32;
  return s3rec_lds_bytes(E, L) + (size_t)2 * LP * sizeof(float);
}

// The encoder in both modes.  TRAIN = false (yr_s3rec_encode) reads enc alone and honours last_only; TRAIN = true
// (yr_s3rec_encode_train) stores the stash and drops out where p > 0.  At p = 0 both run the same arithmetic in the
// same order: `out` is equal bit for bit.  The body is the kernel itself, not a device function under two kernels:
// a function body is optimised on its own before it is inlined, which moved the registers of all eight instances.
template <int E, bool TRAIN>
__global__ __launch_bounds__(kBlock, TRAIN ? 2 : 1) void s3rec_encode_kernel(S3Train tp) {
  extern __shared__ float s3_lds[];
  const S3Enc& p = tp.enc;
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
  const S3Layout lay = s3_layout(p.B * L, E, H);
  const uint2 key = make_uint2((uint32_t)tp.seed, (uint32_t)(tp.seed >> 32));
  const bool drop = TRAIN && tp.p > 0.0f;

  for (int64_t seq = blockIdx.x; seq < p.B; seq += gridDim.x) {
    // h = item_embedding[X] + positional_encoding (the positional row at padded positions too)
    const int64_t row0 = seq * L;
    const int64_t* X = p.X + row0;
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
      float* ws = tp.ws + blk * lay.block;
      const int HE = H * E;

      if (TRAIN) {                                      // the block's input
        float* dst = ws + lay.h_in + row0 * E;
        for (int e = tid; e < L * E; e += kBlock) {
          const int i = e / E;
          dst[e] = sH[i * P + (e - i * E)];
        }
      }
      f32x16 oacc[2] = {zero16(), zero16()};          // attn tiles wave, wave + 4 across the heads
      for (int h = 0; h < H; ++h) {
        // Q, K, V of head h: 3 ntile tiles dealt to the waves
        for (int w = wave; w < 3 * ntile; w += kWavesPerBlock) {
          const int m = w / ntile, t = w - m * ntile, it = t / NT, jt = t - it * NT;
          const float* W = Wq + (m * H + h) * EE + (int64_t)jt * 32 * E;
          const f32x16 acc = mma_weights<E>(sH + it * 32 * P, P, W, E, E - jt * 32, zero16(), lane);
          float* dst = m == 0 ? sQ : m == 1 ? sK : sV;
          float* gq = ws + lay.qkv + row0 * 3 * HE + (m * H + h) * E;
          const int col = jt * 32 + r;
          if (col < E) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
              const int row = it * 32 + acc_row(q, lane);
              const float v = m == 1 ? acc[q] * sPad[row] : acc[q];
              dst[row * P + col] = v;
              if (TRAIN && row < L) gq[(int64_t)row * 3 * HE + col] = v;
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
        softmax_causal_rows(sS, PS, LP, sqrtE, lane, wave);
        __syncthreads();
        // A_h = P V into sQ
        for (int t = wave; t < ntile; t += kWavesPerBlock) {
          const int it = t / NT, jt = t - it * NT;
          const f32x16 acc = mma_lds(sS + it * 32 * PS, PS, sV + jt * 32, 1, P, E - jt * 32, (it + 1) * 32, zero16(), lane);
          float* ga = ws + lay.A + row0 * HE + h * E;
          const int col = jt * 32 + r;
          if (col < E) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
              const int row = it * 32 + acc_row(q, lane);
              sQ[row * P + col] = acc[q];
              if (TRAIN && row < L) ga[(int64_t)row * HE + col] = acc[q];
            }
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
      // h + dropout(attn + b_o) -> sK, x1 = LayerNorm1 -> sV
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int t = wave + kWavesPerBlock * u;
        const int it = t / NT, jt = t - it * NT, col = jt * 32 + r;
        if (t < ntile && col < E) {
          const float bias = bo[col];
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int row = it * 32 + acc_row(q, lane);
            const float a = oacc[u][q] + bias;
            sK[row * P + col] = drop ? a : sH[row * P + col] + a;
          }
        }
      }
      __syncthreads();
      if (drop) {
        dropout_tile<E>(sK, sH, P, L, LP, key, 2 * blk, row0 * E, tp.p, tp.scale, nullptr, tid);
        __syncthreads();
      }
      layernorm_rows<E, TRAIN>(sK, sV, P, LP, L, g1, be1, ws + lay.xh1 + row0 * E, ws + lay.rstd + row0 * 4,
                               ws + lay.x1 + row0 * E, lane, wave);
      __syncthreads();
      // relu(W_1 x1 + b_1) -> sQ
      for (int t = wave; t < ntile; t += kWavesPerBlock) {
        const int it = t / NT, jt = t - it * NT, col = jt * 32 + r;
        const f32x16 acc = mma_weights<E>(sV + it * 32 * P, P, W1 + (int64_t)jt * 32 * E, E, E - jt * 32, zero16(), lane);
        float* gr = ws + lay.relu + row0 * E;
        if (col < E) {
          const float bias = b1[col];
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int row = it * 32 + acc_row(q, lane);
            const float v = fmaxf(acc[q] + bias, 0.0f);
            sQ[row * P + col] = v;
            if (TRAIN && row < L) gr[row * E + col] = v;
          }
        }
      }
      __syncthreads();
      // h + dropout(W_2 (.) + b_2) -> sK (the reference adds the block's INPUT here, not x1), LayerNorm2 -> sH
      for (int t = wave; t < ntile; t += kWavesPerBlock) {
        const int it = t / NT, jt = t - it * NT, col = jt * 32 + r;
        const f32x16 acc = mma_weights<E>(sQ + it * 32 * P, P, W2 + (int64_t)jt * 32 * E, E, E - jt * 32, zero16(), lane);
        if (col < E) {
          const float bias = b2[col];
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int row = it * 32 + acc_row(q, lane);
            const float a = acc[q] + bias;
            sK[row * P + col] = drop ? a : sH[row * P + col] + a;
          }
        }
      }
      __syncthreads();
      if (drop) {
        dropout_tile<E>(sK, sH, P, L, LP, key, 2 * blk + 1, row0 * E, tp.p, tp.scale, nullptr, tid);
        __syncthreads();
      }
      layernorm_rows<E, TRAIN>(sK, sH, P, LP, L, g2, be2, ws + lay.xh2 + row0 * E, ws + lay.rstd + row0 * 4 + 1,
                               nullptr, lane, wave);
      __syncthreads();
    }

    if (!TRAIN && p.last_only) {
      for (int d = tid; d < E; d += kBlock) p.out[seq * E + d] = sH[(L - 1) * P + d];
    } else {
      float* out = p.out + row0 * E;
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

// ================================================================================================ backward

// LayerNorm backward of the rows of sG (the gradient g arriving at the LayerNorm's output): stores g and g * xh for
// the gamma / beta column sums, then d = rstd (dy - mean(dy) - xh mean(dy xh)), dy = g gamma.  ACC: sAcc += d, else
// sAcc = d; sM = d, also stored to dm_out where given (the caller applies the dropout mask).  sG and sM may be the
// same tile.
template <int E, bool ACC>
__device__ __forceinline__ void layernorm_bwd_rows(const float* sG, float* sAcc, float* sM, int P, int rows, int L,
                                                   const float* __restrict__ gamma, const float* xh_in,
                                                   const float* rstd_in, float* g_out, float* gx_out, float* dm_out,
                                                   int lane, int wave) {
  constexpr int EPL = E > kWave ? E / kWave : 1;
  for (int i = wave; i < rows; i += kWavesPerBlock) {
    const bool real = i < L;
    float dy[EPL], xh[EPL], s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int t = 0; t < EPL; ++t) {
      const int e = lane + kWave * t;
      const bool on = e < E;
      const float g = on ? sG[i * P + e] : 0.0f;
      xh[t] = on && real ? xh_in[i * E + e] : 0.0f;
      if (on && real) {
        g_out[i * E + e] = g;
        gx_out[i * E + e] = g * xh[t];
      }
      dy[t] = on ? g * gamma[e] : 0.0f;
      s1 += dy[t];
      s2 += dy[t] * xh[t];
    }
    const float m1 = wave_sum(s1) / (float)E, m2 = wave_sum(s2) / (float)E;
    const float rstd = real ? rstd_in[i * 4] : 0.0f;
#pragma unroll
    for (int t = 0; t < EPL; ++t) {
      const int e = lane + kWave * t;
      if (e < E) {
        const float d = rstd * ((dy[t] - m1) - xh[t] * m2);
        sAcc[i * P + e] = ACC ? sAcc[i * P + e] + d : d;
        sM[i * P + e] = d;
        if (real && dm_out) dm_out[i * E + e] = d;
      }
    }
  }
}

// tile[i][:] = src[(i) * ld + 0 .. E) for the rows i < L, zeros for L <= i < LP
template <int E>
__device__ __forceinline__ void load_rows(float* tile, int P, const float* src, int64_t ld, int L, int LP, int tid) {
  for (int e = tid; e < LP * E; e += kBlock) {
    const int i = e / E, d = e - i * E;
    tile[i * P + d] = i < L ? src[(int64_t)i * ld + d] : 0.0f;
  }
}

template <int E>
__global__ __launch_bounds__(kBlock) void s3rec_backward_kernel(S3Train tp) {
  extern __shared__ float s3_lds[];
  const S3Enc& p = tp.enc;
  constexpr int P = E + 1;
  constexpr int NT = E >= 32 ? E / 32 : 1;
  const int L = p.L, H = p.heads, HE = H * E;
  const int LP = L > 32 ? 64 : 32, MT = LP / 32, PS = LP + 1;
  const int ntile = MT * NT;
  float* T0 = s3_lds;                                 // the gradient g at the block's output, then d_s2 + d_s1, then dA_h
  float* T1 = T0 + LP * P;                            // d2m, d_x1, d1m, then Q
  float* T2 = T1 + LP * P;                            // dz1, then K
  float* T3 = T2 + LP * P;                            // V
  float* sS = T3 + LP * P;                            // S, P, then dS
  float* sPad = sS + LP * PS;
  float* sDelta = sPad + LP;                          // [2][LP]: rowsum(dP * P) per column tile
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int r = lane & 31;
  const float sqrtE = sqrtf((float)E);
  const int64_t EE = (int64_t)E * E;
  const int64_t block_stride = (4 * H + 2) * EE + 7 * E;
  const S3Layout lay = s3_layout(p.B * L, E, H);
  const uint2 key = make_uint2((uint32_t)tp.seed, (uint32_t)(tp.seed >> 32));
  const bool drop = tp.p > 0.0f;

  for (int64_t seq = blockIdx.x; seq < p.B; seq += gridDim.x) {
    const int64_t row0 = seq * L;
    const int64_t* X = p.X + row0;
    float* dh = p.out + row0 * E;                     // d_s2 + d_s1 of the block, then its dh_in; after block 0: d_emb
    load_rows<E>(T0, P, tp.dh_out + row0 * E, E, L, LP, tid);
    if (tid < LP) sPad[tid] = (tid < L && X[tid] > 0) ? 0.0f : 1.0f;

    for (int blk = p.blocks - 1; blk >= 0; --blk) {
      const float* Wq = p.params + blk * block_stride;
      const float* Wo = Wq + 3 * H * EE;
      const float* g1 = Wo + H * EE + E;
      const float* W1 = g1 + 2 * E;
      const float* W2 = W1 + EE + E;
      const float* g2 = W2 + EE + E;
      float* ws = tp.ws + blk * lay.block;
      const float* rstd = ws + lay.rstd + row0 * 4;
      __syncthreads();
      // LayerNorm2: T0 = d_s2, T1 = d2m
      layernorm_bwd_rows<E, false>(T0, T0, T1, P, LP, L, g2, ws + lay.xh2 + row0 * E, rstd + 1, ws + lay.g2 + row0 * E,
                                   ws + lay.gx2 + row0 * E, drop ? nullptr : ws + lay.d2m + row0 * E, lane, wave);
      __syncthreads();
      if (drop) {
        dropout_tile<E>(T1, nullptr, P, L, LP, key, 2 * blk + 1, row0 * E, tp.p, tp.scale, ws + lay.d2m + row0 * E, tid);
        __syncthreads();
      }
      // dz1 = (d2m W_2) * (relu > 0) -> T2
      for (int t = wave; t < ntile; t += kWavesPerBlock) {
        const int it = t / NT, jt = t - it * NT, col = jt * 32 + r;
        const f32x16 acc = mma_weights_n<E>(T1 + it * 32 * P, P, W2 + jt * 32, E, E - jt * 32, zero16(), lane);
        const float* relu = ws + lay.relu + row0 * E;
        float* gz = ws + lay.dz1 + row0 * E;
        if (col < E) {
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int row = it * 32 + acc_row(q, lane);
            const float v = (row < L && relu[row * E + col] > 0.0f) ? acc[q] : 0.0f;
            T2[row * P + col] = v;
            if (row < L) gz[row * E + col] = v;
          }
        }
      }
      __syncthreads();
      // d_x1 = dz1 W_1 -> T1
      for (int t = wave; t < ntile; t += kWavesPerBlock) {
        const int it = t / NT, jt = t - it * NT, col = jt * 32 + r;
        const f32x16 acc = mma_weights_n<E>(T2 + it * 32 * P, P, W1 + jt * 32, E, E - jt * 32, zero16(), lane);
        if (col < E) {
#pragma unroll
          for (int q = 0; q < 16; ++q) T1[(it * 32 + acc_row(q, lane)) * P + col] = acc[q];
        }
      }
      __syncthreads();
      // LayerNorm1: T0 += d_s1 (both residuals add the block's input), T1 = d1m
      layernorm_bwd_rows<E, true>(T1, T0, T1, P, LP, L, g1, ws + lay.xh1 + row0 * E, rstd, ws + lay.g1 + row0 * E,
                                  ws + lay.gx1 + row0 * E, drop ? nullptr : ws + lay.d1m + row0 * E, lane, wave);
      __syncthreads();
      if (drop) {
        dropout_tile<E>(T1, nullptr, P, L, LP, key, 2 * blk, row0 * E, tp.p, tp.scale, ws + lay.d1m + row0 * E, tid);
        __syncthreads();
      }
      for (int e = tid; e < L * E; e += kBlock) {
        const int i = e / E;
        dh[e] = T0[i * P + (e - i * E)];
      }
      // dA = d1m W_o, head after head, to the workspace
      for (int w = wave; w < H * ntile; w += kWavesPerBlock) {
        const int h = w / ntile, t = w - h * ntile, it = t / NT, jt = t - it * NT, col = jt * 32 + r;
        const f32x16 acc = mma_weights_n<E>(T1 + it * 32 * P, P, Wo + h * E + jt * 32, HE, E - jt * 32, zero16(), lane);
        float* ga = ws + lay.dA + row0 * HE + h * E;
        if (col < E) {
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int row = it * 32 + acc_row(q, lane);
            if (row < L) ga[(int64_t)row * HE + col] = acc[q];
          }
        }
      }
      float* gq = ws + lay.dqkv + row0 * 3 * HE;
      for (int h = 0; h < H; ++h) {
        __syncthreads();
        const float* qkv = ws + lay.qkv + row0 * 3 * HE;
        load_rows<E>(T1, P, qkv + h * E, 3 * HE, L, LP, tid);
        load_rows<E>(T2, P, qkv + (H + h) * E, 3 * HE, L, LP, tid);
        load_rows<E>(T3, P, qkv + (2 * H + h) * E, 3 * HE, L, LP, tid);
        load_rows<E>(T0, P, ws + lay.dA + row0 * HE + h * E, HE, L, LP, tid);
        __syncthreads();
        for (int w = wave; w < MT * (MT + 1) / 2; w += kWavesPerBlock) {
          const int it = w == 0 ? 0 : 1, jt = w == 2 ? 1 : 0;
          const f32x16 acc = mma_lds(T1 + it * 32 * P, P, T2 + jt * 32 * P, P, 1, 32, E, zero16(), lane);
#pragma unroll
          for (int q = 0; q < 16; ++q) sS[(it * 32 + acc_row(q, lane)) * PS + jt * 32 + r] = acc[q];
        }
        __syncthreads();
        softmax_causal_rows(sS, PS, LP, sqrtE, lane, wave);
        __syncthreads();
        // dV = P^T dA_h (queries i >= the tile's first key)
        for (int t = wave; t < ntile; t += kWavesPerBlock) {
          const int it = t / NT, jt = t - it * NT, col = jt * 32 + r;
          const f32x16 acc = mma_lds_s(sS + it * 32, 1, PS, T0 + jt * 32, 1, P, E - jt * 32, it * 32, LP, zero16(), lane);
          if (col < E) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
              const int row = it * 32 + acc_row(q, lane);
              if (row < L) gq[(int64_t)row * 3 * HE + (2 * H + h) * E + col] = acc[q];
            }
          }
        }
        // dP = dA_h V^T on the tiles on and below the diagonal, a tile per wave; delta = rowsum(dP * P) from the
        // tile's own values (at one key dP - delta is exactly zero), the two tiles of the rows >= 32 added in a fixed
        // order; then dS = P (dP - delta) / sqrt(E) in place of P
        const bool has = wave < MT * (MT + 1) / 2;
        const int sit = wave == 0 ? 0 : 1, sjt = wave == 2 ? 1 : 0;
        f32x16 dp = zero16();
        if (has) {
          dp = mma_lds(T0 + sit * 32 * P, P, T3 + sjt * 32 * P, P, 1, 32, E, zero16(), lane);
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int row = sit * 32 + acc_row(q, lane);
            const float part = group_sum<32>(dp[q] * sS[row * PS + sjt * 32 + r]);
            if (r == 0) sDelta[sjt * LP + row] = part;
          }
        }
        __syncthreads();
        if (has) {
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int row = sit * 32 + acc_row(q, lane);
            const float delta = row < 32 ? sDelta[row] : sDelta[row] + sDelta[LP + row];
            float* s = sS + row * PS + sjt * 32 + r;
            *s = *s * (dp[q] - delta) / sqrtE;
          }
        }
        __syncthreads();
        // dQ = dS K (keys up to the tile's last row), dK = (dS^T Q) * pad[j] (queries from the tile's first key)
        for (int w = wave; w < 2 * ntile; w += kWavesPerBlock) {
          const int m = w / ntile, t = w - m * ntile, it = t / NT, jt = t - it * NT, col = jt * 32 + r;
          const f32x16 acc = m == 0
              ? mma_lds_s(sS + it * 32 * PS, PS, 1, T2 + jt * 32, 1, P, E - jt * 32, 0, (it + 1) * 32, zero16(), lane)
              : mma_lds_s(sS + it * 32, 1, PS, T1 + jt * 32, 1, P, E - jt * 32, it * 32, LP, zero16(), lane);
          if (col < E) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
              const int row = it * 32 + acc_row(q, lane);
              if (row < L) gq[(int64_t)row * 3 * HE + (m * H + h) * E + col] = m == 1 ? acc[q] * sPad[row] : acc[q];
            }
          }
        }
      }
      // dh_in = (d_s2 + d_s1) + dqkv [LP][3 H E] . (W_q | W_k | W_v) [3 H E][E], E columns of dqkv at a time
      f32x16 hacc[2] = {zero16(), zero16()};
      for (int c = 0; c < 3 * H; ++c) {
        float* tile = (c & 1) ? T1 : T0;
        if (c < 2) __syncthreads();
        load_rows<E>(tile, P, gq + c * E, 3 * HE, L, LP, tid);
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int t = wave + kWavesPerBlock * u;
          if (t < ntile) {
            const int it = t / NT, jt = t - it * NT;
            hacc[u] = mma_weights_n<E>(tile + it * 32 * P, P, Wq + c * EE + jt * 32, E, E - jt * 32, hacc[u], lane);
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int t = wave + kWavesPerBlock * u;
        const int it = t / NT, jt = t - it * NT, col = jt * 32 + r;
        if (t < ntile && col < E) {
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int row = it * 32 + acc_row(q, lane);
            const float v = row < L ? dh[row * E + col] + hacc[u][q] : 0.0f;
            T0[row * P + col] = v;
            if (row < L) dh[row * E + col] = v;
          }
        }
      }
    }
    __syncthreads();                                  // the next sequence overwrites the tiles
  }
}

// dh_out[r] = dpos[r] I[pos_items[r]] + dneg[r] I[neg_items[r]]; a bad id raises the flag and contributes nothing
__global__ __launch_bounds__(kBlock) void s3rec_score_grad_kernel(const float* __restrict__ item_emb,
                                                                  const int64_t* __restrict__ pos_items,
                                                                  const int64_t* __restrict__ neg_items,
                                                                  const float* __restrict__ dpos,
                                                                  const float* __restrict__ dneg, int64_t rows, int E,
                                                                  int64_t num_items, float* __restrict__ dh_out,
                                                                  int32_t* err_flag) {
  const int64_t total = rows * E, stride = (int64_t)gridDim.x * kBlock;
  int flag = 0;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += stride) {
    const int64_t row = e / E;
    const int d = (int)(e - row * E);
    const int64_t ip = pos_items[row], in = neg_items[row];
    float v = 0.0f;
    if (ip >= 0 && ip <= num_items) v += dpos[row] * item_emb[ip * E + d];
    else flag = YR_FLAG_BAD_ITEM;
    if (in >= 0 && in <= num_items) v += dneg[row] * item_emb[in * E + d];
    else flag = YR_FLAG_BAD_ITEM;
    dh_out[e] = v;
  }
  if (flag && err_flag) atomicOr(err_flag, flag);
}

// d_item[X[r]] += d_emb[r], d_item[pos_items[r]] += dpos[r] h[r], d_item[neg_items[r]] += dneg[r] h[r].  The rows
// repeat within a step (id 0 at every padded position), and the sums are taken in a fixed order, without atomics,
// over the 3 R lookups sorted by id (sorted_ids / order from a stable sort of X | pos_items | neg_items: order[k] =
// s R + r is lookup r of source s):
//   partials   a wave per kItemChunk sorted lookups walks them in order and stores the running sum of each run of
//              equal ids at the run's last lookup inside the chunk (partial [3 R][E], written at those places only);
//   combine    a wave per item finds its lookups [lo, hi) by bisection and adds the partials of the chunks they
//              span, first to last.
constexpr int kItemChunk = 256;

__global__ __launch_bounds__(kBlock) void s3rec_item_partials_kernel(const int64_t* __restrict__ sorted_ids,
                                                                     const int64_t* __restrict__ order,
                                                                     const float* __restrict__ d_emb,
                                                                     const float* __restrict__ h,
                                                                     const float* __restrict__ dpos,
                                                                     const float* __restrict__ dneg, int64_t rows, int E,
                                                                     int64_t num_items, float* __restrict__ partial,
                                                                     int32_t* err_flag) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t n = 3 * rows, chunks = (n + kItemChunk - 1) / kItemChunk;
  const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  int flag = 0;
  for (int64_t c = wave0; c < chunks; c += (int64_t)gridDim.x * kWavesPerBlock) {
    const int64_t k1 = min(n, (c + 1) * kItemChunk);
    float acc[2] = {0.0f, 0.0f};
    for (int64_t k = c * kItemChunk; k < k1; ++k) {
      const int64_t id = sorted_ids[k], at = order[k];
      const int src = (int)(at / rows);
      const int64_t row = at - src * rows;
      const float coeff = src == 0 ? 1.0f : src == 1 ? dpos[row] : dneg[row];
      const float* v = (src == 0 ? d_emb : h) + row * E;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int e = lane + kWave * t;
        if (e < E) acc[t] += src == 0 ? v[e] : coeff * v[e];
      }
      if (id < 0 || id > num_items) flag = YR_FLAG_BAD_ITEM;
      if (k + 1 == k1 || sorted_ids[k + 1] != id) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int e = lane + kWave * t;
          if (e < E) partial[k * E + e] = acc[t];
          acc[t] = 0.0f;
        }
      }
    }
  }
  if (flag && err_flag) atomicOr(err_flag, flag);
}

// first k in [0, n) with sorted_ids[k] >= id
__device__ __forceinline__ int64_t s3_lower_bound(const int64_t* __restrict__ sorted_ids, int64_t n, int64_t id) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (sorted_ids[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kBlock) void s3rec_item_combine_kernel(const int64_t* __restrict__ sorted_ids, int64_t n,
                                                                    const float* __restrict__ partial, int E,
                                                                    int64_t num_items, float* __restrict__ d_item) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  for (int64_t id = wave0; id <= num_items; id += (int64_t)gridDim.x * kWavesPerBlock) {
    const int64_t lo = s3_lower_bound(sorted_ids, n, id), hi = s3_lower_bound(sorted_ids, n, id + 1);
    if (lo == hi) continue;
    float acc[2] = {0.0f, 0.0f};
    for (int64_t c = lo / kItemChunk; c <= (hi - 1) / kItemChunk; ++c) {
      const int64_t last = min(hi, (c + 1) * kItemChunk) - 1;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int e = lane + kWave * t;
        if (e < E) acc[t] += partial[last * E + e];
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int e = lane + kWave * t;
      if (e < E) d_item[id * E + e] += acc[t];
    }
  }
}

}  // namespace yr

using namespace yr;

static bool s3rec_width_ok(int E) { return E == 16 || E == 32 || E == 64 || E == 128; }

// BADARG for a dimension that cannot be, UNSUPPORTED for one past what the per-sequence kernels are built for
static int s3rec_shape_status(int64_t B, int L, int E, int heads, int blocks) {
  if (B < 0 || L <= 0 || E <= 0 || heads <= 0 || blocks <= 0) return YR_ERR_BADARG;
  if (!s3rec_width_ok(E) || L > kS3MaxL || heads > kS3MaxHeads || blocks > kS3MaxBlocks) return YR_ERR_UNSUPPORTED;
  return 0;
}

// One of the three per-sequence kernels: the dynamic-LDS raise once per kernel, the launch, its status
template <auto KERNEL>
static int s3rec_launch(const S3Train& p, size_t lds, int grid, void* stream) {
  static bool raised = false;                        // per kernel: this function has one instantiation for each
  if (!raised && lds > 65536) {                      // more than the default 64 KB of dynamic LDS: once per process
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256);
    if (e != hipSuccess) return (int)e;
    raised = true;
  }
  hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(kBlock), lds, (hipStream_t)stream, p);
  return launch_status();
}

// a workgroup per sequence, the kernel's own loop past 2^20 sequences
template <bool TRAIN>
static int s3rec_encode_launch(const S3Train& p, int E, void* stream) {
  const size_t lds = TRAIN ? s3rec_train_lds_bytes(E, p.enc.L) : s3rec_lds_bytes(E, p.enc.L);
  const int grid = (int)std::min<int64_t>(p.enc.B, 1 << 20);
  switch (E) {
    case 16: return s3rec_launch<&s3rec_encode_kernel<16, TRAIN>>(p, lds, grid, stream);
    case 32: return s3rec_launch<&s3rec_encode_kernel<32, TRAIN>>(p, lds, grid, stream);
    case 64: return s3rec_launch<&s3rec_encode_kernel<64, TRAIN>>(p, lds, grid, stream);
    default: return s3rec_launch<&s3rec_encode_kernel<128, TRAIN>>(p, lds, grid, stream);
  }
}

static int s3rec_backward_launch(const S3Train& p, int E, void* stream) {
  const size_t lds = s3rec_train_lds_bytes(E, p.enc.L);
  const int grid = (int)std::min<int64_t>(p.enc.B, 1 << 20);
  switch (E) {
    case 16: return s3rec_launch<&s3rec_backward_kernel<16>>(p, lds, grid, stream);
    case 32: return s3rec_launch<&s3rec_backward_kernel<32>>(p, lds, grid, stream);
    case 64: return s3rec_launch<&s3rec_backward_kernel<64>>(p, lds, grid, stream);
    default: return s3rec_launch<&s3rec_backward_kernel<128>>(p, lds, grid, stream);
  }
}

extern "C" int yr_s3rec_encode(const float* item_emb, const float* pos_enc, const float* params, const int64_t* X,
                               int64_t B, int L, int E, int heads, int blocks, int64_t num_items, int last_only,
                               float* out, int32_t* err_flag, void* stream) {
  if (num_items < 0) return YR_ERR_BADARG;
  if (const int s = s3rec_shape_status(B, L, E, heads, blocks)) return s;
  if (B == 0) return 0;
  if (!item_emb || !pos_enc || !params || !X || !out) return YR_ERR_BADARG;
  if ((reinterpret_cast<uintptr_t>(params) & 15) != 0) return YR_ERR_BADARG;
  const S3Train t{S3Enc{item_emb, pos_enc, params, X, B, num_items, L, heads, blocks, last_only != 0, out, err_flag},
                  nullptr, nullptr, 0, 0.0f, 1.0f};
  return s3rec_encode_launch<false>(t, E, stream);
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

extern "C" int64_t yr_s3rec_train_workspace_floats(int64_t B, int L, int E, int heads, int blocks) {
  if (const int s = s3rec_shape_status(B, L, E, heads, blocks)) return s;
  return blocks * s3_layout(B * L, E, heads).block;
}

static int s3rec_train_args(int64_t B, int L, int E, int heads, int blocks, double p, int64_t workspace_floats) {
  if (!(p >= 0.0 && p < 1.0)) return YR_ERR_BADARG;
  if (const int s = s3rec_shape_status(B, L, E, heads, blocks)) return s;
  if (B > 0 && workspace_floats < blocks * s3_layout(B * L, E, heads).block) return YR_ERR_BADARG;
  return 0;
}

extern "C" int yr_s3rec_encode_train(const float* item_emb, const float* pos_enc, const float* params,
                                     const int64_t* X, int64_t B, int L, int E, int heads, int blocks,
                                     int64_t num_items, uint64_t seed, double p, float* out, float* workspace,
                                     int64_t workspace_floats, int32_t* err_flag, void* stream) {
  if (num_items < 0) return YR_ERR_BADARG;
  if (const int s = s3rec_train_args(B, L, E, heads, blocks, p, workspace_floats)) return s;
  if (B == 0) return 0;
  if (!item_emb || !pos_enc || !params || !X || !out || !workspace) return YR_ERR_BADARG;
  if (((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(workspace)) & 15) != 0) return YR_ERR_BADARG;
  const S3Train t{S3Enc{item_emb, pos_enc, params, X, B, num_items, L, heads, blocks, 0, out, err_flag}, workspace,
                  nullptr, seed, (float)p, (float)(1.0 / (1.0 - p))};
  return s3rec_encode_launch<true>(t, E, stream);
}

extern "C" int yr_s3rec_backward(const float* params, const int64_t* X, const float* dh_out, int64_t B, int L, int E,
                                 int heads, int blocks, uint64_t seed, double p, float* workspace,
                                 int64_t workspace_floats, float* d_emb, void* stream) {
  if (const int s = s3rec_train_args(B, L, E, heads, blocks, p, workspace_floats)) return s;
  if (B == 0) return 0;
  if (!params || !X || !dh_out || !workspace || !d_emb) return YR_ERR_BADARG;
  if (((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(workspace)) & 15) != 0) return YR_ERR_BADARG;
  const S3Train t{S3Enc{nullptr, nullptr, params, X, B, 0, L, heads, blocks, 0, d_emb, nullptr}, workspace, dh_out, seed,
                  (float)p, (float)(1.0 / (1.0 - p))};
  return s3rec_backward_launch(t, E, stream);
}

extern "C" int yr_s3rec_score_grad(const float* item_emb, const int64_t* pos_items, const int64_t* neg_items,
                                   const float* dpos_preds, const float* dneg_preds, int64_t rows, int E,
                                   int64_t num_items, float* dh_out, int32_t* err_flag, void* stream) {
  if (rows < 0 || E <= 0 || num_items < 0) return YR_ERR_BADARG;
  if (!s3rec_width_ok(E)) return YR_ERR_UNSUPPORTED;
  if (rows == 0) return 0;
  if (!item_emb || !pos_items || !neg_items || !dpos_preds || !dneg_preds || !dh_out) return YR_ERR_BADARG;
  hipLaunchKernelGGL(s3rec_score_grad_kernel, dim3(grid_for(rows * E, kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                     item_emb, pos_items, neg_items, dpos_preds, dneg_preds, rows, E, num_items, dh_out, err_flag);
  return launch_status();
}

extern "C" int yr_s3rec_item_grad(const int64_t* sorted_ids, const int64_t* order, const float* d_emb, const float* h,
                                  const float* dpos_preds, const float* dneg_preds, int64_t rows, int E,
                                  int64_t num_items, float* partial, float* d_item, int32_t* err_flag, void* stream) {
  if (rows < 0 || E <= 0 || num_items < 0) return YR_ERR_BADARG;
  if (!s3rec_width_ok(E)) return YR_ERR_UNSUPPORTED;
  if (rows == 0) return 0;
  if (!sorted_ids || !order || !d_emb || !h || !dpos_preds || !dneg_preds || !partial || !d_item) return YR_ERR_BADARG;
  const int64_t chunks = (3 * rows + kItemChunk - 1) / kItemChunk;
  hipLaunchKernelGGL(s3rec_item_partials_kernel, dim3(grid_for(chunks, kWavesPerBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, sorted_ids, order, d_emb, h, dpos_preds, dneg_preds, rows, E, num_items,
                     partial, err_flag);
  if (const int s = launch_status()) return s;
  hipLaunchKernelGGL(s3rec_item_combine_kernel, dim3(grid_for(num_items + 1, kWavesPerBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, sorted_ids, 3 * rows, partial, E, num_items, d_item);
  return launch_status();
}
