// DCN (deep & cross network) kernels for gfx950 (MI355X).
//
// Replaces, for reference models/dcn.py:41-62 and trainers/dcn_trainer.py:102-165 (+ their autograd):
//   * the input assembly  x0 = [user_emb | item_emb | mean_c cat_emb[c] | statecity_emb]  (four nn.Embedding
//     lookups, a mean over the padded category list, torch.cat) and its scatter-add backward;
//   * the head: the cross network, the output layer, the sigmoid and BPRLoss (forward and backward) in one
//     kernel over the rows — the cross network in closed form (below);
//   * the full-catalogue scorer of evaluation: every (user, item) pair through the deep tower on the matrix
//     cores without materialising the pair rows.
// The deep tower of a training step is yr_gemm_f32 (act = 2: ReLU) plus yr_relu_bwd.
//
// Cross network in closed form.  x_{l+1} = x0 (x_l . w_l) + b_l + x_l keeps x_l = alpha_l x0 + beta_l with a scalar
// alpha_l per row and beta_l = sum_{j<l} b_j the same for every row:
//   s_l = x_l . w_l = alpha_l (x0 . w_l) + beta_l . w_l,   alpha_{l+1} = alpha_l + s_l,   alpha_0 = 1,
// so a row costs L + 1 dot products of length F instead of L outer products F x F.  Backward, with
// g_l = dLoss / dx_l (g_L = dz W_oc) and c_l = g_{l+1} . x0:
//   c_l = dz (W_oc . x0) + sum_{j>l} c_j (w_j . x0)        (scalars: one recursion)
//   g_l = g_{l+1} + c_l w_l,   dx0 = g_0 + sum_l s_l g_{l+1},   dw_l += c_l x_l,   db_l += g_{l+1}.
#include "common.h"
#include "dcn_parts.h"

namespace yr {

// The limits live in dcn_parts.h (shared with csrc/dcn_owned.hip): kDcnMaxF = 512 (4 * D, D <= 128), kDcnMaxH = 1024
// (width of the last hidden layer), kDcnMaxL = 8 (cross orders).
static_assert(kDcnMaxF == 512 && kDcnMaxH == 1024 && kDcnMaxL == 8, "the comment above states the limits");

// --------------------------------------------------------------------------- input assembly
// Row r of x (B rows, or 2B with item_b: rows [0, B) pair user[b] with item_a[b], rows [B, 2B) with item_b[b]):
//   [U[user] | I[item] | sum_j C[cat_ids[a, j]] / Lmax | S[sc_ids[a]]]   (no user segment when user == NULL)
// a = item (attribute tables indexed by item) or r (attr_per_row: the caller's own per-row lists).
// item_a == NULL: item = r (the item-only form of evaluation, x_item for every item).  Bad ids set the flag and
// leave zeros in their segment.
struct DcnIds {
  const int32_t* cat_ids;
  const int32_t* sc_ids;
  int Lmax;
  int D;
  int64_t num_users, num_items, num_cats, num_sc;
  const int64_t* user;
  const int64_t* item_a;
  const int64_t* item_b;
  int64_t B;
  int attr_per_row;
};

__device__ __forceinline__ void dcn_row_ids(const DcnIds& a, int64_t r, int64_t& u, int64_t& it, int64_t& ar,
                                            bool& ok_u, bool& ok_i) {
  const int64_t b = r < a.B ? r : r - a.B;
  it = a.item_a ? (r < a.B ? a.item_a[b] : a.item_b[b]) : r;
  u = a.user ? a.user[b] : 0;
  ok_u = a.user == nullptr || (u >= 0 && u < a.num_users);
  ok_i = it >= 0 && it < a.num_items;
  ar = a.attr_per_row ? r : it;
}

__global__ __launch_bounds__(kBlock) void dcn_assemble_kernel(const float* __restrict__ U, const float* __restrict__ I,
                                                              const float* __restrict__ C, const float* __restrict__ S,
                                                              DcnIds a, int64_t rows, float* __restrict__ x,
                                                              int64_t ldx, int32_t* __restrict__ err_flag) {
  const int D = a.D;
  int flag = 0;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < rows * D; e += (int64_t)gridDim.x * kBlock) {
    const int64_t r = e / D;
    const int d = (int)(e - r * D);
    int64_t u, it, ar;
    bool ok_u, ok_i;
    dcn_row_ids(a, r, u, it, ar, ok_u, ok_i);
    float* out = x + r * ldx;
    int off = 0;
    if (a.user) {
      out[d] = ok_u ? U[u * D + d] : 0.0f;
      if (!ok_u) flag |= YR_FLAG_BAD_USER;
      off = D;
    }
    if (!ok_i) flag |= YR_FLAG_BAD_ITEM;
    const bool ok_a = ok_i || a.attr_per_row;
    out[off + d] = ok_i ? I[it * D + d] : 0.0f;
    float s = 0.0f;
    if (ok_a) {
      for (int j = 0; j < a.Lmax; ++j) {
        const int64_t c = a.cat_ids[ar * a.Lmax + j];
        if (c >= 0 && c < a.num_cats) s += C[c * D + d]; else flag |= YR_FLAG_BAD_ITEM;
      }
    }
    out[off + D + d] = s / (float)a.Lmax;
    float t = 0.0f;
    if (ok_a) {
      const int64_t c = a.sc_ids[ar];
      if (c >= 0 && c < a.num_sc) t = S[c * D + d]; else flag |= YR_FLAG_BAD_ITEM;
    }
    out[off + 2 * D + d] = t;
  }
  if (flag && err_flag) atomicOr(err_flag, flag);
}

// embedding_dense_backward of the four lookups (the mean hands dx / Lmax to every slot, padding included)
__global__ __launch_bounds__(kBlock) void dcn_assemble_bwd_kernel(const float* __restrict__ dx, int64_t ldx, DcnIds a,
                                                                  int64_t rows, float* __restrict__ gU,
                                                                  float* __restrict__ gI, float* __restrict__ gC,
                                                                  float* __restrict__ gS, int32_t* __restrict__ err_flag) {
  const int D = a.D;
  int flag = 0;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < rows * D; e += (int64_t)gridDim.x * kBlock) {
    const int64_t r = e / D;
    const int d = (int)(e - r * D);
    int64_t u, it, ar;
    bool ok_u, ok_i;
    dcn_row_ids(a, r, u, it, ar, ok_u, ok_i);
    const float* g = dx + r * ldx;
    int off = 0;
    if (a.user) {
      if (ok_u) atomicAdd(gU + u * D + d, g[d]); else flag |= YR_FLAG_BAD_USER;
      off = D;
    }
    if (ok_i) atomicAdd(gI + it * D + d, g[off + d]); else flag |= YR_FLAG_BAD_ITEM;
    if (ok_i || a.attr_per_row) {
      const float gc = g[off + D + d] / (float)a.Lmax;
      for (int j = 0; j < a.Lmax; ++j) {
        const int64_t c = a.cat_ids[ar * a.Lmax + j];
        if (c >= 0 && c < a.num_cats) atomicAdd(gC + c * D + d, gc); else flag |= YR_FLAG_BAD_ITEM;
      }
      const int64_t c = a.sc_ids[ar];
      if (c >= 0 && c < a.num_sc) atomicAdd(gS + c * D + d, g[off + 2 * D + d]); else flag |= YR_FLAG_BAD_ITEM;
    }
  }
  if (flag && err_flag) atomicOr(err_flag, flag);
}

__global__ __launch_bounds__(kBlock) void relu_bwd_kernel(float* __restrict__ g, const float* __restrict__ y, int64_t n) {
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n; e += (int64_t)gridDim.x * kBlock)
    if (!(y[e] > 0.0f)) g[e] = 0.0f;
}

// --------------------------------------------------------------------------- fused head (row loop: dcn_head_rows.h)
__global__ __launch_bounds__(kBlock) void dcn_head_kernel(DcnHead p) {
  __shared__ float sAcc[kHeadAcc];             // [dcw: L*F | dcb: L*F | dWo: H + F | dbo]
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int F = p.F, H = p.H, L = p.L;
  const bool grads = p.dx0 != nullptr;
  const int oDcb = L * F, oWo = 2 * L * F, oBo = 2 * L * F + H + F;
  if (grads)
    for (int e = threadIdx.x; e <= oBo; e += kBlock) sAcc[e] = 0.0f;
  // terms into the workgroup's one accumulator, shared by its four waves: LDS float atomics (arrival order)
#define DCN_HEAD_TERM(e, v) atomicAdd(&sAcc[e], v)
#include "dcn_head_rows.h"
#undef DCN_HEAD_TERM
  if (!grads) return;
  __syncthreads();
  for (int e = threadIdx.x; e <= oBo; e += kBlock) {
    const float v = sAcc[e];
    if (v == 0.0f) continue;
    float* dst = e < oDcb ? p.dcw + e : e < oWo ? p.dcb + (e - oDcb) : e < oBo ? p.dWo + (e - oWo) : p.dbo;
    atomicAdd(dst, v);
  }
}

// --------------------------------------------------------------------------- fused full-catalogue scorer
// score(u, i) = sigmoid(deep(u, i) + alpha_L q + boc) for 8 users x 32 items per workgroup, where
//   h1 = relu(Au[u] + Bi[i])                                  (the first layer split over the concatenation)
//   deep = sum_n W_od[n] relu((W2 h1)[n] + b2[n])             (two hidden layers: W2 h1 on the matrix cores)
//   deep = sum_k W_od[k] h1[k]                                (one hidden layer: VALU)
//   p_l = Pu[u, l] + Pi[i, l], q = Pu[u, L] + Pi[i, L]        (x0 . w_l and x0 . W_oc split the same way)
// Two layers: the 256 pairs are the columns of 32 x 32 MFMA tiles (lane i = item), H2 is walked in slices of 128
// rows and H1 (= K) in chunks of 32 staged in LDS: W2 as [n][k] and Bi as [item][k] with pitch 33 (conflict-free
// row-of-k reads), Au as [user][k] with pitch 32 (its reads are wave-wide broadcasts).  Wave w owns the pairs of users 2w, 2w + 1 and all 128 rows of the slice (4 x 2 tiles): it
// builds h1 for each (pair, k) once per slice as the MFMA's B operand and reads W2 as the A operand; the epilogue
// of a slice folds relu(acc + b2) W_od into one partial per lane and pair tile.  The next chunk is fetched into
// registers while the MFMAs of the current one run.
constexpr int kSU = 8, kSI = 32, kSK = 32, kSN = 128, kSP = kSK + 1;

struct DcnScore {
  const float* Au;
  int64_t ldau;
  const float* Bi;
  int64_t ldbi;
  const float* Pu;
  const float* Pi;
  const int64_t* users;
  int64_t n_eval, num_users, num_items;
  int H1, H2;
  const float *W2, *b2, *Wo, *bo, *cw, *cb;
  int L, F;
  float* scores;
  int64_t row_stride;
  int32_t* err_flag;
};

template <bool TWO>
__global__ __launch_bounds__(kBlock) void dcn_score_kernel(DcnScore p) {
  __shared__ float sW[TWO ? kSN * kSP : 1];
  __shared__ float sB[kSI * kSP];
  __shared__ float sA[kSU * kSK];
  __shared__ float sWod[kDcnMaxH];
  __shared__ float sb2[kDcnMaxH];
  __shared__ int64_t sUser[kSU];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int i = lane & 31, hh = lane >> 5;
  const int64_t it0 = (int64_t)blockIdx.x * kSI, ug0 = (int64_t)blockIdx.y * kSU;
  const int Hd = TWO ? p.H2 : p.H1;                    // width that W_od covers
  const int Hpad = TWO ? (p.H2 + kSN - 1) / kSN * kSN : p.H1;
  for (int e = tid; e < Hpad; e += kBlock) {
    sWod[e] = e < Hd ? p.Wo[e] : 0.0f;
    if (TWO) sb2[e] = e < Hd ? p.b2[e] : 0.0f;
  }
  if (tid < kSU) {
    int64_t row = -1;
    if (ug0 + tid < p.n_eval) {
      const int64_t uid = p.users[ug0 + tid];
      if (uid >= 0 && uid < p.num_users) row = uid;
      else if (p.err_flag) atomicOr(p.err_flag, YR_FLAG_BAD_USER);
    }
    sUser[tid] = row;
  }
  float bw[kDcnMaxL], boc, betaL[kDcnEF];
  dcn_cross_consts(p.cw, p.cb, p.Wo + Hd, p.bo, p.L, p.F, lane, bw, boc, betaL);
  __syncthreads();

  // this thread's pieces of a chunk: 4 float4 of W2 (n = idx / 8, k = 4 (idx % 8)), one float4 of Bi, one Au value
  const int fB_item = tid >> 3, fB_k = (tid & 7) * 4;
  const int fA_u = tid >> 5, fA_k = tid & 31;
  const int64_t aRow = sUser[fA_u];
  const int64_t bItem = it0 + fB_item;
  float4 rW[TWO ? 4 : 1], rB;
  float rA;
  auto fetch = [&](int n0, int k0) {
    if (TWO) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int idx = tid + kBlock * j;
        const int n = n0 + (idx >> 3);
        rW[j] = n < p.H2 ? *reinterpret_cast<const float4*>(p.W2 + (int64_t)n * p.H1 + k0 + (idx & 7) * 4)
                         : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    rB = bItem < p.num_items ? *reinterpret_cast<const float4*>(p.Bi + bItem * p.ldbi + k0 + fB_k)
                             : make_float4(0.f, 0.f, 0.f, 0.f);
    rA = aRow >= 0 ? p.Au[aRow * p.ldau + k0 + fA_k] : 0.0f;
  };
  auto stash = [&]() {
    if (TWO) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int idx = tid + kBlock * j;
        float* d = sW + (idx >> 3) * kSP + (idx & 7) * 4;
        d[0] = rW[j].x; d[1] = rW[j].y; d[2] = rW[j].z; d[3] = rW[j].w;
      }
    }
    float* d = sB + fB_item * kSP + fB_k;
    d[0] = rB.x; d[1] = rB.y; d[2] = rB.z; d[3] = rB.w;
    sA[fA_u * kSK + fA_k] = rA;
  };

  const int nchunks = p.H1 / kSK;
  const int nslices = TWO ? Hpad / kSN : 1;
  const int steps = nchunks * nslices;
  float part[2] = {0.0f, 0.0f};
  f32x16 acc[4][2];
  fetch(0, 0);
  for (int t = 0; t < steps; ++t) {
    const int slice = t / nchunks, chunk = t - slice * nchunks;
    __syncthreads();                                    // everyone is done with the previous chunk
    stash();
    __syncthreads();
    if (t + 1 < steps) {
      const int s2 = (t + 1) / nchunks;
      fetch(s2 * kSN, ((t + 1) - s2 * nchunks) * kSK);
    }
    if (TWO) {
      if (chunk == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[r][c][q] = 0.0f;
      }
#pragma unroll
      for (int s = 0; s < kSK / 2; ++s) {
        const int kk = hh * (kSK / 2) + s;
        const float bi = sB[i * kSP + kk];
        const float h0 = fmaxf(sA[(2 * wave) * kSK + kk] + bi, 0.0f);
        const float h1 = fmaxf(sA[(2 * wave + 1) * kSK + kk] + bi, 0.0f);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float a = sW[(32 * r + i) * kSP + kk];
          acc[r][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, h0, acc[r][0], 0, 0, 0);
          acc[r][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, h1, acc[r][1], 0, 0, 0);
        }
      }
      if (chunk == nchunks - 1) {
        const int n0 = slice * kSN;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int n = n0 + 32 * r + (q & 3) + 8 * (q >> 2) + 4 * hh;
            const float wo = sWod[n], bb = sb2[n];
            part[0] += wo * fmaxf(acc[r][0][q] + bb, 0.0f);
            part[1] += wo * fmaxf(acc[r][1][q] + bb, 0.0f);
          }
      }
    } else {
      // one hidden layer: thread (user tid / 32, item tid % 32) sums its pair over the chunk
      const int k0 = chunk * kSK;
      const int uu = tid >> 5, ii = tid & 31;
#pragma unroll
      for (int k = 0; k < kSK; ++k)
        part[0] += sWod[k0 + k] * fmaxf(sA[uu * kSK + k] + sB[ii * kSP + k], 0.0f);
    }
  }

  // pairs of this thread: two layers -> lanes hh == 0 hold (user 2w + c, item i); one layer -> (tid / 32, tid % 32)
  const int L = p.L;
  const int ldp = L + 1;
#pragma unroll
  for (int c = 0; c < (TWO ? 2 : 1); ++c) {
    float deep = part[c];
    int uu, ii;
    if (TWO) {
      deep += __shfl_xor(deep, 32, kWave);
      uu = 2 * wave + c;
      ii = i;
      if (hh) continue;
    } else {
      uu = tid >> 5;
      ii = tid & 31;
    }
    const int64_t urow = sUser[uu];
    const int64_t item = it0 + ii;
    if (ug0 + uu >= p.n_eval || item >= p.num_items) continue;
    float z = 0.0f;
    if (urow >= 0) {
      const float* pu = p.Pu + urow * ldp;
      const float* pi = p.Pi + item * ldp;
      float alpha = 1.0f;
#pragma unroll
      for (int l = 0; l < kDcnMaxL; ++l)
        if (l < L) alpha += alpha * (pu[l] + pi[l]) + bw[l];
      z = deep + alpha * (pu[L] + pi[L]) + boc;
    }
    p.scores[(ug0 + uu) * p.row_stride + item] = sigmoidf(z);
  }
}

}  // namespace yr

using namespace yr;

static bool dcn_ids(DcnIds& a, const int32_t* cat_ids, const int32_t* sc_ids, int Lmax, int D, int64_t num_users,
                    int64_t num_items, int64_t num_cats, int64_t num_sc, const int64_t* user, const int64_t* item_a,
                    const int64_t* item_b, int64_t B, int attr_per_row) {
  if (!cat_ids || !sc_ids || Lmax <= 0 || D <= 0 || B < 0 || num_items <= 0 || num_cats <= 0 || num_sc <= 0)
    return false;
  if (user && num_users <= 0) return false;
  if (item_b && (!item_a || !user)) return false;
  a = DcnIds{cat_ids, sc_ids, Lmax, D, num_users, num_items, num_cats, num_sc, user, item_a, item_b, B,
             attr_per_row};
  return true;
}

extern "C" int yr_dcn_assemble(const float* U, const float* I, const float* C, const float* S, const int32_t* cat_ids,
                               const int32_t* sc_ids, int Lmax, int D, int64_t num_users, int64_t num_items,
                               int64_t num_cats, int64_t num_sc, const int64_t* user, const int64_t* item_a,
                               const int64_t* item_b, int64_t B, int attr_per_row, float* x, int64_t ldx,
                               int32_t* err_flag, void* stream) {
  DcnIds a;
  if (!dcn_ids(a, cat_ids, sc_ids, Lmax, D, num_users, num_items, num_cats, num_sc, user, item_a, item_b, B,
               attr_per_row))
    return YR_ERR_BADARG;
  if (!I || !C || !S || !x || (user && !U) || ldx < (user ? 4 : 3) * D) return YR_ERR_BADARG;
  const int64_t rows = item_b ? 2 * B : B;
  if (rows == 0) return 0;
  hipLaunchKernelGGL(dcn_assemble_kernel, dim3(grid_for(rows * D, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, U,
                     I, C, S, a, rows, x, ldx, err_flag);
  return launch_status();
}

extern "C" int yr_dcn_assemble_bwd(const float* dx, int64_t ldx, const int32_t* cat_ids, const int32_t* sc_ids,
                                   int Lmax, int D, int64_t num_users, int64_t num_items, int64_t num_cats,
                                   int64_t num_sc, const int64_t* user, const int64_t* item_a, const int64_t* item_b,
                                   int64_t B, int attr_per_row, float* gU, float* gI, float* gC, float* gS,
                                   int32_t* err_flag, void* stream) {
  DcnIds a;
  if (!dcn_ids(a, cat_ids, sc_ids, Lmax, D, num_users, num_items, num_cats, num_sc, user, item_a, item_b, B,
               attr_per_row))
    return YR_ERR_BADARG;
  if (!dx || !gI || !gC || !gS || (user && !gU) || ldx < (user ? 4 : 3) * D) return YR_ERR_BADARG;
  const int64_t rows = item_b ? 2 * B : B;
  if (rows == 0) return 0;
  hipLaunchKernelGGL(dcn_assemble_bwd_kernel, dim3(grid_for(rows * D, kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, dx, ldx, a, rows, gU, gI, gC, gS, err_flag);
  return launch_status();
}

extern "C" int yr_relu_bwd(float* g, const float* y, int64_t n, void* stream) {
  if (n < 0 || (n > 0 && (!g || !y))) return YR_ERR_BADARG;
  if (n == 0) return 0;
  hipLaunchKernelGGL(relu_bwd_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, g, y, n);
  return launch_status();
}

extern "C" int yr_dcn_head(const float* x0, int64_t ldx, const float* h, int64_t ldh, int64_t units, int F, int H,
                           int L, const float* cw, const float* cb, const float* Wo, const float* bo, int bpr,
                           float inv_batch, float* pred, const float* gpred, float* dh, int64_t lddh, float* dx0,
                           int64_t lddx, float* dcw, float* dcb, float* dWo, float* dbo, float* loss_partials,
                           void* stream) {
  if (units < 0 || F <= 0 || H <= 0 || L <= 0) return YR_ERR_BADARG;
  if (F > kDcnMaxF || H > kDcnMaxH || L > kDcnMaxL) return YR_ERR_UNSUPPORTED;
  if (!x0 || !h || !cw || !cb || !Wo || !bo || ldx < F || ldh < H) return YR_ERR_BADARG;
  if (bpr && !loss_partials) return YR_ERR_BADARG;
  if (dx0 && (!dh || !dcw || !dcb || !dWo || !dbo || lddh < H || lddx < F || (!bpr && !gpred))) return YR_ERR_BADARG;
  const int grid = (int)std::min<int64_t>(std::max<int64_t>((units + kWavesPerBlock - 1) / kWavesPerBlock, 1), 256);
  DcnHead p{x0, ldx, h, ldh, units, F, H, L, cw, cb, Wo, bo, bpr, inv_batch, pred, gpred, dh, lddh, dx0, lddx,
            dcw, dcb, dWo, dbo, loss_partials};
  hipLaunchKernelGGL(dcn_head_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, p);
  return launch_status();
}

extern "C" int yr_dcn_score(const float* Au, int64_t ldau, const float* Bi, int64_t ldbi, const float* Pu,
                            const float* Pi, const int64_t* users, int64_t n_eval, int64_t num_users,
                            int64_t num_items, int H1, int H2, const float* W2, const float* b2, const float* Wo,
                            const float* bo, const float* cw, const float* cb, int L, int F, float* scores,
                            int64_t row_stride, int32_t* err_flag, void* stream) {
  if (n_eval < 0 || num_users <= 0 || num_items <= 0 || L <= 0 || F <= 0) return YR_ERR_BADARG;
  const bool two = W2 != nullptr;
  if (H1 <= 0 || H1 % 32 || H1 > kDcnMaxH || (two && (H2 <= 0 || H2 % 32 || H2 > kDcnMaxH))) return YR_ERR_UNSUPPORTED;
  if (L > kDcnMaxL || F > kDcnMaxF) return YR_ERR_UNSUPPORTED;
  if (!Au || !Bi || !Pu || !Pi || !users || !Wo || !bo || !cw || !cb || !scores || (two && !b2)) return YR_ERR_BADARG;
  if (ldau < H1 || ldbi < H1 || ldbi % 4 || row_stride < num_items) return YR_ERR_BADARG;
  if (((reinterpret_cast<uintptr_t>(Bi) | reinterpret_cast<uintptr_t>(W2)) & 15) != 0) return YR_ERR_BADARG;
  if (n_eval == 0) return 0;
  const int64_t gy = (n_eval + kSU - 1) / kSU;
  if (gy > 65535) return YR_ERR_BADARG;
  const dim3 grid((unsigned)((num_items + kSI - 1) / kSI), (unsigned)gy);
  DcnScore p{Au, ldau, Bi, ldbi, Pu, Pi, users, n_eval, num_users, num_items, H1, two ? H2 : 0, W2, b2, Wo, bo,
             cw, cb, L, F, scores, row_stride, err_flag};
  if (two)
    hipLaunchKernelGGL(dcn_score_kernel<true>, grid, dim3(kBlock), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(dcn_score_kernel<false>, grid, dim3(kBlock), 0, (hipStream_t)stream, p);
  return launch_status();
}
