// S3Rec full-catalogue evaluation for gfx950 (MI355X): the rank of one held-out item per sequence among ALL columns
// of the item table — what reference trainers/s3rec_trainer.py:264-283 measures over 1 + 99 sampled candidates, taken
// over the whole catalogue instead, so that HR@k, NDCG@k and MRR of a leave-one-out split are exact and comparable
// with the other models' full-catalogue figures.
//
//   s[n, r]  = <H[n], T[r]>                                    (f32, v_mfma_f32_32x32x2_f32, k ascending)
//   rank[n]  = #{ r in [first_col, R) : r != target[n], r not excluded for n,
//                 s[n, r] > s[n, target[n]]  or  (s[n, r] == s[n, target[n]] and r < target[n]) }
//
// the 0-based place of the target in the project's list order (score descending, id ascending among equal scores).
// The geometry is s3rec_cbce_kernel<E, true>'s (csrc/s3rec_pretrain.hip): a wave OWNS 32 rows of H in registers as
// the B operand and SWEEPS 32-row tiles of T read 16 bytes per lane from global memory; a workgroup is (row tile,
// chunk of kSweepColChunk columns) and its four waves take kSweepTilesPerWave tiles each.  No [N][R] array exists.
// One arithmetic: the target's score comes from rank_tile() too — a first "diagonal" tile whose swept row in lane r is
// T[target of owned row r] — so a column whose row of T is bit-identical to the target's ties exactly and the id
// decides.  Counts are integers: lanes by a shuffle, waves by an LDS integer add, chunks by per-chunk partials in the
// workspace that s3rec_rank_sum_kernel adds up; every sum is exact, so a row's rank does not depend on N, on its place
// in the batch or on the other rows.
#include <algorithm>

#include "s3rec_cb.h"

namespace yr {

struct Rank {
  const float* H;             // [N][E]
  const float* T;             // [R][E]
  const int64_t* target;      // [N]
  const int64_t *excl_ptr, *excl_idx, *excl_rows;   // CSR over K rows (or null), the CSR row of each n (or null: n)
  int64_t N, R, K, first_col, chunks;
  int32_t* part;              // [chunks][N]
  float* target_score;        // [N] or null
  int32_t* err_flag;
};

// rank_tile(), rank_own(), rank_diagonal() and low_bits(): s3rec_cb.h, shared with csrc/catalogue_rank.hip
template <int E>
__global__ __launch_bounds__(kBlock, E <= 64 ? 2 : 1) void s3rec_rank_kernel(Rank p) {
  __shared__ int32_t sC[kSweepTile];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int r = lane & 31, hh = lane >> 5;
  const int64_t row_tiles = (p.N + kSweepTile - 1) / kSweepTile, units = row_tiles * p.chunks;
  const int64_t col_tiles = (p.R + kSweepTile - 1) / kSweepTile;
  int flag = 0;

  for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int64_t ot = unit / p.chunks, chunk = unit - ot * p.chunks;
    const int64_t j0 = ot * kSweepTile, j = j0 + r;      // the lane's owned row
    const bool own_ok = j < p.N;
    if (tid < kSweepTile) sC[tid] = 0;

    // the owned rows, k = 8 c + 4 hh + t at own[4 c + t]: the order of the swept rows' 16-byte loads
    float own[E / 2];
    rank_own<E>(own, p.H + j * E + 4 * hh, own_ok);

    const int64_t t_begin = chunk * (kSweepColChunk / kSweepTile) + (int64_t)wave * kSweepTilesPerWave;
    const int64_t t_end = std::min<int64_t>(t_begin + kSweepTilesPerWave, col_tiles);

    // the lane's target (-1: none) and the cursor over its exclude list
    int64_t tgt = -1, cur = 0, end = 0;
    if (own_ok) {
      const int64_t t = p.target[j];
      if (t < 0 || t >= p.R) flag |= YR_FLAG_BAD_ITEM;
      else if (t >= p.first_col) tgt = t;
      if (p.excl_ptr) {
        const int64_t e = p.excl_rows ? p.excl_rows[j] : j;
        if (e < 0 || e >= p.K) {
          flag |= YR_FLAG_BAD_USER;
        } else if (tgt >= 0) {
          end = p.excl_ptr[e + 1];
          cur = cb_lower_bound(p.excl_idx, p.excl_ptr[e], end, t_begin * kSweepTile);
        }
      }
    }

    // the diagonal tile: lane r sweeps T[target of owned row r] (rank_diagonal, s3rec_cb.h)
    const float ts = rank_diagonal(rank_tile<E>(p.T + (tgt >= 0 ? tgt : 0) * E + 4 * hh, tgt >= 0, own), lane);

    int32_t cnt = 0;
    for (int64_t t = t_begin; t < t_end; ++t) {
      const int64_t i0 = t * kSweepTile, i = i0 + r;     // the lane's swept row
      const bool swp_ok = i < p.R;
      const uint32_t excl = cb_mask(p.excl_idx, cur, end, i0);
      // the candidates of this tile for the lane's owned row, and the target's place relative to the tile
      const int trel = (int)std::min<int64_t>(std::max<int64_t>(tgt - i0, -1), kSweepTile);
      uint32_t cand = 0;
      if (tgt >= 0) {
        cand = low_bits((int)std::min<int64_t>(p.R - i0, kSweepTile)) &
               ~low_bits((int)std::min<int64_t>(std::max<int64_t>(p.first_col - i0, 0), kSweepTile)) & ~excl;
        if (trel >= 0 && trel < kSweepTile) cand &= ~(1u << trel);
      }

      const f32x16 acc = rank_tile<E>(p.T + (swp_ok ? i : 0) * E + 4 * hh, swp_ok, own);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int ri = cb_acc_row(q, lane);           // the swept row of this element inside the tile
        const float s = acc[q];
        const bool above = s > ts || (s == ts && ri < trel);
        cnt += (int32_t)(((cand >> ri) & 1u) != 0 && above);
      }
    }

    cnt += __shfl_xor(cnt, 32, kWave);
    __syncthreads();                                  // sC is zero
    if (hh == 0 && cnt) atomicAdd(&sC[r], cnt);
    if (chunk == 0 && wave == 0 && hh == 0 && own_ok && p.target_score) p.target_score[j] = tgt >= 0 ? ts : 0.0f;
    __syncthreads();
    if (tid < kSweepTile && j0 + tid < p.N) p.part[chunk * p.N + j0 + tid] = sC[tid];
    __syncthreads();                                  // the next unit clears sC
  }
  if (flag && p.err_flag) atomicOr(p.err_flag, flag);
}

// rank[n] = the chunks' counts, or -1 for a row without a target
__global__ __launch_bounds__(kBlock) void s3rec_rank_sum_kernel(const int32_t* __restrict__ part,
                                                                const int64_t* __restrict__ target, int64_t chunks,
                                                                int64_t N, int64_t R, int64_t first_col,
                                                                int64_t* __restrict__ rank) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t n = (int64_t)blockIdx.x * kBlock + threadIdx.x; n < N; n += stride) {
    const int64_t t = target[n];
    int64_t s = -1;
    if (t >= first_col && t < R) {
      s = 0;
      for (int64_t c = 0; c < chunks; ++c) s += part[c * N + n];
    }
    rank[n] = s;
  }
}

}  // namespace yr

using namespace yr;

static bool rank_width_ok(int E) { return E == 16 || E == 32 || E == 64 || E == 128; }   // s3rec_width_ok

static int64_t rank_chunks(int64_t R) { return (R + kSweepColChunk - 1) / kSweepColChunk; }

extern "C" int64_t yr_s3rec_catalogue_rank_workspace_bytes(int64_t N, int64_t R, int E) {
  if (N < 0 || R < 0 || E <= 0) return YR_ERR_BADARG;
  if (!rank_width_ok(E)) return YR_ERR_UNSUPPORTED;
  return N * rank_chunks(R) * (int64_t)sizeof(int32_t);
}

extern "C" int yr_s3rec_catalogue_rank(const float* H, const float* T, const int64_t* target, const int64_t* excl_ptr,
                                       const int64_t* excl_idx, const int64_t* excl_rows, int64_t N, int64_t R,
                                       int64_t K, int E, int64_t first_col, int64_t* rank, float* target_score,
                                       void* workspace, int64_t workspace_bytes, int32_t* err_flag, void* stream) {
  if (N < 0 || R < 0 || K < 0 || E <= 0 || workspace_bytes < 0 || first_col < 0 || first_col > 1) return YR_ERR_BADARG;
  if (!rank_width_ok(E)) return YR_ERR_UNSUPPORTED;
  if (N == 0 || R == 0) return 0;
  if (!H || !T || !target || !rank || !workspace) return YR_ERR_BADARG;
  if ((excl_ptr == nullptr) != (excl_idx == nullptr)) return YR_ERR_BADARG;
  if (((reinterpret_cast<uintptr_t>(H) | reinterpret_cast<uintptr_t>(T)) & 15) != 0) return YR_ERR_BADARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 3) != 0) return YR_ERR_BADARG;
  const int64_t chunks = rank_chunks(R);
  if (workspace_bytes < N * chunks * (int64_t)sizeof(int32_t)) return YR_ERR_BADARG;
  const Rank p{H, T, target, excl_ptr, excl_idx, excl_ptr ? excl_rows : nullptr, N, R, K, first_col, chunks,
               static_cast<int32_t*>(workspace), target_score, err_flag};
  hipStream_t st = (hipStream_t)stream;
  const int64_t units = (N + kSweepTile - 1) / kSweepTile * chunks;
  const dim3 grid((unsigned)std::min<int64_t>(units, kSweepGridMax)), block(kBlock);
  switch (E) {
    case 16: hipLaunchKernelGGL(s3rec_rank_kernel<16>, grid, block, 0, st, p); break;
    case 32: hipLaunchKernelGGL(s3rec_rank_kernel<32>, grid, block, 0, st, p); break;
    case 64: hipLaunchKernelGGL(s3rec_rank_kernel<64>, grid, block, 0, st, p); break;
    default: hipLaunchKernelGGL(s3rec_rank_kernel<128>, grid, block, 0, st, p); break;
  }
  if (const int s = launch_status()) return s;
  hipLaunchKernelGGL(s3rec_rank_sum_kernel, dim3(grid_for(N, kBlock)), dim3(kBlock), 0, st,
                     static_cast<const int32_t*>(workspace), target, chunks, N, R, first_col, rank);
  return launch_status();
}
