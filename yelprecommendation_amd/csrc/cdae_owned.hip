// Owner-pass gradients of a CDAE list-batch step for gfx950: the reproducible form of yr_cdae_sampled_decode and
// yr_cdae_hidden_bwd_dwh_t (csrc/cdae_sparse.hip) — reference trainers/cdae_trainer.py:36-54, whose runs repeat bit for
// bit under one seed.  Those two kernels add dW_o, db_o, dz (across the splits of a row), db_h, dV and dW_h^T with
// global float atomics, i.e. in arrival order.  Here every gradient element is summed by the one lane group that owns
// its destination, over the batch rows in ASCENDING order, and written once with a plain store:
//
//   rows -> columns   a counting sort of the batch's list entries by column: integer counts per column (atomic
//                     increments: order-free), one exclusive integer scan, and an integer cursor per column that hands
//                     every entry a slot of its column's segment.  WHICH slot depends on arrival, so the owner of a column
//                     walks its segment by ascending row (rows are distinct inside a column: a total order), never by
//                     slot.  Chosen over a [I][B / 32] bitmap because an entry carries its own scalar (the decoder's
//                     g, the encoder's input value) — nothing is fetched back from the row lists or computed twice —
//                     and because one column-owner kernel then serves both dW_o / db_o and dW_h^T.
//   row owners        cdae_owned_decode_kernel: the default decoder's geometry, loop order and loss partials; g goes
//                     into the column's segment instead of into float atomics, the dz partial of a split into a
//                     workspace row (summed in split order by cdae_owned_sum_splits_kernel).
//                     cdae_owned_hidden_rows_kernel: dz' = dz (/ count) act'(z) into the workspace, the row's input
//                     entries into their columns' segments, the marks and the step's loss.
//   column owners     cdae_owned_gather_kernel: out[c, :] = sum_r s(r, c) M[r, :] (and out_b[c] = sum_r s(r, c)) for
//                     every column with an entry; H / EPL = 16, 32 or 64 lanes per column, EPL floats per lane.
//   cdae_owned_hidden_sums_kernel   db_h: the rows in four contiguous quarters, each added serially in ascending order,
//                     the quarters in quarter order (a fixed shape for a given B); dV[u]: the first batch row of user
//                     u adds the rows of u in ascending order.
// The counters are cleared by the entry points themselves (one memset): the workspace may hold anything on entry.
#include <algorithm>
#include <climits>
#include "common.h"
#include "cdae_rows.h"
#include "owned_scan.h"

namespace yr {

// f(column, place in cols / vals) for every entry of row r: eight threads per sub-list
template <typename F>
__device__ __forceinline__ void for_row_entries(const int32_t* __restrict__ cols, const int32_t* __restrict__ count,
                                                int64_t cpp, int64_t r, F f) {
  constexpr int kTpp = kBlock / kListParts;
  const int q = threadIdx.x / kTpp;
  const int n = count[r * kListParts + q];
  const int64_t at0 = (r * kListParts + q) * cpp;
  for (int k = threadIdx.x % kTpp; k < n; k += kTpp) f(cols[at0 + k], at0 + k);
}

__global__ __launch_bounds__(kBlock) void cdae_owned_count_kernel(const int32_t* __restrict__ cols,
                                                                  const int32_t* __restrict__ count, int64_t cpp,
                                                                  int32_t* __restrict__ cnt) {
  for_row_entries(cols, count, cpp, blockIdx.x, [&](int32_t c, int64_t) { atomicAdd(cnt + c, 1); });
}

// (start[c] = entries of the columns before c, start[I] = all of them: owned_scan_kernel<false>, owned_scan.h)

// The decoder on the loss positions, a workgroup per (row, split): geometry, position order and loss sums of
// cdae_sampled_decode_kernel<LPP, EPL, EXACT, false>, so the loss partials and the count are the default kernel's.
// dz_part: [B][splits][H] — dz itself when splits == 1.
template <int LPP, int EPL, bool EXACT>
__global__ __launch_bounds__(kBlock) void cdae_owned_decode_kernel(
    const int32_t* __restrict__ lcols, const float* __restrict__ lvals, const int32_t* __restrict__ lcount,
    int64_t cpp, const float* __restrict__ z, const float* __restrict__ Wo, const float* __restrict__ bo, int H_arg,
    int act, int splits, float* __restrict__ dz_part, const int32_t* __restrict__ start, int32_t* __restrict__ cursor,
    int32_t* __restrict__ ent_row, float* __restrict__ ent_val, float* __restrict__ partial_loss,
    int32_t* __restrict__ count) {
  constexpr int kGroups = kBlock / LPP;
  constexpr int kRow = LPP * EPL;
  __shared__ int s_pre[kListParts + 1];
  __shared__ int32_t s_col[kListCap];
  __shared__ float s_val[kListCap];
  __shared__ float s_dz[kGroups][kRow];
  __shared__ float s_loss[kGroups];
  __shared__ int s_done[kGroups];
  const int H = EXACT ? kRow : H_arg;
  const int64_t r = blockIdx.x;
  const int split = blockIdx.y;
  const int lane = threadIdx.x & (LPP - 1), group = threadIdx.x / LPP;
  // lane l holds floats l + LPP k of a row; past H the load is clamped into the row and masked
  auto load = [&](const float* __restrict__ row, float (&v)[EPL]) {
#pragma unroll
    for (int k = 0; k < EPL; ++k) v[k] = row[EXACT ? lane + LPP * k : min(lane + LPP * k, H - 1)];
  };
  float zr[EPL], acc[EPL];
  bool in[EPL];
  load(z + r * H, zr);
#pragma unroll
  for (int k = 0; k < EPL; ++k) {
    in[k] = EXACT || lane + LPP * k < H;
    if (!in[k]) zr[k] = 0.0f;
    acc[k] = 0.0f;
  }
  float loss = 0.0f;
  int done = 0;
  for (int skip = 0;; skip += kListCap) {
    const int n = gather_row_list(lcols, lvals, lcount, cpp, r, skip, s_pre, s_col, s_val);
    for (int j0 = split + group * splits; j0 < n; j0 += 2 * kGroups * splits) {
      const int j1 = j0 + kGroups * splits;
      const bool two = j1 < n;
      const int col0 = s_col[j0], col1 = s_col[two ? j1 : j0];
      float w0[EPL], w1[EPL];
      load(Wo + (int64_t)col0 * H, w0);
      load(Wo + (int64_t)col1 * H, w1);
      const float b0 = bo ? bo[col0] : 0.0f, b1 = bo ? bo[col1] : 0.0f;
#pragma unroll
      for (int which = 0; which < 2; ++which) {
        if (which == 1 && !two) break;
        const float (&w)[EPL] = which ? w1 : w0;
        const int col = which ? col1 : col0;
        float d = 0.0f;
#pragma unroll
        for (int k = 0; k < EPL; ++k) d += in[k] ? w[k] * zr[k] : 0.0f;
        const float pre = group_sum_dpp<LPP>(d) + (which ? b1 : b0);
        ++done;
        const float t = s_val[which ? j1 : j0];
        const float y = decode_output(pre, act);
        loss += bce_term(y, t);
        const float g = bce_grad(y, t, act);
#pragma unroll
        for (int k = 0; k < EPL; ++k) acc[k] += g * w[k];
        if (lane == 0) {                              // (row, g) into the column's segment: its owner sums by row
          const int at = start[col] + atomicAdd(cursor + col, 1);
          ent_row[at] = (int32_t)r;
          ent_val[at] = g;
        }
      }
    }
    const bool more = skip + n < s_pre[kListParts];
    __syncthreads();                                  // the staged list is overwritten by the next pass
    if (!more) break;
  }
#pragma unroll
  for (int k = 0; k < EPL; ++k) s_dz[group][lane + LPP * k] = acc[k];
  if (lane == 0) { s_loss[group] = loss; s_done[group] = done; }
  __syncthreads();
  for (int h = threadIdx.x; h < H; h += kBlock) {    // the lane groups in fixed order
    float tsum = 0.0f;
#pragma unroll
    for (int k = 0; k < kGroups; ++k) tsum += s_dz[k][h];
    dz_part[(r * splits + split) * H + h] = tsum;
  }
  if (threadIdx.x == 0) {
    float tl = 0.0f;
    int tot = 0;
#pragma unroll
    for (int k = 0; k < kGroups; ++k) { tl += s_loss[k]; tot += s_done[k]; }
    partial_loss[r * splits + split] = tl;
    spread_count_add(count, blockIdx.y * gridDim.x + blockIdx.x, tot);
  }
}

// dz[r, h] = the splits' partials in split order
__global__ __launch_bounds__(kBlock) void cdae_owned_sum_splits_kernel(const float* __restrict__ dz_part, int64_t B,
                                                                       int H, int splits, float* __restrict__ dz) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= B * H) return;
  const int64_t r = e / H, h = e % H;
  float acc = 0.0f;
  for (int s = 0; s < splits; ++s) acc += dz_part[(r * splits + s) * H + h];
  dz[e] = acc;
}

// A column's owner: H / EPL lanes, lane l holding floats l + (H / EPL) k of the output row.  The column's n entries
// are taken by ascending batch row — n rounds of "smallest row above the last one", each a scan of the segment by
// the lanes and a minimum over them — so the sum does not depend on the slots the cursor handed out.
template <int EPL, bool BIAS>
__global__ __launch_bounds__(kBlock) void cdae_owned_gather_kernel(
    const int32_t* __restrict__ start, const int32_t* __restrict__ ent_row, const float* __restrict__ ent_val,
    const float* __restrict__ M, int64_t I, int H, float* __restrict__ out, float* __restrict__ out_b) {
  const int G = H / EPL;
  const int lane = threadIdx.x & (G - 1);
  const int64_t c = (int64_t)blockIdx.x * (kBlock / G) + threadIdx.x / G;
  if (c >= I) return;
  const int s0 = start[c], n = start[c + 1] - s0;
  if (n == 0) return;
  const int r0 = lane < n ? ent_row[s0 + lane] : INT_MAX;      // the lane's first entry stays in registers
  const float v0 = lane < n ? ent_val[s0 + lane] : 0.0f;
  float acc[EPL];
#pragma unroll
  for (int k = 0; k < EPL; ++k) acc[k] = 0.0f;
  float bsum = 0.0f;
  int last = -1;
  for (int i = 0; i < n; ++i) {
    int best = r0 > last ? r0 : INT_MAX;
    float bv = v0;
    for (int j = lane + G; j < n; j += G) {
      const int rj = ent_row[s0 + j];
      if (rj > last && rj < best) { best = rj; bv = ent_val[s0 + j]; }
    }
    for (int m = G / 2; m >= 1; m >>= 1) {
      const int o = __shfl_xor(best, m, kWave);
      const float ov = __shfl_xor(bv, m, kWave);
      if (o < best) { best = o; bv = ov; }
    }
    if (best == INT_MAX) break;                       // a row twice in one column: not a list this layout produces
    const float* __restrict__ row = M + (int64_t)best * H;
#pragma unroll
    for (int k = 0; k < EPL; ++k) acc[k] += bv * row[lane + G * k];
    bsum += bv;
    last = best;
  }
#pragma unroll
  for (int k = 0; k < EPL; ++k) out[c * H + lane + G * k] = acc[k];
  if (BIAS && lane == 0) out_b[c] = bsum;
}

// The hidden layer's backward, a workgroup per batch row: dzp[r, :] = dz[r, :] (/ count) act'(z[r, :]), the row's input
// entries into their columns' segments, the user and item marks, and (workgroup 0) the step's loss from the partials.
__global__ __launch_bounds__(kBlock) void cdae_owned_hidden_rows_kernel(
    const int32_t* __restrict__ cols, const float* __restrict__ vals, const int32_t* __restrict__ count, int64_t cpp,
    const float* __restrict__ dz, const float* __restrict__ z, int act, int scale_dz,
    const int32_t* __restrict__ pos_count, const int64_t* __restrict__ user, int64_t num_users, int H,
    uint8_t* __restrict__ touched_users, uint8_t* __restrict__ touched_items, const int32_t* __restrict__ start,
    int32_t* __restrict__ cursor, int32_t* __restrict__ ent_row, float* __restrict__ ent_val, float* __restrict__ dzp,
    const float* __restrict__ partial_loss, int64_t n_partials, float* __restrict__ stats,
    double* __restrict__ loss_accum) {
  __shared__ float s_red[kWavesPerBlock];
  const int lane = threadIdx.x & (kWave - 1);
  const int32_t npos = spread_count(pos_count, lane);
  const float alpha = scale_dz ? (npos > 0 ? 1.0f / (float)npos : 0.0f) : 1.0f;
  const int64_t r = blockIdx.x;
  for (int h = threadIdx.x; h < H; h += kBlock) {
    float g = dz[r * H + h];
    g *= alpha;
    if (act == 1) {
      const float y = z[r * H + h];
      g *= y * (1.0f - y);
    }
    dzp[r * H + h] = g;
  }
  const int64_t u = user[r];
  if ((uint64_t)u < (uint64_t)num_users && threadIdx.x == 0 && touched_users) touched_users[u] = 1;
  for_row_entries(cols, count, cpp, r, [&](int32_t c, int64_t at) {
    const int to = start[c] + atomicAdd(cursor + c, 1);
    ent_row[to] = (int32_t)r;
    ent_val[to] = vals[at];
    touched_items[c] = 1;
  });
  if (blockIdx.x == 0 && n_partials > 0) {
    float sacc = 0.0f;
    for (int64_t k = threadIdx.x; k < n_partials; k += kBlock) sacc += partial_loss[k];
    const float tot = block_sum(sacc, s_red);
    if (threadIdx.x == 0) {
      const float mean = npos > 0 ? tot / (float)npos : 0.0f;
      stats[0] = mean;
      stats[1] = (float)npos;
      if (loss_accum) loss_accum[0] += (double)mean;
    }
  }
}

// Workgroups [0, B): batch row r, if it is the first row of its user u, writes dV[u, :] = the sum of dzp over the rows
// of u in ascending order (out-of-range users: nothing; a user with one row: a copy).  Workgroups from B on, 64 hidden
// units each: db_h[h] over a fixed shape — wave w adds the w-th quarter of the rows (ceil(B / 4) each) serially in
// ascending order, and the four quarters are added in quarter order.
__global__ __launch_bounds__(kBlock) void cdae_owned_hidden_sums_kernel(const float* __restrict__ dzp,
                                                                        const int64_t* __restrict__ user, int64_t B,
                                                                        int64_t num_users, int H,
                                                                        float* __restrict__ dV,
                                                                        float* __restrict__ dbh) {
  if (blockIdx.x >= B) {
    __shared__ float s_part[kWavesPerBlock][kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int h = (int)(blockIdx.x - B) * kWave + lane;
    const int64_t quarter = (B + kWavesPerBlock - 1) / kWavesPerBlock;
    const int64_t r_lo = min(B, wave * quarter), r_hi = min(B, r_lo + quarter);
    float acc = 0.0f;
    if (h < H) {
      int64_t r = r_lo;
      for (; r + 8 <= r_hi; r += 8) {               // eight loads in flight, added in row order
        float t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = dzp[(r + k) * H + h];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += t[k];
      }
      for (; r < r_hi; ++r) acc += dzp[r * H + h];
    }
    s_part[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && h < H) {
      float t = s_part[0][lane];
#pragma unroll
      for (int w = 1; w < kWavesPerBlock; ++w) t += s_part[w][lane];
      dbh[h] = t;
    }
    return;
  }
  const int64_t r = blockIdx.x;
  const int64_t u = user[r];
  if ((uint64_t)u >= (uint64_t)num_users) return;   // workgroup-uniform
  int earlier = 0, later = 0;
  for (int64_t q = threadIdx.x; q < B; q += kBlock) {
    const bool same = user[q] == u;
    earlier |= same && q < r;
    later |= same && q > r;
  }
  if (__syncthreads_or(earlier)) return;            // an earlier row of this user owns the sum
  const bool shared_user = __syncthreads_or(later);
  for (int h = threadIdx.x; h < H; h += kBlock) {
    float acc = dzp[r * H + h];
    if (shared_user)
      for (int64_t q = r + 1; q < B; ++q)
        if (user[q] == u) acc += dzp[q * H + h];
    dV[u * H + h] = acc;
  }
}

}  // namespace yr

using namespace yr;

namespace {

bool owned_width_ok(int H) { return H >= 16 && H <= 1024 && (H & (H - 1)) == 0; }

struct OwnedWorkspace {
  int64_t counters, start, ent_row, ent_val, rows, bytes;   // byte offsets, each a multiple of 16
};

// 0 or a YR_ERR_*
int owned_layout(int64_t B, int64_t I, int H, OwnedWorkspace* w) {
  if (B < 0 || I <= 0 || H <= 0) return YR_ERR_BADARG;
  if (!owned_width_ok(H)) return YR_ERR_UNSUPPORTED;
  const int64_t cpp = yr_cdae_sparse_part_columns(I);
  if (B >= INT32_MAX || I >= INT32_MAX - 1 || (B > 0 && cpp > (INT32_MAX - 1) / kListParts / B))
    return YR_ERR_UNSUPPORTED;                           // rows, columns and slots are 32-bit
  const int64_t entries = B * kListParts * cpp;
  const int64_t row_floats = B * H * std::max(1, yr_cdae_sampled_decode_splits(B));
  auto up = [](int64_t bytes) { return (bytes + 15) / 16 * 16; };
  int64_t off = 0;
  w->counters = off; off += up(4 * 2 * I);                // counts [I], then cursors [I]: one memset
  w->start = off;   off += up(4 * (I + 1));
  w->ent_row = off; off += up(4 * entries);
  w->ent_val = off; off += up(4 * entries);
  w->rows = off;    off += up(4 * row_floats);
  w->bytes = off;
  return 0;
}

struct OwnedPointers {
  int32_t *cnt, *cursor, *start, *ent_row;
  float *ent_val, *rows;
};

OwnedPointers owned_pointers(void* workspace, const OwnedWorkspace& w, int64_t I) {
  char* base = static_cast<char*>(workspace);
  int32_t* counters = reinterpret_cast<int32_t*>(base + w.counters);
  return {counters, counters + I, reinterpret_cast<int32_t*>(base + w.start),
          reinterpret_cast<int32_t*>(base + w.ent_row), reinterpret_cast<float*>(base + w.ent_val),
          reinterpret_cast<float*>(base + w.rows)};
}

// the lists' entries counted per column and scanned; the cursors zero
int owned_sort_prologue(const int32_t* cols, const int32_t* count, int64_t B, int64_t I, const OwnedPointers& p,
                        hipStream_t s) {
  const hipError_t e = hipMemsetAsync(p.cnt, 0, sizeof(int32_t) * 2 * I, s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(cdae_owned_count_kernel, dim3((unsigned)B), dim3(kBlock), 0, s, cols, count,
                     yr_cdae_sparse_part_columns(I), p.cnt);
  hipLaunchKernelGGL(owned_scan_kernel<false>, dim3((unsigned)owned_scan_grid(I)), dim3(kBlock), 0, s, p.cnt, I,
                     p.start, (int32_t*)nullptr);
  return launch_status();
}

template <bool BIAS>
int owned_gather(const OwnedPointers& p, const float* M, int64_t I, int H, float* out, float* out_b, hipStream_t s) {
  const int epl = H <= kWave ? 1 : H / kWave;
  const int per_block = kBlock / (H / epl);
  const dim3 grid((unsigned)((I + per_block - 1) / per_block));
#define YR_OG(EPL)                                                                                                    \
  hipLaunchKernelGGL((cdae_owned_gather_kernel<EPL, BIAS>), grid, dim3(kBlock), 0, s, p.start, p.ent_row, p.ent_val, \
                     M, I, H, out, out_b)
  switch (epl) {
    case 1: YR_OG(1); break;
    case 2: YR_OG(2); break;
    case 4: YR_OG(4); break;
    case 8: YR_OG(8); break;
    default: YR_OG(16); break;
  }
#undef YR_OG
  return launch_status();
}

}  // namespace

extern "C" int64_t yr_cdae_owned_workspace_bytes(int64_t B, int64_t I, int H) {
  OwnedWorkspace w;
  if (const int s = owned_layout(B, I, H, &w)) return s;
  return w.bytes;
}

extern "C" int yr_cdae_owned_decode(const int32_t* loss_cols, const float* loss_targets, const int32_t* loss_count,
                                    const float* z, const float* Wo, const float* bo, int64_t B, int64_t I, int H,
                                    int act, float* dz, float* dWo, float* dbo, float* partial_loss, int32_t* count,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
  if (workspace_bytes < 0 || (act != 0 && act != 1)) return YR_ERR_BADARG;
  OwnedWorkspace w;
  if (const int s = owned_layout(B, I, H, &w)) return s;
  if (B == 0) return 0;
  if (!loss_cols || !loss_targets || !loss_count || !z || !Wo || !dz || !dWo || !dbo || !partial_loss || !count ||
      !workspace)
    return YR_ERR_BADARG;
  if ((reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(Wo) | reinterpret_cast<uintptr_t>(workspace)) & 15)
    return YR_ERR_BADARG;
  if (workspace_bytes < w.bytes) return YR_ERR_BADARG;
  const OwnedPointers p = owned_pointers(workspace, w, I);
  hipStream_t s = (hipStream_t)stream;
  if (const int st = owned_sort_prologue(loss_cols, loss_count, B, I, p, s)) return st;
  const int splits = yr_cdae_sampled_decode_splits(B);
  const int64_t cpp = yr_cdae_sparse_part_columns(I);
  const dim3 grid((unsigned)B, (unsigned)splits);
  float* dz_part = splits > 1 ? p.rows : dz;
#define YR_OD(LPP, EPL, EXACT)                                                                                        \
  hipLaunchKernelGGL((cdae_owned_decode_kernel<LPP, EPL, EXACT>), grid, dim3(kBlock), 0, s, loss_cols, loss_targets, \
                     loss_count, cpp, z, Wo, bo, H, act, splits, dz_part, p.start, p.cursor, p.ent_row, p.ent_val,   \
                     partial_loss, count)
  if (H <= 128) YR_OD(32, 4, false);
  else if (H <= 256) YR_OD(32, 8, false);
  else if (H == 512) YR_OD(64, 8, true);
  else YR_OD(64, 16, true);
#undef YR_OD
  if (const int st = launch_status()) return st;
  if (splits > 1) {
    hipLaunchKernelGGL(cdae_owned_sum_splits_kernel, dim3((unsigned)((B * H + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       s, p.rows, B, H, splits, dz);
    if (const int st = launch_status()) return st;
  }
  return owned_gather<true>(p, z, I, H, dWo, dbo, s);
}

extern "C" int yr_cdae_owned_hidden_bwd(const int32_t* cols, const float* vals, const int32_t* count, const float* dz,
                                        const float* z, int act, int scale_dz, const int32_t* pos_count,
                                        const int64_t* user, int64_t B, int64_t I, int H, int64_t num_users,
                                        float* dV, uint8_t* touched_users, float* dbh, float* dWhT,
                                        uint8_t* touched_items, const float* partial_loss, int64_t n_partials,
                                        float* stats, double* loss_accum, void* workspace, int64_t workspace_bytes,
                                        void* stream) {
  if (workspace_bytes < 0 || num_users <= 0 || n_partials < 0 || (act != 0 && act != 1)) return YR_ERR_BADARG;
  OwnedWorkspace w;
  if (const int s = owned_layout(B, I, H, &w)) return s;
  if (B == 0) return 0;
  if (!cols || !vals || !count || !dz || !z || !pos_count || !user || !dV || !dbh || !dWhT || !touched_items ||
      !workspace)
    return YR_ERR_BADARG;
  if (n_partials > 0 && (!partial_loss || !stats)) return YR_ERR_BADARG;
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return YR_ERR_BADARG;
  if (workspace_bytes < w.bytes) return YR_ERR_BADARG;
  const OwnedPointers p = owned_pointers(workspace, w, I);
  hipStream_t s = (hipStream_t)stream;
  if (const int st = owned_sort_prologue(cols, count, B, I, p, s)) return st;
  hipLaunchKernelGGL(cdae_owned_hidden_rows_kernel, dim3((unsigned)B), dim3(kBlock), 0, s, cols, vals, count,
                     yr_cdae_sparse_part_columns(I), dz, z, act, scale_dz ? 1 : 0, pos_count, user, num_users, H,
                     touched_users, touched_items, p.start, p.cursor, p.ent_row, p.ent_val, p.rows, partial_loss,
                     n_partials, stats, loss_accum);
  if (const int st = launch_status()) return st;
  if (const int st = owned_gather<false>(p, p.rows, I, H, dWhT, nullptr, s)) return st;
  hipLaunchKernelGGL(cdae_owned_hidden_sums_kernel, dim3((unsigned)(B + (H + kWave - 1) / kWave)), dim3(kBlock), 0,
                     s, p.rows, user, B, num_users, H, dV, dbh);
  return launch_status();
}
