// Owner-pass gradients of the fused NGCF step for gfx950: the reproducible forms of ngcf_score_bwd_kernel,
// ngcf_dense_bwd_weight_kernel and the batch's row sets (csrc/ngcf.hip) — reference trainers/ngcf_trainer.py:104-116,
// whose runs repeat bit for bit under one seed.  The default kernels add the layer gradients and dW with global float
// atomics (arrival order) and list a row set's members in arrival order.  Here no float atomic is issued: every
// gradient element is summed by the one owner of its destination in the order written below and stored once.
//
//   score backward   The 3 B (destination row, triplet, role) entries of a batch are counting-sorted by row: integer
//                    counts per row (atomic increments, which also hand every entry its arrival slot), one exclusive
//                    integer scan (owned_scan.h), the entries into their rows' segments.  WHICH slot of its segment
//                    an entry takes depends on arrival, so ngcf_owned_rank_kernel rewrites every segment by ascending
//                    key = 4 x triplet + role (user 0, positive 1, negative 2; the keys of a row are distinct) — an
//                    entry's place is the number of smaller keys in its segment, an integer that no order of
//                    execution changes.  ngcf_owned_score_bwd_kernel: one lane group (D / 4 lanes, 16 bytes each)
//                    per graph row with a non-empty segment, all K + 1 layers:
//                        acc = dlayers[k][row];  for every entry in ascending key:  acc += c;  dlayers[k][row] = acc
//                    with c = fmaf(gn, E_k[U + neg], gp * E_k[U + pos]) on a user row (gp * E_k[U + pos] without
//                    negatives) and c = gp * E_k[user] (role 1) or gn * E_k[user] (role 2) on an item row — the
//                    default kernel's values, each added with a single f32 add.  The order is strictly serial for a
//                    segment of ANY length (the "shape" is a chain); four entries' rows are loaded ahead of their
//                    adds.  Rows without an entry are not written.  Out-of-range ids raise the flag and skip the
//                    triplet before any counter is indexed.  Cost of a segment of m entries: m^2 integer compares in
//                    the rank pass, m dependent adds per layer — made for batches whose rows carry tens of entries.
//   weight gradient  ngcf_owned_dw_slots_kernel is ngcf_dense_bwd_weight_kernel (same chunk walk and MFMA loop,
//                    ngcf_parts.h) storing its 2 D^2 partial sums into the workgroup's own slot of a scratch array;
//                    ngcf_owned_dw_reduce_kernel: dW[e] = (((dW[e] + slot_0[e]) + slot_1[e]) + ...) over the
//                    workgroups that had rows — g < min(grid, ceil(rows / ROWS)) with rows = n or *count —, in
//                    ascending workgroup order; a slot that was not written this call is never read.  The grid is
//                    capped at kOwnedDwGrid workgroups (the default form's 512 would need 67 MB of slots at D = 128).
//   row sets         yr_ngcf_frontier_order: rows[0 .. *count) rebuilt ASCENDING from the flags by the compacting
//                    form of the scan, *count = the set's size.
// Everything else of the step has one owner per output already: the pull SpMM (a wave per row, the lanes' partial
// sums combined by a fixed butterfly; a heavy row's four wave sums through LDS in wave order), ngcf_dense_fwd and
// ngcf_dense_bwd_data (a row's outputs depend on that row alone, one k-ordered fmaf chain each), the loss (a fixed
// workgroup tree, partials by workgroup index, yr_loss_finalize in a fixed shape) and Adam (element-wise).
// The counters are cleared by the entry points themselves: the workspace may hold anything on entry.
#include "common.h"
#include "ngcf_parts.h"
#include "owned_scan.h"
#include "owned_triplets.h"

#ifndef YR_NGCF_OWNED_DW_GRID
#define YR_NGCF_OWNED_DW_GRID 256
#endif

namespace yr {

constexpr int kOwnedDwGrid = YR_NGCF_OWNED_DW_GRID;   // slots of the ordered weight gradient: one workgroup per CU
// the counting sort of the batch by destination row (count, fill, rank): owned_triplets.h

constexpr int kOwnedAhead = 4;     // entries whose rows are loaded before the first of their adds

template <int D, bool NEG>
__global__ __launch_bounds__(kBlock) void ngcf_owned_score_bwd_kernel(LayerPtrs L, LayerGradPtrs G, int n_layers,
                                                                      const int64_t* __restrict__ user,
                                                                      const int64_t* __restrict__ pos,
                                                                      const int64_t* __restrict__ neg,
                                                                      const float* __restrict__ gpos,
                                                                      const float* __restrict__ gneg,
                                                                      int64_t num_users, int64_t n_rows,
                                                                      const int32_t* __restrict__ start,
                                                                      const int32_t* __restrict__ sorted) {
  constexpr int LPR = D / 4, GPW = kWave / LPR;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int grp = lane / LPR, l = lane % LPR;
  const int64_t groups = (int64_t)gridDim.x * kWavesPerBlock * GPW;
  for (int64_t row = ((int64_t)blockIdx.x * kWavesPerBlock + wave) * GPW + grp; row < n_rows; row += groups) {
    const int s0 = start[row], s1 = start[row + 1];
    if (s0 == s1) continue;                               // no triplet touches the row: not written
    const bool user_row = row < num_users;
#pragma unroll 1
    for (int k = 0; k < n_layers; ++k) {
      const float* __restrict__ E = L.p[k] + 4 * l;
      float* dst = G.p[k] + row * D + 4 * l;
      float4 acc = ld4(dst);
      for (int i = s0; i < s1; i += kOwnedAhead) {
        float4 c[kOwnedAhead];
#pragma unroll
        for (int q = 0; q < kOwnedAhead; ++q) {
          c[q] = zero4();
          if (i + q < s1) {
            const int32_t key = sorted[i + q];
            const int64_t b = key >> 2;
            if (user_row) {
              const float gp = gpos[b];
              const float4 rp = ld4(E + (num_users + pos[b]) * D);
              c[q] = make_float4(gp * rp.x, gp * rp.y, gp * rp.z, gp * rp.w);
              if (NEG) {
                const float gn = gneg[b];
                const float4 rn = ld4(E + (num_users + neg[b]) * D);
                c[q] = make_float4(fmaf(gn, rn.x, c[q].x), fmaf(gn, rn.y, c[q].y), fmaf(gn, rn.z, c[q].z),
                                   fmaf(gn, rn.w, c[q].w));
              }
            } else {
              const float g = (NEG && (key & 3) == kRoleNeg) ? gneg[b] : gpos[b];
              const float4 ru = ld4(E + user[b] * D);
              c[q] = make_float4(g * ru.x, g * ru.y, g * ru.z, g * ru.w);
            }
          }
        }
#pragma unroll
        for (int q = 0; q < kOwnedAhead; ++q)
          if (i + q < s1) { acc.x += c[q].x; acc.y += c[q].y; acc.z += c[q].z; acc.w += c[q].w; }
      }
      st4(dst, acc);
    }
  }
}

template <int D, bool SUB>
__global__ __launch_bounds__(kBlock) void ngcf_owned_dw_slots_kernel(
    const float* __restrict__ dEout, const float* __restrict__ Eout, const float* __restrict__ E,
    const float* __restrict__ Z, int n_all, float* __restrict__ slots, const int32_t* __restrict__ rows,
    const int32_t* __restrict__ count) {
  float* mine = slots + (int64_t)blockIdx.x * (2 * D * D);
  ngcf_dense_bwd_weight_body<D, SUB, true>(dEout, Eout, E, Z, n_all, mine, mine + D * D, rows, count);
}

// dW1 | dW2 += the written slots in ascending workgroup order, a thread per element (2 D^2 threads: 32 workgroups at
// D = 64 — the chain of an element is serial, so the launch lives on loads in flight: sixteen slots ahead of their adds)
constexpr int kOwnedDwAhead = 16;

__global__ __launch_bounds__(kBlock) void ngcf_owned_dw_reduce_kernel(const float* __restrict__ slots, int grid_w,
                                                                      int chunk_rows, int n_all,
                                                                      const int32_t* __restrict__ count, int dd,
                                                                      float* __restrict__ dW1,
                                                                      float* __restrict__ dW2) {
  const int64_t n = count ? *count : n_all;
  const int64_t chunks = (n + chunk_rows - 1) / chunk_rows;
  const int written = (int)(chunks < grid_w ? chunks : grid_w);
  const int e = (int)blockIdx.x * kBlock + (int)threadIdx.x;
  if (e >= 2 * dd || written == 0) return;
  float* dst = e < dd ? dW1 + e : dW2 + (e - dd);
  float acc = *dst;
  const float* src = slots + e;
  const int64_t pitch = 2 * (int64_t)dd;
  int g = 0;
  for (; g + kOwnedDwAhead <= written; g += kOwnedDwAhead) {
    float t[kOwnedDwAhead];
#pragma unroll
    for (int q = 0; q < kOwnedDwAhead; ++q) t[q] = src[(g + q) * pitch];
#pragma unroll
    for (int q = 0; q < kOwnedDwAhead; ++q) acc += t[q];
  }
  for (; g < written; ++g) acc += src[g * pitch];
  *dst = acc;
}

}  // namespace yr

using namespace yr;

namespace {

bool ngcf_width_ok(int D) { return D == 16 || D == 32 || D == 64 || D == 128; }

int64_t up256(int64_t x) { return (x + 255) & ~(int64_t)255; }

struct OwnedScoreLayout {
  int64_t cnt, start, slot, ent, sorted, bytes;      // byte offsets, each a multiple of 256
  OwnedScoreLayout(int64_t n, int64_t B) {
    int64_t at = 0;
    cnt = at;    at += up256(4 * n);
    start = at;  at += up256(4 * (n + 1));
    slot = at;   at += up256(12 * B);
    ent = at;    at += up256(12 * B);
    sorted = at; at += up256(12 * B);
    bytes = at;
  }
};

// keys are 4 b + role in an int32, segment offsets int32
bool owned_score_sizes_ok(int64_t n, int64_t B) { return n > 0 && n < 0x7fffffff && B >= 0; }
bool owned_score_sizes_supported(int64_t B) { return B <= (0x7fffffff >> 2); }

int owned_dw_grid(int64_t rows, int D) {
  const int64_t chunk = 4096 / D;
  const int64_t chunks = (rows + chunk - 1) / chunk;
  const int64_t per_block = (chunks + kOwnedDwGrid - 1) / kOwnedDwGrid;            // equal shares
  return per_block ? (int)((chunks + per_block - 1) / per_block) : 0;
}

}  // namespace

#define YR_NGCF_OWNED_DISPATCH(D, ...)                         \
  switch (D) {                                                 \
    case 16: { constexpr int kD = 16; __VA_ARGS__; } break;    \
    case 32: { constexpr int kD = 32; __VA_ARGS__; } break;    \
    case 64: { constexpr int kD = 64; __VA_ARGS__; } break;    \
    case 128: { constexpr int kD = 128; __VA_ARGS__; } break;  \
    default: return YR_ERR_UNSUPPORTED;                        \
  }

extern "C" int64_t yr_ngcf_owned_score_workspace_bytes(int64_t n, int64_t B) {
  if (!owned_score_sizes_ok(n, B)) return YR_ERR_BADARG;
  if (!owned_score_sizes_supported(B)) return YR_ERR_UNSUPPORTED;
  return OwnedScoreLayout(n, B).bytes;
}

extern "C" int yr_ngcf_owned_score_bwd(const float* const* layers, float* const* dlayers, int n_layers,
                                       const int64_t* user, const int64_t* pos, const int64_t* neg, const float* gpos,
                                       const float* gneg, int64_t B, int D, int64_t num_users, int64_t num_items,
                                       void* workspace, int64_t workspace_bytes, int32_t* err_flag, void* stream) {
  if (B < 0 || num_users <= 0 || num_items <= 0 || n_layers <= 0 || n_layers > YR_NGCF_MAX_LAYERS ||
      workspace_bytes < 0)
    return YR_ERR_BADARG;
  const int64_t n = num_users + num_items;
  if (!owned_score_sizes_ok(n, B)) return YR_ERR_BADARG;
  if (!ngcf_width_ok(D) || !owned_score_sizes_supported(B)) return YR_ERR_UNSUPPORTED;
  if (B == 0) return 0;
  if (!layers || !dlayers || !user || !pos || !gpos || (neg != nullptr) != (gneg != nullptr) || !workspace)
    return YR_ERR_BADARG;
  const OwnedScoreLayout lay(n, B);
  if (workspace_bytes < lay.bytes || ((uintptr_t)workspace & 15)) return YR_ERR_BADARG;
  LayerPtrs L{};
  LayerGradPtrs G{};
  for (int k = 0; k < n_layers; ++k) {
    if (!layers[k] || !dlayers[k] || (((uintptr_t)layers[k] | (uintptr_t)dlayers[k]) & 15)) return YR_ERR_BADARG;
    L.p[k] = layers[k];
    G.p[k] = dlayers[k];
  }
  char* ws = static_cast<char*>(workspace);
  int32_t* cnt = reinterpret_cast<int32_t*>(ws + lay.cnt);
  int32_t* start = reinterpret_cast<int32_t*>(ws + lay.start);
  int32_t* slot = reinterpret_cast<int32_t*>(ws + lay.slot);
  int32_t* ent = reinterpret_cast<int32_t*>(ws + lay.ent);
  int32_t* sorted = reinterpret_cast<int32_t*>(ws + lay.sorted);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(cnt, 0, sizeof(int32_t) * n, s) != hipSuccess) return (int)hipGetLastError();
  const int tgrid = grid_for(B, kBlock);
  if (neg) {
    hipLaunchKernelGGL(ngcf_owned_count_kernel<true>, dim3(tgrid), dim3(kBlock), 0, s, user, pos, neg, B, num_users,
                       num_items, cnt, slot, err_flag);
  } else {
    hipLaunchKernelGGL(ngcf_owned_count_kernel<false>, dim3(tgrid), dim3(kBlock), 0, s, user, pos, neg, B, num_users,
                       num_items, cnt, slot, err_flag);
  }
  hipLaunchKernelGGL(owned_scan_kernel<false>, dim3(owned_scan_grid(n)), dim3(kBlock), 0, s, cnt, n, start,
                     (int32_t*)nullptr);
  if (neg) {
    hipLaunchKernelGGL(ngcf_owned_fill_kernel<true>, dim3(tgrid), dim3(kBlock), 0, s, user, pos, neg, B, num_users,
                       num_items, start, slot, ent);
  } else {
    hipLaunchKernelGGL(ngcf_owned_fill_kernel<false>, dim3(tgrid), dim3(kBlock), 0, s, user, pos, neg, B, num_users,
                       num_items, start, slot, ent);
  }
  hipLaunchKernelGGL(ngcf_owned_rank_kernel, dim3(grid_for((neg ? 3 : 2) * B, kBlock)), dim3(kBlock), 0, s, user, pos,
                     neg, num_users, n, start, ent, sorted);
  if (const int st = launch_status()) return st;
  YR_NGCF_OWNED_DISPATCH(D, {
    constexpr int kRowsPerBlock = kWavesPerBlock * (kWave / (kD / 4));
    int64_t g = (n + kRowsPerBlock - 1) / kRowsPerBlock;
    if (g > 65536) g = 65536;
    if (neg) {
      hipLaunchKernelGGL((ngcf_owned_score_bwd_kernel<kD, true>), dim3((unsigned)g), dim3(kBlock), 0, s, L, G,
                         n_layers, user, pos, neg, gpos, gneg, num_users, n, start, sorted);
    } else {
      hipLaunchKernelGGL((ngcf_owned_score_bwd_kernel<kD, false>), dim3((unsigned)g), dim3(kBlock), 0, s, L, G,
                         n_layers, user, pos, neg, gpos, gneg, num_users, n, start, sorted);
    }
  });
  return launch_status();
}

extern "C" int64_t yr_ngcf_owned_dw_workspace_bytes(int64_t rows, int D) {
  if (rows < 0 || rows > 0x7fffffff) return YR_ERR_BADARG;
  if (!ngcf_width_ok(D)) return YR_ERR_UNSUPPORTED;
  // enough for every call over at most `rows` rows (the grid of fewer rows can be the larger one: equal shares)
  const int64_t chunks = (rows + 4096 / D - 1) / (4096 / D);
  return up256((chunks < kOwnedDwGrid ? chunks : kOwnedDwGrid) * 2 * D * D * 4);
}

extern "C" int yr_ngcf_owned_dense_bwd_weight(const float* dEout, const float* Eout, const float* E, const float* Z,
                                              int64_t n, int D, float* dW1, float* dW2, const int32_t* rows,
                                              const int32_t* count, int64_t max_rows, void* workspace,
                                              int64_t workspace_bytes, void* stream) {
  if (n < 0 || n > 0x7fffffff || workspace_bytes < 0) return YR_ERR_BADARG;
  if (rows && (!count || max_rows < 0 || max_rows > n)) return YR_ERR_BADARG;
  if (!rows && count) return YR_ERR_BADARG;
  if (!ngcf_width_ok(D)) return YR_ERR_UNSUPPORTED;
  const int64_t bound = rows ? max_rows : n;
  if (bound == 0) return 0;
  if (!dEout || !Eout || !E || !Z || !dW1 || !dW2 || !workspace) return YR_ERR_BADARG;
  if (((uintptr_t)dW1 | (uintptr_t)dW2 | (uintptr_t)workspace) & 15) return YR_ERR_BADARG;
  const int grid = owned_dw_grid(bound, D);
  if (workspace_bytes < (int64_t)grid * 2 * D * D * 4) return YR_ERR_BADARG;
  float* slots = static_cast<float*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  YR_NGCF_OWNED_DISPATCH(D, {
    if (rows) {
      hipLaunchKernelGGL((ngcf_owned_dw_slots_kernel<kD, true>), dim3(grid), dim3(kBlock), 0, s, dEout, Eout, E, Z,
                         (int)n, slots, rows, count);
    } else {
      hipLaunchKernelGGL((ngcf_owned_dw_slots_kernel<kD, false>), dim3(grid), dim3(kBlock), 0, s, dEout, Eout, E, Z,
                         (int)n, slots, rows, count);
    }
  });
  if (const int st = launch_status()) return st;
  const int dd = D * D;
  hipLaunchKernelGGL(ngcf_owned_dw_reduce_kernel, dim3((2 * dd + kBlock - 1) / kBlock), dim3(kBlock), 0, s, slots,
                     grid, 4096 / D, (int)n, rows ? count : (const int32_t*)nullptr, dd, dW1, dW2);
  return launch_status();
}

extern "C" int yr_ngcf_frontier_order(const int32_t* flags, int64_t n, int32_t* rows, int32_t* count, void* stream) {
  if (n < 0 || n > 0x7fffffff || !count) return YR_ERR_BADARG;
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return hipMemsetAsync(count, 0, 4, s) == hipSuccess ? 0 : (int)hipGetLastError();
  if (!flags || !rows || flags == rows || ((uintptr_t)flags & 15)) return YR_ERR_BADARG;
  hipLaunchKernelGGL(owned_scan_kernel<true>, dim3(owned_scan_grid(n)), dim3(kBlock), 0, s, flags, n, rows, count);
  return launch_status();
}
