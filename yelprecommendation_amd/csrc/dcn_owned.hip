// Owner-pass gradients of the DCN training step for gfx950: the reproducible forms of dcn_head_kernel's weight gradients
// and of dcn_assemble_bwd_kernel (csrc/dcn.hip) — reference trainers/dcn_trainer.py:102-116, whose runs repeat bit for
// bit under one seed.  The default kernels add dcw / dcb / dWo / dbo and the four table gradients with float atomics
// (arrival order).  Here no float atomic is issued: every gradient element is summed by one owner in an order that is a
// pure function of the batch's ids and of the static item -> attribute table, and stored once.
//
//   head     dcn_head_ordered_kernel is dcn_head_kernel (one row loop: dcn_head_rows.h) with a PRIVATE accumulator per wave
//            in LDS, (2 L + 1) F + H + 1 floats sized by the launch's own L, F and H.  G = the head's grid =
//            min(max(ceil(units / 4), 1), 256).  Wave w of workgroup g sums, from 0.0f, the terms of its units
//            4 g + w, 4 g + w + 4 G, ... in ascending order, the pos row of a unit before its neg row (lane e mod 64
//            is the only lane that names element e: plain LDS read-add-write).  The workgroup's value
//            ((W0 + W1) + W2) + W3 goes to slot g of the workspace; dcn_head_reduce_kernel, a thread per element:
//                dst = (((dst + P_0) + P_1) + ...) + P_{G-1}.
//            Every one of the G slots is written by the call before it is read.  pred, the loss partials, dh and dx0
//            are the default kernel's, bit for bit.
//   scatter  triplet form only (user, item_a = pos, item_b = neg; row(b, pos) = b, row(b, neg) = B + b), two levels.
//            Level 1, by id: the 3 B entries counting-sorted by destination row and ranked by key = 4 b + role
//            (owned_triplets.h, owned_scan.h; an entry with a bad id is dropped, the other entries of its triplet stay).
//            dcn_owned_rows_kernel, a lane group (D / 4 lanes, 16 bytes each) per touched row, entries in ascending key:
//                user u:  acc = gU[u];  per triplet b:  acc += dx[b, 0:D];  acc += dx[B + b, 0:D];   gU[u] = acc
//                item i:  acc = gI[i], tc = ts = 0.0f;  per entry (row r = b as pos, then B + b as neg):
//                         acc += dx[r, D:2D];  tc += dx[r, 2D:3D];  ts += dx[r, 3D:4D];   gI[i] = acc,  T[i] = [tc | ts]
//            Rows without an entry are not written (T neither: it is read for touched items only).  The item's owner
//            also raises YR_FLAG_BAD_ITEM for an out-of-range category slot or state-city of its item.
//            Level 2, by attribute, over the inverted static table (cat_ptr / cat_item / cat_mult: per category its
//            items ascending, each with the number m of its slots naming the category; sc_ptr / sc_item likewise):
//            every list is cut into chunks of YR_DCN_OWNED_CHUNK entries.  dcn_owned_chunk_kernel, a thread per (chunk,
//            column): q = 0.0f;  for the chunk's TOUCHED items (batch count != 0) in ascending order:
//                q += T_sc[i]                                  (state-city)
//                q += (float(m) * T_cat[i]) / float(Lmax)      (category)
//            dcn_owned_attr_rows_kernel, a thread per (attribute row, column):
//                acc = dst;  for the row's chunks WITH a touched item, ascending:  acc += q_chunk;   dst = acc
//            A row without a touched item is not written.  The tree depends on the static table alone; no pass is
//            quadratic in the entries of an attribute row.
// The counters are cleared by the entry points themselves: the workspaces may hold anything on entry.
#include <algorithm>

#include "common.h"
#include "dcn_parts.h"
#include "owned_scan.h"
#include "owned_triplets.h"

namespace yr {

constexpr int kChunk = YR_DCN_OWNED_CHUNK;

// --------------------------------------------------------------------------- ordered head
__global__ __launch_bounds__(kBlock) void dcn_head_ordered_kernel(DcnHead p, float* __restrict__ slots) {
  extern __shared__ float sWave[];             // [4 waves][dcw: L*F | dcb: L*F | dWo: H + F | dbo]
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int F = p.F, H = p.H, L = p.L;
  const bool grads = p.dx0 != nullptr;
  const int oDcb = L * F, oWo = 2 * L * F, oBo = 2 * L * F + H + F;
  const int nacc = oBo + 1;
  float* mine = sWave + wave * nacc;
  if (grads)
    for (int e = lane; e < nacc; e += kWave) mine[e] = 0.0f;
  // terms into the wave's own accumulator: element e is named by one lane of the wave only, in program order
#define DCN_HEAD_TERM(e, v) mine[e] += v
#include "dcn_head_rows.h"
#undef DCN_HEAD_TERM
  if (!grads) return;
  __syncthreads();
  float* out = slots + (int64_t)blockIdx.x * nacc;
  for (int e = threadIdx.x; e < nacc; e += kBlock)
    out[e] = ((sWave[e] + sWave[nacc + e]) + sWave[2 * nacc + e]) + sWave[3 * nacc + e];
}

constexpr int kHeadAhead = 16;                 // slots loaded ahead of their adds

__global__ __launch_bounds__(kBlock) void dcn_head_reduce_kernel(const float* __restrict__ slots, int G, int L, int F,
                                                                 int H, float* __restrict__ dcw, float* __restrict__ dcb,
                                                                 float* __restrict__ dWo, float* __restrict__ dbo) {
  const int oDcb = L * F, oWo = 2 * L * F, oBo = 2 * L * F + H + F;
  const int e = (int)blockIdx.x * kBlock + (int)threadIdx.x;
  if (e > oBo) return;
  float* dst = e < oDcb ? dcw + e : e < oWo ? dcb + (e - oDcb) : e < oBo ? dWo + (e - oWo) : dbo;
  const int64_t nacc = oBo + 1;
  const float* src = slots + e;
  float acc = *dst;
  int g = 0;
  for (; g + kHeadAhead <= G; g += kHeadAhead) {
    float t[kHeadAhead];
#pragma unroll
    for (int q = 0; q < kHeadAhead; ++q) t[q] = src[(g + q) * nacc];
#pragma unroll
    for (int q = 0; q < kHeadAhead; ++q) acc += t[q];
  }
  for (; g < G; ++g) acc += src[g * nacc];
  *dst = acc;
}

// --------------------------------------------------------------------------- ordered scatter, level 1
struct DcnOwnedRows {
  const float* dx;
  int64_t ldx;
  const int64_t* user;
  const int64_t* pos;
  const int64_t* neg;
  int64_t B;
  int D, Lmax;
  int64_t num_users, num_items, num_cats, num_sc;
  const int32_t* cat_ids;
  const int32_t* sc_ids;
  const int32_t* start;
  const int32_t* sorted;
  float* gU;
  float* gI;
  float* T;                                    // [num_items, 2 D]: T_cat | T_sc of the touched items
  int32_t* err_flag;
};

__device__ __forceinline__ void add4(float4& a, const float4& b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }

constexpr int kRowsAhead = 4;                  // entries whose dx rows are loaded before the first of their adds

__global__ __launch_bounds__(kBlock) void dcn_owned_rows_kernel(DcnOwnedRows p) {
  const int D = p.D, LPR = D / 4, GPW = kWave / LPR;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int grp = lane / LPR, l = lane % LPR;
  const int64_t n_rows = p.num_users + p.num_items;
  const int64_t groups = (int64_t)gridDim.x * kWavesPerBlock * GPW;
  int bad = 0;
  for (int64_t row = ((int64_t)blockIdx.x * kWavesPerBlock + wave) * GPW + grp; row < n_rows; row += groups) {
    const int s0 = p.start[row], s1 = p.start[row + 1];
    if (s0 == s1) continue;                    // no triplet touches the row: not written
    if (row < p.num_users) {
      float* dst = p.gU + row * D + 4 * l;
      float4 acc = ld4(dst);
      for (int i = s0; i < s1; i += kRowsAhead) {
        float4 a[kRowsAhead], b[kRowsAhead];
#pragma unroll
        for (int q = 0; q < kRowsAhead; ++q) {
          a[q] = b[q] = zero4();
          if (i + q < s1) {
            const int64_t t = p.sorted[i + q] >> 2;
            a[q] = ld4(p.dx + t * p.ldx + 4 * l);
            b[q] = ld4(p.dx + (p.B + t) * p.ldx + 4 * l);
          }
        }
#pragma unroll
        for (int q = 0; q < kRowsAhead; ++q)
          if (i + q < s1) { add4(acc, a[q]); add4(acc, b[q]); }
      }
      st4(dst, acc);
    } else {
      const int64_t item = row - p.num_users;
      float* dst = p.gI + item * D + 4 * l;
      float4 acc = ld4(dst), tc = zero4(), ts = zero4();
      for (int i = s0; i < s1; i += kRowsAhead) {
        float4 a[kRowsAhead], b[kRowsAhead], c[kRowsAhead];
#pragma unroll
        for (int q = 0; q < kRowsAhead; ++q) {
          a[q] = b[q] = c[q] = zero4();
          if (i + q < s1) {
            const int32_t key = p.sorted[i + q];
            const int64_t r = (key >> 2) + ((key & 3) == kRoleNeg ? p.B : 0);
            const float* g = p.dx + r * p.ldx + 4 * l;
            a[q] = ld4(g + D);
            b[q] = ld4(g + 2 * D);
            c[q] = ld4(g + 3 * D);
          }
        }
#pragma unroll
        for (int q = 0; q < kRowsAhead; ++q)
          if (i + q < s1) { add4(acc, a[q]); add4(tc, b[q]); add4(ts, c[q]); }
      }
      st4(dst, acc);
      st4(p.T + item * 2 * D + 4 * l, tc);
      st4(p.T + item * 2 * D + D + 4 * l, ts);
      // the item's slots: the default kernel's flag for an attribute id out of range
      for (int j = l; j <= p.Lmax; j += LPR) {
        const int64_t c = j < p.Lmax ? p.cat_ids[item * p.Lmax + j] : p.sc_ids[item];
        if (c < 0 || c >= (j < p.Lmax ? p.num_cats : p.num_sc)) bad |= YR_FLAG_BAD_ITEM;
      }
    }
  }
  if (bad && p.err_flag) atomicOr(p.err_flag, bad);
}

// --------------------------------------------------------------------------- ordered scatter, level 2
// One inverted table: rows [0, rows), entries [ptr[r], ptr[r + 1]) of row r, chunks [chunk_ptr[r], chunk_ptr[r + 1]).
struct DcnAttrList {
  const int32_t* ptr;
  const int32_t* item;
  const int32_t* mult;                         // NULL: state-city (the term is T_sc[i])
  const int32_t* chunk_ptr;
  int64_t rows;
  int64_t chunks;
  float* q;                                    // [chunks, D] chunk partials
  int32_t* hit;                                // [chunks] touched items of the chunk
  float* dst;                                  // gC / gS
};

struct DcnOwnedAttr {
  DcnAttrList cat, sc;
  const int32_t* cnt_items;                    // batch count per item (cnt + num_users of level 1)
  const float* T;
  int64_t num_items;
  int D;
  float Lmax;
};

// the row whose chunk range holds chunk c: the last r with chunk_ptr[r] <= c
__device__ __forceinline__ int64_t chunk_row(const int32_t* __restrict__ chunk_ptr, int64_t rows, int64_t c) {
  int64_t lo = 0, hi = rows;                   // chunk_ptr[lo] <= c < chunk_ptr[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (chunk_ptr[mid] <= c) lo = mid; else hi = mid;
  }
  return lo;
}

constexpr int kChunkAhead = 8;                 // entries whose item, count and T element are loaded ahead

__global__ __launch_bounds__(kBlock) void dcn_owned_chunk_kernel(DcnOwnedAttr p) {
  const int D = p.D;
  const int64_t total = (p.cat.chunks + p.sc.chunks) * D;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
    int64_t c = e / D;
    const int d = (int)(e - c * D);
    const bool is_cat = c < p.cat.chunks;
    const DcnAttrList& t = is_cat ? p.cat : p.sc;
    if (!is_cat) c -= p.cat.chunks;
    const int64_t row = chunk_row(t.chunk_ptr, t.rows, c);
    const int64_t lo = t.ptr[row] + (c - t.chunk_ptr[row]) * kChunk;
    const int64_t end = t.ptr[row + 1];
    const int64_t hi = lo + kChunk < end ? lo + kChunk : end;
    const float* T = p.T + (is_cat ? 0 : D) + d;
    float q = 0.0f;
    int hit = 0;
    for (int64_t i = lo; i < hi; i += kChunkAhead) {
      int32_t it[kChunkAhead], n[kChunkAhead], m[kChunkAhead];
      float v[kChunkAhead];
#pragma unroll
      for (int k = 0; k < kChunkAhead; ++k) {
        it[k] = i + k < hi ? t.item[i + k] : -1;
        m[k] = (is_cat && i + k < hi) ? t.mult[i + k] : 1;
      }
#pragma unroll
      for (int k = 0; k < kChunkAhead; ++k) n[k] = (it[k] >= 0 && it[k] < p.num_items) ? p.cnt_items[it[k]] : 0;
#pragma unroll
      for (int k = 0; k < kChunkAhead; ++k) v[k] = n[k] != 0 ? T[(int64_t)it[k] * 2 * D] : 0.0f;
#pragma unroll
      for (int k = 0; k < kChunkAhead; ++k) {
        if (n[k] != 0) {
          q += is_cat ? ((float)m[k] * v[k]) / p.Lmax : v[k];
          ++hit;
        }
      }
    }
    t.q[c * D + d] = q;
    if (d == 0) t.hit[c] = hit;
  }
}

__global__ __launch_bounds__(kBlock) void dcn_owned_attr_rows_kernel(DcnOwnedAttr p) {
  const int D = p.D;
  const int64_t total = (p.cat.rows + p.sc.rows) * D;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
    int64_t row = e / D;
    const int d = (int)(e - row * D);
    const bool is_cat = row < p.cat.rows;
    const DcnAttrList& t = is_cat ? p.cat : p.sc;
    if (!is_cat) row -= p.cat.rows;
    const int c0 = t.chunk_ptr[row], c1 = t.chunk_ptr[row + 1];
    float* dst = t.dst + row * D + d;
    float acc = 0.0f;
    bool any = false;
    for (int c = c0; c < c1; c += kChunkAhead) {
      int hit[kChunkAhead];
      float v[kChunkAhead];
#pragma unroll
      for (int k = 0; k < kChunkAhead; ++k) {
        hit[k] = c + k < c1 ? t.hit[c + k] : 0;
        v[k] = c + k < c1 ? t.q[(int64_t)(c + k) * D + d] : 0.0f;
      }
#pragma unroll
      for (int k = 0; k < kChunkAhead; ++k) {
        if (hit[k] != 0) {
          if (!any) { acc = *dst; any = true; }
          acc += v[k];
        }
      }
    }
    if (any) *dst = acc;
  }
}

}  // namespace yr

using namespace yr;

namespace {

int64_t up256(int64_t x) { return (x + 255) & ~(int64_t)255; }

int head_grid(int64_t units) {
  return (int)std::min<int64_t>(std::max<int64_t>((units + kWavesPerBlock - 1) / kWavesPerBlock, 1), 256);
}

int head_shape_status(int64_t units, int F, int H, int L) {
  if (units < 0 || F <= 0 || H <= 0 || L <= 0) return YR_ERR_BADARG;
  if (F > kDcnMaxF || H > kDcnMaxH || L > kDcnMaxL) return YR_ERR_UNSUPPORTED;
  return 0;
}

int64_t head_nacc(int F, int H, int L) { return (int64_t)(2 * L + 1) * F + H + 1; }

bool scatter_width_ok(int D) { return D == 16 || D == 32 || D == 64 || D == 128; }

struct ScatterLayout {
  int64_t cnt, start, slot, ent, sorted, T, qc, qs, hc, hs, bytes;      // byte offsets, each a multiple of 256
  ScatterLayout(int64_t n, int64_t num_items, int64_t B, int D, int64_t cat_chunks, int64_t sc_chunks) {
    int64_t at = 0;
    cnt = at;    at += up256(4 * n);
    start = at;  at += up256(4 * (n + 1));
    slot = at;   at += up256(12 * B);
    ent = at;    at += up256(12 * B);
    sorted = at; at += up256(12 * B);
    T = at;      at += up256(8 * num_items * D);
    qc = at;     at += up256(4 * cat_chunks * D);
    qs = at;     at += up256(4 * sc_chunks * D);
    hc = at;     at += up256(4 * cat_chunks);
    hs = at;     at += up256(4 * sc_chunks);
    bytes = at;
  }
};

// sizes first (BADARG), then what the kernels are not built for (UNSUPPORTED); keys are 4 b + role in an int32
int scatter_size_status(int64_t num_users, int64_t num_items, int64_t B, int D, int64_t cat_chunks, int64_t sc_chunks) {
  if (num_users <= 0 || num_items <= 0 || B < 0 || D <= 0 || cat_chunks < 0 || sc_chunks < 0) return YR_ERR_BADARG;
  if (num_users + num_items >= 0x7fffffff || cat_chunks > 0x7fffffff || sc_chunks > 0x7fffffff) return YR_ERR_BADARG;
  if (!scatter_width_ok(D) || B > (0x7fffffff >> 2)) return YR_ERR_UNSUPPORTED;
  return 0;
}

}  // namespace

extern "C" int64_t yr_dcn_owned_head_workspace_bytes(int64_t units, int F, int H, int L) {
  if (const int st = head_shape_status(units, F, H, L)) return st;
  return up256(head_grid(units) * head_nacc(F, H, L) * 4);
}

extern "C" int yr_dcn_head_ordered(const float* x0, int64_t ldx, const float* h, int64_t ldh, int64_t units, int F,
                                   int H, int L, const float* cw, const float* cb, const float* Wo, const float* bo,
                                   int bpr, float inv_batch, float* pred, const float* gpred, float* dh, int64_t lddh,
                                   float* dx0, int64_t lddx, float* dcw, float* dcb, float* dWo, float* dbo,
                                   float* loss_partials, void* workspace, int64_t workspace_bytes, void* stream) {
  if (const int st = head_shape_status(units, F, H, L)) return st;
  if (workspace_bytes < 0) return YR_ERR_BADARG;
  if (!x0 || !h || !cw || !cb || !Wo || !bo || ldx < F || ldh < H) return YR_ERR_BADARG;
  if (bpr && !loss_partials) return YR_ERR_BADARG;
  if (dx0 && (!dh || !dcw || !dcb || !dWo || !dbo || lddh < H || lddx < F || (!bpr && !gpred))) return YR_ERR_BADARG;
  const int grid = head_grid(units);
  const int64_t nacc = head_nacc(F, H, L);
  if (dx0 && (!workspace || ((uintptr_t)workspace & 3) || workspace_bytes < grid * nacc * 4)) return YR_ERR_BADARG;
  const size_t lds = dx0 ? (size_t)(kWavesPerBlock * nacc * 4) : 0;
  static bool raised = false;                  // more than the default 64 KB of dynamic LDS: once per process
  if (!raised && lds > 65536) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&dcn_head_ordered_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256);
    if (e != hipSuccess) return (int)e;
    raised = true;
  }
  DcnHead p{x0, ldx, h, ldh, units, F, H, L, cw, cb, Wo, bo, bpr, inv_batch, pred, gpred, dh, lddh, dx0, lddx,
            dcw, dcb, dWo, dbo, loss_partials};
  float* slots = static_cast<float*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(dcn_head_ordered_kernel, dim3(grid), dim3(kBlock), lds, s, p, slots);
  if (const int st = launch_status()) return st;
  if (!dx0 || units == 0) return 0;            // no unit: no term, the gradients stay as they are
  hipLaunchKernelGGL(dcn_head_reduce_kernel, dim3((unsigned)((nacc + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, slots,
                     grid, L, F, H, dcw, dcb, dWo, dbo);
  return launch_status();
}

extern "C" int64_t yr_dcn_owned_scatter_workspace_bytes(int64_t num_users, int64_t num_items, int64_t B, int D,
                                                        int64_t cat_chunks, int64_t sc_chunks) {
  if (const int st = scatter_size_status(num_users, num_items, B, D, cat_chunks, sc_chunks)) return st;
  return ScatterLayout(num_users + num_items, num_items, B, D, cat_chunks, sc_chunks).bytes;
}

extern "C" int yr_dcn_owned_assemble_bwd(const float* dx, int64_t ldx, const int32_t* cat_ids, const int32_t* sc_ids,
                                         int Lmax, int D, int64_t num_users, int64_t num_items, int64_t num_cats,
                                         int64_t num_sc, const int64_t* user, const int64_t* item_a,
                                         const int64_t* item_b, int64_t B, int attr_per_row, const int32_t* cat_ptr,
                                         const int32_t* cat_item, const int32_t* cat_mult,
                                         const int32_t* cat_chunk_ptr, int64_t cat_chunks, const int32_t* sc_ptr,
                                         const int32_t* sc_item, const int32_t* sc_chunk_ptr, int64_t sc_chunks,
                                         float* gU, float* gI, float* gC, float* gS, void* workspace,
                                         int64_t workspace_bytes, int32_t* err_flag, void* stream) {
  if (Lmax <= 0 || num_cats <= 0 || num_sc <= 0 || num_cats > 0x7fffffff || num_sc > 0x7fffffff ||
      workspace_bytes < 0)
    return YR_ERR_BADARG;
  if (const int st = scatter_size_status(num_users, num_items, B, D, cat_chunks, sc_chunks)) return st;
  if (attr_per_row) return YR_ERR_UNSUPPORTED;                                   // the triplet form only
  if (B == 0) return 0;
  if (!user || !item_a || !item_b) return YR_ERR_UNSUPPORTED;
  if (!dx || !cat_ids || !sc_ids || !cat_ptr || !cat_item || !cat_mult || !cat_chunk_ptr || !sc_ptr || !sc_item ||
      !sc_chunk_ptr || !gU || !gI || !gC || !gS || !workspace)
    return YR_ERR_BADARG;
  if (ldx < 4 * D || (ldx & 3) ||
      (((uintptr_t)dx | (uintptr_t)gU | (uintptr_t)gI | (uintptr_t)workspace) & 15))
    return YR_ERR_BADARG;
  const int64_t n = num_users + num_items;
  const ScatterLayout lay(n, num_items, B, D, cat_chunks, sc_chunks);
  if (workspace_bytes < lay.bytes) return YR_ERR_BADARG;
  char* ws = static_cast<char*>(workspace);
  int32_t* cnt = reinterpret_cast<int32_t*>(ws + lay.cnt);
  int32_t* start = reinterpret_cast<int32_t*>(ws + lay.start);
  int32_t* slot = reinterpret_cast<int32_t*>(ws + lay.slot);
  int32_t* ent = reinterpret_cast<int32_t*>(ws + lay.ent);
  int32_t* sorted = reinterpret_cast<int32_t*>(ws + lay.sorted);
  float* T = reinterpret_cast<float*>(ws + lay.T);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(cnt, 0, sizeof(int32_t) * n, s) != hipSuccess) return (int)hipGetLastError();
  const int tgrid = grid_for(B, kBlock);
  hipLaunchKernelGGL((ngcf_owned_count_kernel<true, true>), dim3(tgrid), dim3(kBlock), 0, s, user, item_a, item_b, B,
                     num_users, num_items, cnt, slot, err_flag);
  hipLaunchKernelGGL(owned_scan_kernel<false>, dim3(owned_scan_grid(n)), dim3(kBlock), 0, s, cnt, n, start,
                     (int32_t*)nullptr);
  hipLaunchKernelGGL((ngcf_owned_fill_kernel<true, true>), dim3(tgrid), dim3(kBlock), 0, s, user, item_a, item_b, B,
                     num_users, num_items, start, slot, ent);
  hipLaunchKernelGGL(ngcf_owned_rank_kernel, dim3(grid_for(3 * B, kBlock)), dim3(kBlock), 0, s, user, item_a, item_b,
                     num_users, n, start, ent, sorted);
  if (const int st = launch_status()) return st;
  DcnOwnedRows r{dx, ldx, user, item_a, item_b, B, D, Lmax, num_users, num_items, num_cats, num_sc, cat_ids, sc_ids,
                 start, sorted, gU, gI, T, err_flag};
  const int rows_per_block = kWavesPerBlock * (kWave / (D / 4));
  hipLaunchKernelGGL(dcn_owned_rows_kernel, dim3((unsigned)std::min<int64_t>((n + rows_per_block - 1) / rows_per_block,
                                                                              65536)),
                     dim3(kBlock), 0, s, r);
  if (const int st = launch_status()) return st;
  DcnOwnedAttr a{};
  a.cat = DcnAttrList{cat_ptr, cat_item, cat_mult, cat_chunk_ptr, num_cats, cat_chunks,
                      reinterpret_cast<float*>(ws + lay.qc), reinterpret_cast<int32_t*>(ws + lay.hc), gC};
  a.sc = DcnAttrList{sc_ptr, sc_item, nullptr, sc_chunk_ptr, num_sc, sc_chunks, reinterpret_cast<float*>(ws + lay.qs),
                     reinterpret_cast<int32_t*>(ws + lay.hs), gS};
  a.cnt_items = cnt + num_users;
  a.T = T;
  a.num_items = num_items;
  a.D = D;
  a.Lmax = (float)Lmax;
  if (cat_chunks + sc_chunks > 0) {
    hipLaunchKernelGGL(dcn_owned_chunk_kernel, dim3(grid_for((cat_chunks + sc_chunks) * D, kBlock)), dim3(kBlock), 0,
                       s, a);
    hipLaunchKernelGGL(dcn_owned_attr_rows_kernel, dim3(grid_for((num_cats + num_sc) * D, kBlock)), dim3(kBlock), 0, s,
                       a);
  }
  return launch_status();
}
