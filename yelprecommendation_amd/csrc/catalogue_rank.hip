// Full-catalogue ranks of EVERY held-out item of a user for gfx950 (MI355X): what the reference's evaluation
// (trainers/mf_trainer.py:134-178, metric.py) needs from a score row — the places of the `actual` items in the masked,
// sorted prediction — counted in one sweep of the catalogue, for any cutoff k at once (csrc/metrics.hip,
// yr_metrics_from_ranks, turns them into precision / recall / MAP / NDCG / HR @k, MRR and AUC).
//
//   s(u, i)  = sum_l <Ul[u], Il[i]>         one f32 accumulator started at 0, layers ascending, k ascending inside a
//                                           layer, v_mfma_f32_32x32x2_f32 (rank_tile_add, s3rec_cb.h): MF is L = 1;
//                                           NGCF passes layer l as (E_l, E_l + num_users D) — the order
//                                           ngcf_eval_topk_kernel documents
//   list order of row n: unmasked items by (score descending, id ascending), then the masked items by id ascending
//                        (the reference's pred[mask] = -3.40282e+38 under the project's tie rule)
//   rank[e]  = the 0-based place of target pos_idx[e] of row n in that order:
//              unmasked target t:  #{ unmasked i != t : s_i > s_t  or  (s_i == s_t and i < t) }
//              masked target t:    #unmasked items + #{ masked ids below t }
//
// The geometry is s3rec_rank_kernel's (csrc/s3rec_rank.hip, s3rec_cb.h): a wave OWNS 32 rows as the B operand and
// SWEEPS 32-item tiles read 16 bytes per lane; a workgroup is (row tile, chunk of kSweepColChunk items), its four waves
// take kSweepTilesPerWave tiles each.  An owned row is a SLOT: a row of `users` with up to kCrCap of its targets.  A
// row with more targets takes several slots, so only such rows repeat matrix work.  Four launches:
//   cr_slots_kernel    rows -> slots (an integer scan of ceil(len / kCrCap))
//   cr_targets_kernel  the targets' scores from the SAME tile function as the swept scores (the diagonal of a tile
//                      whose swept rows are the slots' c-th targets), then every slot's targets sorted best first by
//                      (score, id) — a row of the item table bit-identical to a target's row ties with it exactly
//   cr_sweep_kernel    every unmasked item of the chunk finds the first target of the slot it is ahead of (one compare
//                      against the slot's worst target settles most; one against the best the next; else a binary search
//                      of the slot's list in LDS) and bumps that target's integer bin
//   cr_finish_kernel   rank = the bins up to the target's place, summed over the chunks; the masked targets' formula
// A target is an item like any other to the other targets' counts; it never counts itself because its id is not below
// its id and its score, from the same instructions, is not above its score — excluded by id, never by score.
// Integers only: lanes of a slot by a shuffle (bin 0) and LDS integer adds, waves by LDS integer adds, chunks by
// per-chunk partial bins in the workspace that cr_finish_kernel adds.  Every sum is exact, so a rank does not depend on
// N, on the row's place in the batch, on the other rows or on the grid; no float atomics; no [N][items] array.
// Outside the contract (no pipeline produces them): non-finite scores, duplicate entries inside one pos row, duplicate
// or descending entries inside one mask row.  They give unspecified ranks, never an out-of-bounds access.
#include <algorithm>

#include "s3rec_cb.h"

namespace yr {

constexpr int kCrCap = YR_CATALOGUE_RANK_CAP;      // targets per slot
constexpr int kCrPitch = kCrCap + 1;               // LDS row pitch of a slot's list: lanes of a wave on distinct banks
constexpr int kCrHead = 64;                        // words in front of the workspace arrays ([0]: the slot count)
static_assert(kSweepTile * kCrCap % kBlock == 0, "the list passes take whole rounds of the workgroup");

struct CatRank {
  LayerPtrs user, item;       // L pairs of tables, [num_users][E] and [num_items][E]
  int L;
  const int64_t *users, *pos_ptr, *pos_idx, *mask_ptr, *mask_idx;   // mask_ptr null: nothing masked
  int64_t N, nnz, num_users, num_items, chunks, max_slots;
  int32_t* head;              // [kCrHead]; [0] = slots in use
  int32_t* slot_row;          // [max_slots] the row of `users` a slot belongs to
  int32_t* slot_part;         // [max_slots] which kCrCap entries of the row's targets it holds
  float* tgt_score;           // [max_slots][kCrCap] the slot's targets best first; entries without a target last
  int32_t* tgt_id;            // [max_slots][kCrCap] their ids, -1 for an entry without a (valid) target
  int32_t* tgt_place;         // [max_slots][kCrCap] entry c of the slot (pos order) -> its place in the sorted list
  int32_t* part;              // [chunks][max_slots][kCrCap] the bins of one chunk
  int64_t* rank;              // [nnz]
  float* target_score;        // [nnz] or null
  int32_t* err_flag;
};

// x = (score s, id i) is ahead of target (ts, ti) in the list order
__device__ __forceinline__ bool cr_ahead(float s, int i, float ts, int ti) { return s > ts || (s == ts && i < ti); }

// One workgroup: thread t takes a contiguous share of the rows, the shares' slot counts are scanned in LDS.
__global__ __launch_bounds__(kBlock) void cr_slots_kernel(CatRank p) {
  __shared__ int64_t sBase[kBlock];
  const int tid = threadIdx.x;
  const int64_t per = (p.N + kBlock - 1) / kBlock;
  const int64_t lo = std::min<int64_t>(tid * per, p.N), hi = std::min<int64_t>(lo + per, p.N);
  int64_t cnt = 0;
  for (int64_t n = lo; n < hi; ++n) {
    const int64_t len = p.pos_ptr[n + 1] - p.pos_ptr[n];
    if (len > 0) cnt += (len + kCrCap - 1) / kCrCap;
  }
  sBase[tid] = cnt;
  __syncthreads();
  if (tid == 0) {
    int64_t run = 0;
    for (int t = 0; t < kBlock; ++t) {
      const int64_t c = sBase[t];
      sBase[t] = run;
      run += c;
    }
    p.head[0] = (int32_t)std::min<int64_t>(run, p.max_slots);   // (more than max_slots: pos_ptr disagrees with nnz)
  }
  __syncthreads();
  int64_t s = sBase[tid];
  for (int64_t n = lo; n < hi; ++n) {
    const int64_t len = p.pos_ptr[n + 1] - p.pos_ptr[n];
    for (int64_t q = 0; q * kCrCap < len; ++q, ++s) {
      if (s >= p.max_slots) return;
      p.slot_row[s] = (int32_t)n;
      p.slot_part[s] = (int32_t)q;
    }
  }
}

// acc[q] in lane j = s(user of owned slot j, swept item cb_acc_row(q, lane)): `own` is the owned row of the single
// table (LAYERED false: in registers for the whole unit); with layers the owned half rows are read again per layer —
// 32 rows per table that stay in the cache, E / 8 loads beside the swept rows' E / 8
template <int E, bool LAYERED>
__device__ __forceinline__ f32x16 cr_tile(const CatRank& p, int64_t item, bool item_ok, const float (&own)[E / 2],
                                          int64_t user, bool user_ok, int hh) {
  if constexpr (!LAYERED) {
    return rank_tile<E>(p.item.p[0] + item * E + 4 * hh, item_ok, own);
  } else {
    f32x16 acc = zero16();
    for (int l = 0; l < p.L; ++l) {
      float o[E / 2];
      rank_own<E>(o, p.user.p[l] + user * E + 4 * hh, user_ok);
      acc = rank_tile_add<E>(acc, p.item.p[l] + item * E + 4 * hh, item_ok, o);
    }
    return acc;
  }
}

// the slot of a lane: its row, its user id (0 with ok false: nothing of the user tables is read) and its targets
struct CrSlot {
  int64_t row, user, off0;    // off0: the slot's first entry of pos_idx
  int m;                      // entries in use, 0 .. kCrCap
  bool ok, user_ok;
};

__device__ __forceinline__ CrSlot cr_slot(const CatRank& p, int64_t slot, int64_t n_slots) {
  CrSlot s{0, 0, 0, 0, slot < n_slots, false};
  if (s.ok) {
    s.row = p.slot_row[slot];
    const int64_t u = p.users[s.row];
    s.user_ok = u >= 0 && u < p.num_users;
    s.user = s.user_ok ? u : 0;
    s.off0 = p.pos_ptr[s.row] + (int64_t)p.slot_part[slot] * kCrCap;
    s.m = (int)std::min<int64_t>(std::max<int64_t>(p.pos_ptr[s.row + 1] - s.off0, 0), kCrCap);
  }
  return s;
}

template <int E, bool LAYERED>
__global__ __launch_bounds__(kBlock, E <= 64 ? 2 : 1) void cr_targets_kernel(CatRank p) {
  __shared__ float sS[kSweepTile * kCrPitch];
  __shared__ int32_t sI[kSweepTile * kCrPitch];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int r = lane & 31, hh = lane >> 5;
  const int64_t n_slots = p.head[0], units = (n_slots + kSweepTile - 1) / kSweepTile;
  int flag = 0;

  for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const CrSlot s = cr_slot(p, unit * kSweepTile + r, n_slots);
    if (s.ok && !s.user_ok) flag |= YR_FLAG_BAD_USER;
    float own[E / 2];
    if constexpr (!LAYERED) rank_own<E>(own, p.user.p[0] + s.user * E + 4 * hh, s.user_ok);

    // tile c: lane r sweeps the c-th target of slot r; the waves take c = wave, wave + 4, ...
    for (int c = wave; c < kCrCap; c += kWavesPerBlock) {
      int64_t t = -1;
      if (c < s.m) {
        const int64_t off = s.off0 + c;
        if (off >= 0 && off < p.nnz) t = p.pos_idx[off];
        if (t < 0 || t >= p.num_items) {
          flag |= YR_FLAG_BAD_ITEM;
          t = -1;
        }
        if (!s.user_ok) t = -1;
      }
      const float ts = rank_diagonal(cr_tile<E, LAYERED>(p, t >= 0 ? t : 0, t >= 0, own, s.user, s.user_ok, hh), lane);
      if (hh == 0) {
        sS[r * kCrPitch + c] = t >= 0 ? ts : 0.0f;
        sI[r * kCrPitch + c] = (int32_t)t;
      }
    }
    __syncthreads();

    // every slot's entries to their places: best first by (score, id); entries without a target last, in pos order.
    // The entry's own index decides last, so the places of a slot are a permutation whatever the ids
    for (int e = tid; e < kSweepTile * kCrCap; e += kBlock) {
      const int sl = e / kCrCap, c = e - sl * kCrCap;
      const int64_t slot = unit * kSweepTile + sl;
      const float sc = sS[sl * kCrPitch + c];
      const int id = sI[sl * kCrPitch + c];
      int place = 0;
#pragma unroll
      for (int c2 = 0; c2 < kCrCap; ++c2) {
        const float s2 = sS[sl * kCrPitch + c2];
        const int id2 = sI[sl * kCrPitch + c2];
        bool ahead;
        if (id2 < 0 || id < 0) ahead = id2 >= 0 || (id < 0 && c2 < c);
        else ahead = s2 > sc || (s2 == sc && (id2 < id || (id2 == id && c2 < c)));
        place += (int)(ahead && c2 != c);
      }
      if (slot < n_slots) {
        p.tgt_score[slot * kCrCap + place] = sc;
        p.tgt_id[slot * kCrCap + place] = id;
        p.tgt_place[slot * kCrCap + c] = place;
      }
    }
    __syncthreads();                                  // the next unit overwrites sS / sI
  }
  if (flag && p.err_flag) atomicOr(p.err_flag, flag);
}

template <int E, bool LAYERED>
__global__ __launch_bounds__(kBlock, E <= 64 ? 2 : 1) void cr_sweep_kernel(CatRank p) {
  __shared__ float sS[kSweepTile * kCrPitch];
  __shared__ int32_t sI[kSweepTile * kCrPitch];
  __shared__ int32_t sB[kSweepTile * kCrPitch];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int r = lane & 31, hh = lane >> 5;
  const int64_t n_slots = p.head[0];
  const int64_t units = (n_slots + kSweepTile - 1) / kSweepTile * p.chunks;
  const int64_t col_tiles = (p.num_items + kSweepTile - 1) / kSweepTile;

  for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int64_t ot = unit / p.chunks, chunk = unit - ot * p.chunks;
    const int64_t slot0 = ot * kSweepTile;
    for (int e = tid; e < kSweepTile * kCrCap; e += kBlock) {
      const int sl = e / kCrCap, c = e - sl * kCrCap;
      const bool ok = slot0 + sl < n_slots;
      sS[sl * kCrPitch + c] = ok ? p.tgt_score[(slot0 + sl) * kCrCap + c] : 0.0f;
      sI[sl * kCrPitch + c] = ok ? p.tgt_id[(slot0 + sl) * kCrCap + c] : -1;
      sB[sl * kCrPitch + c] = 0;
    }
    const CrSlot s = cr_slot(p, slot0 + r, n_slots);
    float own[E / 2];
    if constexpr (!LAYERED) rank_own<E>(own, p.user.p[0] + s.user * E + 4 * hh, s.user_ok);

    const int64_t t_begin = chunk * (kSweepColChunk / kSweepTile) + (int64_t)wave * kSweepTilesPerWave;
    const int64_t t_end = std::min<int64_t>(t_begin + kSweepTilesPerWave, col_tiles);
    int64_t cur = 0, end = 0;                         // the cursor over the row's mask list
    if (s.ok && p.mask_ptr) {
      end = p.mask_ptr[s.row + 1];
      cur = cb_lower_bound(p.mask_idx, p.mask_ptr[s.row], end, t_begin * kSweepTile);
    }
    __syncthreads();                                  // the lists are staged, the bins zero

    // the slot's valid targets are its first m entries; the best and the worst of them stay in registers
    const float* lS = sS + r * kCrPitch;
    const int32_t* lI = sI + r * kCrPitch;
    int m = 0;
#pragma unroll
    for (int c = 0; c < kCrCap; ++c) m += (int)(lI[c] >= 0);
    const float best_s = lS[0], worst_s = lS[m > 0 ? m - 1 : 0];
    const int best_i = lI[0], worst_i = lI[m > 0 ? m - 1 : 0];

    int32_t cnt0 = 0;                                 // bin 0: ahead of the slot's best target
    for (int64_t t = t_begin; t < t_end; ++t) {
      const int64_t i0 = t * kSweepTile, i = i0 + r;  // the lane's swept item
      const bool swp_ok = i < p.num_items;
      const uint32_t excl = cb_mask(p.mask_idx, cur, end, i0);
      const uint32_t cand =
          m > 0 ? low_bits((int)std::min<int64_t>(p.num_items - i0, kSweepTile)) & ~excl : 0u;
      const f32x16 acc = cr_tile<E, LAYERED>(p, swp_ok ? i : 0, swp_ok, own, s.user, s.user_ok, hh);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int ri = cb_acc_row(q, lane);
        const int id = (int)i0 + ri;
        const float sc = acc[q];
        if (((cand >> ri) & 1u) == 0 || !cr_ahead(sc, id, worst_s, worst_i)) continue;   // ahead of no target
        if (cr_ahead(sc, id, best_s, best_i)) {
          ++cnt0;
          continue;
        }
        int lo = 1, hi = m - 1;                       // not ahead of entry 0, ahead of entry m - 1
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (cr_ahead(sc, id, lS[mid], lI[mid])) hi = mid;
          else lo = mid + 1;
        }
        atomicAdd(&sB[r * kCrPitch + lo], 1);
      }
    }
    cnt0 += __shfl_xor(cnt0, 32, kWave);
    if (hh == 0 && cnt0) atomicAdd(&sB[r * kCrPitch], cnt0);
    __syncthreads();
    for (int e = tid; e < kSweepTile * kCrCap; e += kBlock) {
      const int sl = e / kCrCap, c = e - sl * kCrCap;
      if (slot0 + sl < n_slots) p.part[(chunk * p.max_slots + slot0 + sl) * kCrCap + c] = sB[sl * kCrPitch + c];
    }
    __syncthreads();                                  // the next unit restages the lists
  }
}

// one thread per (slot, entry): the entry's rank from the bins up to its place, or the masked target's formula
__global__ __launch_bounds__(kBlock) void cr_finish_kernel(CatRank p) {
  const int64_t n_slots = p.head[0], total = n_slots * kCrCap;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += stride) {
    const int64_t slot = e / kCrCap;
    const int c = (int)(e - slot * kCrCap);
    const int64_t row = p.slot_row[slot];
    const int64_t off = p.pos_ptr[row] + (int64_t)p.slot_part[slot] * kCrCap + c;
    if (off >= p.pos_ptr[row + 1] || off < 0 || off >= p.nnz) continue;
    const int place = p.tgt_place[e];
    const int64_t id = p.tgt_id[slot * kCrCap + place];
    int64_t rank = -1;
    float score = 0.0f;
    if (id >= 0) {
      score = p.tgt_score[slot * kCrCap + place];
      int64_t mb = 0, me = 0, k = 0;
      if (p.mask_ptr) {
        mb = p.mask_ptr[row];
        me = p.mask_ptr[row + 1];
        k = cb_lower_bound(p.mask_idx, mb, me, id);
      }
      if (k < me && p.mask_idx[k] == id) {            // masked: after every unmasked item, by id among the masked
        const int64_t k0 = cb_lower_bound(p.mask_idx, mb, me, 0);
        const int64_t k1 = cb_lower_bound(p.mask_idx, mb, me, p.num_items);
        rank = p.num_items - (k1 - k0) + (k - k0);
      } else {
        rank = 0;
        for (int64_t ch = 0; ch < p.chunks; ++ch) {
          const int32_t* bins = p.part + (ch * p.max_slots + slot) * kCrCap;
          for (int j = 0; j <= place; ++j) rank += bins[j];
        }
      }
    }
    p.rank[off] = rank;
    if (p.target_score) p.target_score[off] = score;
  }
}

}  // namespace yr

using namespace yr;

static bool cr_width_ok(int D) { return D == 16 || D == 32 || D == 64 || D == 128; }

static int64_t cr_chunks(int64_t num_items) { return (num_items + kSweepColChunk - 1) / kSweepColChunk; }

// sum over the rows of ceil(len / kCrCap) <= (rows with a target) + nnz / kCrCap
static int64_t cr_max_slots(int64_t nrows, int64_t nnz) { return std::min(nrows, nnz) + nnz / kCrCap; }

static int cr_check(int64_t nrows, int64_t nnz, int64_t num_items, int n_layers, int D) {
  if (nrows < 0 || nnz < 0 || num_items < 0 || D <= 0) return YR_ERR_BADARG;
  if (n_layers < 1 || n_layers > YR_NGCF_MAX_LAYERS) return YR_ERR_BADARG;
  if (!cr_width_ok(D)) return YR_ERR_UNSUPPORTED;
  // rows, slots and item ids are 32-bit words of the workspace
  if (nrows > 0x7fffffff || num_items > 0x7fffffff - kSweepTile || cr_max_slots(nrows, nnz) > 0x7fffffff / kCrCap)
    return YR_ERR_UNSUPPORTED;
  return 0;
}

static int64_t cr_words(int64_t nrows, int64_t nnz, int64_t num_items) {
  const int64_t slots = cr_max_slots(nrows, nnz);
  return kCrHead + slots * (2 + 3 * kCrCap) + cr_chunks(num_items) * slots * kCrCap;
}

extern "C" int64_t yr_catalogue_ranks_workspace_bytes(int64_t nrows, int64_t nnz, int64_t num_items, int n_layers,
                                                      int D) {
  if (const int bad = cr_check(nrows, nnz, num_items, n_layers, D)) return bad;
  return cr_words(nrows, nnz, num_items) * (int64_t)sizeof(int32_t);
}

template <int E>
static void cr_launch(const CatRank& p, dim3 tgrid, dim3 sgrid, hipStream_t st) {
  if (p.L == 1) {
    hipLaunchKernelGGL((cr_targets_kernel<E, false>), tgrid, dim3(kBlock), 0, st, p);
    hipLaunchKernelGGL((cr_sweep_kernel<E, false>), sgrid, dim3(kBlock), 0, st, p);
  } else {
    hipLaunchKernelGGL((cr_targets_kernel<E, true>), tgrid, dim3(kBlock), 0, st, p);
    hipLaunchKernelGGL((cr_sweep_kernel<E, true>), sgrid, dim3(kBlock), 0, st, p);
  }
}

extern "C" int yr_catalogue_ranks(const float* const* user_layers, const float* const* item_layers, int n_layers, int D,
                                  const int64_t* users, int64_t nrows, int64_t num_users, int64_t num_items,
                                  const int64_t* pos_ptr, const int64_t* pos_idx, int64_t nnz, const int64_t* mask_ptr,
                                  const int64_t* mask_idx, int64_t* rank, float* target_score, void* workspace,
                                  int64_t workspace_bytes, int32_t* err_flag, void* stream) {
  if (num_users < 0 || workspace_bytes < 0) return YR_ERR_BADARG;
  if (const int bad = cr_check(nrows, nnz, num_items, n_layers, D)) return bad;
  if (nrows == 0 || nnz == 0) return 0;
  if (num_users == 0 || num_items == 0) return YR_ERR_BADARG;        // targets, and no table to score them in
  if (!user_layers || !item_layers || !users || !pos_ptr || !pos_idx || !rank || !workspace) return YR_ERR_BADARG;
  if ((mask_ptr == nullptr) != (mask_idx == nullptr)) return YR_ERR_BADARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 3) != 0) return YR_ERR_BADARG;
  if (workspace_bytes < cr_words(nrows, nnz, num_items) * (int64_t)sizeof(int32_t)) return YR_ERR_BADARG;
  CatRank p{};
  for (int l = 0; l < n_layers; ++l) {
    if (!user_layers[l] || !item_layers[l]) return YR_ERR_BADARG;
    if (((reinterpret_cast<uintptr_t>(user_layers[l]) | reinterpret_cast<uintptr_t>(item_layers[l])) & 15) != 0)
      return YR_ERR_BADARG;
    p.user.p[l] = user_layers[l];
    p.item.p[l] = item_layers[l];
  }
  p.L = n_layers;
  p.users = users; p.pos_ptr = pos_ptr; p.pos_idx = pos_idx; p.mask_ptr = mask_ptr; p.mask_idx = mask_idx;
  p.N = nrows; p.nnz = nnz; p.num_users = num_users; p.num_items = num_items;
  p.chunks = cr_chunks(num_items);
  p.max_slots = cr_max_slots(nrows, nnz);
  int32_t* w = static_cast<int32_t*>(workspace);
  p.head = w;                                   w += kCrHead;
  p.slot_row = w;                               w += p.max_slots;
  p.slot_part = w;                              w += p.max_slots;
  p.tgt_score = reinterpret_cast<float*>(w);    w += p.max_slots * kCrCap;
  p.tgt_id = w;                                 w += p.max_slots * kCrCap;
  p.tgt_place = w;                              w += p.max_slots * kCrCap;
  p.part = w;
  p.rank = rank; p.target_score = target_score; p.err_flag = err_flag;

  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cr_slots_kernel, dim3(1), dim3(kBlock), 0, st, p);
  if (const int s = launch_status()) return s;
  // the slot count stays on the device: the grids are sized for max_slots and the kernels' loops end at the count
  const int64_t tiles = (p.max_slots + kSweepTile - 1) / kSweepTile;
  const dim3 tgrid((unsigned)std::min<int64_t>(tiles, kSweepGridMax));
  const dim3 sgrid((unsigned)std::min<int64_t>(tiles * p.chunks, kSweepGridMax));
  switch (D) {
    case 16: cr_launch<16>(p, tgrid, sgrid, st); break;
    case 32: cr_launch<32>(p, tgrid, sgrid, st); break;
    case 64: cr_launch<64>(p, tgrid, sgrid, st); break;
    default: cr_launch<128>(p, tgrid, sgrid, st); break;
  }
  if (const int s = launch_status()) return s;
  hipLaunchKernelGGL(cr_finish_kernel, dim3(grid_for(p.max_slots * kCrCap, kBlock)), dim3(kBlock), 0, st, p);
  return launch_status();
}
