// Pull-based BPR-MF training step for gfx950 (MI355X): no float atomics, no global integer
// atomics, no gradient buffers — the whole reference step
//   2 x forward, BPRLoss, loss.backward() (embedding_dense_backward), Adam.step()
//   (reference trainers/mf_trainer.py:106-112, trainers/base_trainer.py:34-36)
// in THREE launches: tile partition -> owner pass over the USER rows -> owner pass over the ITEM rows.
//
// Why pull: the push form (csrc/bpr_mf.hip) is capped by the memory-side float-atomic rate
// (~1.3 TB/s of added bytes, 3 rows per triplet).  Here every destination row is owned by one
// lane group of one workgroup, which PULLS the partner rows it needs with plain 16-byte loads, sums
// them in registers, applies Adam to its own row and writes it once.  Dense-Adam semantics are
// kept: every row of both tables is visited every step, rows without contributions get grad = 0
// (their m/v still decay).
//
// Rows are cut into buckets of R = 1024/D consecutive rows (4 KB of table: one 256-thread owner
// workgroup, one row per lane group of D/4 lanes).
//   1  tile_partition_kernel   a workgroup takes one TILE of the batch (1024..8192 triplets) and one
//        side (user / item), counting-sorts the tile by destination bucket in LDS (integer LDS
//        atomics give the rank inside (tile, bucket)) and writes the records into the tile's OWN
//        region of the record array, bucket by bucket, plus the tile's bucket offsets
//          rec[tile]  = {pos, neg, triplet id b, local user row}            (16 B, by user bucket)
//          occ[tile]  = {user | local item row << 26, b | sign}              ( 8 B, by item bucket,
//                                                       one per pos / neg occurrence)
//        A tile's region is written by one workgroup only: no global atomics, no count/scan passes,
//        no partial lines shared between workgroups.
//   2  owner_pass_kernel<USER>  the owner of bucket k reads segment k of every tile (offsets ->
//        LDS prefix, flattened index -> (tile, position) by binary search), ranks the records by
//        local row with LDS integer atomics and so gets ONE stream sorted by row in LDS.  A row is finished by one
//        lane group of one wave (its SLOT, wave * RPW + group; a wave finishes RPW rows and keeps their running sums
//        in registers).  Which slot takes which row is dealt by load once the first chunk's counts are known
//        (deal_rows: longest row first to the least-loaded wave) and kept for the bucket; the stream is laid out in
//        slot order and wave w walks the records of ITS slots, GPW records per step (one per lane group), several
//        steps in flight: x_b = U[u].(I[p_b]-I[n_b]); loss += softplus(-x_b); g_b = -sigmoid(-x_b)/B;
//        cur += g_b (I[p_b]-I[n_b]); coeff[b] = g_b (4 B per triplet for the item side).  When a lane group's row
//        changes, the groups closing that row combine their sums with shuffles and the row's slot adds the result
//        to its register total (no atomics anywhere).  A row with more than YR_HEAVY_ROW records in a chunk is
//        walked by all four waves together, their partial sums meet in LDS in wave order.  More than kCap records
//        per bucket: further chunks into the same totals.  Finally each lane group applies Adam to the row it was
//        dealt: U_new[u] = Adam(U[u], acc).
//   3  owner_pass_kernel<ITEM>  the same over the item buckets: {user, (+/-) coeff[b]} per
//        occurrence, acc = sum g * U_old[user], I[i] = Adam(I[i], acc) (or the dense gradient rows
//        for the multi-GPU all-reduce); workgroup 0 also reduces the loss partials of launch 2
//        (fixed order) into the step loss and the running epoch loss.
//        Item buckets far above the average are shared between workgroups: by tile range with a combine (oversize
//        buckets, see kSplitMin) or, below that, by ROW without one (heavy buckets, see YR_ROWSPLIT).
// The user table is double-buffered (U -> U_new) because the item pass needs the OLD user rows;
// the item table is updated in place (a row is read only by its own lane group).
//
// Layout: a row of D floats sits on LPR = D/4 lanes as float4 (16-byte loads/stores); a wave
// works on GPW = 64/LPR contributions at once; the per-contribution dot product is a reduction
// over LPR lanes only.  At the end a wave holds GPW rows of its bucket, one per lane group: own row,
// m, v and the Adam update stream 256 B per lane group and instruction.
#include "adam.h"
#include "common.h"
#include "pull_placement.h"

namespace yr {

constexpr int kPartThreads = 1024;              // partition workgroup
#ifndef YR_ITEM_CAP
#define YR_ITEM_CAP 1024
#endif
constexpr int kCap = YR_ITEM_CAP;                      // records an owner workgroup sorts per chunk (item side)
constexpr int kUserCap = 768;                   // user side (12 B of LDS per record instead of 8)
constexpr int kTileGroup = 256;                 // tiles whose segment descriptors an owner holds at once
constexpr int kOccShift = 26;                   // occ.x = user | local item row << 26
constexpr int kOccMask = (1 << kOccShift) - 1;
constexpr int kMaxBuckets = 16383;              // (buckets + 1) * 4 B of dynamic LDS <= 64 KB
constexpr int kMaxOwnerGrid = 4096;
// which owner workgroup takes which bucket: owner_slots / owner_bucket of pull_placement.h
static_assert(kMaxOwnerGrid % kXcdRound == 0 && YR_LOSS_PARTIALS % kXcdRound == 0,
              "a capped grid strides by whole rounds of runs: ks += owners keeps owner_bucket a bijection");
#ifndef YR_HEAVY_ROW
#define YR_HEAVY_ROW 96
#endif
constexpr int kHeavyRow = YR_HEAVY_ROW;          // records per row and chunk from which all four waves share the row
// Oversize item buckets (a few rows that take several per cent of a batch: one workgroup would walk them chunk after
// chunk, 1.3 ms at 2^20 triplets): the bucket's tiles are shared out between `parts` workgroups — the owner and
// parts - 1 helpers —, each leaves the partial sums of its tile range in a scratch slot, the LAST to arrive adds
// the slots in part order (a fixed order: the deterministic mode survives) and applies Adam.
#ifndef YR_SPLIT_MIN
#define YR_SPLIT_MIN 2048
#endif
constexpr int kSplitMin = YR_SPLIT_MIN;          // records of a bucket from which it is split
#ifndef YR_SPLIT_AVG_MIN
#define YR_SPLIT_AVG_MIN 2.5
#endif
#ifndef YR_SPLIT_AVG_TARGET
#define YR_SPLIT_AVG_TARGET 1.25
#endif
#ifndef YR_SPLIT_TARGET
#define YR_SPLIT_TARGET 1024
#endif
constexpr int kSplitTarget = YR_SPLIT_TARGET;    // records per part (one chunk of the item pass)
constexpr int kMaxParts = 64;
constexpr int kMaxTasks = 512;                   // helper workgroups at the front of the item pass's grid
static_assert(kMaxTasks % 8 == 0, "the owners behind the helpers keep slot % 8 == blockIdx.x % 8 (owner_bucket)");
constexpr int kMaxSlots = 1024;                  // scratch slots of 1024 floats (one bucket's rows)
// Heavy item buckets below that size (a few hundred buckets of two to three times the average one, whose owners end
// the item pass long after the rest): the bucket's ROWS are shared out between S = 2 or 4 workgroups, the owner
// (part 0) and S - 1 row helpers.  Part q finishes the local rows r with (r & (S - 1)) == q: every part reads the
// whole bucket, drops the records of the other parts' rows while it loads them, and updates its own rows.  The parts
// write disjoint rows: no scratch slot, no arrival counter, no fence, no atomic.
#ifndef YR_ROWSPLIT
#define YR_ROWSPLIT 1                 // 0: compiled out (no bucket is split by row, no row helper in the grid)
#endif
#ifndef YR_ROWSPLIT_MIN
#define YR_ROWSPLIT_MIN 1024
#endif
#ifndef YR_ROWSPLIT_AVG_MIN
#define YR_ROWSPLIT_AVG_MIN 2.32
#endif
#ifndef YR_ROWSPLIT_TARGET
#define YR_ROWSPLIT_TARGET 512
#endif
#ifndef YR_ROWSPLIT_AVG_TARGET
#define YR_ROWSPLIT_AVG_TARGET 1.16
#endif
constexpr int kRowSplitMin = YR_ROWSPLIT_MIN;        // records of a bucket from which its rows are shared out
constexpr int kRowSplitTarget = YR_ROWSPLIT_TARGET;  // records per row part
constexpr int kMaxRowTasks = YR_ROWSPLIT ? 512 : 0;  // entries of the row-task list (served by the free helper workgroups)
constexpr int kBuildLanes = 4;                   // lanes that share one item bucket in the sizing workgroups of the USER pass
#ifndef YR_DEAL
#define YR_DEAL 1                     // 0: wave w finishes rows [w RPW, (w + 1) RPW) of its bucket (measurement only)
#endif
#ifndef YR_DEAL_MIN
#define YR_DEAL_MIN 256
#endif
constexpr int kDealMin = YR_DEAL_MIN;            // records in a bucket's first chunk from which its rows are dealt (at R = 16)
#ifndef YR_OWNER_WAVES
#define YR_OWNER_WAVES 8              // waves per SIMD the owner pass is compiled for (8 workgroups per CU: <= 64 VGPRs)
#endif
#ifndef YR_USER_UNROLL
#define YR_USER_UNROLL 1
#endif
#ifndef YR_ITEM_UNROLL
#define YR_ITEM_UNROLL 2
#endif
constexpr int kUserUnroll = YR_USER_UNROLL;   // steps in flight per lane group; two gathered rows per contribution
constexpr int kItemUnroll = YR_ITEM_UNROLL;

struct PullAdam {
  AdamScalars c;
  int decoupled;               // AdamW: a run-time value here, one set of owner-pass kernels for both
};

// row gathers: uniform base + 32-bit element offset (a table holds at most 16383 buckets x 1024
// floats), so the address stays one VGPR next to an SGPR pair
__device__ __forceinline__ float4 ld4o(const float* base, uint32_t off) {
  return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(base) + (uint32_t)(off * 4u));
}

template <int D>
struct PullGeom {
  static_assert(D == 16 || D == 32 || D == 64 || D == 128, "unsupported width");
  static constexpr int LPR = D / 4;              // lanes per row (float4 each)
  static constexpr int GPW = kWave / LPR;        // lane groups (= contributions per pass) per wave
  static constexpr int R = kWavesPerBlock * GPW; // rows per bucket = 1024 / D (a wave owns GPW rows)
};
// A table with few rows and many contributions per row (a rank's user shard of an 8-GPU run: 3,959 rows,
// 133 triplets per row and step) would leave most CUs without a bucket: then a wave owns ONE row and a
// bucket is 4 rows (kNarrowRows), four times the workgroups.
#ifndef YR_MIN_TILES
#define YR_MIN_TILES 64
#endif
constexpr int kMinTiles = YR_MIN_TILES;
constexpr int kNarrowRows = kWavesPerBlock;
constexpr int kNarrowShift = 2;
#ifndef YR_NARROW_BELOW
#define YR_NARROW_BELOW 768
#endif
constexpr int kNarrowBelow = YR_NARROW_BELOW;                // ... when there would be fewer 1024/D-row buckets than this

inline int bucket_shift(int D) { return D == 16 ? 6 : D == 32 ? 5 : D == 64 ? 4 : 3; }

// --------------------------------------------------------------------------- 1: tile partition
// grid (tiles, 2): blockIdx.y = 0 sorts the tile's triplets by user bucket, 1 its 2 x TILE item
// occurrences by item bucket.  off[tile][0..nb] = start of every bucket inside the tile's region.
template <int PT>
__global__ __launch_bounds__(kPartThreads) void tile_partition_kernel(
    const int64_t* __restrict__ user, const int64_t* __restrict__ pos, const int64_t* __restrict__ neg, int64_t B,
    int64_t nU, int64_t nI, int shiftU, int shiftI, int nbU, int nbI, int32_t* __restrict__ offU,
    int32_t* __restrict__ offI,
    int4* __restrict__ rec, int2* __restrict__ occ, int32_t* __restrict__ err_flag, int stage_off,
    int32_t* __restrict__ split_counters) {
  extern __shared__ int32_t s_cnt[];            // [nb + 1] bucket counters, then (16-byte aligned) the staged tile
  __shared__ int s_wave[kPartThreads / kWave];
  int4* s_stage = reinterpret_cast<int4*>(s_cnt + stage_off);   // TILE records of 16 B, or 2 TILE of 8 B
  constexpr int TILE = kPartThreads * PT;
  const int side = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  // the split block of this batch starts clean: no tasks, no slots, every item bucket whole (the user pass's sizing
  // workgroups overwrite it; an item pass run without them must not meet the previous batch's parts)
  if (side == 0 && tile == 0) {
    if (tid < 3) split_counters[tid] = 0;     // tasks, slots, row tasks
    for (int i = tid; i < nbI; i += kPartThreads) split_counters[4 + i] = 1;
  }
  const int nb = side ? nbI : nbU;
  const int shift = side ? shiftI : shiftU;
  const int rmask = (1 << shift) - 1;

  int32_t u[PT], p[PT], n[PT];
  int bad = 0;
#pragma unroll
  for (int k = 0; k < PT; ++k) {
    const int64_t b = (int64_t)tile * TILE + (int64_t)k * kPartThreads + tid;
    u[k] = -1; p[k] = 0; n[k] = 0;
    if (b < B) {
      const int64_t uu = user[b], pp = pos[b], nn = neg[b];
      int f = 0;
      if ((uint64_t)uu >= (uint64_t)nU) f |= YR_FLAG_BAD_USER;
      if ((uint64_t)pp >= (uint64_t)nI || (uint64_t)nn >= (uint64_t)nI) f |= YR_FLAG_BAD_ITEM;
      if (f) bad |= f;
      else { u[k] = (int32_t)uu; p[k] = (int32_t)pp; n[k] = (int32_t)nn; }
    }
  }
  for (int i = tid; i <= nb; i += kPartThreads) s_cnt[i] = 0;
  __syncthreads();
  int ra[PT], rb[PT];                           // rank inside (tile, bucket)
#pragma unroll
  for (int k = 0; k < PT; ++k) {
    ra[k] = 0; rb[k] = 0;
    if (u[k] >= 0) {
      if (side == 0) {
        ra[k] = atomicAdd(&s_cnt[u[k] >> shift], 1);
      } else {
        ra[k] = atomicAdd(&s_cnt[p[k] >> shift], 1);
        rb[k] = atomicAdd(&s_cnt[n[k] >> shift], 1);
      }
    }
  }
  __syncthreads();
  // exclusive scan of s_cnt[0..nb) in place, s_cnt[nb] = total: each thread owns `per` consecutive entries
  {
    const int per = (nb + kPartThreads - 1) / kPartThreads;
    const int i0 = tid * per;
    int sum = 0;
    for (int i = i0; i < i0 + per && i < nb; ++i) sum += s_cnt[i];
    const int lane = tid & (kWave - 1), wave = tid / kWave;
    int inc = sum;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const int o = __shfl_up(inc, d, kWave);
      if (lane >= d) inc += o;
    }
    if (lane == kWave - 1) s_wave[wave] = inc;
    __syncthreads();
    int before = inc - sum;
    for (int w = 0; w < wave; ++w) before += s_wave[w];
    for (int i = i0; i < i0 + per && i < nb; ++i) {
      const int c = s_cnt[i];
      s_cnt[i] = before;
      before += c;
    }
    if (tid == kPartThreads - 1) s_cnt[nb] = before;
  }
  __syncthreads();
  int32_t* off = (side ? offI : offU) + (int64_t)tile * (nb + 1);
  for (int i = tid; i <= nb; i += kPartThreads) off[i] = s_cnt[i];
  // The records are first placed bucket by bucket in LDS and then written out with 16-byte coalesced
  // stores: scattering them straight to global memory (8/16 bytes per lane to 64 different lines per wave
  // instruction) was bound by the request rate of the L2, not by bytes.
  const int total = s_cnt[nb];
  if (side == 0) {
#pragma unroll
    for (int k = 0; k < PT; ++k)
      if (u[k] >= 0) {
        const int b = tile * TILE + k * kPartThreads + tid;
        s_stage[s_cnt[u[k] >> shift] + ra[k]] = make_int4(p[k], n[k], b, u[k] & rmask);
      }
    if (bad && err_flag) atomicOr(err_flag, bad);
    __syncthreads();
    int4* out = rec + (int64_t)tile * TILE;
    for (int i = tid; i < total; i += kPartThreads) out[i] = s_stage[i];
  } else {
    int2* stage2 = reinterpret_cast<int2*>(s_stage);
#pragma unroll
    for (int k = 0; k < PT; ++k)
      if (u[k] >= 0) {
        const int b = tile * TILE + k * kPartThreads + tid;
        stage2[s_cnt[p[k] >> shift] + ra[k]] = make_int2(u[k] | ((p[k] & rmask) << kOccShift), b);
        stage2[s_cnt[n[k] >> shift] + rb[k]] = make_int2(u[k] | ((n[k] & rmask) << kOccShift), b | (int)0x80000000);
      }
    __syncthreads();
    int4* out = reinterpret_cast<int4*>(occ + (int64_t)tile * TILE * 2);   // two occurrences per 16 bytes
    const int n16 = (total + 1) >> 1;
    for (int i = tid; i < n16; i += kPartThreads) out[i] = s_stage[i];
  }
}

#ifdef YR_STAMPS
__device__ long long g_stamps[8192 * 8];
__device__ int g_walk_iters[8192 * 4];           // walk iterations of each wave over the workgroup's first bucket
#define YR_STAMP(i) do { if (threadIdx.x == 0 && first_bucket) g_stamps[(blockIdx.x + (USER ? 0 : 4096)) * 8 + (i)] = wall_clock64(); } while (0)
#else
#define YR_STAMP(i)
#endif

// --------------------------------------------------------------------------- 2, 3: owner passes
struct OwnerArgs {
  const float* own_old;      // table whose rows are updated (read)
  float* own_new;            // where the updated rows go (== own_old for the item pass)
  const float* other;        // table whose rows are gathered
  float* m;
  float* v;
  float* grad_out;           // item pass, FUSE_ADAM = false: dense gradient rows instead of Adam
  const int32_t* off;        // [T][nb + 1] bucket offsets inside every tile region
  const void* recs;          // int4 rec (user side) / int2 occ (item side), tile-major
  float* coeff;              // [B] g_b by triplet id: written by the user pass, read by the item pass
  float* loss_partials;      // user pass: one slot per workgroup; item pass workgroup 0 reduces them
  float* loss_out;           // item pass: step loss (may be null)
  double* loss_accum;        // item pass: running epoch loss (may be null)
  int finalize;              // item pass: workgroup 0 reduces the loss partials
  int nb, T, tile_stride;    // buckets on this side, tiles, records per tile region
  int rows;                  // rows of the own table
  int bucket_begin, bucket_end;
  int slots;                 // owner slots: bucket_end with an order, else owner_slots(bucket_end - bucket_begin)
  const int32_t* order;      // optional: workgroup slot -> bucket (a permutation of [0, nb): heaviest buckets first)
  int heavy_t;               // rows with more records in a chunk are walked by all four waves
  float inv_batch;
  PullAdam adam;
  // oversize item buckets (see kSplitMin): `split` = the bookkeeping block of the workspace — {tasks, slots, row
  // tasks} counters (16 B), then parts[nbI], slot[nbI], arrive[nbI] (each padded to 16 B), then the task list and
  // the row-task list.  Item pass: the first helper_blocks workgroups are helpers, of a tile-range task (task j) from
  // the first one up and of a row task from the last one down; parts[k] > 1 marks a bucket split by tile range whose
  // parts leave their sums in scratch slot slot[k] + part, parts[k] = -S < 0 a bucket whose rows are shared by S
  // parts.  User pass: its first build_blocks workgroups fill the
  // block for the item pass that follows, from the item-side offsets b_off [T][b_nb + 1].
  // (One pointer instead of seven: the kernel arguments live in scalar registers, and the item pass has none to spare.)
  char* split;
  float* scratch;
  const int32_t* b_off;
  int helper_blocks, build_blocks, b_nb;
  int b_split_min, b_split_target;   // records from which a bucket is split / per part (host: scaled with the batch)
  int b_rowsplit_min, b_rowsplit_quad;   // records from which a bucket's rows are shared by 2 / by 4 parts (host)
};

// the pieces of the `split` block
__host__ __device__ __forceinline__ size_t split_per(int nbI) { return ((size_t)nbI * 4 + 15) & ~(size_t)15; }
__device__ __forceinline__ int32_t* split_counters(char* b) { return (int32_t*)b; }
__device__ __forceinline__ int32_t* split_parts(char* b) { return (int32_t*)(b + 16); }
__device__ __forceinline__ int32_t* split_slot(char* b, int nbI) { return (int32_t*)(b + 16 + split_per(nbI)); }
__device__ __forceinline__ int32_t* split_arrive(char* b, int nbI) { return (int32_t*)(b + 16 + 2 * split_per(nbI)); }
__device__ __forceinline__ int4* split_tasks(char* b, int nbI) { return (int4*)(b + 16 + 3 * split_per(nbI)); }
__device__ __forceinline__ int2* split_row_tasks(char* b, int nbI) { return (int2*)(split_tasks(b, nbI) + kMaxTasks); }

// Sizing of the item buckets (first workgroups of the user pass): kBuildLanes lanes per bucket add up its records
// over the tiles (lane j takes tiles j, j + kBuildLanes, ...), the group's first lane decides the parts; split
// buckets get scratch slots and helper tasks.
__device__ __forceinline__ void build_splits(const OwnerArgs& a, int builder) {
  const int k = (builder * kBlock + (int)threadIdx.x) / kBuildLanes, j = threadIdx.x % kBuildLanes;
  int total = 0;
  if (k < a.b_nb) {
    int t = j;
    const int64_t pitch = a.b_nb + 1;
    for (; t + 3 * kBuildLanes < a.T; t += 4 * kBuildLanes) {           // four tiles in flight per lane
      const int32_t* o0 = a.b_off + (int64_t)t * pitch + k;
      const int32_t* o1 = o0 + kBuildLanes * pitch;
      const int32_t* o2 = o1 + kBuildLanes * pitch;
      const int32_t* o3 = o2 + kBuildLanes * pitch;
      const int a0 = o0[0], b0 = o0[1], a1 = o1[0], b1 = o1[1], a2 = o2[0], b2 = o2[1], a3 = o3[0], b3 = o3[1];
      total += ((b0 - a0) + (b1 - a1)) + ((b2 - a2) + (b3 - a3));
    }
    for (; t < a.T; t += kBuildLanes) {
      const int32_t* orow = a.b_off + (int64_t)t * (a.b_nb + 1) + k;
      total += orow[1] - orow[0];
    }
  }
#pragma unroll
  for (int m = 1; m < kBuildLanes; m <<= 1) total += __shfl_xor(total, m, kWave);
  if (k >= a.b_nb || j != 0) return;
  int parts = 1;
  if (total >= a.b_split_min) {
    parts = (total + a.b_split_target - 1) / a.b_split_target;
    parts = min(parts, min(kMaxParts, a.T));
  }
  int slot = 0;
  if (parts > 1) {
    slot = atomicAdd(split_counters(a.split) + 1, parts);
    const int first = atomicAdd(split_counters(a.split), parts - 1);
    // no room left (more than kMaxSlots / kMaxTasks parts in one batch): the task entries it took are marked void.
    // The counters go on counting what the batch wants: the item pass reads them, and past either pool it treats
    // EVERY bucket as whole, whatever this workgroup found room for (see pools_hold there)
    const bool fits = slot + parts <= kMaxSlots && first + parts - 1 <= kMaxTasks;
    for (int q = 1; q < parts; ++q)
      if (first + q - 1 < kMaxTasks) split_tasks(a.split, a.b_nb)[first + q - 1] = make_int4(fits ? k : -1, q, 0, 0);
    if (!fits) parts = 1;
  }
#if YR_ROWSPLIT
  else if (total < a.b_split_min && total >= a.b_rowsplit_min) {
    // rows shared out: S - 1 row tasks {bucket, part}.  As above the counter counts what the batch WANTS, and the
    // item pass shares no bucket's rows when that is more than the pool holds (the entries past it are not written)
    const int S = total >= a.b_rowsplit_quad ? 4 : 2;
    const int first = atomicAdd(split_counters(a.split) + 2, S - 1);
    for (int q = 1; q < S; ++q)
      if (first + q - 1 < kMaxRowTasks) split_row_tasks(a.split, a.b_nb)[first + q - 1] = make_int2(k, q);
    parts = -S;
  }
#endif
  split_parts(a.split)[k] = parts;
  split_slot(a.split, a.b_nb)[k] = slot;
  split_arrive(a.split, a.b_nb)[k] = 0;
}

// sum a float4 over the lane groups of a wave (lanes with equal l)
template <int LPR>
__device__ __forceinline__ void cross_group_sum(float4& a) {
#pragma unroll
  for (int m = LPR; m < kWave; m <<= 1) {
    a.x += __shfl_xor(a.x, m, kWave);
    a.y += __shfl_xor(a.y, m, kWave);
    a.z += __shfl_xor(a.z, m, kWave);
    a.w += __shfl_xor(a.w, m, kWave);
  }
}

// inclusive scan over the 64 lanes of a wave
__device__ __forceinline__ int wave_inclusive_scan(int x, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const int t = __shfl_up(x, d, kWave);
    if (lane >= d) x += t;
  }
  return x;
}

// Per lane group: the sum of the row this group finishes (a wave owns GPW rows, one per lane group at the end).
// A wave's stream is sorted by row, so a lane group sums into `cur` while its row stays the same; when the row
// changes, the groups closing the same row combine with shuffles and the owning group adds the result.  (One
// register accumulator per row with predicated adds — no cross-lane traffic until the bucket is finished — cost 12
// more VGPRs and with them the eighth workgroup per CU: measured slower and removed.)
template <int LPR, int GPW>
struct RowSums {
  float4 total;                                   // running sum of this group's own row
  __device__ __forceinline__ void clear() { total = zero4(); }
  // `cur_row` = row index inside the wave (0..GPW-1)
  __device__ __forceinline__ void book(bool closing, int cur_row, const float4& cur, int grp) {
#pragma unroll 1
    for (int j = 0; j < GPW; ++j) {
      const bool sel = closing && cur_row == j;
      if (!__ballot(sel)) continue;               // wave-uniform
      float4 v = sel ? cur : zero4();
      cross_group_sum<LPR>(v);
      if (grp == j) { total.x += v.x; total.y += v.y; total.z += v.z; total.w += v.w; }
    }
  }
  __device__ __forceinline__ float4 finish(int) { return total; }
};

// Which lane group finishes which row.  A wave walks the records of the RPW rows it finishes, so a wave whose rows
// are long keeps the workgroup alive while the others idle.  Once the first chunk's counts are known, wave 0 deals
// the R local rows to the R slots (slot = wave * RPW + lane group): rows by descending light count (ties: lower row
// first), each to the least-loaded wave that still has a free slot (ties: lower wave first).  Heavy rows are walked
// by all waves and count as empty.  A pure function of the counts: the deterministic mode depends on that.
// Lane w < 4 keeps wave w's key (load << 2 | w, INT_MAX once its slots are taken): scalar registers are scarce here.
template <int R, int RPW>
__device__ __forceinline__ void deal_rows(const int* s_cnt, unsigned char* s_slotof, unsigned char* s_rowof, int lane,
                                          int heavy_t) {
  static_assert(kWavesPerBlock == 4 && R == 4 * RPW, "four waves of RPW slots");
  const int c = s_cnt[lane];
  const int load = (lane < R && c <= heavy_t) ? c : 0;
  // one key per row that orders them: longer rows first, equal rows by index (a single compare per pair: a separate
  // `j < lane` is the same for every chunk, and the compiler keeps all R of them in scalar registers for the kernel's life)
  const int order = (load << 6) | (kWave - 1 - lane);
  int rank = 0;
  for (int j = 0; j < R; ++j) rank += __builtin_amdgcn_readlane(order, j) > order ? 1 : 0;
  int wkey = lane < kWavesPerBlock ? lane : 0x7fffffff, wused = 0;   // lane w < 4: wave w's key and slots taken
  int slot = lane;                                // lanes past the bucket's rows keep the identity
  for (int i = 0; i < R; ++i) {
    const int src = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)__ballot(lane < R && rank == i)) - 1);
    const int ci = __builtin_amdgcn_readlane(load, src);
    const int w = min(min(__builtin_amdgcn_readlane(wkey, 0), __builtin_amdgcn_readlane(wkey, 1)),
                      min(__builtin_amdgcn_readlane(wkey, 2), __builtin_amdgcn_readlane(wkey, 3))) & 3;
    const int s = w * RPW + __builtin_amdgcn_readlane(wused, w);
    if (lane == w) {
      wused += 1;
      wkey = wused == RPW ? 0x7fffffff : wkey + (ci << 2);
    }
    if (lane == src) slot = s;
  }
  s_slotof[lane] = (unsigned char)slot;
  s_rowof[slot] = (unsigned char)lane;
}

constexpr int kTagShift = 10;    // s_idx entry = load-order index (< kCap) | local row << 10
constexpr int kTagMask = (1 << kTagShift) - 1;

// One pass of a wave over the stream positions lo + first + k * stride < hi (sorted by row); books
// row sums into `sums` (slots relative to `row_base`; LOOKUP: the entries are tagged with rows, whose slot is looked
// up in s_slotof when the row closes; otherwise the tag is the slot) or, with HEAVY, returns the sum of ONE row in `cur`.
template <int D, bool USER, bool HEAVY, bool LOOKUP>
__device__ __forceinline__ void walk_stream(const OwnerArgs& a, const unsigned short* s_idx, const int* s_x,
                                            const int* s_y, const int* s_z, const float4* s_own,
                                            const unsigned char* s_slotof, int lo, int hi,
                                            int first, int stride, int row_base, int grp, int l,
                                            RowSums<PullGeom<D>::LPR, PullGeom<D>::GPW>& sums, float4& cur,
                                            float& loss) {
  using G = PullGeom<D>;
  constexpr int LPR = G::LPR;
  constexpr int N = USER ? kUserUnroll : kItemUnroll;
  int cur_row = -1;
  // the trip count is the same for every lane of the wave (the start is common, `first` only offsets
  // the position): the loop body holds cross-lane operations
  for (int base = lo; base < hi; base += stride * N) {
    bool valid[N];
    int tag[N], ia[N], ib[N], ic[N];
    float4 r0[N], r1[N];
#pragma unroll
    for (int q = 0; q < N; ++q) {
      const int pos = base + first + q * stride;
      valid[q] = pos < hi;
      const int e = s_idx[min(pos, hi - 1)];                    // past the end: the last record, weight 0
      tag[q] = e >> kTagShift;
      const int c = e & kTagMask;
      ia[q] = s_x[c];
      ib[q] = s_y[c];
      ic[q] = USER ? s_z[c] : 0;
    }
#pragma unroll
    for (int q = 0; q < N; ++q) {
      r0[q] = ld4o(a.other, (uint32_t)(ia[q] * D + 4 * l));
      if (USER) r1[q] = ld4o(a.other, (uint32_t)(ib[q] * D + 4 * l));
    }
#pragma unroll
    for (int q = 0; q < N; ++q) {
      if (!HEAVY) {
        const bool closing = valid[q] && cur_row >= 0 && tag[q] != cur_row;
        if (__ballot(closing)) {
          const int slot = LOOKUP ? (int)s_slotof[max(cur_row, 0)] : cur_row;
          sums.book(closing, slot - row_base, cur, grp);
          if (closing) cur = zero4();
        }
        if (valid[q]) cur_row = tag[q];
      }
      if (USER) {
        const float4 ownj = s_own[tag[q] * LPR + l];
        float4 d;
        d.x = r0[q].x - r1[q].x; d.y = r0[q].y - r1[q].y; d.z = r0[q].z - r1[q].z; d.w = r0[q].w - r1[q].w;
        float part = ownj.x * d.x;
        part = fmaf(ownj.y, d.y, part);
        part = fmaf(ownj.z, d.z, part);
        part = fmaf(ownj.w, d.w, part);
        const float x = group_sum_dpp<LPR>(part);
        float sp, sg;
        bpr_terms(x, sp, sg);
        const float gg = valid[q] ? -sg * a.inv_batch : 0.0f;
        cur.x = fmaf(gg, d.x, cur.x); cur.y = fmaf(gg, d.y, cur.y);
        cur.z = fmaf(gg, d.z, cur.z); cur.w = fmaf(gg, d.w, cur.w);
        if (valid[q] && l == 0) {
          a.coeff[ic[q]] = gg;                    // one hand-off word per triplet; the item side applies the sign
          loss += sp;
        }
      } else {
        const float gg = valid[q] ? __int_as_float(ib[q]) : 0.0f;
        cur.x = fmaf(gg, r0[q].x, cur.x); cur.y = fmaf(gg, r0[q].y, cur.y);
        cur.z = fmaf(gg, r0[q].z, cur.z); cur.w = fmaf(gg, r0[q].w, cur.w);
      }
    }
  }
  if (!HEAVY) {
    const int slot = LOOKUP ? (int)s_slotof[max(cur_row, 0)] : cur_row;
    sums.book(cur_row >= 0, slot - row_base, cur, grp);
  }
}

// row split: whether local row `row` is one of part `part` of a bucket with the parts word `parts` (-S: the rows
// with (row & (S - 1)) == part; 1 or a tile-range split: every row)
__device__ __forceinline__ bool row_kept(int row, int part, int parts) {
  return !YR_ROWSPLIT || ((row ^ part) & max(-parts - 1, 0)) == 0;
}

// steps of one walk_stream call over n records taken `groups` at a time (instrumented builds count them)
template <bool USER>
__device__ __forceinline__ int walk_steps(int n, int groups) {
  const int per = groups * (USER ? kUserUnroll : kItemUnroll);
  return (n + per - 1) / per;
}

// --------------------------------------------------------------------------- the phases of an owner pass
// owner_pass_kernel below is this sequence, per bucket (or part of a bucket) of its workgroup:
//   bucket selection;  for tile groups: scan_segments;  for chunks: cut_chunk_at_tiles (DET), load_window (DET) or the
//   plain loader, stream layout, rerank_by_id (DET), walk_stream over the light rows, the heavy-row loop;
//   final row binding, leave_part_sums + sum_part_slots (a part by tile range), row update;  after the last bucket the loss.
// The phases with a name are functions, inlined into the kernel; the others are delimited blocks of its body, because
// as functions they changed the machine code of the forms the trainers run (profiles/owner_pass_phases_resources.txt
// has every shape that was tried and what it did).  The kernel declares the LDS arrays (their order and sizes are its
// layout) and hands them to the functions as pointers; a function gets every other value it works on as an argument,
// and its comment says which of them must be uniform over the workgroup (it holds barriers that depend on them).

// What one instance of the kernel is compiled for: the geometry and the paths its template arguments select.
template <int D_, bool USER_, bool FUSE_ADAM_, bool DET_, int RPWX>
struct OwnerForm {
  static constexpr int D = D_;
  static constexpr bool USER = USER_, FUSE_ADAM = FUSE_ADAM_, DET = DET_;
  static constexpr int LPR = PullGeom<D>::LPR, GPW = PullGeom<D>::GPW;
  static constexpr int RPW = RPWX ? RPWX : GPW;         // rows a wave owns (RPWX = 0: one per lane group)
  static_assert(RPW <= GPW, "a wave finishes at most one row per lane group");
  static constexpr int R = kWavesPerBlock * RPW;        // rows per bucket
  static constexpr int DEAL_BAR = kDealMin * (kWavesPerBlock * GPW) * (kWavesPerBlock * GPW) / 256;   // records in the first chunk
  // rows dealt to the lane groups by load: not with one row per wave (nothing to deal), and not where a chunk can never
  // hold DEAL_BAR records (D = 16, the user side at D = 32): those forms compile to the index-order binding
  static constexpr bool DEAL = RPWX == 0 && YR_DEAL && DEAL_BAR <= (USER ? kUserCap : kCap);
  // The tag of a stream entry names what the walk needs without a further lookup.  Item pass: the SLOT (the walk only
  // books sums, as it did before rows were dealt: it has no register to spare).  User pass: the local ROW (every
  // record reads the row's own embedding from s_own), and the slot is looked up when a row closes.
  static constexpr bool TAG_SLOT = DEAL && !USER, LOOKUP = DEAL && USER;
  static constexpr int CAP = USER ? kUserCap : kCap;    // records per chunk
  static constexpr int PT = CAP / kBlock;               // records per thread and chunk
};

// the kernel's LDS arrays that the phases below work on (see their declarations there); dissolved by the optimiser
struct OwnerLds {
  int *pre, *base, *cnt, *start;
  unsigned char* rowof;
  int *x, *y, *z;
  unsigned short* idx;
  int *scan, *n, *last;
};

// The tile whose segment holds flattened index j: the last of the nt tiles with s_pre[tile] <= j (a tile whose
// segment STARTS at j wins over the empty ones before it).
__device__ __forceinline__ int tile_of(const int* s_pre, int nt, int j) {
  int tlo = 0, thi = nt;
  while (thi - tlo > 1) {
    const int mid = (tlo + thi) >> 1;
    if (s_pre[mid] <= j) tlo = mid; else thi = mid;
  }
  return tlo;
}

// Segment descriptors of bucket k in the tiles [tg0, tg0 + nt), nt <= kTileGroup: s_base[i] = where tile tg0 + i's
// segment sits in the record array, s_pre[0..nt] = exclusive scan of the segments' lengths.  Returns s_pre[nt], the
// records of the tile group.  k, tg0 and nt are workgroup-uniform (one or two barriers; up to 64 tiles one wave
// scans); writes s_base, s_pre, s_scan, and ends on a barrier.  tid = the thread of the workgroup, here and below.
__device__ __forceinline__ int scan_segments(const OwnerArgs& a, const OwnerLds& s, int tid, int k, int tg0,
                                             int nt) {
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  int len = 0;
  if (tid < nt) {
    const int32_t* orow = a.off + (int64_t)(tg0 + tid) * (a.nb + 1) + k;
    const int o0 = orow[0], o1 = orow[1];
    len = o1 - o0;
    s.base[tid] = (tg0 + tid) * a.tile_stride + o0;
  }
  int inc = 0, before = 0;
  if (nt > kWave) {
    inc = wave_inclusive_scan(len, lane);
    if (lane == kWave - 1) s.scan[wave] = inc;
    __syncthreads();
    for (int w = 0; w < wave; ++w) before += s.scan[w];
  } else if (wave == 0) {                    // up to 64 tiles: one wave scans
    inc = wave_inclusive_scan(len, lane);
  }
  if (nt > kWave || wave == 0) {
    s.pre[tid] = before + inc - len;
    if (lane == kWave - 1) s.pre[tid + 1] = before + inc;   // entry after a wave's last (the total after the last wave)
  }
  __syncthreads();
  return s.pre[nt];
}

// DET: which records share a chunk must not depend on the (arbitrary) order inside a tile's segment.  Chunks
// are cut at tile boundaries; a segment larger than a chunk is taken in WINDOWS of triplet ids (a window of
// CAP ids holds at most CAP user-side records, one of CAP / 2 ids at most CAP item occurrences): every window
// scans the whole segment and keeps what falls into it — a fixed set, ranked by triplet id in rerank_by_id.
// Here: wt = the tile whose segment starts at c0 (chunks start at boundaries); returns whether that segment is
// oversize (the chunk is one of its windows); otherwise cuts cend back to the last tile boundary after c0, if there
// is one.  Reads s_pre; every argument is workgroup-uniform, and so are the results.
template <int CAP>
__device__ __forceinline__ bool cut_chunk_at_tiles(const int* s_pre, int nt, int c0, int total, int& cend, int& wt) {
  wt = tile_of(s_pre, nt, c0);
  const bool windowed = s_pre[wt + 1] - s_pre[wt] > CAP;
  if (!windowed && cend < total) {
    const int tb = tile_of(s_pre, nt, cend);
    if (s_pre[tb] > c0) cend = s_pre[tb];
  }
  return windowed;
}

// DET, an oversize segment (tile tg0 + wt of the group): the records of id window `sub` go into s_x / s_y / s_z in
// arrival order (s_n counts them, s_idx holds their local rows until the keys are taken), then every thread takes the
// keys of its PT records, key = local row | rank inside the row << 8 (s_cnt), -1 for none.  Moves on to the next
// window (sub + 1, cend = c0: the same segment again) or past the segment (sub = 0, cend = its end).  Returns the
// records kept: 0 is possible, and the caller then skips the chunk.  Expects s_cnt and s_n zeroed behind a barrier;
// one barrier inside.  part / parts (the rows this workgroup keeps), tg0, wt, c0, sub, cend are workgroup-uniform.
template <class F>
__device__ __forceinline__ int load_window(const OwnerArgs& a, const OwnerLds& s, int tid, int part,
                                           int parts, int tg0, int wt, int c0, int& sub, int& cend,
                                           int (&key)[F::PT]) {
  constexpr bool USER = F::USER;
  constexpr int CAP = F::CAP, PT = F::PT;
  constexpr int W = USER ? CAP : CAP / 2;
  const int tile_ids = USER ? a.tile_stride : a.tile_stride >> 1;
  const int seg = s.pre[wt + 1] - s.pre[wt];
  const uint32_t rbase = (uint32_t)s.base[wt];
  const uint32_t id_lo = (uint32_t)(tg0 + wt) * (uint32_t)tile_ids + (uint32_t)sub * (uint32_t)W;
  for (int sidx = tid; sidx < seg; sidx += kBlock) {
    if (USER) {
      const int4 r = static_cast<const int4*>(a.recs)[rbase + sidx];
      if ((uint32_t)r.z - id_lo < (uint32_t)W) {
        const int slot = atomicAdd(s.n, 1);
        s.x[slot] = r.x; s.y[slot] = r.y; s.z[slot] = r.z;
        s.idx[slot] = (unsigned short)r.w;     // the local row, until the keys below are taken
      }
    } else {
      const int2 oc = static_cast<const int2*>(a.recs)[rbase + sidx];
      const uint32_t b = (uint32_t)(oc.y & 0x7fffffff);
      if (b - id_lo < (uint32_t)W && row_kept((int)((uint32_t)oc.x >> kOccShift), part, parts)) {
        const float g = a.coeff[b];
        const int slot = atomicAdd(s.n, 1);
        s.x[slot] = oc.x & kOccMask;
        s.y[slot] = __float_as_int(oc.y < 0 ? -g : g);
        s.z[slot] = oc.y;
        s.idx[slot] = (unsigned short)((uint32_t)oc.x >> kOccShift);
      }
    }
  }
  __syncthreads();
  const int n_rec = *s.n;
#pragma unroll
  for (int q = 0; q < PT; ++q) {
    const int c = tid + q * kBlock;
    key[q] = -1;
    if (c < n_rec) {
      const int local = s.idx[c];
      key[q] = local | (atomicAdd(&s.cnt[local], 1) << 8);
    }
  }
  ++sub;                                       // the next window of this segment, or the next tile boundary
  if (sub * W >= tile_ids) { sub = 0; cend = s.pre[wt + 1]; }
  else cend = c0;
  return n_rec;
}

// DET: the ranks inside a row came from LDS atomics in arrival order: re-rank every row of the stream by triplet id
// (s_z; unique inside a row), so that the order of every floating-point sum of the walks is fixed.  Reads s_idx,
// s_start, s_cnt, s_z (s_rowof), rewrites s_idx between two barriers.  n_rec = entries of the stream, workgroup-uniform.
template <class F>
__device__ __forceinline__ void rerank_by_id(const OwnerLds& s, int tid, int n_rec) {
  constexpr int PT = F::PT;
  int at[PT];
  unsigned short ent[PT];
#pragma unroll
  for (int q = 0; q < PT; ++q) {
    const int pos = tid + q * kBlock;
    at[q] = -1;
    if (pos < n_rec) {
      ent[q] = s.idx[pos];
      const int r = F::TAG_SLOT ? (int)s.rowof[ent[q] >> kTagShift] : ent[q] >> kTagShift;
      const uint32_t mine = (uint32_t)s.z[ent[q] & kTagMask];
      const int lo = s.start[r], cnt = s.cnt[r];
      int before = 0;
      for (int j = lo; j < lo + cnt; ++j)
        before += (uint32_t)s.z[s.idx[j] & kTagMask] < mine ? 1 : 0;
      at[q] = lo + before;
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < PT; ++q)
    if (at[q] >= 0) s.idx[at[q]] = ent[q];
  __syncthreads();
}

// A bucket split by tile range (parts > 1), first half: this part leaves its sums (acc) in its scratch slot and
// learns whether it was the last part to arrive; the last one goes on with sum_part_slots and the update, the others
// are done with the bucket.  The arrival counter is left at 0 for a further item pass over the same partition.
// `slots` (the bucket's slots) and `lc` (this lane's column) come back for the second half.  k, part and parts are
// workgroup-uniform (three barriers, and s_last decides for the whole workgroup); row_t is the TRUE local row of this
// lane group: slots are indexed by it, every part deals its own rows.
// (Two functions and the caller's `continue` between them: one function that returned early for the other parts
// changed the code of the loaders' binary search in the fused and unfused D = 64 item forms.)
template <class F>
__device__ __forceinline__ bool leave_part_sums(const OwnerArgs& a, const OwnerLds& s, int tid, int k, int part,
                                                int parts, bool finisher, int row_t, const float4& acc, float*& slots,
                                                int& lc) {
  constexpr int D = F::D, R = F::R;
  // (the base goes through an empty asm: otherwise scratch + this lane's offset is hoisted out of the bucket
  // loop into a VGPR pair the item pass does not have — it was spilled to scratch memory)
  float* sbase = a.scratch;
  asm volatile("" : "+s"(sbase));
  slots = sbase + (int64_t)split_slot(a.split, a.nb)[k] * (R * D);
  // (the lane's column is taken afresh from the thread index here too: kept from the kernel's start for this
  // rare path, it was the register pair the fused D = 64 form went to scratch memory for)
  int t3 = tid;
  asm volatile("" : "+v"(t3));
  lc = 4 * (t3 % F::LPR);
  if (finisher) st4(slots + (int64_t)part * (R * D) + row_t * D + lc, acc);
  __threadfence();
  __syncthreads();
  if (tid == 0) {
    *s.last = atomicAdd(split_arrive(a.split, a.nb) + k, 1) == parts - 1;
    // every part has arrived: the counter starts clean for a further item pass over the same partition
    if (*s.last) split_arrive(a.split, a.nb)[k] = 0;
  }
  __syncthreads();
  const bool last = *s.last != 0;
  __syncthreads();                           // s_last may be rewritten by the next bucket
  return last;
}

// Second half, the last part only: the sums of all parts of this lane group's row, added in part order (a fixed order:
// the deterministic mode survives).
template <class F>
__device__ __forceinline__ float4 sum_part_slots(const float* slots, int lc, int parts, int row_t, bool finisher) {
  constexpr int D = F::D, R = F::R;
  __threadfence();
  float4 acc = zero4();
  if (finisher) {
    for (int q = 0; q < parts; ++q) {
      const float4 p = ld4(slots + (int64_t)q * (R * D) + row_t * D + lc);
      acc.x += p.x; acc.y += p.y; acc.z += p.z; acc.w += p.w;
    }
  }
  return acc;
}

template <int D, bool USER, bool FUSE_ADAM, bool DET, int RPWX = 0>
__global__ __launch_bounds__(kBlock, YR_OWNER_WAVES) void owner_pass_kernel(OwnerArgs a) {
  using F = OwnerForm<D, USER, FUSE_ADAM, DET, RPWX>;
  constexpr int LPR = F::LPR, GPW = F::GPW, RPW = F::RPW, R = F::R, DEAL_BAR = F::DEAL_BAR, CAP = F::CAP, PT = F::PT;
  constexpr bool DEAL = F::DEAL, TAG_SLOT = F::TAG_SLOT, LOOKUP = F::LOOKUP;
  __shared__ int s_pre[kTileGroup + 1];          // flattened start of every tile's segment
  __shared__ int s_base[kTileGroup];             // where the segment sits in the record array
  __shared__ int s_cnt[kWave];                   // records per local row in this chunk
  __shared__ int s_start[kWave];                 // where a row's records start in the sorted stream
  __shared__ int s_light[kWave + 1];             // light rows only, by SLOT: wave w walks [s_light[w RPW], s_light[(w + 1) RPW])
  __shared__ unsigned char s_slotof[DEAL ? kWave : 1];   // local row -> slot (wave * RPW + lane group) that finishes it
  __shared__ unsigned char s_rowof[DEAL ? kWave : 1];    // slot -> local row; both valid once the bucket is `bound`
  __shared__ int s_x[CAP];                       // user: pos     item: user            (load order)
  __shared__ int s_y[CAP];                       // user: neg     item: signed coefficient (float bits)
  __shared__ int s_z[(USER || DET) ? CAP : 1];   // triplet id (item pass: | sign bit, kept for the deterministic order only)
  __shared__ unsigned short s_idx[CAP];          // row order -> load order | local row << 10
  __shared__ float4 s_own[USER ? R * LPR : 1];   // user pass: the bucket's own rows (they enter the scores)
  __shared__ float4 s_heavy[kWavesPerBlock][LPR];
  __shared__ float s_red[kWavesPerBlock];
  __shared__ int s_scan[kWavesPerBlock];
  __shared__ int s_n;                            // DET: records kept by the current window of an oversize segment
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int grp = lane / LPR, l = lane % LPR;
  const bool finisher = grp < RPW;                // lane groups that finish a row (all of them unless RPW < GPW)
  const int row_l = wave * RPW + (finisher ? grp : 0);   // this lane group's slot (= its row until the bucket is bound)
  float loss = 0.0f;
  __shared__ int s_last;
  const OwnerLds s = {s_pre, s_base, s_cnt, s_start, s_rowof, s_x, s_y, s_z, s_idx, s_scan, &s_n, &s_last};
  if (USER && (int)blockIdx.x < a.build_blocks) {
    // the user pass's first workgroups size the item buckets for the item pass that follows (no launch of its own;
    // first, so that they are done long before the owners)
    build_splits(a, blockIdx.x);
    return;
  }
  // item pass: the first hb workgroups are helpers of split buckets (by tile range from the first one up, by row
  // from the last one down); user pass: the first hb are the sizing ones
  const int hb = USER ? a.build_blocks : a.helper_blocks;
  const bool helper = !USER && (int)blockIdx.x < hb;
  const int owners = (int)gridDim.x - hb;
#ifdef YR_STAMPS
  bool first_bucket = true;
  int walk_iters = 0, heavy_iters = 0;
#endif
  YR_STAMP(0);

  for (int ks = helper ? (int)blockIdx.x : (int)blockIdx.x - hb;
       helper ? ks == (int)blockIdx.x : ks < a.slots; ks += owners) {
    // ---- bucket selection: which bucket k, which part of how many, and which tiles [t_begin, t_end) this trip works
    // on, for an owner, a tile-range helper and a row helper.  (inline: as a function with `int&` results, and with
    // only the pool rules or only the tile range lifted, the item forms changed by 87 to 2,970 lines, some to 64 VGPRs)
    // workgroups start in slot order: the caller may put heavy buckets first (wave-uniform: kept in a scalar register)
    int k, part = 0, parts = 1;
    // rows shared out (YR_ROWSPLIT): parts = -S < 0, and this workgroup keeps the local rows r with
    // (r & (S - 1)) == part (see row_kept: a whole bucket and a part by tile range keep every row, so the load phase
    // and the tail below have one form).  The two words that describe a tile-range part serve: the item pass has no
    // further scalar register to spare, and every one it lacks costs it a vector register, which it lacks too
    // Which buckets are shared is a function of the batch alone: the sizing workgroups count every task and slot the
    // batch WANTS (their sums do not depend on arrival order); a batch that wants more than the pools hold shares no
    // bucket at all — every bucket is summed whole, the helpers leave at once.  (Which buckets had found room
    // depended on the order of two global atomics; a whole and a shared bucket add in different orders.)
    // (the counter block in ONE 16-byte load, and the owner's bucket before either is waited for: every load of this
    // prologue is a round trip to the L2 that the whole workgroup waits for)
    int4 cnt = make_int4(0, 0, 0, 0);
    if (!USER && a.split) cnt = *reinterpret_cast<const int4*>(a.split);
    // (slot -> bucket: the caller's start order, else owner_bucket: one XCD's workgroups on neighbouring buckets)
    int k_own = a.bucket_begin + owner_bucket(ks);
    if (!helper && a.order) k_own = a.order[ks];
    const int c_tasks = __builtin_amdgcn_readfirstlane(cnt.x), c_slots = __builtin_amdgcn_readfirstlane(cnt.y);
    const int c_rows = __builtin_amdgcn_readfirstlane(cnt.z);
    const bool pools_hold = USER || !a.split || (c_tasks <= kMaxTasks && c_slots <= kMaxSlots);
    // The same rule for the row tasks, with a list, a counter and a pool of their own.  They are served by the helper
    // workgroups the tile-range tasks leave free, from the last one down (row task j by helper kMaxTasks - 1 - j: 512
    // more workgroups that find nothing to do cost every step 1 us, measured), so both kinds must fit into them
    const int tile_tasks = (USER || !a.split || !pools_hold) ? 0 : c_tasks;
    const bool rows_hold = !USER && YR_ROWSPLIT && a.split && c_rows <= kMaxRowTasks && tile_tasks + c_rows <= kMaxTasks;
    const bool row_helper = YR_ROWSPLIT && helper && ks >= tile_tasks;
    if (row_helper) {
      const int j = kMaxTasks - 1 - ks;
      if (!rows_hold || j >= c_rows) break;
      const int2 task = split_row_tasks(a.split, a.nb)[j];
      k = __builtin_amdgcn_readfirstlane(task.x);
      part = __builtin_amdgcn_readfirstlane(task.y);
      if (k < a.bucket_begin || k >= a.bucket_end) break;       // a bucket of another item chunk
    } else if (helper) {
      if (ks >= tile_tasks) break;
      const int4 task = split_tasks(a.split, a.nb)[ks];
      k = __builtin_amdgcn_readfirstlane(task.x);
      part = __builtin_amdgcn_readfirstlane(task.y);
      if (k < a.bucket_begin || k >= a.bucket_end) break;       // void task, or a bucket of another item chunk
    } else {
      k = __builtin_amdgcn_readfirstlane(k_own);
      if (k >= a.bucket_end) continue;                          // a padded slot: no bucket
    }
    if (!USER && a.split) {
      const int word = __builtin_amdgcn_readfirstlane(split_parts(a.split)[k]);
      if (word > 1 && pools_hold) parts = word;
      if (YR_ROWSPLIT && word < 0 && rows_hold) parts = word;
    }
    if (row_helper && parts >= 0) break;         // a row task without its bucket's word: never
    // this workgroup's share of the bucket: the tiles [t_begin, t_end)
    // (an integer division runs on the vector unit: the results are moved back to scalar registers, or they would
    // cost the item pass two VGPRs it does not have — 12 B of scratch per lane, caught by scripts/kernel_resources.py)
    // (a row part reads every tile)
    const int t_begin = parts < 0 ? 0 : __builtin_amdgcn_readfirstlane(a.T * part / parts);
    const int t_end = parts < 0 ? a.T : __builtin_amdgcn_readfirstlane(a.T * (part + 1) / parts);
    // ---- the row this lane group finishes, until the deal: slot = row
    int row_t = row_l;                           // the local row this lane group finishes
    int row_f = k * R + row_t;
    bool valid_f = finisher && row_f < a.rows && (USER || row_kept(row_t, part, parts));
    uint32_t o_f = (uint32_t)(row_f * D + 4 * l);
    // DEAL: the binding of rows to slots is fixed by the first chunk that holds a record and kept for the bucket
    // (the register totals persist over chunks, tile groups and windows); workgroup-uniform
    bool bound = false;
    if (USER && finisher) s_own[row_l * LPR + l] = valid_f ? ld4o(a.own_old, o_f) : zero4();
    YR_STAMP(1);
    RowSums<LPR, GPW> sums;
    sums.clear();

    for (int tg0 = t_begin; tg0 < t_end; tg0 += kTileGroup) {
      const int nt = min(kTileGroup, t_end - tg0);
      const int total = scan_segments(a, s, tid, k, tg0, nt);
      YR_STAMP(2);

      for (int c0 = 0, cend = 0, sub = 0; c0 < total; c0 = cend) {
        cend = min(total, c0 + CAP);
        int wt = 0;
        bool windowed = false;
        if (DET) windowed = cut_chunk_at_tiles<CAP>(s_pre, nt, c0, total, cend, wt);
        if (tid < kWave) s_cnt[tid] = 0;
        if (DET && tid == 0) s_n = 0;
        __syncthreads();
        // ---- loaders: this chunk's records into s_x / s_y (/ s_z) in load order, ranked by local row (s_cnt);
        // key = local row | rank << 8, -1 for none
        int key[PT];
        int n_rec = cend - c0;
        if (DET && windowed) {
          n_rec = load_window<F>(a, s, tid, part, parts, tg0, wt, c0, sub, cend, key);
          if (n_rec == 0) {                            // workgroup-uniform: nothing in this window
            __syncthreads();
            continue;
          }
        } else {
        // plain loader: record c0 + tid + q kBlock of the flattened stream (index -> tile by the search of tile_of,
        // address from s_base) goes to position tid + q kBlock.  (inline: as a function, whole or per role, with
        // the keys by reference or by value, 42 to 94 lines of the D = 64 forms changed; so did tile_of alone here)
        uint32_t addr[PT];
#pragma unroll
        for (int q = 0; q < PT; ++q) {
          const int j = c0 + tid + q * kBlock;
          key[q] = j < cend ? 0 : -1;
          int tlo = 0, thi = nt;
          while (thi - tlo > 1) {
            const int mid = (tlo + thi) >> 1;
            if (s_pre[mid] <= j) tlo = mid; else thi = mid;
          }
          addr[q] = j < cend ? (uint32_t)(s_base[tlo] + (j - s_pre[tlo])) : 0u;
        }
        if (USER) {
          int4 r[PT];                             // lanes past the end re-read record 0 of the array
#pragma unroll
          for (int q = 0; q < PT; ++q)
            r[q] = *reinterpret_cast<const int4*>(static_cast<const char*>(a.recs) + (uint32_t)(addr[q] * 16u));
#pragma unroll
          for (int q = 0; q < PT; ++q)
            if (key[q] >= 0) {
              const int c = tid + q * kBlock;
              s_x[c] = r[q].x; s_y[c] = r[q].y; s_z[c] = r[q].z;
              key[q] = r[q].w | (atomicAdd(&s_cnt[r[q].w], 1) << 8);
            }
        } else {
          int2 oc[PT];
          float g[PT];
#pragma unroll
          for (int q = 0; q < PT; ++q)
            oc[q] = *reinterpret_cast<const int2*>(static_cast<const char*>(a.recs) + (uint32_t)(addr[q] * 8u));
          // records of another part's rows are dropped here: their coefficient load reads index 0, and the counts,
          // the deal, the stream and the heavy rows below see the kept records only
#pragma unroll
          for (int q = 0; q < PT; ++q)
            if (!row_kept((int)((uint32_t)oc[q].x >> kOccShift), part, parts)) key[q] = -1;
#pragma unroll
          for (int q = 0; q < PT; ++q) {
            const uint32_t b = key[q] >= 0 ? (uint32_t)(oc[q].y & 0x7fffffff) : 0u;
            g[q] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.coeff) + (uint32_t)(b * 4u));
          }
#pragma unroll
          for (int q = 0; q < PT; ++q)
            if (key[q] >= 0) {
              const int c = tid + q * kBlock;
              const int local = (int)((uint32_t)oc[q].x >> kOccShift);
              s_x[c] = oc[q].x & kOccMask;
              s_y[c] = __float_as_int(oc[q].y < 0 ? -g[q] : g[q]);
              if (DET) s_z[c] = oc[q].y;
              key[q] = local | (atomicAdd(&s_cnt[local], 1) << 8);
            }
        }
        }
        __syncthreads();
        // ---- stream layout: sorted stream = light rows in slot order, then the heavy rows (more than heavy_t records).
        // Wave 0 binds rows to slots (once per bucket: s_slotof, s_rowof) and scans the counts into s_light, s_start
        // (s_n: records in the stream); after a barrier every thread puts its records into s_idx.  (inline: as one
        // function or as its two halves, 9 to 122 lines of the D = 64 forms changed)
        if (wave == 0) {
          if (DEAL && !bound) {
            // the deal is R serial steps of wave 0 (about 1.4 us at R = 16) while the other waves wait, and a walk
            // step takes 16 R records off the stream: a first chunk with few records (a short walk: nothing to win
            // back) keeps the identity.  The bar grows with R * R — 64 records at D = 128, 256 at D = 64, a full item
            // chunk at D = 32 (DEAL is off where no chunk can reach it)
            // (a row part: what counts is what it kept)
            int n_deal = n_rec;
            if (!USER && YR_ROWSPLIT && parts < 0) {
              n_deal = s_cnt[lane];
#pragma unroll
              for (int m = 1; m < kWave; m <<= 1) n_deal += __shfl_xor(n_deal, m, kWave);
            }
            if (n_deal >= DEAL_BAR) {
              deal_rows<R, RPW>(s_cnt, s_slotof, s_rowof, lane, a.heavy_t);
            } else {
              s_slotof[lane] = (unsigned char)lane;
              s_rowof[lane] = (unsigned char)lane;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
          }
          // lane = slot: the stream is laid out in slot order
          const int row = DEAL ? (int)s_rowof[lane] : lane;
          const int c = s_cnt[row];
          const bool heavy = c > a.heavy_t;
          const int cl = heavy ? 0 : c, ch = heavy ? c : 0;
          const int il = wave_inclusive_scan(cl, lane), ih = wave_inclusive_scan(ch, lane);
          const int total_light = __shfl(il, kWave - 1, kWave);
          s_light[lane] = il - cl;
          if (lane == kWave - 1) s_light[kWave] = il;
          if (!USER && YR_ROWSPLIT && lane == kWave - 1) s_n = il + ih;   // records in the stream (a row part: the kept ones)
          s_start[row] = heavy ? total_light + ih - ch : il - cl;
        }
        bound = true;
        __syncthreads();
        if (!USER && YR_ROWSPLIT && parts < 0) n_rec = __builtin_amdgcn_readfirstlane(s_n);   // gates the re-ranking and the heavy rows below
#pragma unroll
        for (int q = 0; q < PT; ++q)
          if (key[q] >= 0) {
            const int row = key[q] & 255;
            const int tag = TAG_SLOT ? (int)s_slotof[row] : row;
            s_idx[s_start[row] + (key[q] >> 8)] = (unsigned short)((tid + q * kBlock) | (tag << kTagShift));
          }
        __syncthreads();
        if (DET) rerank_by_id<F>(s, tid, n_rec);
        // ---- light rows: wave w walks the records of ITS slots [w RPW, (w+1) RPW), one per lane group and step
        {
          float4 cur = zero4();
          walk_stream<D, USER, false, LOOKUP>(a, s_idx, s_x, s_y, s_z, s_own, s_slotof, s_light[wave * RPW],
                                            s_light[wave * RPW + RPW], grp, GPW, wave * RPW, grp, l, sums, cur, loss);
#ifdef YR_STAMPS
          if (first_bucket) walk_iters += walk_steps<USER>(s_light[wave * RPW + RPW] - s_light[wave * RPW], GPW);
#endif
        }
        // ---- heavy rows of the chunk: all waves on one row, partial sums combined in wave order (s_heavy).  (inline: as
        // a function, the loop or one row of it, 15 to 32 lines of the D = 64 user forms changed)
        if (n_rec - s_light[kWave] > 0) {   // workgroup-uniform
#pragma unroll 1
          for (int r = 0; r < R; ++r) {
            const int cnt = s_cnt[r];
            if (cnt <= a.heavy_t) continue;       // workgroup-uniform
            const int lo = s_start[r];
            float4 t = zero4();
            walk_stream<D, USER, true, LOOKUP>(a, s_idx, s_x, s_y, s_z, s_own, s_slotof, lo, lo + cnt, wave * GPW + grp,
                                             kWavesPerBlock * GPW, 0, grp, l, sums, t, loss);
#ifdef YR_STAMPS
            if (first_bucket) { walk_iters += walk_steps<USER>(cnt, kWavesPerBlock * GPW); heavy_iters += 1; }
#endif
            cross_group_sum<LPR>(t);
            if (grp == 0) s_heavy[wave][l] = t;
            __syncthreads();
            if (finisher && row_l == (DEAL ? (int)s_slotof[r] : r)) {
#pragma unroll
              for (int w = 0; w < kWavesPerBlock; ++w) {
                const float4 h = s_heavy[w][l];
                sums.total.x += h.x; sums.total.y += h.y; sums.total.z += h.z; sums.total.w += h.w;
              }
            }
            __syncthreads();
          }
        }
        __syncthreads();                         // LDS records are reused by the next chunk
      }
    }

    YR_STAMP(3);
    float4 acc = sums.finish(grp);
    // ---- final row binding.  (inline: with reference results or a struct returned, 18 to 845 lines of the D = 64 forms changed)
    if (DEAL) {                                  // the row this slot was dealt (a bucket without records: the identity)
      if (bound) row_t = s_rowof[row_l];
      row_f = k * R + row_t;
      valid_f = row_f < a.rows && (USER || row_kept(row_t, part, parts));
      // (the lane's column offset is taken afresh from the thread index, through an empty asm: otherwise 4 * l is kept
      // over the whole walk for this one use — the register the D = 128 user pass then lacks went to scratch memory)
      int t2 = tid;
      asm volatile("" : "+v"(t2));
      o_f = (uint32_t)(row_f * D + 4 * (t2 % LPR));
    }
    // ---- cross-part combine: a bucket split by tile range; the last part to arrive goes on with the sum of all parts
    if (!USER && parts > 1) {
      float* slots;
      int lc;
      if (!leave_part_sums<F>(a, s, tid, k, part, parts, finisher, row_t, acc, slots, lc)) continue;
      acc = sum_part_slots<F>(slots, lc, parts, row_t, finisher);
    }
    // ---- row update: fused Adam, or the dense gradient row.  (inline: as a function, whole or the four adam_element
    // calls alone, 14 to 1,441 lines of the D = 64 forms changed: the kernel-argument loads move)
    if (valid_f) {
      if (FUSE_ADAM) {
        float4 own = USER ? s_own[row_t * LPR + l] : ld4o(a.own_old, o_f);
        float4 M = ld4o(a.m, o_f), V = ld4o(a.v, o_f);
        adam_element(own.x, acc.x, M.x, V.x, a.adam.c, a.adam.decoupled);
        adam_element(own.y, acc.y, M.y, V.y, a.adam.c, a.adam.decoupled);
        adam_element(own.z, acc.z, M.z, V.z, a.adam.c, a.adam.decoupled);
        adam_element(own.w, acc.w, M.w, V.w, a.adam.c, a.adam.decoupled);
        st4(a.own_new + o_f, own);
        st4(a.m + o_f, M);
        st4(a.v + o_f, V);
      } else {
        st4(a.grad_out + o_f, acc);
      }
    }
    YR_STAMP(4);
    if (USER) __syncthreads();                   // s_own is rewritten for the next bucket
    YR_STAMP(5);
#ifdef YR_STAMPS
    if (first_bucket) {
      if (lane == 0) g_walk_iters[(blockIdx.x + (USER ? 0 : 4096)) * 4 + wave] = walk_iters;
      if (tid == 0) {                            // which bucket this was, and how many heavy-row walks it took
        g_stamps[(blockIdx.x + (USER ? 0 : 4096)) * 8 + 6] = k;
        g_stamps[(blockIdx.x + (USER ? 0 : 4096)) * 8 + 7] = heavy_iters;
      }
    }
    first_bucket = false;
#endif
  }

  if (USER) {
    const float total = block_sum(loss, s_red);
    if (tid == 0) a.loss_partials[(int)blockIdx.x - hb] = total;
    if ((int)blockIdx.x == hb)                    // slots no workgroup owns
      for (int i = owners + tid; i < YR_LOSS_PARTIALS; i += kBlock) a.loss_partials[i] = 0.0f;
  } else if (a.finalize && (int)blockIdx.x == hb) {
    // ---- loss reduction, as pull_loss_finalize_kernel.  (inline, twice: one function for both, in four shapes,
    // reordered four instructions of the D = 64 item forms)
    // the user pass (previous launch) left one partial per workgroup: fixed-order sum -> step loss
    float s = 0.0f;
    for (int i = tid; i < YR_LOSS_PARTIALS; i += kBlock) s += a.loss_partials[i];
    const float total = block_sum(s, s_red);
    if (tid == 0) {
      const float v = total * a.inv_batch;
      if (a.loss_out) a.loss_out[0] = v;
      if (a.loss_accum) a.loss_accum[0] += (double)v;
    }
  }
}

__global__ __launch_bounds__(kBlock) void pull_loss_finalize_kernel(const float* __restrict__ partials, float scale,
                                                                    float* __restrict__ loss_out,
                                                                    double* __restrict__ loss_accum) {
  __shared__ float s_red[kWavesPerBlock];
  float s = 0.0f;
  for (int i = threadIdx.x; i < YR_LOSS_PARTIALS; i += kBlock) s += partials[i];
  const float total = block_sum(s, s_red);
  if (threadIdx.x == 0) {
    const float v = total * scale;
    if (loss_out) loss_out[0] = v;
    if (loss_accum) loss_accum[0] += (double)v;
  }
}

// --------------------------------------------------------------------------- host side
// How a batch of B triplets is cut into tiles, and the workspace carve-up (all 16-byte aligned).
inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }
struct PullPlan {
  int pt, tile, T, shiftU, shiftI, narrow_users, nbU, nbI;
  size_t o_offU, o_offI, o_rec, o_occ, o_coeff, o_split, o_scratch, bytes;
};
// split bookkeeping inside the workspace: {tasks, slots, row tasks} counters (16 B), parts / slot / arrivals per item
// bucket, the task list, the row-task list; then the scratch slots
inline size_t split_bytes(int nbI) {
  return 16 + (size_t)3 * align16((size_t)nbI * 4) + (size_t)kMaxTasks * sizeof(int4) + (size_t)kMaxRowTasks * sizeof(int2);
}

// tiles of 4096 triplets, halved while there would be fewer than kMinTiles of them (the partition launch
// and the owners' segment runs both want tiles that are neither too few nor too small)
inline int tile_pt(int64_t B) {
  int pt = 4;                                    // a staged tile of 4096 triplets is 64 KB of LDS
  while (pt > 1 && (B + (int64_t)kPartThreads * pt - 1) / ((int64_t)kPartThreads * pt) < kMinTiles) pt >>= 1;
  return pt;
}

inline PullPlan make_plan(int64_t B, int64_t nU, int64_t nI, int D, bool upper_bound) {
  PullPlan p;
  p.shiftI = bucket_shift(D);
  const int R = 1 << p.shiftI;
  // user buckets of 4 rows (a wave per row) when buckets of 1024/D rows would leave most of the 2,048
  // resident owner workgroups without work (user shards of a multi-GPU run, small tables)
  p.narrow_users = (nU + R - 1) / R < kNarrowBelow && R > kNarrowRows;
  p.shiftU = p.narrow_users ? kNarrowShift : p.shiftI;
  p.nbU = (int)((nU + (1 << p.shiftU) - 1) >> p.shiftU);
  p.nbI = (int)((nI + (1 << p.shiftI) - 1) >> p.shiftI);
  p.pt = tile_pt(B);
  p.tile = kPartThreads * p.pt;
  p.T = (int)((B + p.tile - 1) / p.tile);
  // upper bound over every batch size <= B (workspace sizing): T < 2 kMinTiles whenever pt < 4
  const int64_t T = upper_bound ? ((B + 4095) / 4096 > 2 * kMinTiles ? (B + 4095) / 4096 : 2 * kMinTiles) : p.T;
  const int64_t slots = upper_bound ? B + 4096 : (int64_t)p.T * p.tile;
  size_t o = 0;
  p.o_offU = o; o += align16((size_t)T * (p.nbU + 1) * 4);
  p.o_offI = o; o += align16((size_t)T * (p.nbI + 1) * 4);
  p.o_rec = o; o += align16((size_t)slots * sizeof(int4));
  p.o_occ = o; o += align16((size_t)slots * 2 * sizeof(int2));
  p.o_coeff = o; o += align16((size_t)(B > 0 ? B : 1) * 4);
  p.o_split = o; o += align16(split_bytes(p.nbI));
  p.o_scratch = o; o += (size_t)kMaxSlots * 1024 * 4;
  p.bytes = o;
  return p;
}

// Which item buckets are shared, for a batch of B triplets.  By tile range: oversize = well above the average bucket
// of THIS batch (2B occurrences over nbI buckets), and never below the floors: at one epoch per step the average
// bucket already holds 770 records.  By row (below that): the same rule with floors and multiples of its own; two
// parts up to three times the target, four from there on where a part then keeps at least four rows (D <= 64).
struct SplitRule {
  int split_min, split_target, row_min, row_target, row_quad, row_max_parts;
};
inline SplitRule split_rule(int64_t B, int nbI, int D) {
  SplitRule r;
  const double avg = 2.0 * (double)B / (double)nbI;
  const int by_avg_min = (int)(YR_SPLIT_AVG_MIN * avg), by_avg_target = (int)(YR_SPLIT_AVG_TARGET * avg);
  r.split_min = by_avg_min > kSplitMin ? by_avg_min : kSplitMin;
  r.split_target = by_avg_target > kSplitTarget ? by_avg_target : kSplitTarget;
  const int row_avg_min = (int)(YR_ROWSPLIT_AVG_MIN * avg), row_avg_target = (int)(YR_ROWSPLIT_AVG_TARGET * avg);
  r.row_min = row_avg_min > kRowSplitMin ? row_avg_min : kRowSplitMin;
  r.row_target = row_avg_target > kRowSplitTarget ? row_avg_target : kRowSplitTarget;
  r.row_max_parts = D == 128 ? 2 : 4;
  r.row_quad = r.row_max_parts >= 4 && r.row_target < 0x7fffffff / 3 ? 3 * r.row_target : 0x7fffffff;
  if (!YR_ROWSPLIT) { r.row_min = 0x7fffffff; r.row_quad = 0x7fffffff; r.row_max_parts = 1; }
  return r;
}

}  // namespace yr

using namespace yr;

static int pull_check_common(int64_t B, int D, int64_t num_users, int64_t num_items, const void* workspace,
                             int64_t workspace_bytes) {
  if (B < 0 || num_users <= 0 || num_items <= 0 || B > 0x3fffffff) return YR_ERR_BADARG;
  if (D != 16 && D != 32 && D != 64 && D != 128) return YR_ERR_UNSUPPORTED;
  // the partition's LDS histogram holds one counter per bucket of 1024/D rows; user ids share a
  // word with the local item row
  const PullPlan pl = make_plan(0, num_users, num_items, D, false);
  if (pl.nbU > kMaxBuckets || pl.nbI > kMaxBuckets) return YR_ERR_UNSUPPORTED;
  if (num_users > kOccMask) return YR_ERR_UNSUPPORTED;
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u) != 0) return YR_ERR_BADARG;
  if ((int64_t)make_plan(B, num_users, num_items, D, false).bytes > workspace_bytes) return YR_ERR_BADARG;
  return 0;
}

#ifdef YR_STAMPS
extern "C" int yr_debug_read_stamps(long long* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps), sizeof(long long) * n);
}
extern "C" int yr_debug_read_walk_iters(int* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_walk_iters), sizeof(int) * n);
}
#endif

extern "C" int64_t yr_bpr_mf_pull_workspace_bytes(int64_t max_batch, int64_t num_users, int64_t num_items, int D) {
  if (max_batch < 0 || num_users <= 0 || num_items <= 0) return YR_ERR_BADARG;
  if (D != 16 && D != 32 && D != 64 && D != 128) return YR_ERR_UNSUPPORTED;
  return (int64_t)make_plan(max_batch, num_users, num_items, D, true).bytes;
}

// phase 1: tile partition (independent of the tables: may run ahead, e.g. under the previous
// step's all-reduce) -> workspace
extern "C" int yr_bpr_mf_pull_index(const int64_t* user, const int64_t* pos, const int64_t* neg, int64_t B, int D,
                                    int64_t num_users, int64_t num_items, void* workspace, int64_t workspace_bytes,
                                    int32_t* err_flag, void* stream) {
  const int rc = pull_check_common(B, D, num_users, num_items, workspace, workspace_bytes);
  if (rc) return rc;
  if (B == 0) return 0;
  if (!user || !pos || !neg) return YR_ERR_BADARG;
  const PullPlan p = make_plan(B, num_users, num_items, D, false);
  char* w = static_cast<char*>(workspace);
  int32_t* offU = (int32_t*)(w + p.o_offU);
  int32_t* offI = (int32_t*)(w + p.o_offI);
  int4* rec = (int4*)(w + p.o_rec);
  int2* occ = (int2*)(w + p.o_occ);
  // dynamic LDS: the bucket counters, then the staged tile (16 B per triplet on either side)
  const int stage_off = (((p.nbU > p.nbI ? p.nbU : p.nbI) + 1) + 3) & ~3;           // in ints, 16-byte aligned
  const size_t lds = (size_t)stage_off * 4 + (size_t)p.tile * 16;
  const dim3 grid(p.T, 2);
  hipStream_t s = (hipStream_t)stream;
#define YR_PART_CASE(PT)                                                                                         \
  case PT: {                                                                                                     \
    static bool raised = false;                   /* more than the default 64 KB of dynamic LDS: once per process */ \
    if (!raised && lds > 65536) {                                                                                \
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&tile_partition_kernel<PT>),        \
                                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256);    \
      if (e != hipSuccess) return (int)e;                                                                        \
      raised = true;                                                                                             \
    }                                                                                                            \
    hipLaunchKernelGGL((tile_partition_kernel<PT>), grid, dim3(kPartThreads), lds, s, user, pos, neg, B, num_users, \
                       num_items, p.shiftU, p.shiftI, p.nbU, p.nbI, offU, offI, rec, occ, err_flag, stage_off,   \
                       (int32_t*)(w + p.o_split));                                                              \
  } break
  switch (p.pt) {
    YR_PART_CASE(1);
    YR_PART_CASE(2);
    YR_PART_CASE(4);
    default: return YR_ERR_BADARG;
  }
#undef YR_PART_CASE
  return launch_status();
}

// phase 2: the two owner passes over a partition built by phase 1 for the same batch
template <int D>
static int pull_apply_impl(const float* U_old, float* U_new, float* I, float* mU, float* vU, float* mI, float* vI,
                           float* gradI_out, int64_t B, int64_t nU, int64_t nI, float inv_batch, const PullAdam& adam,
                           int deterministic, void* workspace, float* loss_partials, float* loss_out,
                           double* loss_accum, int phases, int64_t item_begin, int64_t item_end,
                           const int32_t* item_order, hipStream_t s) {
  const PullPlan p = make_plan(B, nU, nI, D, false);
  char* w = static_cast<char*>(workspace);
  const bool want_loss = loss_out || loss_accum;
  if (phases & YR_PULL_USER_PHASE) {
    OwnerArgs ua{};
    ua.own_old = U_old; ua.own_new = U_new; ua.other = I; ua.m = mU; ua.v = vU; ua.grad_out = nullptr;
    ua.off = (const int32_t*)(w + p.o_offU); ua.recs = w + p.o_rec; ua.coeff = (float*)(w + p.o_coeff);
    ua.loss_partials = loss_partials;
    ua.nb = p.nbU; ua.T = p.T; ua.tile_stride = p.tile; ua.rows = (int)nU;
    ua.bucket_begin = 0; ua.bucket_end = p.nbU;
    ua.slots = owner_slots(p.nbU);
    ua.order = nullptr;
    ua.heavy_t = kHeavyRow; ua.inv_batch = inv_batch; ua.adam = adam;
    // the first build_blocks workgroups size the item buckets (oversize ones are shared out in the item pass)
    ua.build_blocks = (p.nbI * kBuildLanes + kBlock - 1) / kBlock;
    ua.b_off = (const int32_t*)(w + p.o_offI); ua.b_nb = p.nbI;
    const SplitRule rule = split_rule(B, p.nbI, D);
    ua.b_split_min = rule.split_min; ua.b_split_target = rule.split_target;
    ua.b_rowsplit_min = rule.row_min; ua.b_rowsplit_quad = rule.row_quad;
    ua.split = w + p.o_split;
    const int gu = (ua.slots < YR_LOSS_PARTIALS ? ua.slots : YR_LOSS_PARTIALS) + ua.build_blocks;   // one loss-partial slot per owner
    if (p.narrow_users && deterministic)
      hipLaunchKernelGGL((owner_pass_kernel<D, true, true, true, 1>), dim3(gu), dim3(kBlock), 0, s, ua);
    else if (p.narrow_users)
      hipLaunchKernelGGL((owner_pass_kernel<D, true, true, false, 1>), dim3(gu), dim3(kBlock), 0, s, ua);
    else if (deterministic)
      hipLaunchKernelGGL((owner_pass_kernel<D, true, true, true>), dim3(gu), dim3(kBlock), 0, s, ua);
    else
      hipLaunchKernelGGL((owner_pass_kernel<D, true, true, false>), dim3(gu), dim3(kBlock), 0, s, ua);
  }
  const bool items = (phases & YR_PULL_ITEM_PHASE) && item_end > item_begin;
  if (items) {
    OwnerArgs ia{};
    ia.own_old = I; ia.own_new = I; ia.other = U_old; ia.m = mI; ia.v = vI; ia.grad_out = gradI_out;
    ia.off = (const int32_t*)(w + p.o_offI); ia.recs = w + p.o_occ; ia.coeff = (float*)(w + p.o_coeff);
    ia.loss_partials = loss_partials; ia.loss_out = loss_out; ia.loss_accum = loss_accum;
    ia.finalize = want_loss ? 1 : 0;
    ia.nb = p.nbI; ia.T = p.T; ia.tile_stride = 2 * p.tile; ia.rows = (int)nI;
    ia.bucket_begin = (int)(item_begin >> p.shiftI);
    ia.bucket_end = (int)((item_end + (1 << p.shiftI) - 1) >> p.shiftI);
    // a start order is a permutation of ALL item buckets: used when the call covers all of them
    ia.order = (item_order && ia.bucket_begin == 0 && ia.bucket_end == p.nbI) ? item_order : nullptr;
    ia.slots = ia.order ? ia.bucket_end : owner_slots(ia.bucket_end - ia.bucket_begin);
    ia.heavy_t = kHeavyRow; ia.inv_batch = inv_batch; ia.adam = adam;
    ia.helper_blocks = kMaxTasks;
    // (an empty batch has no partition launch, so nothing has reset the counters where ITS plan puts the block: the
    // words there are left over from an earlier batch, and a helper that took one for a task would update a whole
    // bucket a second time next to its owner.  Without the block every bucket is whole and the helpers leave.)
    ia.split = B > 0 ? w + p.o_split : nullptr;
    ia.scratch = (float*)(w + p.o_scratch);
    int gi = ia.slots;
    if (gi > kMaxOwnerGrid) gi = kMaxOwnerGrid;
    gi += ia.helper_blocks;                       // helpers first: they start before the owners
    if (gradI_out && deterministic)
      hipLaunchKernelGGL((owner_pass_kernel<D, false, false, true>), dim3(gi), dim3(kBlock), 0, s, ia);
    else if (gradI_out)
      hipLaunchKernelGGL((owner_pass_kernel<D, false, false, false>), dim3(gi), dim3(kBlock), 0, s, ia);
    else if (deterministic)
      hipLaunchKernelGGL((owner_pass_kernel<D, false, true, true>), dim3(gi), dim3(kBlock), 0, s, ia);
    else
      hipLaunchKernelGGL((owner_pass_kernel<D, false, true, false>), dim3(gi), dim3(kBlock), 0, s, ia);
  } else if (want_loss) {
    hipLaunchKernelGGL(pull_loss_finalize_kernel, dim3(1), dim3(kBlock), 0, s, loss_partials, inv_batch, loss_out,
                       loss_accum);
  }
  return launch_status();
}

extern "C" int yr_bpr_mf_pull_item_buckets(int64_t num_items, int D) {
  if (num_items <= 0 || (D != 16 && D != 32 && D != 64 && D != 128)) return YR_ERR_BADARG;
  const int sh = bucket_shift(D);
  return (int)((num_items + (1 << sh) - 1) >> sh);
}

// The bucket of an owner slot over nb buckets (owner_bucket), -1 for a padded slot without one; host only.
extern "C" int yr_bpr_mf_pull_owner_bucket(int slot, int nb) {
  if (nb <= 0 || nb > kMaxBuckets || slot < 0 || slot >= owner_slots(nb)) return YR_ERR_BADARG;
  const int k = owner_bucket(slot);
  return k < nb ? k : -1;
}

// The item pass's start order for the buckets' expected loads (owner_start_order); host only.
extern "C" int yr_bpr_mf_pull_item_start_order(const double* bucket_load_host, int nb, int32_t* order_out) {
  if (!bucket_load_host || !order_out || nb <= 0 || nb > kMaxBuckets) return YR_ERR_BADARG;
  for (int k = 0; k < nb; ++k)
    if (!(bucket_load_host[k] == bucket_load_host[k])) return YR_ERR_BADARG;   // NaN: no order
  owner_start_order(bucket_load_host, nb, order_out);
  return 0;
}

// What build_splits decided for the partition in `workspace` (tests and measurement scripts; synchronises `stream`).
extern "C" int yr_bpr_mf_pull_split_summary(const void* workspace, int64_t workspace_bytes, int64_t B, int D,
                                            int64_t num_users, int64_t num_items, int32_t* counters_out,
                                            int32_t* parts_out, int32_t* rule_out, void* stream) {
  if (!rule_out || B <= 0 || num_users <= 0 || num_items <= 0) return YR_ERR_BADARG;
  if (D != 16 && D != 32 && D != 64 && D != 128) return YR_ERR_UNSUPPORTED;
  const PullPlan p = make_plan(B, num_users, num_items, D, false);
  const SplitRule r = split_rule(B, p.nbI, D);
  const int32_t rule[8] = {r.split_min, r.split_target, r.row_min, r.row_target, r.row_quad, r.row_max_parts,
                           kMaxRowTasks, YR_ROWSPLIT};
  for (int i = 0; i < 8; ++i) rule_out[i] = rule[i];
  if (!workspace) return (counters_out || parts_out) ? YR_ERR_BADARG : 0;
  const int rc = pull_check_common(B, D, num_users, num_items, workspace, workspace_bytes);
  if (rc) return rc;
  const char* blk = static_cast<const char*>(workspace) + p.o_split;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipSuccess;
  if (counters_out) e = hipMemcpyAsync(counters_out, blk, 16, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && parts_out)
    e = hipMemcpyAsync(parts_out, blk + 16, (size_t)p.nbI * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  return (int)e;
}

extern "C" int yr_bpr_mf_pull_apply_ordered(const float* U_old, float* U_new, float* I, float* mU, float* vU,
                                            float* mI, float* vI, float* gradI_out, int64_t B, int D,
                                            int64_t num_users, int64_t num_items, float inv_batch, double lr,
                                            double step_size, double bc2_sqrt, double beta1, double beta2, double eps,
                                            double weight_decay, int mode, int deterministic, void* workspace,
                                            int64_t workspace_bytes, float* loss_partials, float* loss_out,
                                            double* loss_accum, int phases, int64_t item_row_begin,
                                            int64_t item_row_end, const int32_t* item_bucket_order, void* stream) {
  int rc = pull_check_common(B, D, num_users, num_items, workspace, workspace_bytes);
  if (rc) return rc;
  if (!(phases & (YR_PULL_USER_PHASE | YR_PULL_ITEM_PHASE))) return YR_ERR_BADARG;
  if (item_row_begin < 0 || item_row_end > num_items || item_row_begin > item_row_end) return YR_ERR_BADARG;
  // item chunks are whole buckets of 1024/D rows (the last one may end with the table)
  const int R = 1 << bucket_shift(D);
  if (item_row_begin % R != 0 || (item_row_end % R != 0 && item_row_end != num_items)) return YR_ERR_BADARG;
  if (!U_old || !U_new || U_old == U_new || !I || !mU || !vU || !loss_partials) return YR_ERR_BADARG;
  if (!gradI_out && (!mI || !vI)) return YR_ERR_BADARG;
  if (mode != YR_OPT_ADAM && mode != YR_OPT_ADAMW) return YR_ERR_UNSUPPORTED;
  const PullAdam c = {adam_scalars(lr, step_size, bc2_sqrt, beta1, beta2, eps, weight_decay), mode == YR_OPT_ADAMW};
  hipStream_t s = (hipStream_t)stream;
#define YR_APPLY_CASE(DD)                                                                                       \
  case DD:                                                                                                      \
    return pull_apply_impl<DD>(U_old, U_new, I, mU, vU, mI, vI, gradI_out, B, num_users, num_items, inv_batch,  \
                               c, deterministic ? 1 : 0, workspace, loss_partials, loss_out, loss_accum, phases,      \
                               item_row_begin, item_row_end, item_bucket_order, s)
  switch (D) {
    YR_APPLY_CASE(16);
    YR_APPLY_CASE(32);
    YR_APPLY_CASE(64);
    YR_APPLY_CASE(128);
    default: return YR_ERR_UNSUPPORTED;
  }
#undef YR_APPLY_CASE
}

extern "C" int yr_bpr_mf_pull_apply(const float* U_old, float* U_new, float* I, float* mU, float* vU, float* mI,
                                    float* vI, float* gradI_out, int64_t B, int D, int64_t num_users,
                                    int64_t num_items, float inv_batch, double lr, double step_size, double bc2_sqrt,
                                    double beta1, double beta2, double eps, double weight_decay, int mode,
                                    int deterministic, void* workspace, int64_t workspace_bytes,
                                    float* loss_partials, float* loss_out, double* loss_accum, int phases,
                                    int64_t item_row_begin, int64_t item_row_end, void* stream) {
  return yr_bpr_mf_pull_apply_ordered(U_old, U_new, I, mU, vU, mI, vI, gradI_out, B, D, num_users, num_items,
                                      inv_batch, lr, step_size, bc2_sqrt, beta1, beta2, eps, weight_decay, mode,
                                      deterministic, workspace, workspace_bytes, loss_partials, loss_out, loss_accum,
                                      phases, item_row_begin, item_row_end, nullptr, stream);
}

extern "C" int yr_bpr_mf_pull_step(const float* U_old, float* U_new, float* I, float* mU, float* vU, float* mI,
                                   float* vI, float* gradI_out, const int64_t* user, const int64_t* pos,
                                   const int64_t* neg, int64_t B, int D, int64_t num_users, int64_t num_items,
                                   float inv_batch, double lr, double step_size, double bc2_sqrt, double beta1,
                                   double beta2, double eps, double weight_decay, int mode, int deterministic,
                                   void* workspace, int64_t workspace_bytes, float* loss_partials, float* loss_out,
                                   double* loss_accum, int32_t* err_flag, void* stream) {
  if (mode != YR_OPT_ADAM && mode != YR_OPT_ADAMW) return YR_ERR_UNSUPPORTED;
  if (!U_old || !U_new || U_old == U_new || !I || !mU || !vU || !loss_partials) return YR_ERR_BADARG;
  if (!gradI_out && (!mI || !vI)) return YR_ERR_BADARG;
  int rc = yr_bpr_mf_pull_index(user, pos, neg, B, D, num_users, num_items, workspace, workspace_bytes, err_flag,
                                stream);
  if (rc) return rc;
  return yr_bpr_mf_pull_apply(U_old, U_new, I, mU, vU, mI, vI, gradI_out, B, D, num_users, num_items, inv_batch, lr,
                              step_size, bc2_sqrt, beta1, beta2, eps, weight_decay, mode, deterministic, workspace,
                              workspace_bytes, loss_partials, loss_out, loss_accum,
                              YR_PULL_USER_PHASE | YR_PULL_ITEM_PHASE, 0, num_items, stream);
}
