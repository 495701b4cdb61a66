// Device-side BPR triplet stream for gfx950 — the producer side of the reference's
//   DataLoader(MFDataset, shuffle=True)      (train.py:76-77)
//   MFDataset.__getitem__ / _negative_sampling (data/datasets/mf_dataset.py:18-32)
// i.e. one random permutation of the rows per epoch and, for every row, a negative item drawn
// uniformly from [0, num_items) and redrawn while it is one of that user's positives.  The
// reference does this per row on the host (pandas .iloc + a Python `in list` test, ~65 us per row);
// here position t of epoch e is a pure function of (seed, e, t): no state, no host round trip, any
// slice [first, first + count) of an epoch can be produced on its own (a batch, a rank's share).
//
//   row(t)  = P(t), P a keyed bijection of [0, n_rows): a 4-round Feistel network over the smallest
//             even-width bit domain that holds n_rows, cycle-walked back into range
//   neg(t)  = first draw d = 0, 1, ... of  floor(u32 * num_items / 2^32)  (Lemire's unbiased
//             multiply-shift; u32 from Philox4x32-7 keyed by (seed, epoch), counter (t, d)) that is
//             not in the user's sorted avoid-list (binary search)
// Integer work: the CPU statement oracle/triplet_sampler.py gives the same words bit for bit.
#include "common.h"
#include "sample.h"

namespace yr {

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {       // murmur3 finaliser
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}

// keyed bijection of [0, 2^(2 half_bits)): balanced Feistel, 4 rounds
__device__ __forceinline__ uint64_t feistel(uint64_t x, int half_bits, uint32_t k0, uint32_t k1) {
  const uint32_t mask = half_bits >= 32 ? 0xFFFFFFFFu : ((1u << half_bits) - 1u);
  uint32_t L = (uint32_t)(x >> half_bits) & mask, R = (uint32_t)x & mask;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint32_t f = fmix32(R ^ (r & 1 ? k1 : k0) ^ (0x9E3779B9u * (uint32_t)(r + 1))) & mask;
    const uint32_t t = L ^ f;
    L = R;
    R = t;
  }
  return ((uint64_t)L << half_bits) | R;
}

__global__ __launch_bounds__(kBlock) void triplet_sample_kernel(
    const int64_t* __restrict__ row_user, const int64_t* __restrict__ row_item, int64_t n_rows,
    const int64_t* __restrict__ avoid_ptr, const int64_t* __restrict__ avoid_idx, int64_t num_users,
    int64_t num_items, uint64_t seed, uint64_t epoch, int shuffle, int half_bits, int64_t first, int64_t count,
    int64_t* __restrict__ user_out, int64_t* __restrict__ pos_out, int64_t* __restrict__ neg_out,
    int32_t* __restrict__ err_flag) {
  const uint32_t k0 = fmix32((uint32_t)seed ^ 0x243F6A88u) ^ (uint32_t)epoch;
  const uint32_t k1 = fmix32((uint32_t)(seed >> 32) ^ 0x85A308D3u) ^ (uint32_t)(epoch >> 32) ^ fmix32((uint32_t)epoch);
  const uint2 key = sample_key(seed, epoch);
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) {
    const int64_t t = first + i;
    uint64_t r = (uint64_t)t;
    if (shuffle) {
      do { r = feistel(r, half_bits, k0, k1); } while (r >= (uint64_t)n_rows);   // cycle walking: < 4 rounds expected
    }
    const int64_t u = row_user[r], p = row_item[r];
    int64_t neg = 0;
    if ((uint64_t)u >= (uint64_t)num_users || (uint64_t)p >= (uint64_t)num_items) {
      if (err_flag) atomicOr(err_flag, (uint64_t)u >= (uint64_t)num_users ? YR_FLAG_BAD_USER : YR_FLAG_BAD_ITEM);
      user_out[i] = u; pos_out[i] = p; neg_out[i] = 0;
      continue;
    }
    const int64_t lo0 = avoid_ptr[u], hi0 = avoid_ptr[u + 1];
    for (int d = 0;; ++d) {
      neg = (int64_t)sample_draw((uint64_t)t, (uint32_t)d, (uint32_t)num_items, key);
      if (!sorted_contains(avoid_idx, lo0, hi0, neg)) break;
      if (d + 1 >= kMaxDraws) {
        // a user whose avoid list covers (almost) the whole catalogue: walk to the next free item
        // (the reference would loop forever on a full list; here: flag and emit item 0)
        int64_t c = neg, steps = 0;
        while (steps < num_items) {
          c = c + 1 == num_items ? 0 : c + 1;
          ++steps;
          if (!sorted_contains(avoid_idx, lo0, hi0, c)) break;
        }
        if (steps >= num_items) {
          if (err_flag) atomicOr(err_flag, YR_FLAG_BAD_ITEM);
          c = 0;
        }
        neg = c;
        break;
      }
    }
    user_out[i] = u;
    pos_out[i] = p;
    neg_out[i] = neg;
  }
}

}  // namespace yr

using namespace yr;

extern "C" int yr_triplet_sample(const int64_t* row_user, const int64_t* row_item, int64_t n_rows,
                                 const int64_t* avoid_ptr, const int64_t* avoid_idx, int64_t num_users,
                                 int64_t num_items, uint64_t seed, uint64_t epoch, int shuffle, int64_t first,
                                 int64_t count, int64_t* user_out, int64_t* pos_out, int64_t* neg_out,
                                 int32_t* err_flag, void* stream) {
  if (n_rows < 0 || count < 0 || first < 0 || first + count > n_rows || num_users <= 0 || num_items <= 0)
    return YR_ERR_BADARG;
  if (num_items > 0xFFFFFFFFll) return YR_ERR_UNSUPPORTED;
  if (count == 0) return 0;
  if (!row_user || !row_item || !avoid_ptr || !avoid_idx || !user_out || !pos_out || !neg_out) return YR_ERR_BADARG;
  // smallest even-width domain 2^(2 h) >= n_rows (at least 2 bits so that both halves exist)
  int half_bits = 1;
  while (half_bits < 32 && ((uint64_t)1 << (2 * half_bits)) < (uint64_t)n_rows) ++half_bits;
  hipLaunchKernelGGL(triplet_sample_kernel, dim3(grid_for(count, kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                     row_user, row_item, n_rows, avoid_ptr, avoid_idx, num_users, num_items, seed, epoch, shuffle,
                     half_bits, first, count, user_out, pos_out, neg_out, err_flag);
  return launch_status();
}
