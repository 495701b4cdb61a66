// Device-side S3Rec sequence batches for gfx950 — the producer side of the reference's
//   S3RecDataPipeline.split / _adjust_seq_len   (data/datasets/s3rec_data_pipeline.py:13-50)
//   S3RecDataset.__getitem__ / _negative_sampling (data/datasets/s3rec_dataset.py:21-57)
// i.e. per user the last L entries of a prefix of the behaviour row (X) and of the same prefix moved on (Y), left
// padded, ids shifted by one so that 0 is the pad; per training position one negative in 1..num_items that is not an
// avoided value; per test user n_neg mutually distinct ones.  The reference does this per user on the host, a Python
// `in list` test per draw; here a user's rows are a pure function of (seed, epoch, mode, user): no state, no host
// round trip, any batch of users on its own equals the same rows of the whole epoch.
//
//   windows, n = row length, cut = 3 / 2 / 1 for train / valid / test:
//     X = row[0, max(0, n - cut)),  Y = row[4 - cut, n - cut + 1)   (empty when the start is not below the end)
//   train / valid: neg[j] = 1 + first draw d = 0, 1, ... of element t = user L + j that is not avoided; after
//     kMaxDraws rejected draws the next free value after the last draw, walking 1..num_items cyclically
//   test: the first n_neg of the candidates c_d = 1 + draw(user, d), d < kMaxDraws, that are neither avoided nor equal
//     to an earlier accepted one; the rest from an ascending scan of 1..num_items
//   nothing free: 0 and YR_FLAG_BAD_ITEM (the reference would loop forever)
// The draw is csrc/sample.h's, as in csrc/triplets.hip.  Integer work: the CPU statement tests/s3rec_batches_ref.py
// gives the same words bit for bit.
#include "common.h"
#include "sample.h"

namespace yr {

constexpr int kS3MaxNeg = 128;   // the accepted list of a test user lives in LDS

// entry j of a window: the last L entries of row[start, end), left padded with 0, ids + 1
__device__ __forceinline__ int64_t window_entry(const int64_t* __restrict__ row, int64_t start, int64_t end, int L,
                                                int j, int64_t num_items, bool& bad) {
  const int64_t at = end - L + j;
  if (at < start) return 0;                       // the pad; an empty slice (end <= start) is all pad
  const int64_t v = row[at];
  if ((uint64_t)v >= (uint64_t)num_items) { bad = true; return 0; }
  return v + 1;
}

// train / valid: a thread per (sequence, position)
__global__ __launch_bounds__(kBlock) void s3rec_seq_batches_kernel(
    const int64_t* __restrict__ beh_ptr, const int64_t* __restrict__ beh_idx, const int64_t* __restrict__ avoid_ptr,
    const int64_t* __restrict__ avoid_idx, int64_t num_users, int64_t num_items, const int64_t* __restrict__ users,
    int64_t B, int L, int cut, uint64_t seed, uint64_t epoch, int64_t* __restrict__ X, int64_t* __restrict__ pos,
    int64_t* __restrict__ neg, int32_t* __restrict__ err_flag) {
  const uint2 key = sample_key(seed, epoch);
  const uint32_t n32 = (uint32_t)num_items;
  const int64_t total = B * L, stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
    const int64_t b = i / L;
    const int j = (int)(i - b * L);
    const int64_t u = users[b];
    if ((uint64_t)u >= (uint64_t)num_users) {
      if (err_flag) atomicOr(err_flag, YR_FLAG_BAD_USER);
      X[i] = 0; pos[i] = 0; neg[i] = 0;
      continue;
    }
    const int64_t r0 = beh_ptr[u], n = beh_ptr[u + 1] - r0;
    bool bad = false;
    X[i] = window_entry(beh_idx + r0, 0, n - cut > 0 ? n - cut : 0, L, j, num_items, bad);
    pos[i] = window_entry(beh_idx + r0, 4 - cut, n - cut + 1, L, j, num_items, bad);
    // one negative per position, the pad positions too (s3rec_dataset.py:45 draws pos_items.shape[0] of them)
    const int64_t lo0 = avoid_ptr[u], hi0 = avoid_ptr[u + 1];
    const uint64_t t = (uint64_t)u * (uint64_t)L + (uint64_t)j;
    int64_t c = 0;
    for (int d = 0;; ++d) {
      c = 1 + (int64_t)sample_draw(t, (uint32_t)d, n32, key);
      if (!sorted_contains(avoid_idx, lo0, hi0, c)) break;
      if (d + 1 >= kMaxDraws) {
        int64_t steps = 0;
        while (steps < num_items) {
          c = c == num_items ? 1 : c + 1;
          ++steps;
          if (!sorted_contains(avoid_idx, lo0, hi0, c)) break;
        }
        if (steps >= num_items) { bad = true; c = 0; }
        break;
      }
    }
    neg[i] = c;
    if (bad && err_flag) atomicOr(err_flag, YR_FLAG_BAD_ITEM);
  }
}

// One round of a test user's wave: lane l holds candidate c (live: it is one).  A candidate is accepted when it is
// not avoided, not in the accepted list and not the value of a lower live lane (distinct: candidates that cannot
// repeat inside a round skip that test); the accepted ones keep their lane order.  Returns the new length of the list.
__device__ __forceinline__ int s3rec_accept_round(uint32_t c, bool live, bool distinct,
                                                  const int64_t* __restrict__ avoid_idx, int64_t lo0, int64_t hi0,
                                                  uint32_t* acc, int count, int n_neg, int64_t* __restrict__ out,
                                                  int lane) {
  bool ok = live && !sorted_contains(avoid_idx, lo0, hi0, (int64_t)c);
  if (ok) {
    for (int k = 0; k < count; ++k) {
      if (acc[k] == c) { ok = false; break; }
    }
  }
  if (!distinct) {
    // only the first occurrence inside a round can be accepted: equal values share the two answers above, so a lower
    // lane with this value is either refused with it or accepted before it
    for (int k = 0; k < kWave - 1; ++k) {
      const uint32_t ck = (uint32_t)__shfl((int)c, k, kWave);
      if (k < lane && ck == c) ok = false;
    }
  }
  const unsigned long long m = __ballot(ok);
  const int slot = count + __popcll(m & ((1ull << lane) - 1ull));
  if (ok && slot < n_neg) {
    acc[slot] = c;
    out[slot] = (int64_t)c;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the list is read by every lane of the next round
  __builtin_amdgcn_wave_barrier();
  const int have = count + __popcll(m);
  return have < n_neg ? have : n_neg;
}

// test: a wave per user
__global__ __launch_bounds__(kBlock) void s3rec_test_batches_kernel(
    const int64_t* __restrict__ beh_ptr, const int64_t* __restrict__ beh_idx, const int64_t* __restrict__ avoid_ptr,
    const int64_t* __restrict__ avoid_idx, int64_t num_users, int64_t num_items, const int64_t* __restrict__ users,
    int64_t B, int L, int n_neg, uint64_t seed, uint64_t epoch, int64_t* __restrict__ X, int64_t* __restrict__ pos,
    int64_t* __restrict__ neg, int32_t* __restrict__ err_flag) {
  __shared__ uint32_t s_acc[kWavesPerBlock][kS3MaxNeg];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  uint32_t* acc = s_acc[wave];
  const uint2 key = sample_key(seed, epoch);
  const uint32_t n32 = (uint32_t)num_items;
  for (int64_t b = (int64_t)blockIdx.x * kWavesPerBlock + wave; b < B; b += (int64_t)gridDim.x * kWavesPerBlock) {
    const int64_t u = users[b];
    int64_t* xo = X + b * L;
    int64_t* no = neg + b * n_neg;                 // dereferenced below n_neg only
    if ((uint64_t)u >= (uint64_t)num_users) {
      if (lane == 0 && err_flag) atomicOr(err_flag, YR_FLAG_BAD_USER);
      for (int j = lane; j < L; j += kWave) xo[j] = 0;
      for (int k = lane; k < n_neg; k += kWave) no[k] = 0;
      if (lane == 0) pos[b] = 0;
      continue;
    }
    const int64_t r0 = beh_ptr[u], n = beh_ptr[u + 1] - r0;
    bool bad = false;
    for (int j = lane; j < L; j += kWave) xo[j] = window_entry(beh_idx + r0, 0, n - 1 > 0 ? n - 1 : 0, L, j, num_items, bad);
    if (lane == 0) pos[b] = window_entry(beh_idx + r0, 3, n, L, L - 1, num_items, bad);   // Y[-1]
    const int64_t lo0 = avoid_ptr[u], hi0 = avoid_ptr[u + 1];
    int count = 0;
    for (int r = 0; r < kMaxDraws / kWave && count < n_neg; ++r) {
      const uint32_t c = 1u + sample_draw((uint64_t)u, (uint32_t)(r * kWave + lane), n32, key);
      count = s3rec_accept_round(c, true, false, avoid_idx, lo0, hi0, acc, count, n_neg, no, lane);
    }
    for (int64_t base = 1; base <= num_items && count < n_neg; base += kWave) {
      const int64_t v = base + lane;
      count = s3rec_accept_round((uint32_t)v, v <= num_items, true, avoid_idx, lo0, hi0, acc, count, n_neg, no, lane);
    }
    for (int k = count + lane; k < n_neg; k += kWave) no[k] = 0;
    if (count < n_neg && lane == 0) bad = true;
    if (bad && err_flag) atomicOr(err_flag, YR_FLAG_BAD_ITEM);
  }
}

}  // namespace yr

using namespace yr;

extern "C" int yr_s3rec_batches(const int64_t* beh_ptr, const int64_t* beh_idx, const int64_t* avoid_ptr,
                                const int64_t* avoid_idx, int64_t num_users, int64_t num_items, const int64_t* users,
                                int64_t B, int L, int mode, int n_neg, uint64_t seed, uint64_t epoch, int64_t* X,
                                int64_t* pos, int64_t* neg, int32_t* err_flag, void* stream) {
  if (B < 0 || L <= 0 || n_neg < 0 || num_users <= 0 || num_items <= 0) return YR_ERR_BADARG;
  if (n_neg > kS3MaxNeg || num_items > 0xFFFFFFFFll ||
      (mode != YR_S3REC_TRAIN && mode != YR_S3REC_VALID && mode != YR_S3REC_TEST))
    return YR_ERR_UNSUPPORTED;
  if (mode != YR_S3REC_TEST && n_neg != L) return YR_ERR_BADARG;     // one negative per position
  if (B == 0) return 0;
  if (!beh_ptr || !beh_idx || !avoid_ptr || !avoid_idx || !users || !X || !pos || (!neg && n_neg > 0))
    return YR_ERR_BADARG;
  if (mode == YR_S3REC_TEST) {
    hipLaunchKernelGGL(s3rec_test_batches_kernel, dim3(grid_for(B, kWavesPerBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, beh_ptr, beh_idx, avoid_ptr, avoid_idx, num_users, num_items, users, B, L,
                       n_neg, seed, epoch, X, pos, neg, err_flag);
  } else {
    hipLaunchKernelGGL(s3rec_seq_batches_kernel, dim3(grid_for(B * L, kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                       beh_ptr, beh_idx, avoid_ptr, avoid_idx, num_users, num_items, users, B, L,
                       mode == YR_S3REC_TRAIN ? 3 : 2, seed, epoch, X, pos, neg, err_flag);
  }
  return launch_status();
}
