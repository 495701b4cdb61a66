// Which owner workgroup of the pull-form BPR step (bpr_pull.hip) takes which bucket: the slot -> bucket map and the
// start order built on it.  Plain C++ (host and device), so that a host program can compile it on its own.
//
// Workgroups are dealt round-robin over the 8 XCDs (blocks b and b + 8 share one) and every XCD has an L2 of its own,
// while the records of neighbouring buckets share 128-byte lines (a bucket's segment in one tile is two to four
// records) and 32 buckets share a line of `off`: with slot = bucket every such line is fetched from the fabric by
// several L2s.  So the slots s with equal s % 8 — one XCD's workgroups — take neighbouring buckets: class c = s % 8 gets
// runs of kXcdRun consecutive buckets, run after run dealt over the eight classes (runs, not eighths of the table: a
// table whose activity follows the id still spreads over all XCDs).  A bijection whatever the dispatcher does:
// placement is a matter of speed only.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define YR_PLACEMENT_FN __host__ __device__ __forceinline__
#else
#define YR_PLACEMENT_FN inline
#endif

#ifndef YR_XCD_RUN
#define YR_XCD_RUN 8
#endif

namespace yr {

constexpr int kXcds = 8;
constexpr int kXcdRun = YR_XCD_RUN;             // G: consecutive buckets of one class
static_assert(kXcdRun >= 1 && kXcdRun <= 256 && (kXcdRun & (kXcdRun - 1)) == 0, "runs of a power of two buckets");
constexpr int kXcdRunShift = __builtin_ctz(kXcdRun);
constexpr int kXcdRound = kXcds * kXcdRun;      // one run for every class

// slots of n buckets: n rounded up to whole rounds (the slots whose bucket is >= n have none)
YR_PLACEMENT_FN int owner_slots(int n) { return (n + kXcdRound - 1) & ~(kXcdRound - 1); }

// slot -> bucket, a bijection of [0, owner_slots(n)): slot s = 8 j + c is the j-th bucket of class c
YR_PLACEMENT_FN int owner_bucket(int s) {
  const int c = s & (kXcds - 1), j = s >> 3;
  return ((((j >> kXcdRunShift) << 3) + c) << kXcdRunShift) + (j & (kXcdRun - 1));
}

// Start order of the item pass: order[s] = the heaviest unused bucket of class s % 8 (the class owner_bucket gives the
// bucket), and the heaviest bucket left over once that class is used up.  A permutation of [0, nb), heaviest first
// inside every class; equal loads by index.
inline void owner_start_order(const double* load, int nb, int32_t* order) {
  std::vector<int32_t> by_load(nb);
  for (int k = 0; k < nb; ++k) by_load[k] = k;
  std::stable_sort(by_load.begin(), by_load.end(), [load](int32_t a, int32_t b) { return load[a] > load[b]; });
  std::vector<unsigned char> cls(nb), used(nb, 0);
  for (int s = 0, n = owner_slots(nb); s < n; ++s)
    if (owner_bucket(s) < nb) cls[owner_bucket(s)] = (unsigned char)(s & (kXcds - 1));
  std::vector<int32_t> queue[kXcds];             // every class's buckets, heaviest first
  for (int i = 0; i < nb; ++i) queue[cls[by_load[i]]].push_back(by_load[i]);
  size_t head[kXcds] = {}, rest = 0;
  for (int s = 0; s < nb; ++s) {
    const int c = s & (kXcds - 1);
    while (head[c] < queue[c].size() && used[queue[c][head[c]]]) ++head[c];
    int32_t k;
    if (head[c] < queue[c].size()) {
      k = queue[c][head[c]++];
    } else {
      while (used[by_load[rest]]) ++rest;
      k = by_load[rest];
    }
    used[k] = 1;
    order[s] = k;
  }
}

}  // namespace yr
