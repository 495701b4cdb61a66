// The counting sort of a triplet batch by destination row, shared by the owner passes of csrc/ngcf_owned.hip and
// csrc/dcn_owned.hip.  The 3 B (destination row, triplet, role) entries — rows [0, num_users) the users, rows
// num_users + item the items — are counted per row with integer atomics (which also hand every entry its arrival slot),
// scanned (owned_scan.h) and filled into their rows' segments; WHICH slot of its segment an entry takes depends on
// arrival, so ngcf_owned_rank_kernel rewrites every segment by ascending key = 4 x triplet + role (user 0, positive 1,
// negative 2; the keys of a row are distinct): an entry's place is the number of smaller keys in its segment, an integer
// that no order of execution changes.  Integer work only.
// EACH = false (NGCF): a triplet with any id out of range is skipped as a whole.  EACH = true (DCN): every entry is
// judged by its own id — a bad user drops the user entry only, a bad item its own entry only.
#pragma once
#include "common.h"

namespace yr {

constexpr int kRoleUser = 0, kRolePos = 1, kRoleNeg = 2;

// ids of triplet b; false (and the flag bits) when one of them is out of range
template <bool NEG>
__device__ __forceinline__ bool owned_triplet(const int64_t* __restrict__ user, const int64_t* __restrict__ pos,
                                              const int64_t* __restrict__ neg, int64_t b, int64_t num_users,
                                              int64_t num_items, int64_t& u, int64_t& p, int64_t& n, int& bad) {
  u = user[b]; p = pos[b]; n = NEG ? neg[b] : 0;
  bool ok = true;
  if (u < 0 || u >= num_users) { bad |= YR_FLAG_BAD_USER; ok = false; }
  if (p < 0 || p >= num_items || n < 0 || n >= num_items) { bad |= YR_FLAG_BAD_ITEM; ok = false; }
  return ok;
}

// cnt[row] = entries of the row; slot[3 b + role] = the entry's arrival number inside its row
template <bool NEG, bool EACH = false>
__global__ __launch_bounds__(kBlock) void ngcf_owned_count_kernel(const int64_t* __restrict__ user,
                                                                  const int64_t* __restrict__ pos,
                                                                  const int64_t* __restrict__ neg, int64_t B,
                                                                  int64_t num_users, int64_t num_items,
                                                                  int32_t* __restrict__ cnt, int32_t* __restrict__ slot,
                                                                  int32_t* __restrict__ err_flag) {
  int bad = 0;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x; b < B; b += stride) {
    int64_t u, p, n;
    const bool ok = owned_triplet<NEG>(user, pos, neg, b, num_users, num_items, u, p, n, bad);
    if (!EACH && !ok) continue;
    if (!EACH || (u >= 0 && u < num_users)) slot[3 * b + kRoleUser] = atomicAdd(cnt + u, 1);
    if (!EACH || (p >= 0 && p < num_items)) slot[3 * b + kRolePos] = atomicAdd(cnt + num_users + p, 1);
    if (NEG && (!EACH || (n >= 0 && n < num_items))) slot[3 * b + kRoleNeg] = atomicAdd(cnt + num_users + n, 1);
  }
  if (bad && err_flag) atomicOr(err_flag, bad);
}

template <bool NEG, bool EACH = false>
__global__ __launch_bounds__(kBlock) void ngcf_owned_fill_kernel(const int64_t* __restrict__ user,
                                                                 const int64_t* __restrict__ pos,
                                                                 const int64_t* __restrict__ neg, int64_t B,
                                                                 int64_t num_users, int64_t num_items,
                                                                 const int32_t* __restrict__ start,
                                                                 const int32_t* __restrict__ slot,
                                                                 int32_t* __restrict__ ent) {
  int bad = 0;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x; b < B; b += stride) {
    int64_t u, p, n;
    const bool ok = owned_triplet<NEG>(user, pos, neg, b, num_users, num_items, u, p, n, bad);
    if (!EACH && !ok) continue;
    const int32_t key = (int32_t)(4 * b);
    if (!EACH || (u >= 0 && u < num_users)) ent[start[u] + slot[3 * b + kRoleUser]] = key + kRoleUser;
    if (!EACH || (p >= 0 && p < num_items)) ent[start[num_users + p] + slot[3 * b + kRolePos]] = key + kRolePos;
    if (NEG && (!EACH || (n >= 0 && n < num_items)))
      ent[start[num_users + n] + slot[3 * b + kRoleNeg]] = key + kRoleNeg;
  }
}

// sorted[segment start + (number of smaller keys in the segment)] = key, a thread per entry
static __global__ __launch_bounds__(kBlock) void ngcf_owned_rank_kernel(const int64_t* __restrict__ user,
                                                                        const int64_t* __restrict__ pos,
                                                                        const int64_t* __restrict__ neg,
                                                                        int64_t num_users, int64_t n_rows,
                                                                        const int32_t* __restrict__ start,
                                                                        const int32_t* __restrict__ ent,
                                                                        int32_t* __restrict__ sorted) {
  const int64_t total = start[n_rows];
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += stride) {
    const int32_t key = ent[e];
    const int64_t b = key >> 2;
    const int role = key & 3;
    const int64_t row = role == kRoleUser ? user[b] : num_users + (role == kRolePos ? pos[b] : neg[b]);
    const int s0 = start[row], s1 = start[row + 1];
    int rank = 0;
    for (int j = s0; j < s1; ++j) rank += ent[j] < key;
    sorted[s0 + rank] = key;
  }
}

}  // namespace yr
