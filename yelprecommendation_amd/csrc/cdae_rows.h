// What the CDAE list kernels of csrc/cdae_sparse.hip and csrc/cdae_owned.hip share: the staging of one row's
// (column, value) list and the BCE term / gradient of one prediction.
#pragma once
#include "common.h"

namespace yr {

// The (column, value) list of one row, gathered from its kListParts sub-lists into LDS in column order, kListCap
// entries at a time.
constexpr int kListCap = 2048;

__device__ __forceinline__ int gather_row_list(const int32_t* __restrict__ cols, const float* __restrict__ vals,
                                               const int32_t* __restrict__ count, int64_t cpp, int64_t r, int skip,
                                               int* s_pre, int32_t* s_col, float* s_val) {
  // s_pre[q] = number of entries before part q; returns the number of entries staged (<= kListCap),
  // starting at overall entry `skip`
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int q = 0; q < kListParts; ++q) { s_pre[q] = acc; acc += count[r * kListParts + q]; }
    s_pre[kListParts] = acc;
  }
  __syncthreads();
  const int total = s_pre[kListParts];
  const int n = min(kListCap, total - skip);
  for (int i = threadIdx.x; i < n; i += kBlock) {
    const int e = skip + i;
    int q = 0;
#pragma unroll
    for (int s = kListParts / 2; s >= 1; s >>= 1)
      if (s_pre[q + s] <= e) q += s;
    const int64_t at = (r * kListParts + q) * cpp + (e - s_pre[q]);
    s_col[i] = cols[at];
    s_val[i] = vals[at];
  }
  __syncthreads();
  return n;
}

__device__ __forceinline__ float decode_output(float pre, int act) {
  return act == 1 ? 1.0f / (1.0f + expf(-pre)) : pre;
}

// the BCE term of a prediction y for target t (logarithms clamped at -100 as torch's BCELoss), and its gradient
// w.r.t. the pre-activation
__device__ __forceinline__ float bce_term(float y, float t) {
  return -(t * fmaxf(logf(y), -100.0f) + (1.0f - t) * fmaxf(logf(1.0f - y), -100.0f));
}

__device__ __forceinline__ float bce_grad(float y, float t, int act) {
  float g = (y - t) / fmaxf((1.0f - y) * y, 1e-12f);
  if (act == 1) g *= y * (1.0f - y);
  return g;
}

}  // namespace yr
