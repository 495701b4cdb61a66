// The DCN head shared by its two kernels (csrc/dcn.hip: dcn_head_kernel, csrc/dcn_owned.hip: dcn_head_ordered_kernel):
// the limits, the row-independent constants of the closed-form cross network and the kernels' argument block.  The row
// loop itself is dcn_head_rows.h, included inside both kernels.
#pragma once
#include "common.h"

namespace yr {

constexpr int kDcnMaxF = 512;                 // 4 * D, D <= 128
constexpr int kDcnMaxH = 1024;                // width of the last hidden layer
constexpr int kDcnMaxL = 8;                   // cross orders
constexpr int kDcnEF = kDcnMaxF / kWave;      // elements of an F-vector per lane
constexpr int kDcnEH = kDcnMaxH / kWave;      // elements of an H-vector per lane

// --------------------------------------------------------------------------- cross-network constants
// The row-independent parts of the closed form, computed by every wave for itself (L * F multiply-adds):
//   bw[l] = beta_l . w_l,   boc = beta_L . W_oc + b_o,   beta[] = this lane's slice of beta_L.
__device__ __forceinline__ void dcn_cross_consts(const float* __restrict__ cw, const float* __restrict__ cb,
                                                 const float* __restrict__ Woc, const float* __restrict__ bo, int L,
                                                 int F, int lane, float (&bw)[kDcnMaxL], float& boc,
                                                 float (&beta)[kDcnEF]) {
#pragma unroll
  for (int j = 0; j < kDcnEF; ++j) beta[j] = 0.0f;
#pragma unroll
  for (int l = 0; l < kDcnMaxL; ++l) {
    bw[l] = 0.0f;
    if (l < L) {
      float t = 0.0f;
#pragma unroll
      for (int j = 0; j < kDcnEF; ++j) {
        const int e = lane + kWave * j;
        if (e < F) {
          t += beta[j] * cw[l * F + e];
          beta[j] += cb[l * F + e];
        }
      }
      bw[l] = wave_sum(t);
    }
  }
  float t = 0.0f;
#pragma unroll
  for (int j = 0; j < kDcnEF; ++j) {
    const int e = lane + kWave * j;
    if (e < F) t += beta[j] * Woc[e];
  }
  boc = wave_sum(t) + bo[0];
}

__device__ __forceinline__ float sigmoidf(float z) { return 1.0f / (1.0f + expf(-z)); }

// --------------------------------------------------------------------------- fused head
// One wave per unit: a triplet (bpr: rows b and B + b, pos and neg side by side) or a row.  Forward:
//   z = W_od . h + alpha_L (W_oc . x0) + boc,  pred = sigmoid(z),  loss += softplus(-(pred_pos - pred_neg)).
// Backward (dx0 != NULL): dpred = the BPR gradient (inv_batch = 1 / B) or gpred[r]; dz = dpred pred (1 - pred);
//   dh = dz W_od gated by h > 0 (h is the post-ReLU activation), dx0 = the cross part of d x0, and the weight
//   gradients accumulated per workgroup in LDS, then added to dcw / dcb / dWo / dbo.
struct DcnHead {
  const float* x0;
  int64_t ldx;
  const float* h;
  int64_t ldh;
  int64_t units;
  int F, H, L;
  const float *cw, *cb, *Wo, *bo;
  int bpr;
  float inv_batch;
  float* pred;
  const float* gpred;
  float* dh;
  int64_t lddh;
  float* dx0;
  int64_t lddx;
  float *dcw, *dcb, *dWo, *dbo;
  float* loss_partials;
};

constexpr int kHeadAcc = (2 * kDcnMaxL + 1) * kDcnMaxF + kDcnMaxH + 1;

}  // namespace yr
