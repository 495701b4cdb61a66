// The Adam / AdamW element update of torch/optim/adam.py::_single_tensor_adam (see oracle/adam.py), its scalar
// block and the host code that fills it.  Built with -ffp-contract=off: the order of the operations below is the
// reference's and is compared bit for bit.
#pragma once
#include <type_traits>

#include "common.h"

namespace yr {

struct AdamScalars {
  float decay_mul, neg_step, bc2_sqrt, one_m_b1, beta2, one_m_b2, eps, wd;
};

// step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) come from the caller (computed in double)
inline AdamScalars adam_scalars(double lr, double step_size, double bc2_sqrt, double beta1, double beta2, double eps,
                                double weight_decay) {
  AdamScalars c;
  c.decay_mul = (float)(1.0 - lr * weight_decay);
  c.neg_step = (float)(-step_size);
  c.bc2_sqrt = (float)bc2_sqrt;
  c.one_m_b1 = (float)(1.0 - beta1);
  c.beta2 = (float)beta2;
  c.one_m_b2 = (float)(1.0 - beta2);
  c.eps = (float)eps;
  c.wd = (float)weight_decay;
  return c;
}

// `decoupled` (AdamW): std::bool_constant in csrc/optim.hip, whose kernels are compiled per mode and keep no branch
// on it, and an int read from the kernel arguments in csrc/bpr_pull.hip, which has one set of kernels for both.
template <typename Flag>
__device__ __forceinline__ void adam_element(float& p, float grad, float& m, float& v, const AdamScalars& c,
                                             Flag decoupled) {
  if (c.wd != 0.0f) {
    if (decoupled) p *= c.decay_mul;
    else grad = grad + c.wd * p;
  }
  m = m + c.one_m_b1 * (grad - m);               // lerp_
  v = v * c.beta2 + (c.one_m_b2 * grad) * grad;   // mul_, addcmul_
  const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
  p = p + (c.neg_step * m) / denom;               // addcdiv_
}

// yr_adam_dense_dual (csrc/optim.hip) for callers inside the library; wide_marks: rows of 512 and 1,024 floats may
// carry touched marks (yr_bpr_mf_scatter_step, csrc/bpr_mf.hip)
int adam_dense_dual_launch(float* p0, float* g0, float* m0, float* v0, int64_t n0, float* p1, float* g1, float* m1,
                           float* v1, int64_t n1, int row_width, uint8_t* touched0, uint8_t* touched1, double lr,
                           double step_size, double bc2_sqrt, double beta1, double beta2, double eps,
                           double weight_decay, int mode, const float* loss_partials, float loss_scale,
                           float* loss_out, double* loss_accum, void* stream, bool wide_marks);

}  // namespace yr
