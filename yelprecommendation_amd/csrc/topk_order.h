// The one order of every top-k list the engine emits (csrc/topk.hip, csrc/eval_topk.hip): score descending, item
// id ascending among equal scores (the reference's order among exact ties is unspecified).
#pragma once
#include "common.h"

namespace yr {

struct TopEntry {
  float s;
  int32_t i;
};

__device__ __forceinline__ bool better(float s, int32_t i, float s2, int32_t i2) {
  return s > s2 || (s == s2 && i < i2);
}

}  // namespace yr
