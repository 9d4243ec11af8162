// The exact-fp32 Gram arithmetic of the [n,128] embedding sweeps (retrieval.hip, knn.hip): one definition, so that an entry of
// G = X Y^T and a row's squared norm are the same bits wherever they are formed.
#pragma once
#include "mdg_common.h"

#include <math.h>

namespace {

// one k step of eight: lane half h holds k = 8 q + 4 h + e (e = 0..3) of its row of A and of B.  Every entry of every block
// runs the same chain (q ascending, then e), so equal rows give bit-equal products wherever they sit in a tile.
__device__ __forceinline__ f32x16 gram_step(const float4 a, const float4 b, f32x16 acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
  return acc;
}

// the same k step of a row's squared norm: lane half h sums its 64 squares in this order, the two halves are then added once
__device__ __forceinline__ float norm2_step(const float4 a, float s) {
  s = fmaf(a.x, a.x, s); s = fmaf(a.y, a.y, s); s = fmaf(a.z, a.z, s); s = fmaf(a.w, a.w, s);
  return s;
}

__device__ __forceinline__ bool finite4(const float4 v) {
  return isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w);
}

}  // namespace
