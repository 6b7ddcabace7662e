// The integer level of one log-mel value, shared by the quiet cuts (quiet_cuts.hip) and the speech segments (speech_segments.hip):
//   q(x) = rint(4096 clamp(x, -8, 8)), ties to even, NaN as 8 (loud). Everything built on it is integer arithmetic, hence exact.
#pragma once
#include <hip/hip_runtime.h>

namespace wca {

__device__ __forceinline__ int quantise(float x) {
  const float c = (x != x) ? 8.0f : fminf(fmaxf(x, -8.0f), 8.0f);
  return __float2int_rn(4096.0f * c);   // (the product is exact: a power of two, |c| <= 8)
}

}  // namespace wca
