// The sliding median of the post-processing kernels (postproc.hip, align_heads.hip): an odd window of W values read from a wave's row
// buffer in LDS, whose reflect halo of HALO floats on each side the caller has filled.
#pragma once
#include <hip/hip_runtime.h>

namespace wca {

constexpr int HALO = 16;      // supports filter widths up to 33

__device__ __forceinline__ void cswap(float& a, float& b) {
  const float lo = fminf(a, b), hi = fmaxf(a, b);
  a = lo;
  b = hi;
}

// median of W values starting at p (LDS), W odd, compile time
template <int W>
__device__ __forceinline__ float median_w(const float* p) {
  if (W == 1) return p[0];
  float v[W];
#pragma unroll
  for (int i = 0; i < W; ++i) v[i] = p[i];
  // odd-even transposition sort, W passes (branch free)
#pragma unroll
  for (int pass = 0; pass < W; ++pass) {
#pragma unroll
    for (int i = (pass & 1); i + 1 < W; i += 2) cswap(v[i], v[i + 1]);
  }
  return v[W / 2];
}

// generic odd width: rank selection by counting (ties broken by index) == sorted[w/2]
__device__ __forceinline__ float median_generic(const float* p, int w) {
  const int target = w >> 1;
  float res = p[0];
  for (int i = 0; i < w; ++i) {
    const float vi = p[i];
    int rank = 0;
    for (int j = 0; j < w; ++j) {
      const float vj = p[j];
      rank += (vj < vi) || (vj == vi && j < i);
    }
    if (rank == target) res = vi;
  }
  return res;
}

__device__ __forceinline__ float median_any(const float* p, int w) {
  switch (w) {
    case 1: return p[0];
    case 3: return median_w<3>(p);
    case 5: return median_w<5>(p);
    case 7: return median_w<7>(p);
    case 9: return median_w<9>(p);
    default: return median_generic(p, w);
  }
}

}  // namespace wca
