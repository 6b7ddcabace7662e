// Per-token log-probabilities of the teacher-forced text (openai-whisper's word `probability`, timing.py:146-150 of the reference:
// softmax over logits[len(sot_sequence):, :eot] at the teacher token, here in log space).
//
//   gather_text_rows_kernel  the f32 residual rows that PREDICT a text token (row sot_len + i of utterance b, i < n_text_b) -> a
//                            compact [R][d] buffer, and the row map r -> b * n_tok_max + i (where the result goes; the target is
//                            the token tokens[b][sot_len + 1 + i] = tokens_flat[map[r] + sot_len + 1])
//   token_logprob_kernel     one workgroup per row: ONE read of the row's [0, vocab_end) logits with float4 loads, a per-lane online
//                            (max, sum of exp) in f32, wave-64 shuffle reduction, LDS combine over the 4 waves;
//                            out = z[target] - (max + log(sum))
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernels.h"

namespace wca {
namespace {

constexpr int TP_THREADS = 256;  // 4 waves: the row (~200 KB of logits) is streamed once, about 50 float4 per lane
constexpr int TP_WAVES = TP_THREADS / 64;

// grid (n_text_max, B): block (i, b) copies row b * n_tok_max + sot_len + i when i < n_text_b
__global__ void __launch_bounds__(256) gather_text_rows_kernel(const float* __restrict__ x, int n_tok_max, int d, int sot_len,
                                                               const int* __restrict__ n_tok, const int* __restrict__ row_off,
                                                               float* __restrict__ out, int* __restrict__ row_map) {
  const int i = blockIdx.x, b = blockIdx.y;
  const int n_text = n_tok[b] - sot_len - 2;
  if (i >= n_text) return;
  const long r = row_off[b] + i;
  const float* src = x + ((long)b * n_tok_max + sot_len + i) * d;
  float* dst = out + r * d;
  for (int c = threadIdx.x; c < d; c += blockDim.x) dst[c] = src[c];
  if (threadIdx.x == 0) row_map[r] = b * n_tok_max + i;
}

// (m, s) pairs: s = sum exp(v - m). Combining with an empty side (m = -inf, s = 0) leaves the other side as it is.
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
  const float mm = fmaxf(m, m2);
  if (mm == -INFINITY) return;
  s = s * __expf(m - mm) + s2 * __expf(m2 - mm);
  m = mm;
}

__device__ __forceinline__ void lse_push4(float& m, float& s, float4 v) {
  const float vm = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
  const float mm = fmaxf(m, vm);
  if (mm == -INFINITY) return;
  s = s * __expf(m - mm) + (__expf(v.x - mm) + __expf(v.y - mm)) + (__expf(v.z - mm) + __expf(v.w - mm));
  m = mm;
}

__device__ __forceinline__ void lse_push1(float& m, float& s, float v) {
  const float mm = fmaxf(m, v);
  if (mm == -INFINITY) return;
  s = s * __expf(m - mm) + __expf(v - mm);
  m = mm;
}

// row r: logits + r * ld, columns [0, vocab_end); idx = row_map ? row_map[r] : r; target = targets[idx + tgt_off]; out[idx] = log p.
// A target outside [0, vocab_end) has no value: NaN, and bit `err_bit` is raised in *err.
__global__ void __launch_bounds__(TP_THREADS) token_logprob_kernel(const float* __restrict__ logits, long ld, int vocab_end,
                                                                   const int64_t* __restrict__ targets, const int* __restrict__ row_map,
                                                                   int tgt_off, float* __restrict__ out, int* __restrict__ err, int err_bit) {
  const int r = blockIdx.x;
  const float* z = logits + (long)r * ld;
  float m = -INFINITY, s = 0.f;
  // float4 body where the row start is 16-byte aligned (every row when ld % 4 == 0 and the base is aligned), scalar head otherwise
  const int head = (int)(((16 - ((uintptr_t)z & 15)) & 15) >> 2);
  const int h = head < vocab_end ? head : vocab_end;
  if ((((uintptr_t)z) & 3) != 0) {
    for (int c = threadIdx.x; c < vocab_end; c += TP_THREADS) lse_push1(m, s, z[c]);
  } else {
    if ((int)threadIdx.x < h) lse_push1(m, s, z[threadIdx.x]);
    const int n4 = (vocab_end - h) >> 2;
    const float4* z4 = reinterpret_cast<const float4*>(z + h);
    int k = threadIdx.x;
    for (; k + TP_THREADS < n4; k += 2 * TP_THREADS) {   // two loads in flight per lane
      const float4 a = z4[k], c = z4[k + TP_THREADS];
      lse_push4(m, s, a);
      lse_push4(m, s, c);
    }
    if (k < n4) lse_push4(m, s, z4[k]);
    const int t = h + 4 * n4 + (int)threadIdx.x;
    if (t < vocab_end) lse_push1(m, s, z[t]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lse_merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
  __shared__ float sm[TP_WAVES], ss[TP_WAVES];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sm[w] = m;
    ss[w] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float M = sm[0], S = ss[0];
    for (int k = 1; k < TP_WAVES; ++k) lse_merge(M, S, sm[k], ss[k]);
    const int idx = row_map ? row_map[r] : r;
    const int64_t tg = targets[(long)idx + tgt_off];
    if (tg < 0 || tg >= vocab_end) {
      out[idx] = NAN;
      atomicOr(err, err_bit);
    } else {
      // one rounding at the end (|log p| reaches ~160 for logits of +-80, where half an f32 ulp is already 7.6e-6)
      out[idx] = (float)(((double)z[tg] - (double)M) - log((double)S));
    }
  }
}

}  // namespace

hipError_t launch_gather_text_rows(const float* x, int n_tok_max, int d, int sot_len, const int* n_tok, const int* row_off, int B, int n_text_max,
                                   float* out, int* row_map, hipStream_t s) {
  if (n_text_max <= 0 || B <= 0) return hipSuccess;
  hipLaunchKernelGGL(gather_text_rows_kernel, dim3((unsigned)n_text_max, (unsigned)B), dim3(256), 0, s, x, n_tok_max, d, sot_len, n_tok, row_off,
                     out, row_map);
  return hipGetLastError();
}

hipError_t launch_token_logprob(const float* logits, long ld, int vocab_end, int rows, const int64_t* targets, const int* row_map, int tgt_off,
                                float* out, int* err, int err_bit, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (vocab_end < 1 || ld < vocab_end || err == nullptr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(token_logprob_kernel, dim3((unsigned)rows), dim3(TP_THREADS), 0, s, logits, ld, vocab_end, targets, row_map, tgt_off, out,
                     err, err_bit);
  return hipGetLastError();
}

}  // namespace wca
