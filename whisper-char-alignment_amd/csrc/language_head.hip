// Language identification head (upstream openai-whisper decoding.py detect_language -- absent third-party dependency, restated from its
// published algorithm): upstream takes the full [n_vocab] logits at the <|startoftranscript|> position, masks everything but the language
// tokens, then argmax and softmax. The language tokens are the contiguous ids [lang_begin, lang_begin + n_lang), so only those ~100 rows
// of the token embedding are read (0.2 MB of whisper-medium's 106 MB matrix) and the masked softmax is the softmax over n_lang logits.
//   * language_head: final LayerNorm of the row (fp32, rounded to f16 as the operand of the vocabulary projection is), n_lang dot
//                    products with fp32 accumulation, softmax, argmax with the lowest index among equals (decode_select's rule);
//                    one workgroup of four waves per batch row.
#include "kernels.h"
#include "wca_common.h"

namespace wca {

namespace {

constexpr int LANG_MAX = 128;     // language tokens per call (99 or 100 in the published vocabularies)
constexpr int LANG_D_MAX = 1280;  // widest n_text_state (the LayerNorm'd row is kept in LDS)
constexpr int LANG_WAVES = 4;

// sum over the workgroup's LANG_WAVES waves (every thread gets it); red: LANG_WAVES floats of LDS
__device__ __forceinline__ float head_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int i = 1; i < LANG_WAVES; ++i) r += red[i];
  return r;
}

__global__ __launch_bounds__(LANG_WAVES * 64) void language_head_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                       const float* __restrict__ beta, const half_t* __restrict__ tok_emb, int d,
                                                                       int lang_begin, int n_lang, float eps, float* __restrict__ probs,
                                                                       int* __restrict__ lang_token) {
  __shared__ __attribute__((aligned(16))) half_t xn[LANG_D_MAX];
  __shared__ float logit[LANG_MAX];
  __shared__ float red[LANG_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* xr = x + (long)b * d;

  // final LayerNorm, two passes in fp32 (the few-row GEMM's prologue computes the same expression), stored as f16
  float s = 0.f;
  for (int c = tid; c < d; c += blockDim.x) s += xr[c];
  const float mean = head_block_sum(s, red) / (float)d;
  float q = 0.f;
  for (int c = tid; c < d; c += blockDim.x) {
    const float t = xr[c] - mean;
    q += t * t;
  }
  const float rs = rsqrtf(head_block_sum(q, red) / (float)d + eps);
  for (int c = tid; c < d; c += blockDim.x) xn[c] = (half_t)((xr[c] - mean) * rs * gamma[c] + beta[c]);
  __syncthreads();

  // one language row per wave at a time: lanes stride over the d / 8 half8 chunks (d = 256: lanes 32..63 hold no chunk and add 0)
  const int chunks = d >> 3;
  for (int j = wave; j < n_lang; j += LANG_WAVES) {
    const half8* w = reinterpret_cast<const half8*>(tok_emb + (long)(lang_begin + j) * d);
    float acc = 0.f;
    for (int c = lane; c < chunks; c += 64) {
      const half8 wv = w[c];
      const half8 xv = *reinterpret_cast<const half8*>(xn + 8 * c);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc = fmaf((float)xv[i], (float)wv[i], acc);
    }
    acc = wave_sum(acc);   // (every lane is back here: the j loop is uniform over the wave)
    if (lane == 0) logit[j] = acc;
  }
  __syncthreads();

  // softmax and argmax over the n_lang <= 128 logits on the first wave: lane l holds languages l and l + 64
  if (wave != 0) return;
  const int j0 = lane, j1 = lane + 64;
  const float l0 = j0 < n_lang ? logit[j0] : -INFINITY;
  const float l1 = j1 < n_lang ? logit[j1] : -INFINITY;
  float best = l0;
  int best_i = j0 < n_lang ? j0 : 0x7fffffff;
  if (l1 > best) {
    best = l1;
    best_i = j1;
  }
  const float m = wave_max(best);
  const float e0 = j0 < n_lang ? expf(l0 - m) : 0.f;
  const float e1 = j1 < n_lang ? expf(l1 - m) : 0.f;
  const float inv = 1.0f / wave_sum(e0 + e1);
  for (int off = 32; off >= 1; off >>= 1) {
    const float ob = __shfl_xor(best, off);
    const int oi = __shfl_xor(best_i, off);
    if (ob > best || (ob == best && oi < best_i)) {
      best = ob;
      best_i = oi;
    }
  }
  float* pr = probs + (long)b * n_lang;
  if (j0 < n_lang) pr[j0] = e0 * inv;
  if (j1 < n_lang) pr[j1] = e1 * inv;
  if (lane == 0) lang_token[b] = lang_begin + (best_i < n_lang ? best_i : 0);   // (best_i is a language: n_lang >= 1 and no logit is below -inf)
}

}  // namespace

hipError_t launch_language_head(const float* x, const float* gamma, const float* beta, const half_t* tok_emb, int B, int d, int n_vocab,
                                int lang_begin, int n_lang, float* probs, int* lang_token, hipStream_t s) {
  if (B < 1 || d < 8 || (d & 7) != 0 || d > LANG_D_MAX) return hipErrorInvalidValue;
  if (n_lang < 1 || n_lang > LANG_MAX) return hipErrorInvalidValue;
  if (lang_begin < 0 || lang_begin > n_vocab - n_lang) return hipErrorInvalidValue;
  hipLaunchKernelGGL(language_head_kernel, dim3(B), dim3(LANG_WAVES * 64), 0, s, x, gamma, beta, tok_emb, d, lang_begin, n_lang, 1e-5f, probs,
                     lang_token);
  return hipGetLastError();
}

}  // namespace wca
