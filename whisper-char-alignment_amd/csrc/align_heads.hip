// openai-whisper's own word aligner (whisper/timing.py find_alignment) on the captured cross-attention logits of a ragged batch, over a
// fixed list of S alignment heads (all HBM / L2-bound, no MFMA). For utterance b, head s, its n = n_tok[b] rows and F = n_frames[b] frames:
//   1. p[t][f]  = softmax_f(qk[t][0:F] * qk_scale)                 the product rounded to fp32, its row maximum and the sum in fp32
//   2. z[t][f]  = (p[t][f] - mean_f) / std_f                       mean and POPULATION std of column f over the n rows, two passes, as
//                                                                  torch.std_mean(unbiased=False) and stdmean_normalize_kernel; a plain
//                                                                  IEEE division with NO guard, as upstream: a constant column gives
//                                                                  0 / 0 = NaN
//   3. y[t][f]  = median of z[t][f - pad .. f + pad], reflect      pad = width / 2; y = z where width == 1 or F <= pad (upstream's early
//                                                                  return, median_filter_kernel's)
//   4. matrix[t - sot_len][f] = (1 / S) sum_s y[s][t][f]           rows t in [sot_len, n - 1), heads summed in list order
// The [B][S][n][F] maps are never written: pass 1 keeps the row statistics (max, sum), pass 2 the column statistics (mean, std) -- holding
// a column's p in registers between its two sums -- and pass 3 rebuilds z from the logits and the two small tables. The selected heads'
// logits are read three times, the second and third time mostly from L2.
// Loads are 16 bytes per lane along f wherever the rows are 16-byte aligned (qk_ld a multiple of 4, as the capture buffer's is); such a
// load may cover up to 3 pad columns of its own row, inside qk_ld, whose values are masked before any use. No other element outside an
// utterance's n_tok[b] x n_frames[b] corner is read, and no sum's order depends on the batch.
#include <stdint.h>

#include "kernels.h"
#include "median.h"
#include "wca_common.h"

namespace wca {

namespace {

constexpr int MAX_CHUNKS = 6;    // row pass: chunks of 256 columns (64 lanes x 4), frames <= 1536 >= 1500
constexpr int COL_WAVES = 16;    // column pass: waves of a workgroup; wave w holds rows w, w + 16, ... of the workgroup's 256 columns
constexpr int COL_ROWS_MAX = 28; // ... so at most 448 / 16 rows per wave

__device__ __forceinline__ bool rows_aligned16(const AlignHeadsArgs& a) {
  return (((long)a.qk_ld | a.qk_hs | a.qk_bs) & 3) == 0 && (reinterpret_cast<uintptr_t>(a.qk) & 15) == 0;
}

// columns f0 .. f0 + 3 of a row (f0 a multiple of 4, f0 < F); what lies at or past F is the caller's to mask
__device__ __forceinline__ f32x4 load4(const float* __restrict__ row, int f0, int F, bool vec) {
  if (vec) return *reinterpret_cast<const f32x4*>(row + f0);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (f0 + c < F) v[c] = row[f0 + c];
  return v;
}

// the product the softmax sees, ROUNDED to fp32 (no contraction into the subtraction of the row maximum, which was taken on the rounded
// products: remat_weight in postproc.hip has the story)
__device__ __forceinline__ float scaled(float x, float scale) {
  float p = x * scale;
  asm("" : "+v"(p));
  return p;
}

// the softmaxed value, the same expression in the column pass and in the final pass: identical bits
__device__ __forceinline__ float prob(float x, float scale, float mx, float sum) { return expf(scaled(x, scale) - mx) / sum; }

// ---- pass 1: one wave per (utterance, head, row): rowstats = (max_f of the scaled products, sum_f exp(product - max))
__global__ __launch_bounds__(256) void heads_rowstats_kernel(AlignHeadsArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = blockIdx.y, b = blockIdx.z, t = blockIdx.x * 4 + wave;
  const int n = a.n_tok[b], F = a.n_frames[b];
  if (t >= n) return;
  const bool vec = rows_aligned16(a);
  const float* row = a.qk + (long)b * a.qk_bs + (long)a.heads[s] * a.qk_hs + (long)t * a.qk_ld;
  f32x4 v[MAX_CHUNKS];
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < MAX_CHUNKS; ++i) {
    const int f0 = 4 * lane + 256 * i;
    v[i] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    if (f0 < F) {
      const f32x4 x = load4(row, f0, F, vec);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        v[i][c] = (f0 + c < F) ? scaled(x[c], a.qk_scale) : -INFINITY;
        mx = fmaxf(mx, v[i][c]);
      }
    }
  }
  mx = wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < MAX_CHUNKS; ++i) {
    const int f0 = 4 * lane + 256 * i;
#pragma unroll
    for (int c = 0; c < 4; ++c) sum += (f0 + c < F) ? expf(v[i][c] - mx) : 0.f;
  }
  // wave_sum leaves sums that differ in the last bits from lane to lane; the row has ONE sum, lane 0's (as head_stats_kernel's)
  sum = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(wave_sum(sum))));
  if (lane == 0) {
    float* rs = a.rowstats + (((long)b * a.S + s) * a.n_tok_max + t) * 2;
    rs[0] = mx;
    rs[1] = sum;
  }
}

// ---- pass 2: one workgroup of 16 waves per (utterance, head, 256 columns): wave w holds p of rows w, w + 16, ... in registers, the 16
// partial column sums meet in LDS (16 bytes per lane, consecutive lanes consecutive: conflict-free) and are added in wave order by every
// thread, so mean and std do not depend on which wave finished first. colstats = (mean, sqrt(sum (p - mean)^2 / n)).
template <int RPW>
__global__ __launch_bounds__(64 * COL_WAVES) void heads_colstats_kernel(AlignHeadsArgs a) {
  __shared__ f32x4 red[2][COL_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = blockIdx.y, b = blockIdx.z, f0 = blockIdx.x * 256 + 4 * lane;
  const int n = a.n_tok[b], F = a.n_frames[b];
  if (n <= 0 || blockIdx.x * 256 >= F) return;   // (the whole workgroup)
  const bool vec = rows_aligned16(a);
  const float* head = a.qk + (long)b * a.qk_bs + (long)a.heads[s] * a.qk_hs;
  const float* rs = a.rowstats + ((long)b * a.S + s) * a.n_tok_max * 2;
  const float scale = a.qk_scale;
  f32x4 p[RPW];
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int t = wave + COL_WAVES * r;
    p[r] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (t < n && f0 < F) {
      const f32x4 x = load4(head + (long)t * a.qk_ld, f0, F, vec);
      const float mx = rs[2 * t], sum = rs[2 * t + 1];
#pragma unroll
      for (int c = 0; c < 4; ++c) p[r][c] = prob(x[c], scale, mx, sum);   // (a column at or past F: computed, never stored)
    }
  }
  f32x4 acc = p[0];
#pragma unroll
  for (int r = 1; r < RPW; ++r) acc += p[r];   // (rows past n add 0)
  red[0][wave][lane] = acc;
  __syncthreads();
  f32x4 tot = red[0][0][lane];
#pragma unroll
  for (int w = 1; w < COL_WAVES; ++w) tot += red[0][w][lane];
  const float fn = (float)n;
  const f32x4 mean = tot / fn;
  f32x4 sq = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < RPW; ++r)
    if (wave + COL_WAVES * r < n) {
      const f32x4 d = p[r] - mean;
      sq = __builtin_elementwise_fma(d, d, sq);
    }
  red[1][wave][lane] = sq;
  __syncthreads();
  if (wave != 0) return;
  f32x4 tsq = red[1][0][lane];
#pragma unroll
  for (int w = 1; w < COL_WAVES; ++w) tsq += red[1][w][lane];
  float* cs = a.colstats + (((long)b * a.S + s) * a.n_frames_max + f0) * 2;
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (f0 + c < F) {
      cs[2 * c] = mean[c];
      cs[2 * c + 1] = sqrtf(tsq[c] / fn);
    }
}

// ---- pass 3: one wave per (utterance, output row). Per head: z of the row from the logits and the two tables into the wave's LDS row
// (16-byte stores), the reflect halo, then the median with lane = column mod 64 (4-byte reads at stride 1: conflict-free), added to the
// running sum of that column. NPL: columns per lane.
template <int NPL>
__global__ __launch_bounds__(256) void heads_matrix_kernel(AlignHeadsArgs a) {
  static_assert(NPL % 4 == 0, "whole chunks of 256 columns");
  constexpr int RB = 64 * NPL + 2 * HALO;   // every column slot of a row has an LDS word
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* rowbuf = reinterpret_cast<float*>(smem) + wave * RB;
  const int b = blockIdx.y, t = a.sot_len + blockIdx.x * 4 + wave;
  const int n = a.n_tok[b], F = a.n_frames[b];
  if (t >= n - 1) return;   // (the whole wave; no workgroup barrier below)
  const bool vec = rows_aligned16(a);
  const bool do_med = a.medfilt_width > 1 && F > (a.medfilt_width >> 1);
  const int w = do_med ? a.medfilt_width : 1, pad = w >> 1;
  const float scale = a.qk_scale;
  float acc[NPL];
#pragma unroll
  for (int j = 0; j < NPL; ++j) acc[j] = 0.f;
  for (int s = 0; s < a.S; ++s) {
    const float* row = a.qk + (long)b * a.qk_bs + (long)a.heads[s] * a.qk_hs + (long)t * a.qk_ld;
    const float* rs = a.rowstats + (((long)b * a.S + s) * a.n_tok_max + t) * 2;
    const float* cs = a.colstats + ((long)b * a.S + s) * a.n_frames_max * 2;
    const float mx = rs[0], sum = rs[1];
#pragma unroll
    for (int i = 0; i < NPL / 4; ++i) {
      const int f0 = 4 * lane + 256 * i;
      if (f0 < F) {
        const f32x4 x = load4(row, f0, F, vec);
        f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (f0 + c < F) z[c] = (prob(x[c], scale, mx, sum) - cs[2 * (f0 + c)]) / cs[2 * (f0 + c) + 1];
        *reinterpret_cast<f32x4*>(rowbuf + HALO + f0) = z;
      }
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < pad) {
      const int k = lane + 1;                        // 1..pad
      rowbuf[HALO - k] = rowbuf[HALO + k];           // x[-k] = x[k]
      rowbuf[HALO + F - 1 + k] = rowbuf[HALO + F - 1 - k];
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
      const int f = lane + 64 * j;
      if (f < F) acc[j] += median_any(rowbuf + HALO + f - pad, w);
    }
    __builtin_amdgcn_wave_barrier();
  }
  float* out = a.matrix + ((long)b * a.n_tok_max + (t - a.sot_len)) * a.n_frames_max;
  const float fs = (float)a.S;
#pragma unroll
  for (int j = 0; j < NPL; ++j) {
    const int f = lane + 64 * j;
    if (f < F) out[f] = acc[j] / fs;
  }
}

}  // namespace

hipError_t launch_align_heads(const AlignHeadsArgs& a, hipStream_t s) {
  if (a.B <= 0) return hipSuccess;
  if (a.S <= 0 || a.sot_len < 0) return hipErrorInvalidValue;
  if (a.n_frames_max <= 0 || a.n_frames_max > 256 * MAX_CHUNKS) return hipErrorInvalidValue;
  if (a.n_tok_max <= 0 || a.n_tok_max > COL_WAVES * COL_ROWS_MAX) return hipErrorInvalidValue;
  if (a.medfilt_width < 1 || (a.medfilt_width & 1) == 0 || (a.medfilt_width >> 1) > HALO) return hipErrorInvalidValue;
  const int n_max = a.n_tok_max, Fmax = a.n_frames_max;
  hipLaunchKernelGGL(heads_rowstats_kernel, dim3((n_max + 3) / 4, a.S, a.B), dim3(256), 0, s, a);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  // rows per wave of the column pass: the smallest of 4, 8, 16, 28 that holds the longest utterance
  const dim3 cgrid((Fmax + 255) / 256, a.S, a.B), cblock(64 * COL_WAVES);
  const int rpw = (n_max + COL_WAVES - 1) / COL_WAVES;
  if (rpw <= 4) hipLaunchKernelGGL(heads_colstats_kernel<4>, cgrid, cblock, 0, s, a);
  else if (rpw <= 8) hipLaunchKernelGGL(heads_colstats_kernel<8>, cgrid, cblock, 0, s, a);
  else if (rpw <= 16) hipLaunchKernelGGL(heads_colstats_kernel<16>, cgrid, cblock, 0, s, a);
  else hipLaunchKernelGGL(heads_colstats_kernel<COL_ROWS_MAX>, cgrid, cblock, 0, s, a);
  err = hipGetLastError();
  if (err != hipSuccess) return err;
  const int rows = n_max - a.sot_len - 1;
  if (rows <= 0) return hipSuccess;
  // columns per lane of the final pass: the smallest of 4, 8, 16, 24 whose 64 lanes hold the longest row
  const dim3 mgrid((rows + 3) / 4, a.B);
  auto launch = [&](auto npl_c) {
    constexpr int NPL = decltype(npl_c)::value;
    hipLaunchKernelGGL(heads_matrix_kernel<NPL>, mgrid, dim3(256), sizeof(float) * 4 * (64 * NPL + 2 * HALO), s, a);
  };
  if (Fmax <= 64 * 4) launch(IntC<4>{});
  else if (Fmax <= 64 * 8) launch(IntC<8>{});
  else if (Fmax <= 64 * 16) launch(IntC<16>{});
  else launch(IntC<24>{});
  return hipGetLastError();
}

}  // namespace wca
