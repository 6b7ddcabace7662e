// Where to cut one long recording into pieces that are transcribed side by side: near each equal-share target the quietest EVEN frame of the
// recording's log-mel (wca_quiet_cuts). Integers from the first sum on, so the summation order cannot matter and the result is exact:
//   q(x)  = rint(4096 clamp(x, -8, 8)), ties to even, NaN as 8 (loud, never preferred)
//   e[t]  = sum over the mel rows of q(mel[m][t])
//   s[t]  = sum over j in [-half_width, half_width] of e[clamp(t + j, 0, content_frames - 1)]     (|s| <= 128 x 32768 x 201 < 2^31)
//   g_k   = floor(k content_frames / n_pieces), k = 1 .. n_pieces - 1
//   cut_k = the even t in [g_k - radius, g_k + radius] with the smallest (s[t], |t - g_k|, t)
//   * quiet_cuts: one workgroup of four waves per interior cut. The frame levels e of the 2 radius + 1 + 2 half_width <= 3201 frames the cut
//                 can see go to LDS (lanes stride over frames, so every mel row is read coalesced), then every even candidate sums its
//                 window from LDS and the three-part key, packed into one 64-bit integer, is reduced by shuffles and through LDS.
#include "kernels.h"
#include "level_quant.h"
#include "wca_common.h"

namespace wca {

namespace {

constexpr int QC_WAVES = 4;
constexpr int QC_SPAN_MAX = 2 * QUIET_RADIUS_MAX + 1 + 2 * QUIET_HALF_WIDTH_MAX;   // 3201 frame levels, 12.5 KiB of LDS

__global__ __launch_bounds__(QC_WAVES * 64) void quiet_cuts_kernel(const float* __restrict__ mel, long ld, int n_mels, long content_frames,
                                                                  int n_pieces, int radius, int half_width, int* __restrict__ cuts,
                                                                  int* __restrict__ level) {
  __shared__ int e[QC_SPAN_MAX];
  __shared__ long long red[QC_WAVES];
  const int k = blockIdx.x + 1, tid = threadIdx.x;
  const long g = (long)k * content_frames / n_pieces;   // (k < 4096, content_frames < 2^31)
  const long first = g - radius - half_width;           // frame of e[0], before the clamp
  const int span = 2 * radius + 1 + 2 * half_width;

  for (int i = tid; i < span; i += QC_WAVES * 64) {
    long t = first + i;
    t = t < 0 ? 0 : (t > content_frames - 1 ? content_frames - 1 : t);
    const float* col = mel + t;
    int acc = 0;
    for (int m = 0; m < n_mels; ++m) acc += quantise(col[(long)m * ld]);
    e[i] = acc;
  }
  __syncthreads();

  // candidate j is frame g - radius + j, its window e[j .. j + 2 half_width]; key = (s, |j - radius|, j) in one signed 64-bit word
  long long best = 0x7fffffffffffffffLL;
  const int j0 = (int)((g - radius) & 1);   // the first even frame of the range
  for (int j = j0 + 2 * tid; j <= 2 * radius; j += 2 * QC_WAVES * 64) {
    int s = 0;
    for (int d = 0; d <= 2 * half_width; ++d) s += e[j + d];
    const int dist = j < radius ? radius - j : j - radius;
    const long long key = (long long)s * 4294967296LL + (long long)(dist * 4096 + j);   // j <= 3000 < 4096, dist <= 1500
    best = key < best ? key : best;
  }
  for (int off = 32; off >= 1; off >>= 1) {
    const long long o = __shfl_xor(best, off);
    best = o < best ? o : best;
  }
  if ((tid & 63) == 0) red[tid >> 6] = best;
  __syncthreads();
  if (tid != 0) return;
#pragma unroll
  for (int w = 1; w < QC_WAVES; ++w) best = red[w] < best ? red[w] : best;
  const int j = (int)(best & 4095);
  cuts[k - 1] = (int)(g - radius + j);
  level[k - 1] = (int)((best - (best & 0xffffffffLL)) / 4294967296LL);
}

}  // namespace

hipError_t launch_quiet_cuts(const float* mel_long, long ld, int n_mels, long content_frames, int n_pieces, int radius, int half_width,
                             int* cuts, int* level, hipStream_t s) {
  if (n_mels < 1 || n_mels > 128 || n_pieces < 2 || radius < 1 || radius > QUIET_RADIUS_MAX || half_width < 0 ||
      half_width > QUIET_HALF_WIDTH_MAX || content_frames > ld || content_frames / n_pieces < 2 * radius + 2)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(quiet_cuts_kernel, dim3(n_pieces - 1), dim3(QC_WAVES * 64), 0, s, mel_long, ld, n_mels, content_frames, n_pieces, radius,
                     half_width, cuts, level);
  return hipGetLastError();
}

}  // namespace wca
