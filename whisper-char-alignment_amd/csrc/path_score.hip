// Per-row score of the DTW path on gfx950: the mean of the aggregated attention matrix (NOT negated) over the cells of the path that lie in
// each text row, and the number of those cells. It runs behind dtw_kernel on the same stream and reads what that kernel left: the jump frames,
// the 2-bit move trace, the path length and (open-end launches) the end rows. dtw_kernel itself is untouched.
//
// Within a text row the path only moves along the frame axis, so row i's cells are the contiguous frames jump[i] .. last[i] of ONE matrix
// row: last = M - 1 for the end row; otherwise the move stored at (i + 1, jump[i+1]) -- the cell at which the backtrace left row i + 1 --
// says how the path entered that row: vertically (1) puts column jump[i+1] in both rows, diagonally (0) ends row i one frame earlier.
//
// Mapping: ONE 64-lane wave per (problem, text row), 4 rows per workgroup, lanes along the frames (a coalesced segment of the row). Each lane
// adds its frames j0 + lane, j0 + lane + 64, ... in f64 in that order, then a 6-step xor butterfly adds the 64 partial sums: the shape of the
// reduction depends on the row's span alone, so the bits are the same from run to run and at every batch position. No atomics, no LDS. The
// worst shapes spread the same way: N = 1, M = 1500 is one wave of 24 loads per lane, N = 512 over two frames is 512 waves of one load each.
// It is latency-bound (at most N + M - 1 floats per problem); the time is reported beside the DTW's in profiles/path_score_bench.txt.
//
// Every index comes from device data and is clamped before the load it feeds: a degenerate trace (non-finite input) can leave -1 in a jump
// frame, rows the DTW did not write hold 0 or -1, a refused problem has path_len 0.
#include "kernels.h"
#include "wca_common.h"

namespace wca {

namespace {

constexpr int PS_WAVES = 4;

__global__ __launch_bounds__(64 * PS_WAVES) void path_score_kernel(PathScoreArgs a) {
  const DtwArgs& d = a.d;
  const int p = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * PS_WAVES + (threadIdx.x >> 6);  // wave-uniform
  if (i >= d.N_max) return;
  const int N = d.N ? d.N[p] : d.N_all;
  const int M = d.M ? d.M[p] : d.M_all;
  // the problems dtw_kernel refuses have no path
  const bool ran = N > 0 && M > 0 && N <= d.N_max && M <= d.M_max && d.path_len[p] > 0;
  int end_i = -1;
  if (ran) {
    end_i = d.end_row ? d.end_row[p] : N - 1;
    end_i = end_i < N ? end_i : N - 1;
  }
  int cells = 0;
  double sum = 0.0;
  if (i <= end_i) {
    const int* __restrict__ jf = d.jump_frame + (long)p * d.jump_ld;
    int j0 = jf[i];
    j0 = j0 < 0 ? 0 : j0;
    int last = M - 1;
    if (i < end_i) {
      int j1 = jf[i + 1];
      j1 = j1 < 0 ? 0 : (j1 >= M ? M - 1 : j1);
      const int wpr = (d.M_max + 15) >> 4;
      const uint32_t w = d.trace[((long)p * d.N_max + (i + 1)) * wpr + (j1 >> 4)];
      const int t = (int)((w >> (2 * (j1 & 15))) & 3u);
      last = t == 1 ? j1 : j1 - 1;
    }
    if (last >= j0) {
      cells = last - j0 + 1;
      const float* __restrict__ x = d.matrix + (long)p * d.m_bs + (long)i * d.ld;
      for (int j = j0 + lane; j <= last; j += 64) sum += (double)x[j];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if (lane == 0) {
    const long at = (long)p * a.out_ld + i;
    a.cells[at] = cells;
    a.mean[at] = cells > 0 ? (float)(sum / (double)cells) : 0.f;
  }
}

}  // namespace

hipError_t launch_path_score(const PathScoreArgs& a, hipStream_t s) {
  const DtwArgs& d = a.d;
  if (d.P <= 0) return hipSuccess;
  if (d.N_max <= 0 || d.M_max <= 0 || d.N_max > 512 || d.P > 65535 || a.out_ld < d.N_max) return hipErrorInvalidValue;
  if (!d.matrix || !d.trace || !d.jump_frame || !d.path_len || !a.mean || !a.cells) return hipErrorInvalidValue;
  dim3 grid((d.N_max + PS_WAVES - 1) / PS_WAVES, d.P), block(64 * PS_WAVES);
  hipLaunchKernelGGL(path_score_kernel, grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace wca
