// DTW cost-table fill + backtrace on gfx950.  Reference call site: timing.py:103 `dtw(-matrix)`, which
// from force_align always reaches openai-whisper's numba `dtw_cpu` (matrix was moved to the CPU at
// timing.py:102) followed by `backtrace`.  This kernel reproduces THAT arithmetic bit for bit:
//   c0 = C[i-1][j-1], c1 = C[i-1][j], c2 = C[i][j-1]
//   diag only if strictly smallest, else up only if strictly smallest, else left (every tie -> left)
//   C[i][j] = float( double(x[i][j]) + double(c) )        (f32 table fed by f64 x, x = -matrix)
//
// Mapping: ONE 64-lane wave per problem, no LDS, no barriers.  Lane l owns R = ceil(N/64) consecutive
// text rows and sweeps them along the frame axis, skewed by one column per lane (lane l is at column
// s - l in step s): a wavefront-parallel anti-diagonal sweep whose only cross-lane traffic is the
// previous lane's last row (two values per step).  The 2-bit move trace is packed 16 columns per word.
// It is neither HBM- nor MFMA-bound: N+M-1 dependent steps, reported as microseconds per utterance.
//
// OPEN (the open-end form, for a window of a long recording that holds only a prefix of the text it is offered): the same recurrence and
// tie rule, but the path may end in the last frame at ANY text row. Every cell also carries L, the number of cells on its chosen path
// (itself included), through the same hand-off as the two cost values; after the sweep the wave picks the end row n* that minimises
// C[i][M-1] / L[i][M-1] -- every visited cell adds a non-positive cost, so the unnormalised minimum would always be the last row. The
// comparison is exact: row a beats row b iff (double)C_a * L_b < (double)C_b * L_a (C has 24 significant bits and L < 2^13, so both
// products are exact in f64), equal scores go to the lower row. Lane 0 then backtraces from (n*, M-1). The closed instantiations carry
// none of this: `if constexpr` keeps their registers and shuffles what they were.
//
// WIN (the windowed form, for text rows whose frames are known to within an interval: subtitle cues): cell (i, j) is allowed iff
// row_lo[p][i] <= j <= row_hi[p][i]; a cell that is not allowed stores C = +inf (its trace bits are unspecified: no backtrace reaches
// it), and the matrix is never modified. Each lane loads the lo / hi of its R rows into registers once, before the sweep; every sweep
// step still runs. One exception to the tie rule: where it chose left, c2 is +inf and c0 == c1 is finite (the left edge of a row's window
// under an exact 0 in the matrix), the move is UP -- left would make a reachable cell infinite. Without windows c2 = +inf only in column
// 0, where c0 is +inf too, so full windows are bit-identical to the closed form. The host checks the windows before the launch
// (dtw_windows_valid): they then hold a finite path from (0, 0) to (N-1, M-1). WIN together with OPEN serves launches that mix open
// problems (full windows only, the host's check again) with windowed closed ones.
#include "kernels.h"
#include "wca_common.h"

namespace wca {

namespace {

// (Ca, La, ia) beats (Cb, Lb, ib) as the end of an open-end path: a valid row (i >= 0) beats none, then the smaller C / L decided on
// the cross-multiplied f64 products, then the lower row
__device__ __forceinline__ bool end_row_beats(float Ca, int La, int ia, float Cb, int Lb, int ib) {
  if (ia < 0) return false;
  if (ib < 0) return true;
  const double pa = (double)Ca * (double)Lb, pb = (double)Cb * (double)La;
  return pa < pb || (pa == pb && ia < ib);
}

template <int R, int U, bool OPEN, bool WIN>
__global__ __launch_bounds__(64) void dtw_kernel(DtwArgs a) {
  const int p = blockIdx.x;
  const int lane = threadIdx.x;
  const int N = a.N ? a.N[p] : a.N_all;
  const int M = a.M ? a.M[p] : a.M_all;
  const int cap = a.N_max + a.M_max + 2;
  int* pt = a.path + (long)p * 2 * cap;
  int* pj = pt + cap;
  if (N <= 0 || M <= 0 || N > 64 * R || N > a.N_max || M > a.M_max) {
    if (lane == 0) {
      a.path_len[p] = 0;
      if constexpr (OPEN) {
        if (a.end_row) a.end_row[p] = -1;
        if (a.score) a.score[p] = 0.f;
      }
    }
    return;
  }
  const float* __restrict__ x = a.matrix + (long)p * a.m_bs;
  const int wpr = (a.M_max + 15) >> 4;
  uint32_t* __restrict__ tr = a.trace + (long)p * a.N_max * wpr;

  const int i0 = lane * R;
  // WIN: the permitted frame interval of each of this lane's rows (rows past N repeat row N - 1's: their cells are never stored)
  int wlo[WIN ? R : 1], whi[WIN ? R : 1];
  if constexpr (WIN) {
    const int* __restrict__ rlo = a.row_lo + (long)p * a.win_ld;
    const int* __restrict__ rhi = a.row_hi + (long)p * a.win_ld;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int i = i0 + r;
      i = i < N ? i : N - 1;
      wlo[r] = rlo[i];
      whi[r] = rhi[i];
    }
  }
  float prev[R];
  uint32_t tw[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    prev[r] = INFINITY;
    tw[r] = 0u;
  }
  float last_cur = INFINITY, last_prev = INFINITY;
  // OPEN: path lengths beside the costs (0 = no path yet; such a cell's cost is INFINITY and is never chosen over a finite one)
  int plen[OPEN ? R : 1];
  int last_cur_len = 0, last_prev_len = 0;
  if constexpr (OPEN) {
#pragma unroll
    for (int r = 0; r < R; ++r) plen[r] = 0;
  }
  const int lane_max = (N - 1) / R;
  const int S = M + lane_max;  // steps 0 .. S-1

  for (int s0 = 0; s0 < S; s0 += U) {
    // loads of the whole block first (addresses do not depend on the recurrence)
    float xv[U][R];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int j = s0 + u - lane;
      j = j < 0 ? 0 : (j >= M ? M - 1 : j);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        int i = i0 + r;
        i = i < N ? i : N - 1;
        xv[u][r] = x[(long)i * a.ld + j];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int s = s0 + u;
      const int j = s - lane;
      float up_in = __shfl_up(last_cur, 1);
      float diag_in = __shfl_up(last_prev, 1);
      if (lane == 0) {
        up_in = INFINITY;
        diag_in = (j == 0) ? 0.f : INFINITY;
      }
      int up_len = 0, diag_len = 0;
      if constexpr (OPEN) {
        up_len = __shfl_up(last_cur_len, 1);
        diag_len = __shfl_up(last_prev_len, 1);
        if (lane == 0) up_len = diag_len = 0;
      }
      const bool active = (s < S) && (j >= 0) && (j < M) && (i0 < N);
      if (active) {
        float newv[R];
        int newl[OPEN ? R : 1];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int i = i0 + r;
          const float c1 = (r == 0) ? up_in : newv[r > 0 ? r - 1 : 0];
          const float c0 = (r == 0) ? diag_in : prev[r > 0 ? r - 1 : 0];
          const float c2 = prev[r];
          float c;
          uint32_t t;
          if (c0 < c1 && c0 < c2) {
            c = c0;
            t = 0u;
          } else if (c1 < c0 && c1 < c2) {
            c = c1;
            t = 1u;
          } else {
            c = c2;
            t = 2u;
            if constexpr (WIN) {
              if (c2 == INFINITY && c0 == c1 && c0 < INFINITY) {   // the one exception (header): up, not left
                c = c1;
                t = 1u;
              }
            }
          }
          const float nv = (float)((double)(-xv[u][r]) + (double)c);
          if constexpr (WIN) {
            newv[r] = (i < N && j >= wlo[r] && j <= whi[r]) ? nv : INFINITY;
          } else {
            newv[r] = (i < N) ? nv : INFINITY;
          }
          if constexpr (OPEN) {
            const int l1 = (r == 0) ? up_len : newl[r > 0 ? r - 1 : 0];
            const int l0 = (r == 0) ? diag_len : plen[r > 0 ? r - 1 : 0];
            newl[r] = (t == 0u ? l0 : (t == 1u ? l1 : plen[r])) + 1;
          }
          if (i < N) {
            tw[r] |= t << (2 * (j & 15));
            if ((j & 15) == 15 || j == M - 1) {
              tr[(long)i * wpr + (j >> 4)] = tw[r];
              tw[r] = 0u;
            }
          }
        }
        last_prev = prev[R - 1];
        last_cur = newv[R - 1];
#pragma unroll
        for (int r = 0; r < R; ++r) prev[r] = newv[r];
        if constexpr (OPEN) {
          last_prev_len = plen[R - 1];
          last_cur_len = newl[R - 1];
#pragma unroll
          for (int r = 0; r < R; ++r) plen[r] = newl[r];
        }
      }
    }
  }

  // OPEN: every lane now holds C[i][M-1] in prev[] and L[i][M-1] in plen[] for its rows i < N: wave arg-min of C / L, per lane over
  // its R rows and then across the lanes (a strict total order, so the butterfly leaves the same winner in every lane)
  int end_i = N - 1;
  if constexpr (OPEN) {
    const bool open = a.open_end ? a.open_end[p] != 0 : a.open_all != 0;
    float bc = 0.f;
    int bl = 0, bi = -1;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = i0 + r;
      const bool counts = open ? i < N : i == N - 1;
      if (counts && end_row_beats(prev[r], plen[r], i, bc, bl, bi)) {
        bc = prev[r];
        bl = plen[r];
        bi = i;
      }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float oc = __shfl_xor(bc, d);
      const int ol = __shfl_xor(bl, d), oi = __shfl_xor(bi, d);
      if (end_row_beats(oc, ol, oi, bc, bl, bi)) {
        bc = oc;
        bl = ol;
        bi = oi;
      }
    }
    end_i = bi;
    if (lane == 0) {
      if (a.end_row) a.end_row[p] = bi;
      if (a.score) a.score[p] = (float)((double)bc / (double)bl);
    }
    // rows past the end row are on no path
    if (a.jump_frame)
      for (int i = end_i + 1 + lane; i < N; i += 64) a.jump_frame[(long)p * a.jump_ld + i] = -1;
  }

  __threadfence();  // trace words written by all lanes -> visible to lane 0's loads below
  if (lane == 0) {
    int i = end_i, j = M - 1, k = cap;
    int* jf = a.jump_frame ? a.jump_frame + (long)p * a.jump_ld : nullptr;
    while ((i >= 0 || j >= 0) && k > 0) {
      --k;
      pt[k] = i;
      pj[k] = j;
      if (jf && i >= 0) jf[i] = j;
      int t;
      if (i < 0) {
        t = 2;
      } else if (j < 0) {
        t = 1;
      } else {
        const uint32_t w = __hip_atomic_load(tr + (long)i * wpr + (j >> 4), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t = (int)((w >> (2 * (j & 15))) & 3u);
      }
      if (t == 0) {
        --i;
        --j;
      } else if (t == 1) {
        --i;
      } else {
        --j;
      }
    }
    a.path_len[p] = cap - k;
  }
}

}  // namespace

namespace {

// the launch of one (OPEN, WIN) form: rows per lane R = ceil(N_max / 64), unroll U by R
template <bool OPEN, bool WIN>
void launch_form(const DtwArgs& a, int R, hipStream_t s) {
  dim3 grid(a.P), block(64);
  switch (R) {
    case 1: hipLaunchKernelGGL((dtw_kernel<1, 8, OPEN, WIN>), grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL((dtw_kernel<2, 8, OPEN, WIN>), grid, block, 0, s, a); break;
    case 3: hipLaunchKernelGGL((dtw_kernel<3, 4, OPEN, WIN>), grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL((dtw_kernel<4, 4, OPEN, WIN>), grid, block, 0, s, a); break;
    case 5: hipLaunchKernelGGL((dtw_kernel<5, 2, OPEN, WIN>), grid, block, 0, s, a); break;
    case 6: hipLaunchKernelGGL((dtw_kernel<6, 2, OPEN, WIN>), grid, block, 0, s, a); break;
    case 7: hipLaunchKernelGGL((dtw_kernel<7, 2, OPEN, WIN>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((dtw_kernel<8, 2, OPEN, WIN>), grid, block, 0, s, a); break;
  }
}

}  // namespace

hipError_t launch_dtw(const DtwArgs& a, hipStream_t s) {
  if (a.P <= 0) return hipSuccess;
  if (a.N_max <= 0 || a.M_max <= 0 || a.N_max > 512) return hipErrorInvalidValue;
  if ((a.row_lo == nullptr) != (a.row_hi == nullptr) || (a.row_lo && a.win_ld < a.N_max)) return hipErrorInvalidValue;
  const int R = (a.N_max + 63) / 64;
  const bool open = a.open_end || a.open_all, win = a.row_lo != nullptr;
  if (open && win) launch_form<true, true>(a, R, s);
  else if (open) launch_form<true, false>(a, R, s);
  else if (win) launch_form<false, true>(a, R, s);
  else launch_form<false, false>(a, R, s);
  return hipGetLastError();
}

// Valid windows of one n x m problem: 0 <= lo[i] <= hi[i] <= m-1, lo[0] == 0, hi[n-1] == m-1, lo and hi non-decreasing, lo[i+1] <= hi[i] + 1.
// They hold a finite path from (0, 0) to (n-1, m-1). Returns nullptr, or which condition fails (*row: at which row).
const char* dtw_windows_invalid(const int* lo, const int* hi, int n, int m, int* row) {
  for (int i = 0; i < n; ++i) {
    *row = i;
    if (lo[i] < 0 || lo[i] > hi[i] || hi[i] > m - 1) return "0 <= lo <= hi <= M-1 fails";
    if (i > 0 && (lo[i] < lo[i - 1] || hi[i] < hi[i - 1])) return "lo and hi must be non-decreasing";
    if (i > 0 && lo[i] > hi[i - 1] + 1) return "lo[i] <= hi[i-1] + 1 fails (no step from the row above)";
  }
  *row = 0;
  if (lo[0] != 0) return "lo[0] must be 0";
  *row = n - 1;
  if (hi[n - 1] != m - 1) return "hi[N-1] must be M-1";
  return nullptr;
}

}  // namespace wca
