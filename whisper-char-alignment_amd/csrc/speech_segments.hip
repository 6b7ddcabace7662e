// Speech activity of one long recording (wca_speech_segments; include/wca.h has the definition): which frame ranges stand out of the
// recording's own noise floor. Integers from the first sum on, so no summation order can change a result. All of it runs on the device,
// one launch after the other on one stream, and nothing returns to the host in between:
//   * level:   one thread per frame sums q over the mel rows (lanes along frames: every row is read coalesced, every value once) -> e [cf]
//   * smooth:  e through an LDS tile of 1024 frames with a halo of half_width on both sides -> s [cf]
//   * select:  lo and hi, two order statistics of s, by an exact radix select on the sign-biased level: four passes of 8 bits, most
//              significant first. A pass counts the digits of the levels that still match each rank's prefix (LDS histograms, merged
//              into a global one with integer atomics; both ranks in the same pass), then one workgroup picks each rank's digit. The
//              last pick forms the thresholds and `flat`. No sort.
//   * stages:  hysteresis, close, open and pad are each "where is the nearest frame with a property, before and after me": an inclusive
//              max-scan of the last such index and a reverse min-scan of the next one. A stage works on tiles of 1024 frames, one
//              workgroup each: it scans inside the tile, takes what enters the tile from either side from the carries, writes its flags
//              and leaves the tile's own first / last index for the NEXT stage's property. Between two stages one workgroup turns those
//              per-tile indices into the carries (an exclusive scan over the tiles, 256 tiles per step).
//                hysteresis  property "decisive" (s >= on_thr or s < off_thr): a0[t] = the last decisive frame <= t is loud
//                close       property a0 = 1: a 0 with a 1 on both sides, next - prev - 1 < min_silence, becomes 1
//                open        property a1 = 0: a 1 whose run, next - prev - 1 long, is shorter than min_speech becomes 0
//                pad         property a2 = 1: a3[t] = a frame of a2 lies within pad frames of t (runs that overlap or touch are one run)
//   * emit:    a run starts where a3 rises; an exclusive sum over the tiles' start counts plus a scan inside the tile numbers the runs, and
//              the frames where a3 rises / falls (or the recording ends) write their run's start / stop.
#include "kernels.h"
#include "level_quant.h"
#include "wca_common.h"

#include <algorithm>
#include <type_traits>

namespace wca {

namespace {

constexpr int VAD_LEVEL_BLOCK = 256;                          // frames per workgroup of the level pass
constexpr int VAD_SMOOTH_TILE = 1024, VAD_SMOOTH_BLOCK = 256;
constexpr int VAD_HIST_BLOCK = 256, VAD_HIST_GRID_MAX = 2048;   // the histogram workgroups stride over the recording
constexpr int VAD_CARRY_BLOCK = 256;                          // tiles per step of the carry scan
constexpr int VAD_NONE = 0x7fffffff;                          // "no such frame after me"
enum { STAGE_DECISIVE = 0, STAGE_HYST, STAGE_CLOSE, STAGE_OPEN, STAGE_PAD };

struct OpMax {
  static constexpr int identity = -1;
  __device__ int operator()(int a, int b) const { return a > b ? a : b; }
};
struct OpMin {
  static constexpr int identity = VAD_NONE;
  __device__ int operator()(int a, int b) const { return a < b ? a : b; }
};
struct OpAdd {
  static constexpr int identity = 0;
  __device__ int operator()(int a, int b) const { return a + b; }
};

// Inclusive scan of v over the workgroup's threads, in thread order or (REVERSE) from the last thread down. The operators commute. Every
// thread of the workgroup calls it; wave_tot is LDS for one int per wave and is free again on return.
template <class Op, bool REVERSE>
__device__ __forceinline__ int block_scan(int v, int* wave_tot) {
  const Op op;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = REVERSE ? __shfl_down(v, d) : __shfl_up(v, d);
    if (REVERSE ? lane + d < 64 : lane >= d) v = op(v, o);
  }
  if (lane == (REVERSE ? 0 : 63)) wave_tot[wave] = v;
  __syncthreads();
  if (REVERSE) {
    for (int w = wave + 1; w < n_waves; ++w) v = op(v, wave_tot[w]);
  } else {
    for (int w = 0; w < wave; ++w) v = op(v, wave_tot[w]);
  }
  __syncthreads();
  return v;
}

// op over the v of all threads of the workgroup, to every thread
template <class Op>
__device__ __forceinline__ int block_reduce(int v, int* wave_tot) {
  const Op op;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = op(v, __shfl_xor(v, d));
  if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = Op::identity;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) r = op(r, wave_tot[w]);
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(VAD_LEVEL_BLOCK) void vad_level_kernel(const float* __restrict__ mel, long ld, int n_mels, long cf,
                                                                    int* __restrict__ e) {
  const long t = (long)blockIdx.x * VAD_LEVEL_BLOCK + threadIdx.x;
  if (t >= cf) return;
  const float* col = mel + t;
  int acc = 0;
#pragma unroll 8
  for (int m = 0; m < n_mels; ++m) acc += quantise(col[(long)m * ld]);
  e[t] = acc;
}

__global__ __launch_bounds__(VAD_SMOOTH_BLOCK) void vad_smooth_kernel(const int* __restrict__ e, long cf, int half_width, int* __restrict__ s) {
  __shared__ int tile[VAD_SMOOTH_TILE + 2 * QUIET_HALF_WIDTH_MAX];
  const long t0 = (long)blockIdx.x * VAD_SMOOTH_TILE;
  for (int i = threadIdx.x; i < VAD_SMOOTH_TILE + 2 * half_width; i += VAD_SMOOTH_BLOCK) {
    long t = t0 - half_width + i;
    t = t < 0 ? 0 : (t > cf - 1 ? cf - 1 : t);
    tile[i] = e[t];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < VAD_SMOOTH_TILE && t0 + i < cf; i += VAD_SMOOTH_BLOCK) {
    int acc = 0;
    for (int d = 0; d <= 2 * half_width; ++d) acc += tile[i + d];
    s[t0 + i] = acc;
  }
}

// pass p (0 = the most significant byte): hist[j][d] += the levels whose bytes above byte p equal rank j's prefix and whose byte p is d
__global__ __launch_bounds__(VAD_HIST_BLOCK) void vad_hist_kernel(const int* __restrict__ s, long cf, int pass, const unsigned* __restrict__ sel,
                                                                  unsigned* __restrict__ hist) {
  __shared__ unsigned h[2 * 256];
  const int tid = threadIdx.x;
  h[tid] = 0;
  h[256 + tid] = 0;
  __syncthreads();
  const unsigned p0 = sel[0], p1 = sel[1];
  const int shift = 24 - 8 * pass;
  for (long i = (long)blockIdx.x * VAD_HIST_BLOCK + tid; i < cf; i += (long)gridDim.x * VAD_HIST_BLOCK) {
    const unsigned u = (unsigned)s[i] ^ 0x80000000u;   // the sign bit biased: unsigned order is the levels' order
    const unsigned d = (u >> shift) & 255u;
    const unsigned above = pass ? u >> (shift + 8) : 0u;
    if (pass == 0 || above == p0) atomicAdd(&h[d], 1u);
    if (pass == 0 || above == p1) atomicAdd(&h[256 + d], 1u);
  }
  __syncthreads();
  if (h[tid]) atomicAdd(&hist[tid], h[tid]);
  if (h[256 + tid]) atomicAdd(&hist[256 + tid], h[256 + tid]);
}

// One workgroup of 256 threads, thread d for digit d: each rank's digit of this pass is the first d whose inclusive count passes the rank
// that is left. Clears the histograms for the next pass; the last pass writes lo, hi, the thresholds and flat.
__global__ __launch_bounds__(256) void vad_pick_kernel(unsigned* __restrict__ hist, unsigned* __restrict__ sel, int pass, unsigned rank_lo,
                                                       unsigned rank_hi, VadOpts o, int n_mels, int* __restrict__ stats) {
  __shared__ int wave_tot[4];
  __shared__ unsigned picked[2];
  const int tid = threadIdx.x;
  for (int j = 0; j < 2; ++j) {
    const unsigned rank = pass ? sel[2 + j] : (j ? rank_hi : rank_lo);
    const unsigned prefix = pass ? sel[j] : 0u;
    const unsigned c = hist[j * 256 + tid];
    const unsigned inc = (unsigned)block_scan<OpAdd, false>((int)c, wave_tot);   // (counts <= cf < 2^31)
    if (inc > rank && inc - c <= rank) {
      sel[j] = (prefix << 8) | (unsigned)tid;
      sel[2 + j] = rank - (inc - c);
      picked[j] = (prefix << 8) | (unsigned)tid;
    }
    hist[j * 256 + tid] = 0;
  }
  __syncthreads();
  if (pass != 3 || tid != 0) return;
  const long long lo = (int)(picked[0] ^ 0x80000000u), hi = (int)(picked[1] ^ 0x80000000u);
  stats[0] = (int)lo;
  stats[1] = (int)hi;
  stats[2] = (int)(lo + (((hi - lo) * o.on_share) >> 10));
  stats[3] = (int)(lo + (((hi - lo) * o.off_share) >> 10));
  stats[4] = (hi - lo) < (long long)o.min_range * n_mels * (2 * o.half_width + 1) ? 1 : 0;
}

struct VadStageArgs {
  const int* s;                  // [cf]
  const int* stats;              // on_thr, off_thr at [2], [3]
  const unsigned char* in;       // the previous stage's flags (unused by DECISIVE and HYST)
  unsigned char* out;            // this stage's flags (unused by DECISIVE)
  const int *carry_f, *carry_b;  // [tiles]: the last frame with the stage's property before the tile (-1: none) / the first after it (VAD_NONE)
  int *agg_last, *agg_first;     // [tiles]: the tile's last / first frame with the NEXT stage's property; PAD: agg_last = the runs that start in the tile
  int cf, min_speech, min_silence, pad;
};

// One tile of VAD_TILE frames per workgroup, one frame per thread (file comment: stages).
template <int STAGE>
__global__ __launch_bounds__(VAD_TILE) void vad_stage_kernel(VadStageArgs a) {
  __shared__ int wave_tot[VAD_TILE / 64];
  __shared__ unsigned char flag[VAD_TILE];
  const int tid = threadIdx.x, tile = blockIdx.x;
  const long tl = (long)tile * VAD_TILE + tid;
  const bool live = tl < a.cf;
  const int t = live ? (int)tl : 0;

  bool has;   // the frame has the property this stage scans for
  if (STAGE == STAGE_DECISIVE || STAGE == STAGE_HYST) {
    const int lvl = live ? a.s[t] : 0;
    has = live && (lvl >= a.stats[2] || lvl < a.stats[3]);
  } else {
    has = live && (a.in[t] != 0) == (STAGE != STAGE_OPEN);
  }
  if (STAGE == STAGE_DECISIVE) {   // only what the hysteresis' carries are made of
    const int last = block_reduce<OpMax>(has ? t : -1, wave_tot);
    if (tid == 0) a.agg_last[tile] = last;
    return;
  }

  const int enter_f = a.carry_f[tile];
  const int prev = OpMax()(block_scan<OpMax, false>(has ? t : -1, wave_tot), enter_f);
  int next = VAD_NONE;
  if (STAGE != STAGE_HYST) next = OpMin()(block_scan<OpMin, true>(has ? t : VAD_NONE, wave_tot), a.carry_b[tile]);

  bool on;
  if (STAGE == STAGE_HYST) {
    on = prev >= 0 && a.s[prev] >= a.stats[2];
  } else if (STAGE == STAGE_CLOSE) {
    on = has || (prev >= 0 && next != VAD_NONE && next - prev - 1 < a.min_silence);
  } else if (STAGE == STAGE_OPEN) {   // (has: the frame is 0; a run of 1 reaches from prev + 1 to next - 1, or to the recording's end)
    on = !has && (next == VAD_NONE ? a.cf : next) - prev - 1 >= a.min_speech;
  } else {
    on = (prev >= 0 && t - prev <= a.pad) || (next != VAD_NONE && next - t <= a.pad);
  }
  on = on && live;
  if (live) a.out[t] = on ? 1 : 0;

  if (STAGE != STAGE_PAD) {   // the next stage scans for 1 (close, pad) or for 0 (open)
    const bool want = live && on == (STAGE != STAGE_CLOSE);
    const int last = block_reduce<OpMax>(want ? t : -1, wave_tot);
    const int first = block_reduce<OpMin>(want ? t : VAD_NONE, wave_tot);
    if (tid == 0) {
      a.agg_last[tile] = last;
      a.agg_first[tile] = first;
    }
    return;
  }
  // pad: the runs that start in this tile. The frame before the tile is padded speech under the same rule: the last a2 frame up to it is
  // what entered the tile, the next one is itself (if it is that frame) or the first one from the tile's first frame on.
  flag[tid] = on ? 1 : 0;
  __syncthreads();
  bool left = tid > 0 && flag[tid - 1];
  if (tid == 0 && t > 0) {
    const int b = t - 1, nb = enter_f == b ? b : next;
    left = (enter_f >= 0 && b - enter_f <= a.pad) || (nb != VAD_NONE && nb - b <= a.pad);
  }
  const int starts = block_reduce<OpAdd>(on && !left ? 1 : 0, wave_tot);
  if (tid == 0) a.agg_last[tile] = starts;
}

// One workgroup turns the tiles' own indices into what enters each tile. CARRY_FWD: carry_f[i] = the maximum over last[0 .. i - 1] (an
// exclusive scan); CARRY_BOTH: also carry_b[i] = the minimum over first[i + 1 .. n - 1]; CARRY_SUM: carry_f[i] = the sum over
// last[0 .. i - 1] and carry_f[n] = the total. VAD_CARRY_BLOCK tiles per step, what the steps so far gave carried along.
enum { CARRY_FWD = 0, CARRY_BOTH, CARRY_SUM };
template <int MODE>
__global__ __launch_bounds__(VAD_CARRY_BLOCK) void vad_carry_kernel(const int* __restrict__ last, const int* __restrict__ first, int n,
                                                                    int* __restrict__ carry_f, int* __restrict__ carry_b) {
  using OpF = typename std::conditional<MODE == CARRY_SUM, OpAdd, OpMax>::type;
  __shared__ int wave_tot[VAD_CARRY_BLOCK / 64];
  __shared__ int inc[VAD_CARRY_BLOCK];
  const int tid = threadIdx.x;
  int run = OpF::identity;
  for (int base = 0; base < n; base += VAD_CARRY_BLOCK) {
    const int i = base + tid;
    inc[tid] = block_scan<OpF, false>(i < n ? last[i] : OpF::identity, wave_tot);
    __syncthreads();
    if (i < n) carry_f[i] = tid ? OpF()(run, inc[tid - 1]) : run;
    run = OpF()(run, inc[VAD_CARRY_BLOCK - 1]);
    __syncthreads();
  }
  if (MODE == CARRY_SUM && tid == 0) carry_f[n] = run;
  if (MODE != CARRY_BOTH) return;
  run = VAD_NONE;
  for (int base = (n - 1) / VAD_CARRY_BLOCK * VAD_CARRY_BLOCK; base >= 0; base -= VAD_CARRY_BLOCK) {
    const int i = base + tid;
    inc[tid] = block_scan<OpMin, true>(i < n ? first[i] : VAD_NONE, wave_tot);
    __syncthreads();
    if (i < n) carry_b[i] = tid + 1 < VAD_CARRY_BLOCK ? OpMin()(run, inc[tid + 1]) : run;
    run = OpMin()(run, inc[0]);
    __syncthreads();
  }
}

// runs_before [tiles + 1]: the runs that start before the tile, and their total. Run k writes segs[k] = (start, stop) while k < cap.
__global__ __launch_bounds__(VAD_TILE) void vad_emit_kernel(const unsigned char* __restrict__ a3, int cf, const int* __restrict__ runs_before,
                                                            int n_tiles, long cap, int* __restrict__ stats, int* __restrict__ segs) {
  __shared__ int wave_tot[VAD_TILE / 64];
  const int tid = threadIdx.x, tile = blockIdx.x;
  if (stats[4]) {   // flat: the whole recording, whatever the stages gave
    if (tile == 0 && tid == 0) {
      stats[5] = 1;
      if (cap > 0) {
        segs[0] = 0;
        segs[1] = cf;
      }
    }
    return;
  }
  if (tile == 0 && tid == 0) stats[5] = runs_before[n_tiles];
  const long tl = (long)tile * VAD_TILE + tid;
  const bool live = tl < cf;
  const int t = live ? (int)tl : 0;
  const bool cur = live && a3[t], left = live && t > 0 && a3[t - 1];
  const long k = (long)block_scan<OpAdd, false>(cur && !left ? 1 : 0, wave_tot) + runs_before[tile] - 1;   // the run at or before this frame
  if (!live || k < 0 || k >= cap) return;
  if (cur && !left) segs[2 * k] = t;
  if (!cur && left) segs[2 * k + 1] = t;
  if (cur && t == cf - 1) segs[2 * k + 1] = cf;
}

}  // namespace

VadScratch vad_scratch(void* base, long content_frames, long cap) {
  const size_t cf = (size_t)content_frames, tiles = (cf + VAD_TILE - 1) / VAD_TILE;
  VadScratch sc{};
  size_t at = 0;
  auto take = [&](size_t bytes) {
    char* p = (char*)base + at;
    at += (bytes + 255) / 256 * 256;
    return (void*)p;
  };
  sc.e = (int*)take(sizeof(int) * cf);
  sc.s = (int*)take(sizeof(int) * cf);
  sc.f0 = (unsigned char*)take(cf);
  sc.f1 = (unsigned char*)take(cf);
  sc.agg_last = (int*)take(sizeof(int) * tiles);
  sc.agg_first = (int*)take(sizeof(int) * tiles);
  sc.carry_f = (int*)take(sizeof(int) * (tiles + 1));
  sc.carry_b = (int*)take(sizeof(int) * (tiles + 1));
  sc.hist = (unsigned*)take(sizeof(unsigned) * (2 * 256 + 4));   // hist, then sel: cleared by one memset
  sc.sel = sc.hist + 2 * 256;
  sc.stats = (int*)take(sizeof(int) * 6);
  sc.segs = (int*)take(sizeof(int) * 2 * (size_t)(cap > 0 ? cap : 0));
  sc.bytes = at;
  return sc;
}

hipError_t launch_speech_segments(const float* mel_long, long ld, int n_mels, long content_frames, const VadOpts& o, long cap,
                                  const VadScratch& sc, hipStream_t s) {
  const long cf = content_frames;
  if (n_mels < 1 || n_mels > 128 || cf < 1 || cf > ld || cf > 0x7fffffffL || o.half_width < 0 || o.half_width > QUIET_HALF_WIDTH_MAX || cap < 0 ||
      cap > (cf + 1) / 2 || !sc.e)
    return hipErrorInvalidValue;
  const int tiles = (int)((cf + VAD_TILE - 1) / VAD_TILE);
  hipError_t err = hipMemsetAsync(sc.hist, 0, sizeof(unsigned) * (2 * 256 + 4), s);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(vad_level_kernel, dim3((unsigned)((cf + VAD_LEVEL_BLOCK - 1) / VAD_LEVEL_BLOCK)), dim3(VAD_LEVEL_BLOCK), 0, s, mel_long, ld,
                     n_mels, cf, sc.e);
  hipLaunchKernelGGL(vad_smooth_kernel, dim3((unsigned)((cf + VAD_SMOOTH_TILE - 1) / VAD_SMOOTH_TILE)), dim3(VAD_SMOOTH_BLOCK), 0, s, sc.e, cf,
                     o.half_width, sc.s);
  const unsigned rank_lo = (unsigned)((long long)(cf - 1) * o.floor_permille / 1000), rank_hi = (unsigned)((long long)(cf - 1) * o.peak_permille / 1000);
  const long hist_grid = std::min<long>((cf + VAD_HIST_BLOCK - 1) / VAD_HIST_BLOCK, VAD_HIST_GRID_MAX);
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(vad_hist_kernel, dim3((unsigned)hist_grid), dim3(VAD_HIST_BLOCK), 0, s, sc.s, cf, pass, sc.sel, sc.hist);
    hipLaunchKernelGGL(vad_pick_kernel, dim3(1), dim3(256), 0, s, sc.hist, sc.sel, pass, rank_lo, rank_hi, o, n_mels, sc.stats);
  }
  VadStageArgs a{};
  a.s = sc.s;
  a.stats = sc.stats;
  a.carry_f = sc.carry_f;
  a.carry_b = sc.carry_b;
  a.agg_last = sc.agg_last;
  a.agg_first = sc.agg_first;
  a.cf = (int)cf;
  a.min_speech = o.min_speech;
  a.min_silence = o.min_silence;
  a.pad = o.pad;
  const dim3 grid(tiles), block(VAD_TILE), one(1), cblock(VAD_CARRY_BLOCK);
  hipLaunchKernelGGL(vad_stage_kernel<STAGE_DECISIVE>, grid, block, 0, s, a);
  hipLaunchKernelGGL(vad_carry_kernel<CARRY_FWD>, one, cblock, 0, s, sc.agg_last, sc.agg_first, tiles, sc.carry_f, sc.carry_b);
  a.out = sc.f0;
  hipLaunchKernelGGL(vad_stage_kernel<STAGE_HYST>, grid, block, 0, s, a);
  hipLaunchKernelGGL(vad_carry_kernel<CARRY_BOTH>, one, cblock, 0, s, sc.agg_last, sc.agg_first, tiles, sc.carry_f, sc.carry_b);
  a.in = sc.f0;
  a.out = sc.f1;
  hipLaunchKernelGGL(vad_stage_kernel<STAGE_CLOSE>, grid, block, 0, s, a);
  hipLaunchKernelGGL(vad_carry_kernel<CARRY_BOTH>, one, cblock, 0, s, sc.agg_last, sc.agg_first, tiles, sc.carry_f, sc.carry_b);
  a.in = sc.f1;
  a.out = sc.f0;
  hipLaunchKernelGGL(vad_stage_kernel<STAGE_OPEN>, grid, block, 0, s, a);
  hipLaunchKernelGGL(vad_carry_kernel<CARRY_BOTH>, one, cblock, 0, s, sc.agg_last, sc.agg_first, tiles, sc.carry_f, sc.carry_b);
  a.in = sc.f0;
  a.out = sc.f1;
  hipLaunchKernelGGL(vad_stage_kernel<STAGE_PAD>, grid, block, 0, s, a);
  hipLaunchKernelGGL(vad_carry_kernel<CARRY_SUM>, one, cblock, 0, s, sc.agg_last, sc.agg_first, tiles, sc.carry_f, sc.carry_b);
  hipLaunchKernelGGL(vad_emit_kernel, grid, block, 0, s, sc.f1, (int)cf, sc.carry_f, tiles, cap, sc.stats, sc.segs);
  return hipGetLastError();
}

}  // namespace wca
