// Sample-rate conversion of a whole recording to 16 kHz on gfx950: what upstream whisper.load_audio leaves to ffmpeg.
//
// The filter is the default of torchaudio.functional.resample (Hann-windowed sinc, lowpass_filter_width 6, rolloff 0.99) as a polyphase
// table h[p][i]: with g = gcd(sr_in, 16000), L = 16000 / g, M = sr_in / g, W = ceil(600 M / (99 min(L, M))), n_taps = 2 W + 2, output j
// reads the inputs k0 + i - W (k0 = floor(j M / L), zero outside the recording) against row p = (j M) mod L:
//   c = 0.99 min(L, M) / M,  t = clip((i - W - p / L) c, -6, 6),  h[p][i] = c sinc(t) cos^2(pi t / 12),  y[j] = sum_i h[p][i] x[k0 + i - W].
// Several channels are averaged first. The table is built on the host in f64 (resample_table) and rounded to f32 for the device.
//
// Kernel: a workgroup walks tiles of `tile` consecutive outputs. Per tile it stages the input span the tile reads (at most
// tile M / L + n_taps samples; channel mean and the zeros beyond both ends of the recording happen here) into LDS with 16-byte global
// loads over the aligned body of every channel row and scalar loads for its head and tail, then every lane accumulates its outputs from
// LDS in f32, taps in ascending order. j M is formed once per tile in 64 bits; inside a tile the offsets fit 32 bits.
// The table has three homes:
//   UNIFORM  L == 1: one row -- read from global memory at an address that is the same in every lane (one cache line per load, served
//            by the vector cache), so the coefficients cost no LDS cycles beside the input reads;
//   LDS      the table fits beside the span: copied once per workgroup (the grid is capped, workgroups stride over the tiles), laid out
//            [n_taps][L] so that the lanes of a wave, whose phases advance by M mod L, read distinct banks (L a multiple of 32 and M odd:
//            conflict-free; broadcast where phases coincide);
//   GLOBAL   larger tables (rates nearly coprime to 16000: 44101 Hz is 16000 x 36) stay [L][n_taps] in global memory: a lane's taps are
//            contiguous, so the loop walks one or two cache lines per lane.
#include "kernels.h"

#include <cmath>
#include <numeric>

namespace wca {

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_LDS_FLOATS = 12288;   // 48 KiB per workgroup: three workgroups per CU
constexpr int RS_TILE_MAX = 2048;

struct ResampleKernelArgs {
  const float* in;
  long ld, n_in;
  float* out;
  long n_out;
  const float* table;
  int channels, L, M, W, n_taps, tile, span_max;
};

// xs[0 .. span) = mean over channels of in[c][s0 + t], zero where s0 + t is outside [0, n_in)
__device__ __forceinline__ void stage_span(const ResampleKernelArgs& a, float* __restrict__ xs, long s0, int span) {
  const int tid = threadIdx.x;
  const long lo = s0 < 0 ? -s0 : 0, hi = a.n_in - s0;
  const int t_lo = (int)(lo < span ? lo : span);
  const int t_hi = (int)(hi < t_lo ? t_lo : (hi < span ? hi : span));
  for (int t = tid; t < t_lo; t += RS_THREADS) xs[t] = 0.f;
  for (int t = t_hi + tid; t < span; t += RS_THREADS) xs[t] = 0.f;
  const int n = t_hi - t_lo;
  float* dst = xs + t_lo;
  const float fc = (float)a.channels;
  for (int c = 0; c < a.channels; ++c) {
    const float* __restrict__ src = a.in + c * a.ld + (s0 + t_lo);
    const bool first = c == 0, last = c == a.channels - 1;
    auto put = [&](int t, float v) {
      if (!first) v += dst[t];
      if (last && !first) v /= fc;
      dst[t] = v;
    };
    // the row's 16-byte aligned body takes dwordx4 loads; its head and tail (at most 3 samples each) scalar ones
    int head = (int)((4 - ((reinterpret_cast<uintptr_t>(src) >> 2) & 3)) & 3);
    head = head < n ? head : n;
    const int nq = (n - head) >> 2;
    const int tail0 = head + 4 * nq;
    if (tid < head) {
      put(tid, src[tid]);
    } else if (tid < head + (n - tail0)) {
      const int t = tail0 + tid - head;
      put(t, src[t]);
    }
    for (int q = tid; q < nq; q += RS_THREADS) {
      const int t = head + 4 * q;
      const float4 v = *reinterpret_cast<const float4*>(src + t);
      put(t, v.x);
      put(t + 1, v.y);
      put(t + 2, v.z);
      put(t + 3, v.w);
    }
    if (!last) __syncthreads();   // the next channel's head differs, and with it the sample a thread adds to
  }
}

template <int HOME>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(ResampleKernelArgs a) {
  extern __shared__ float smem[];
  float* xs = smem;                // [span_max]
  float* hs = smem + a.span_max;   // HOME == RESAMPLE_HOME_LDS: [n_taps][L]
  const int tid = threadIdx.x;
  const float* __restrict__ tab = a.table;
  if (HOME == RESAMPLE_HOME_LDS)
    for (int i = tid; i < a.n_taps * a.L; i += RS_THREADS) hs[i] = tab[i];   // visible after the first tile's barrier
  const long n_tiles = (a.n_out + a.tile - 1) / a.tile;
  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long j0 = tile * a.tile;
    const int tn = (int)(a.n_out - j0 < a.tile ? a.n_out - j0 : a.tile);
    const long jm0 = j0 * (long)a.M;   // passes 2^31 within seconds of audio
    const long q0 = jm0 / a.L;
    const unsigned r0 = (unsigned)(jm0 - q0 * a.L);
    // output j0 + o: k0 - q0 = (r0 + o M) / L, phase (r0 + o M) mod L; r0 + o M < 16000 + 2048 * 384000 < 2^31
    const int span = (int)((r0 + (unsigned)(tn - 1) * (unsigned)a.M) / (unsigned)a.L) + a.n_taps;
    stage_span(a, xs, q0 - a.W, span);
    __syncthreads();
    for (int o = tid; o < tn; o += RS_THREADS) {
      const unsigned u = r0 + (unsigned)o * (unsigned)a.M;
      unsigned d = u, p = 0;
      if (HOME != RESAMPLE_HOME_UNIFORM) {
        d = u / (unsigned)a.L;
        p = u - d * (unsigned)a.L;
      }
      const float* x = xs + d;
      float acc = 0.f;
      if (HOME == RESAMPLE_HOME_UNIFORM) {
#pragma unroll 8
        for (int i = 0; i < a.n_taps; ++i) acc = fmaf(tab[i], x[i], acc);
      } else if (HOME == RESAMPLE_HOME_LDS) {
        const float* h = hs + p;
#pragma unroll 4
        for (int i = 0; i < a.n_taps; ++i) acc = fmaf(h[i * a.L], x[i], acc);
      } else {
        const float* __restrict__ h = tab + (long)p * a.n_taps;
#pragma unroll 4
        for (int i = 0; i < a.n_taps; ++i) acc = fmaf(h[i], x[i], acc);
      }
      a.out[j0 + o] = acc;
    }
    __syncthreads();   // the next tile overwrites xs
  }
}

// sr_in == 16000 with several channels: the plain mean
__global__ __launch_bounds__(RS_THREADS) void channel_mean_kernel(const float* __restrict__ in, int channels, long ld, long n, float* __restrict__ out) {
  const float fc = (float)channels;
  for (long k = (long)blockIdx.x * RS_THREADS + threadIdx.x; k < n; k += (long)gridDim.x * RS_THREADS) {
    float v = in[k];
    for (int c = 1; c < channels; ++c) v += in[c * ld + k];
    out[k] = v / fc;
  }
}

}  // namespace

int resample_plan(int sr_in, ResamplePlan* pl) {
  if (sr_in < RESAMPLE_SR_MIN || sr_in > RESAMPLE_SR_MAX || !pl) return -1;
  const int g = std::gcd(sr_in, RESAMPLE_SR_OUT);
  const long L = RESAMPLE_SR_OUT / g, M = sr_in / g, lo = L < M ? L : M;
  const long W = (600 * M + 99 * lo - 1) / (99 * lo);
  pl->L = (int)L;
  pl->M = (int)M;
  pl->W = (int)W;
  pl->n_taps = (int)(2 * W + 2);
  // the largest tile (a multiple of the workgroup) whose span fits the LDS budget beside the table, if the table goes there
  const long table = L * pl->n_taps;
  auto span_of = [&](long tile) { return ((L - 1) + (tile - 1) * M) / L + pl->n_taps; };
  pl->home = L == 1 ? RESAMPLE_HOME_UNIFORM : (table + span_of(RS_THREADS) <= RS_LDS_FLOATS ? RESAMPLE_HOME_LDS : RESAMPLE_HOME_GLOBAL);
  const long room = RS_LDS_FLOATS - (pl->home == RESAMPLE_HOME_LDS ? table : 0);
  long tile = RS_THREADS;
  while (tile + RS_THREADS <= RS_TILE_MAX && span_of(tile + RS_THREADS) <= room) tile += RS_THREADS;
  if (span_of(tile) > room) return -1;   // (cannot happen for sr_in <= 384000: 256 x 24 + 295 samples)
  pl->tile = (int)tile;
  pl->span_max = (int)span_of(tile);
  return 0;
}

void resample_table(const ResamplePlan& pl, double* h) {
  const double pi = 3.14159265358979323846;
  const double c = 0.99 * (double)(pl.L < pl.M ? pl.L : pl.M) / (double)pl.M;
  for (int p = 0; p < pl.L; ++p)
    for (int i = 0; i < pl.n_taps; ++i) {
      double t = ((double)(i - pl.W) - (double)p / (double)pl.L) * c;
      t = t < -6.0 ? -6.0 : (t > 6.0 ? 6.0 : t);
      const double sinc = t == 0.0 ? 1.0 : std::sin(pi * t) / (pi * t);
      const double w = std::cos(pi * t / 12.0);
      h[(size_t)p * pl.n_taps + i] = c * sinc * w * w;
    }
}

hipError_t launch_resample(const ResampleArgs& a, hipStream_t s) {
  if (!a.in || !a.out || a.channels < 1 || a.n_in < 0 || a.ld < a.n_in || a.n_out < 0 || a.max_blocks < 1) return hipErrorInvalidValue;
  if (a.n_out == 0) return hipSuccess;
  if (!a.plan) {   // 16 kHz in: copy, or the channel mean
    if (a.n_out != a.n_in) return hipErrorInvalidValue;
    if (a.channels == 1) return hipMemcpyAsync(a.out, a.in, sizeof(float) * (size_t)a.n_in, hipMemcpyDeviceToDevice, s);
    const long blocks = (a.n_in + RS_THREADS - 1) / RS_THREADS;
    hipLaunchKernelGGL(channel_mean_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(RS_THREADS), 0, s, a.in, a.channels, a.ld,
                       a.n_in, a.out);
    return hipGetLastError();
  }
  const ResamplePlan& pl = *a.plan;
  if (!a.table || a.n_out != (a.n_in * pl.L + pl.M - 1) / pl.M) return hipErrorInvalidValue;
  ResampleKernelArgs k{a.in, a.ld, a.n_in, a.out, a.n_out, a.table, a.channels, pl.L, pl.M, pl.W, pl.n_taps, pl.tile, pl.span_max};
  const long n_tiles = (a.n_out + pl.tile - 1) / pl.tile;
  const dim3 grid((unsigned)(n_tiles < a.max_blocks ? n_tiles : a.max_blocks));
  const size_t lds = sizeof(float) * (size_t)(pl.span_max + (pl.home == RESAMPLE_HOME_LDS ? pl.L * pl.n_taps : 0));
  if (lds > sizeof(float) * RS_LDS_FLOATS) return hipErrorInvalidValue;
  if (pl.home == RESAMPLE_HOME_UNIFORM)
    hipLaunchKernelGGL(resample_kernel<RESAMPLE_HOME_UNIFORM>, grid, dim3(RS_THREADS), lds, s, k);
  else if (pl.home == RESAMPLE_HOME_LDS)
    hipLaunchKernelGGL(resample_kernel<RESAMPLE_HOME_LDS>, grid, dim3(RS_THREADS), lds, s, k);
  else
    hipLaunchKernelGGL(resample_kernel<RESAMPLE_HOME_GLOBAL>, grid, dim3(RS_THREADS), lds, s, k);
  return hipGetLastError();
}

}  // namespace wca
