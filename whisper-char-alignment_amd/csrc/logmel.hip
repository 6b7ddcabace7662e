// Log-mel front end on gfx950.  Reference call sites: dataset.py:46-48 / dataset.py:107-109 /
// README.md:101-103 -> whisper.pad_or_trim + whisper.log_mel_spectrogram:
//   zero-pad to 480000 samples, STFT(n_fft 400, hop 160, periodic hann, centre/reflect), |.|^2 of the
//   first 3000 frames, mel filterbank, log10(clamp 1e-10), floor at (global max - 8), (x + 4) / 4.
//
// Pass 1 (one workgroup per frame): windowed frame -> LDS, 201-bin real DFT with the n <-> 400-n
//   fold (even part against cos, odd part against sin: 199 steps instead of 399), power spectrum ->
//   LDS, sparse triangular mel filters, log10; per-utterance running max via ordered-int atomicMax.
//   Frames that only see zero padding are skipped: their value is exactly log10(1e-10) = -10.
// Pass 2: floor/scale, writes the API layout [n_mels][3000] f32 and the time-major f16 image
//   [3002][n_mels] (zero rows at both ends) that the conv-stem GEMM reads as overlapping windows.
//
// Whole recordings (upstream whisper.transcribe: log_mel_spectrogram(audio, n_mels, padding=N_SAMPLES)): the same pass 1 per frame on a
//   grid sized from the recording, one device-wide maximum, pass 2 in place; then the window cut pad_or_trim(mel[:, seek:seek+size], 3000).
#include "kernels.h"
#include "wca_common.h"

namespace wca {

namespace {

constexpr int NFFT = 400, HOP = 160, NBIN = 201, NFRAMES = 3000, NSAMP = 480000;

__device__ __forceinline__ unsigned f2ord(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned o) {
  const unsigned u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  return __uint_as_float(u);
}

__device__ __forceinline__ int active_frames(int n_samples) {
  // frame t touches audio indices [t*160 - 200, t*160 + 199]; non-zero iff t*160 - 200 < n_samples
  int na = (n_samples + 200 + HOP - 1) / HOP;
  return na < NFRAMES ? na : NFRAMES;
}

__global__ void logmel_init_kernel(unsigned* gmax, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) gmax[i] = f2ord(-10.0f);
}

// LDS of one frame's pass 1
struct FrameLds {
  float e[NFFT / 2 + 1];   // even part  e[n] = s[n] + s[400-n], n = 1..199 ; e[0] = s[0], e[200] = s[200]
  float o[NFFT / 2 + 1];   // odd part   o[n] = s[n] - s[400-n]
  float raw[NFFT];
  f32x2 tw[NFFT];
  float pow[NBIN + 3];
  float max[4];
};

// Pass 1 of frame t by one 256-thread workgroup: `pcm` holds `ns` samples of a signal that is zero from there up to `total` samples
// (the reflect padding mirrors at 0 and at total - 1). Thread m < n_mels writes log10(clamp(mel m)) to out[m * ld]; thread 0 folds the
// frame's maximum into *gmax.
__device__ __forceinline__ void frame_log_mel(const LogMelTables& a, FrameLds& s, const float* __restrict__ pcm, long ns, long total, long t,
                                              float* __restrict__ out, long ld, unsigned* gmax) {
  const int tid = threadIdx.x;
  for (int n = tid; n < NFFT; n += 256) {
    long idx = t * HOP - NFFT / 2 + n;
    if (idx < 0) idx = -idx;                            // reflect (centre=True)
    if (idx >= total) idx = 2 * (total - 1) - idx;
    const float x = (idx < ns) ? pcm[idx] : 0.f;
    s.raw[n] = x * a.window[n];
    s.tw[n] = reinterpret_cast<const f32x2*>(a.twiddle)[n];
  }
  __syncthreads();
  for (int n = tid; n <= NFFT / 2; n += 256) {
    if (n == 0 || n == NFFT / 2) {
      s.e[n] = s.raw[n];
      s.o[n] = 0.f;
    } else {
      s.e[n] = s.raw[n] + s.raw[NFFT - n];
      s.o[n] = s.raw[n] - s.raw[NFFT - n];
    }
  }
  __syncthreads();
  if (tid < NBIN) {
    const int k = tid;
    if (a.precise) {
      // reference-precision mode: f64 accumulation of the f32 products (the reference's FFT is accurate to ~1e-7 of the frame's
      // magnitude; a 199-term f32 sum is not). Twiddles and folded samples stay the f32 values above.
      double re = (double)s.e[0] + ((k & 1) ? -(double)s.e[NFFT / 2] : (double)s.e[NFFT / 2]);
      double im = 0.0;
      int idx = 0;
      for (int n = 1; n < NFFT / 2; ++n) {
        idx += k;
        if (idx >= NFFT) idx -= NFFT;
        const f32x2 tw = s.tw[idx];
        re = fma((double)s.e[n], (double)tw[0], re);
        im = fma((double)s.o[n], (double)tw[1], im);
      }
      const float ref = (float)re, imf = (float)im;  // torch.stft returns complex64; abs()**2 is then f32 arithmetic
      s.pow[k] = ref * ref + imf * imf;
    } else {
      float re = s.e[0] + ((k & 1) ? -s.e[NFFT / 2] : s.e[NFFT / 2]);
      float im = 0.f;
      int idx = 0;
      for (int n = 1; n < NFFT / 2; ++n) {
        idx += k;
        if (idx >= NFFT) idx -= NFFT;
        const f32x2 tw = s.tw[idx];
        re = fmaf(s.e[n], tw[0], re);
        im = fmaf(s.o[n], tw[1], im);
      }
      s.pow[k] = re * re + im * im;
    }
  }
  __syncthreads();
  float lv = -INFINITY;
  if (tid < a.n_mels) {
    const int m = tid;
    const int lo = a.filt_lo[m], hi = a.filt_hi[m];
    const float* fr = a.filters + (long)m * NBIN;
    float acc = 0.f;
    if (a.precise) {  // the reference's `filters @ magnitudes` is an f32 matmul in some blocked order: the f64 sum is within half an ulp of any
      double acc64 = 0.0;
      for (int k = lo; k < hi; ++k) acc64 = fma((double)fr[k], (double)s.pow[k], acc64);
      acc = (float)acc64;
    } else {
      for (int k = lo; k < hi; ++k) acc = fmaf(fr[k], s.pow[k], acc);
    }
    // a clamped bin is exactly -10, the value the skipped frames get in pass 2 (the device's log10f(1e-10f) is one ulp below it, so
    // silence inside the active frames came out as -1.5000002 beside the -1.5 of the frames after them)
    lv = (acc > 1e-10f) ? log10f(acc) : -10.0f;
    out[(long)m * ld] = lv;
  }
  lv = wave_max(lv);
  if ((tid & 63) == 0) s.max[tid >> 6] = lv;
  __syncthreads();
  if (tid == 0) {
    const float mx = fmaxf(fmaxf(s.max[0], s.max[1]), fmaxf(s.max[2], s.max[3]));
    atomicMax(gmax, f2ord(mx));
  }
}

__global__ __launch_bounds__(256) void logmel_power_kernel(LogMelArgs a) {
  __shared__ FrameLds s;
  const int t = blockIdx.x, b = blockIdx.y;
  const int ns = a.n_samples[b];
  if (t >= active_frames(ns)) return;
  frame_log_mel(a, s, a.pcm + (long)b * a.pcm_stride, ns, NSAMP, t, a.scratch + (long)b * a.n_mels * NFRAMES + t, NFRAMES, a.gmax + b);
}

__global__ __launch_bounds__(256) void logmel_finalize_kernel(LogMelArgs a) {
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * 64;
  const int na = active_frames(a.n_samples[b]);
  const float floorv = ord2f(a.gmax[b]) - 8.0f;
  const float* sc = a.scratch + (long)b * a.n_mels * NFRAMES;
  // API layout [m][t]: threads run along t
  if (a.mel_out) {
    float* mo = a.mel_out + (long)b * a.n_mels * NFRAMES;
    for (int e = threadIdx.x; e < a.n_mels * 64; e += 256) {
      const int m = e >> 6, t = t0 + (e & 63);
      if (t < NFRAMES) {
        const float v = (t < na) ? sc[(long)m * NFRAMES + t] : -10.0f;
        mo[(long)m * NFRAMES + t] = (fmaxf(v, floorv) + 4.0f) * 0.25f;
      }
    }
  }
  // time-major f16 image [t + 1][m]: threads run along m
  if (a.mel_tm) {
    half_t* mt = a.mel_tm + (long)b * (NFRAMES + 2) * a.n_mels_pad;
    for (int e = threadIdx.x; e < a.n_mels * 64; e += 256) {
      const int tt = e / a.n_mels, m = e - tt * a.n_mels;
      const int t = t0 + tt;
      if (t < NFRAMES) {
        const float v = (t < na) ? sc[(long)m * NFRAMES + t] : -10.0f;
        const float y = (fmaxf(v, floorv) + 4.0f) * 0.25f;
        if (a.tm_lo) {
          const HalfPair pr = split_pair(y);
          mt[(long)(t + 1) * a.n_mels_pad + m] = pr.hi;
          mt[(long)(t + 1) * a.n_mels_pad + a.tm_lo + m] = pr.lo;
        } else {
          mt[(long)(t + 1) * a.n_mels_pad + m] = (half_t)y;
        }
      }
    }
  }
}

// ---- whole-recording form: the grid is sized from the recording, pass 1 leaves the raw log10 values in mel_out, pass 2 floors them
// in place with the maximum over all frames.
__device__ __forceinline__ long active_frames_long(long n_samples, long n_frames) {
  const long na = (n_samples + 200 + HOP - 1) / HOP;
  return na < n_frames ? na : n_frames;
}

__global__ void logmel_long_init_kernel(unsigned* gmax) { *gmax = f2ord(-10.0f); }

__global__ __launch_bounds__(256) void logmel_long_power_kernel(LogMelLongArgs a) {
  __shared__ FrameLds s;
  const long t = blockIdx.x;   // the launch covers the active frames only
  frame_log_mel(a, s, a.pcm, a.n_samples, a.n_samples + NSAMP, t, a.mel_out + t, a.ld, a.gmax);
}

__global__ __launch_bounds__(256) void logmel_long_finalize_kernel(LogMelLongArgs a) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.n_frames) return;
  const float floorv = ord2f(*a.gmax) - 8.0f;
  float* p = a.mel_out + (long)blockIdx.y * a.ld + t;
  const float v = (t < active_frames_long(a.n_samples, a.n_frames)) ? *p : -10.0f;
  *p = (fmaxf(v, floorv) + 4.0f) * 0.25f;
}

__global__ __launch_bounds__(256) void mel_window_kernel(const float* __restrict__ mel_long, long ld, const int* __restrict__ seek,
                                                         const int* __restrict__ size, float* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y, b = blockIdx.z;
  if (t >= NFRAMES) return;
  const float v = (t < size[b]) ? mel_long[(long)m * ld + seek[b] + t] : 0.f;
  out[((long)b * gridDim.y + m) * NFRAMES + t] = v;
}

}  // namespace

hipError_t launch_logmel(const LogMelArgs& a, hipStream_t s) {
  if (a.B <= 0) return hipSuccess;
  if (a.n_mels > 256) return hipErrorInvalidValue;
  hipLaunchKernelGGL(logmel_init_kernel, dim3((a.B + 63) / 64), dim3(64), 0, s, a.gmax, a.B);
  hipLaunchKernelGGL(logmel_power_kernel, dim3(NFRAMES, a.B), dim3(256), 0, s, a);
  hipLaunchKernelGGL(logmel_finalize_kernel, dim3((NFRAMES + 63) / 64, a.B), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_logmel_long(const LogMelLongArgs& a, hipStream_t s) {
  if (a.n_mels > 256 || a.n_samples < 0 || a.n_frames != (a.n_samples + NSAMP) / HOP || a.ld < a.n_frames) return hipErrorInvalidValue;
  const long na = (a.n_samples + 200 + HOP - 1) / HOP < a.n_frames ? (a.n_samples + 200 + HOP - 1) / HOP : a.n_frames;
  hipLaunchKernelGGL(logmel_long_init_kernel, dim3(1), dim3(1), 0, s, a.gmax);
  if (na > 0) hipLaunchKernelGGL(logmel_long_power_kernel, dim3((unsigned)na), dim3(256), 0, s, a);
  hipLaunchKernelGGL(logmel_long_finalize_kernel, dim3((unsigned)((a.n_frames + 255) / 256), a.n_mels), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_mel_window(const float* mel_long, long ld, int n_mels, const int* seek, const int* size, int B, float* out, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(mel_window_kernel, dim3((NFRAMES + 255) / 256, n_mels, B), dim3(256), 0, s, mel_long, ld, seek, size, out);
  return hipGetLastError();
}

}  // namespace wca
