// libwca.so engine, audio front end: the resampler to 16 kHz with its table cache (wca_resample_*), the two log-mel forms (wca_log_mel and
// phase 1's run_logmel; wca_log_mel_long) the window cut wca_mel_window, the quiet cuts wca_quiet_cuts and the speech segments wca_speech_segments. Host code only: the kernels
// live in resample.hip / logmel.hip / quiet_cuts.hip / speech_segments.hip.
#include "engine_internal.h"

using namespace wca;

namespace {

// what pass 1 of both log-mel forms reads
int logmel_tables(const wca_engine* e, LogMelTables* t) {
  if (!e->have_filters) return fail(WCA_ERR_STATE, "mel_filters not loaded (wca_load_weight(\"mel_filters\"))");
  t->filters = e->mel_filters;
  t->filt_lo = e->filt_lo;
  t->filt_hi = e->filt_hi;
  t->window = e->window;
  t->twiddle = e->twiddle;
  t->precise = e->split ? 1 : 0;   // split mode: the DFT accumulates in f64
  t->n_mels = e->dims.n_mels;
  return WCA_OK;
}

// The polyphase table of sr_in on the device (f32, in the layout the plan's table home reads): the cached one, or built, uploaded and cached
// now. At most 8 rates stay; the oldest leaves.
int resample_table_dev(wca_engine* e, int sr_in, const ResamplePlan& pl, const wca_engine::ResampleTable** out) {
  constexpr size_t RS_TABLES_MAX = 8;
  auto it = std::find_if(e->rs_tables.begin(), e->rs_tables.end(), [&](const wca_engine::ResampleTable& t) { return t.sr_in == sr_in; });
  if (it == e->rs_tables.end()) {
    const size_t count = (size_t)pl.L * pl.n_taps;
    std::vector<double> h(count);
    resample_table(pl, h.data());
    std::vector<float> hf(count);
    for (int p = 0; p < pl.L; ++p)
      for (int i = 0; i < pl.n_taps; ++i)
        hf[pl.home == RESAMPLE_HOME_LDS ? (size_t)i * pl.L + p : (size_t)p * pl.n_taps + i] = (float)h[(size_t)p * pl.n_taps + i];
    if (e->rs_tables.size() >= RS_TABLES_MAX) {   // (hipFree waits for the launches that still read it)
      HIPCHK(hipFree(e->rs_tables.front().dev));
      e->rs_tables.erase(e->rs_tables.begin());
    }
    float* dev = nullptr;
    HIPCHK(hipMalloc(&dev, sizeof(float) * count));
    hipError_t ce = hipMemcpy(dev, hf.data(), sizeof(float) * count, hipMemcpyHostToDevice);
    if (ce != hipSuccess) {
      (void)hipFree(dev);
      HIPCHK(ce);
    }
    e->rs_tables.push_back({sr_in, pl, dev});
    it = e->rs_tables.end() - 1;
  }
  *out = &*it;
  return WCA_OK;
}

}  // namespace

namespace wca {

int check_pcm_lengths(const int32_t* n_samples_host, int batch, int64_t pcm_stride) {
  for (int b = 0; b < batch; ++b)
    if (n_samples_host[b] < 0 || n_samples_host[b] > 480000 || n_samples_host[b] > pcm_stride)
      return fail(WCA_ERR_INVALID, "n_samples[%d]=%d invalid (pad_or_trim to <= 480000 first)", b, n_samples_host[b]);
  return WCA_OK;
}

int run_logmel(wca_engine* e, const float* pcm_dev, int64_t pcm_stride, const int* n_samples_dev, int B, float* mel_out, bool want_tm) {
  LogMelArgs a{};
  WCA_TRY(logmel_tables(e, &a));
  a.pcm = pcm_dev;
  a.pcm_stride = pcm_stride;
  a.n_samples = n_samples_dev;
  a.mel_out = mel_out;
  a.mel_tm = want_tm ? e->mel_tm : nullptr;
  a.n_mels_pad = (e->split ? 2 : 1) * e->dims.n_mels;   // split mode: the conv stem reads pairs
  a.tm_lo = e->split ? e->dims.n_mels : 0;
  a.scratch = e->mel_scratch;
  a.gmax = e->gmax;
  a.B = B;
  HIPCHK(launch_logmel(a, e->stream));
  return WCA_OK;
}

}  // namespace wca

extern "C" {

int wca_log_mel(wca_engine* e, const float* pcm_dev, int64_t pcm_stride, const int32_t* n_samples_host, int batch, float* mel_out_dev) {
  if (!e || !pcm_dev || !n_samples_host || !mel_out_dev) return fail(WCA_ERR_INVALID, "null argument");
  if (batch < 1 || batch > e->max_batch) return fail(WCA_ERR_INVALID, "batch %d outside [1,%d]", batch, e->max_batch);
  WCA_TRY(check_pcm_lengths(n_samples_host, batch, pcm_stride));
  WCA_TRY(enter(e));
  int* rows[4];
  WCA_TRY(stage_meta(e, batch, n_samples_host, nullptr, nullptr, nullptr, rows));
  return run_logmel(e, pcm_dev, pcm_stride, rows[0], batch, mel_out_dev, false);
}

int wca_log_mel_long(wca_engine* e, const float* pcm_dev, int64_t n_samples, float* mel_out_dev, int64_t ld, int64_t* n_frames_out) {
  if (!e || !mel_out_dev || (!pcm_dev && n_samples > 0)) return fail(WCA_ERR_INVALID, "null argument");
  if (n_samples < 0 || n_samples > INT32_MAX - 480000) return fail(WCA_ERR_INVALID, "n_samples %lld outside [0, 2^31 - 480001]", (long long)n_samples);
  const int64_t T = (n_samples + 480000) / 160;
  if (n_frames_out) *n_frames_out = T;
  if (ld < T) return fail(WCA_ERR_INVALID, "ld %lld < %lld frames of %lld samples + 30 s", (long long)ld, (long long)T, (long long)n_samples);
  LogMelLongArgs a{};
  WCA_TRY(logmel_tables(e, &a));
  WCA_TRY(enter(e));
  a.pcm = pcm_dev;
  a.n_samples = n_samples;
  a.mel_out = mel_out_dev;
  a.ld = ld;
  a.n_frames = T;
  a.gmax = e->gmax;
  HIPCHK(launch_logmel_long(a, e->stream));
  return WCA_OK;
}

int wca_mel_window(wca_engine* e, const float* mel_long_dev, int64_t ld, int64_t n_frames, const int32_t* seek_host, const int32_t* size_host,
                   int batch, float* mel_out_dev) {
  if (!e || !mel_long_dev || !seek_host || !size_host || !mel_out_dev) return fail(WCA_ERR_INVALID, "null argument");
  if (batch < 1 || batch > e->max_batch) return fail(WCA_ERR_INVALID, "batch %d outside [1,%d]", batch, e->max_batch);
  if (n_frames < 1 || ld < n_frames) return fail(WCA_ERR_INVALID, "n_frames %lld / ld %lld invalid", (long long)n_frames, (long long)ld);
  for (int b = 0; b < batch; ++b) {
    if (size_host[b] < 1 || size_host[b] > N_FRAMES) return fail(WCA_ERR_INVALID, "size[%d]=%d outside [1,%d]", b, size_host[b], N_FRAMES);
    if (seek_host[b] < 0 || (int64_t)seek_host[b] + size_host[b] > n_frames)
      return fail(WCA_ERR_INVALID, "window %d: seek %d + size %d outside the %lld frames", b, seek_host[b], size_host[b], (long long)n_frames);
  }
  WCA_TRY(enter(e));
  int* rows[4];
  WCA_TRY(stage_meta(e, batch, seek_host, size_host, nullptr, nullptr, rows));
  HIPCHK(launch_mel_window(mel_long_dev, ld, e->dims.n_mels, rows[0], rows[1], batch, mel_out_dev, e->stream));
  return WCA_OK;
}

int wca_quiet_cuts(wca_engine* e, const float* mel_long_dev, int64_t ld, int64_t content_frames, int n_pieces, int radius, int half_width,
                   int32_t* cuts_host, int32_t* level_host) {
  if (!e || !mel_long_dev || !cuts_host) return fail(WCA_ERR_INVALID, "null argument");
  if (n_pieces < 2 || n_pieces > QUIET_PIECES_MAX) return fail(WCA_ERR_INVALID, "n_pieces %d outside [2,%d]", n_pieces, QUIET_PIECES_MAX);
  if (radius < 1 || radius > QUIET_RADIUS_MAX) return fail(WCA_ERR_INVALID, "radius %d outside [1,%d]", radius, QUIET_RADIUS_MAX);
  if (half_width < 0 || half_width > QUIET_HALF_WIDTH_MAX) return fail(WCA_ERR_INVALID, "half_width %d outside [0,%d]", half_width, QUIET_HALF_WIDTH_MAX);
  if (content_frames > ld || content_frames > INT32_MAX)
    return fail(WCA_ERR_INVALID, "content_frames %lld beyond ld %lld or 2^31 - 1", (long long)content_frames, (long long)ld);
  if (content_frames / n_pieces < 2 * radius + 2)   // (also refuses content_frames < 1): the search ranges stay disjoint and inside (0, content_frames)
    return fail(WCA_ERR_INVALID, "%lld frames in %d pieces leave %lld per piece: fewer than 2 radius + 2 = %d", (long long)content_frames, n_pieces,
                (long long)(content_frames / n_pieces), 2 * radius + 2);
  if (e->dims.n_mels > 128) return fail(WCA_ERR_INVALID, "n_mels %d > 128: the smoothed level would leave int32", e->dims.n_mels);
  WCA_TRY(enter(e));
  const int n = n_pieces - 1;
  HIPCHK(e->quiet_out.ensure(2 * sizeof(int) * (size_t)n));
  int* out_dev = (int*)e->quiet_out.p;
  HIPCHK(launch_quiet_cuts(mel_long_dev, ld, e->dims.n_mels, content_frames, n_pieces, radius, half_width, out_dev, out_dev + n, e->stream));
  std::vector<int32_t> out(2 * (size_t)n);
  HIPCHK(hipMemcpyAsync(out.data(), out_dev, sizeof(int32_t) * out.size(), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  cuts_host[0] = 0;
  memcpy(cuts_host + 1, out.data(), sizeof(int32_t) * (size_t)n);
  cuts_host[n_pieces] = (int32_t)content_frames;
  if (level_host) memcpy(level_host, out.data() + n, sizeof(int32_t) * (size_t)n);
  return WCA_OK;
}

int wca_speech_segments(wca_engine* e, const float* mel_long_dev, int64_t ld, int64_t content_frames, const wca_vad_opts* opts,
                        int32_t* segments_host, int max_segments, int32_t* stats_host) {
  if (!e || !mel_long_dev || !opts || !stats_host || (!segments_host && max_segments != 0)) return fail(WCA_ERR_INVALID, "null argument");
  if (max_segments < 0) return fail(WCA_ERR_INVALID, "max_segments %d negative", max_segments);
  if (content_frames < 1 || content_frames > ld || content_frames > INT32_MAX)
    return fail(WCA_ERR_INVALID, "content_frames %lld outside [1, min(ld = %lld, 2^31 - 1)]", (long long)content_frames, (long long)ld);
  const wca_vad_opts& o = *opts;
  constexpr int DUR_MAX = 1 << 24;
  if (o.half_width < 0 || o.half_width > QUIET_HALF_WIDTH_MAX) return fail(WCA_ERR_INVALID, "half_width %d outside [0,%d]", o.half_width, QUIET_HALF_WIDTH_MAX);
  if (o.floor_permille < 0 || o.floor_permille > o.peak_permille || o.peak_permille > 1000)
    return fail(WCA_ERR_INVALID, "0 <= floor_permille %d <= peak_permille %d <= 1000 does not hold", o.floor_permille, o.peak_permille);
  if (o.on_share < 1 || o.on_share > 1023 || o.off_share < 0 || o.off_share > o.on_share)
    return fail(WCA_ERR_INVALID, "0 <= off_share %d <= on_share %d, 1 <= on_share <= 1023 does not hold", o.off_share, o.on_share);
  if (o.min_range < 0 || o.min_range > 32768) return fail(WCA_ERR_INVALID, "min_range %d outside [0,32768]", o.min_range);
  if (o.min_speech < 1 || o.min_speech > DUR_MAX || o.min_silence < 1 || o.min_silence > DUR_MAX || o.pad < 0 || o.pad > DUR_MAX)
    return fail(WCA_ERR_INVALID, "min_speech %d / min_silence %d outside [1,2^24] or pad %d outside [0,2^24]", o.min_speech, o.min_silence, o.pad);
  if (e->dims.n_mels > 128) return fail(WCA_ERR_INVALID, "n_mels %d > 128: the smoothed level would leave int32", e->dims.n_mels);
  WCA_TRY(enter(e));
  const long cap = std::min<long>(max_segments, (content_frames + 1) / 2);   // more runs than that do not fit into content_frames frames
  HIPCHK(e->vad_buf.ensure(vad_scratch(nullptr, content_frames, cap).bytes));
  const VadScratch sc = vad_scratch(e->vad_buf.p, content_frames, cap);
  const VadOpts vo{o.half_width, o.floor_permille, o.peak_permille, o.on_share, o.off_share, o.min_range, o.min_speech, o.min_silence, o.pad};
  HIPCHK(launch_speech_segments(mel_long_dev, ld, e->dims.n_mels, content_frames, vo, cap, sc, e->stream));
  int32_t stats[6];
  HIPCHK(hipMemcpyAsync(stats, sc.stats, sizeof(stats), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  const long n = std::min<long>(stats[5], cap);
  if (n > 0) {
    HIPCHK(hipMemcpyAsync(segments_host, sc.segs, sizeof(int32_t) * 2 * (size_t)n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  memcpy(stats_host, stats, sizeof(stats));
  return WCA_OK;
}

int wca_resample_plan(int sr_in, int32_t* L, int32_t* M, int32_t* W, int32_t* n_taps) {
  ResamplePlan pl;
  if (resample_plan(sr_in, &pl)) return fail(WCA_ERR_INVALID, "sr_in %d outside [%d, %d]", sr_in, RESAMPLE_SR_MIN, RESAMPLE_SR_MAX);
  if (L) *L = pl.L;
  if (M) *M = pl.M;
  if (W) *W = pl.W;
  if (n_taps) *n_taps = pl.n_taps;
  return WCA_OK;
}

int wca_resample_table(int sr_in, double* table_out) {
  if (!table_out) return fail(WCA_ERR_INVALID, "null argument");
  ResamplePlan pl;
  if (resample_plan(sr_in, &pl)) return fail(WCA_ERR_INVALID, "sr_in %d outside [%d, %d]", sr_in, RESAMPLE_SR_MIN, RESAMPLE_SR_MAX);
  resample_table(pl, table_out);
  return WCA_OK;
}

int wca_resample_16k(wca_engine* e, const float* in_dev, int channels, int64_t ld, int64_t n_in, int sr_in, float* out_dev, int64_t out_cap,
                     int64_t* n_out) {
  if (!e || !n_out || (n_in > 0 && (!in_dev || !out_dev))) return fail(WCA_ERR_INVALID, "null argument");
  if (channels < 1 || channels > 8) return fail(WCA_ERR_INVALID, "channels %d outside [1, 8]", channels);
  ResamplePlan pl;
  if (resample_plan(sr_in, &pl)) return fail(WCA_ERR_INVALID, "sr_in %d outside [%d, %d]", sr_in, RESAMPLE_SR_MIN, RESAMPLE_SR_MAX);
  const int64_t n_max = INT32_MAX - 480000;   // what wca_log_mel_long takes
  if (n_in < 0 || n_in > ld || n_in > n_max * 24) return fail(WCA_ERR_INVALID, "n_in %lld outside [0, ld = %lld]", (long long)n_in, (long long)ld);
  const int64_t n = (n_in * pl.L + pl.M - 1) / pl.M;   // (n_in L < 2^31 x 24 x 16000)
  if (n > n_max) return fail(WCA_ERR_INVALID, "%lld samples at %d Hz give %lld at 16 kHz: more than 2^31 - 480001", (long long)n_in, sr_in, (long long)n);
  *n_out = n;
  if (out_cap < n) return fail(WCA_ERR_INVALID, "out_cap %lld < %lld output samples", (long long)out_cap, (long long)n);
  if (n == 0) return WCA_OK;
  WCA_TRY(enter(e));
  ResampleArgs a{};
  a.in = in_dev;
  a.channels = channels;
  a.ld = ld;
  a.n_in = n_in;
  a.out = out_dev;
  a.n_out = n;
  a.max_blocks = 3 * (e->n_cu > 0 ? e->n_cu : 256);
  if (sr_in != RESAMPLE_SR_OUT) {   // the filter is no identity at equal rates, and upstream does nothing there: a copy (the channel mean)
    const wca_engine::ResampleTable* t = nullptr;
    WCA_TRY(resample_table_dev(e, sr_in, pl, &t));
    a.plan = &t->plan;
    a.table = t->dev;
  }
  HIPCHK(launch_resample(a, e->stream));
  return WCA_OK;
}

}  // extern "C"
