// libwca.so engine, alignment: the step-by-step API (log-mel, attentions, filters, DTW, probes), the batched path
// wca_align_batch_enqueue / _fetch with its two phases, wca_encode_batch and the teacher-token log-probs.
#include "engine_internal.h"

using namespace wca;

namespace {

int check_pcm_lengths(const int32_t* n_samples_host, int batch, int64_t pcm_stride) {
  for (int b = 0; b < batch; ++b)
    if (n_samples_host[b] < 0 || n_samples_host[b] > 480000 || n_samples_host[b] > pcm_stride)
      return fail(WCA_ERR_INVALID, "n_samples[%d]=%d invalid (pad_or_trim to <= 480000 first)", b, n_samples_host[b]);
  return WCA_OK;
}

int validate_lengths(int B, int n_tok_max, const int32_t* n_tok, const int32_t* max_frames, int* Fmax_out) {
  if (n_tok_max > MAX_TOK) return fail(WCA_ERR_TOO_LONG, "n_tok %d > %d", n_tok_max, MAX_TOK);
  if (n_tok_max < 1) return fail(WCA_ERR_INVALID, "n_tok %d < 1", n_tok_max);
  int Fmax = 0;
  for (int b = 0; b < B; ++b) {
    if (n_tok && (n_tok[b] > n_tok_max || n_tok[b] < 0)) return fail(WCA_ERR_INVALID, "n_tok[%d]=%d outside [0,%d]", b, n_tok[b], n_tok_max);
    if (max_frames[b] > N_CTX) return fail(WCA_ERR_TOO_LONG, "max_frames[%d]=%d > %d", b, max_frames[b], N_CTX);
    if (max_frames[b] < 1) return fail(WCA_ERR_INVALID, "max_frames[%d]=%d < 1", b, max_frames[b]);
    Fmax = max_frames[b] > Fmax ? max_frames[b] : Fmax;
  }
  *Fmax_out = Fmax;
  return WCA_OK;
}

// scores/top-k/aggregate/DTW on a dense weights tensor [B][LH][n_max][Fmax] whose column norms and
// scores are already in e->colnorm / e->scores.
struct Remat {
  const float* qk = nullptr;
  long qk_bs = 0, qk_hs = 0;
  int qk_ld = 0;
  const float* rowstats = nullptr;
};

int run_select_aggregate_dtw(wca_engine* e, const float* weights, int B, int LH, int n_max, int Fmax, const int* n_tok_dev,
                             const int* n_frames_dev, const int* dtwN_dev, const wca_align_opts* o, int L_layers,
                             const Remat* rm = nullptr, hipStream_t s_in = nullptr) {
  hipStream_t s = s_in ? s_in : e->stream;
  const int k = o->aggregation == WCA_AGGR_TOPK ? o->topk : 0;
  if (o->aggregation == WCA_AGGR_TOPK) {
    HIPCHK(e->sel.ensure(sizeof(int) * (size_t)B * k));
    HIPCHK(e->selsc.ensure(sizeof(float) * (size_t)B * k));
    HIPCHK(launch_topk((const float*)e->scores.p, LH, B, k, (int*)e->sel.p, (float*)e->selsc.p, s));
  }
  HIPCHK(e->matrix.ensure(sizeof(float) * (size_t)B * n_max * Fmax));
  AggregateArgs g{};
  g.weights = weights;
  g.w_bs = (long)LH * n_max * Fmax;
  g.n_tok_max = n_max;
  g.n_frames_max = Fmax;
  g.colnorm = (const float*)e->colnorm.p;
  g.LH = LH;
  g.B = B;
  g.n_tok = n_tok_dev;
  g.n_frames = n_frames_dev;
  g.row_lo = o->sot_len;
  g.row_hi_trim = 1;
  g.matrix = (float*)e->matrix.p;
  if (rm) {
    g.qk = rm->qk;
    g.qk_bs = rm->qk_bs;
    g.qk_hs = rm->qk_hs;
    g.qk_ld = rm->qk_ld;
    g.rowstats = rm->rowstats;
    g.medfilt_width = o->medfilt_width;
    g.qk_scale = o->qk_scale;
  }
  if (o->aggregation == WCA_AGGR_TOPK) {
    g.sel_idx = (const int*)e->sel.p;
    g.n_sel = k;
  } else {
    g.sel_idx = nullptr;
    const int H = LH / L_layers;
    g.head_lo = (L_layers / 2) * H;  // ws[n_layers//2:]  (timing.py:88)
  }
  HIPCHK(launch_aggregate(g, s));
  record(e, 6, s);

  const int Nmax = n_max - o->sot_len - 1;
  if (Nmax >= 1) {
    const int wpr = (Fmax + 15) / 16;
    const int cap = Nmax + Fmax + 2;
    HIPCHK(e->trace.ensure(sizeof(uint32_t) * (size_t)B * Nmax * wpr));
    HIPCHK(e->path.ensure(sizeof(int) * (size_t)B * 2 * cap));
    HIPCHK(e->pathlen.ensure(sizeof(int) * (size_t)B));
    HIPCHK(e->jump.ensure(sizeof(int) * (size_t)B * n_max));
    // the DTW writes n_tok[b] - sot_len - 1 entries per utterance; the rest of a row is defined as 0 (the buffer is recycled memory, and a
    // caller that compares or stores whole rows must not see what an earlier allocation left there)
    HIPCHK(hipMemsetAsync(e->jump.p, 0, sizeof(int) * (size_t)B * n_max, s));
    DtwArgs dg{};
    dg.matrix = (const float*)e->matrix.p;
    dg.m_bs = (long)n_max * Fmax;
    dg.ld = Fmax;
    dg.N = dtwN_dev;
    dg.M = n_frames_dev;
    dg.N_max = Nmax;
    dg.M_max = Fmax;
    dg.trace = (uint32_t*)e->trace.p;
    dg.path = (int*)e->path.p;
    dg.path_len = (int*)e->pathlen.p;
    dg.jump_frame = (int*)e->jump.p;
    dg.jump_ld = n_max;
    dg.P = B;
    HIPCHK(launch_dtw(dg, s));
  }
  return WCA_OK;
}

int ensure_res_host(wca_engine* e, int slot, size_t ints) {
  if (ints <= e->res_host_ints[slot]) return WCA_OK;
  if (e->res_host[slot]) (void)hipHostFree(e->res_host[slot]);
  e->res_host[slot] = nullptr;
  e->res_host_ints[slot] = 0;
  HIPCHK(hipHostMalloc((void**)&e->res_host[slot], ints * sizeof(int), hipHostMallocDefault));
  e->res_host_ints[slot] = ints;
  return WCA_OK;
}

constexpr int ERR_TARGET_VOCAB = 4;   // err_dev bit: a teacher token outside [0, vocab_end) (its log-prob is NaN)

// Teacher-token log-probs of one aligned micro-batch on stream s (timing.py:146-149 of the reference in log space), after
// run_decoder(..., finish_last = true) left the final residual stream in e->xd. Only the R = sum_b n_text_b rows that predict a text token go
// on: gathered (row_off_dev: device [B] prefix sums of n_text), final LayerNorm (pairs in split mode), the vocabulary projection against
// tok_emb rows [0, vocab_end) in row chunks whose f32 logits stay under 256 MB (1 024 x 50 257 x 4 B = 206 MB), token_logprob_kernel per chunk.
// out [B][n_tok_max]: entries [0, n_text_b) of row b, the rest 0.
int run_token_logprobs(wca_engine* e, hipStream_t s, const int64_t* tokens_dev, int B, int n_tok_max, int sot_len, int vocab_end,
                       const int* n_tok_dev, const int* row_off_dev, int R, int n_text_max, float* out) {
  const int dt = e->dims.n_text_state;
  const bool sp = e->split;
  const int om = sp ? 2 : 1;
  HIPCHK(hipMemsetAsync(out, 0, sizeof(float) * (size_t)B * n_tok_max, s));
  if (R <= 0) return WCA_OK;
  HIPCHK(e->lp_x.ensure(sizeof(float) * (size_t)R * dt));
  HIPCHK(e->lp_xn.ensure(sizeof(half_t) * (size_t)om * R * dt));
  HIPCHK(e->lp_map.ensure(sizeof(int) * (size_t)R));
  float* xr = (float*)e->lp_x.p;
  half_t* xn = (half_t*)e->lp_xn.p;
  int* map = (int*)e->lp_map.p;
  HIPCHK(launch_gather_text_rows(e->xd, n_tok_max, dt, sot_len, n_tok_dev, row_off_dev, B, n_text_max, xr, map, s));
  HIPCHK(launch_layernorm_f16(xr, e->lnf_g, e->lnf_b, xn, R, dt, 1e-5f, s, om * dt, sp ? dt : 0));
  const int ldc = (int)align_up((size_t)vocab_end, 64);   // (the aligned f32 store path of the GEMM epilogue)
  const int chunk = std::min(R, std::max(1, std::min(1024, (int)(((size_t)256 << 20) / ((size_t)ldc * sizeof(float))))));
  HIPCHK(e->lp_logits.ensure(sizeof(float) * (size_t)chunk * ldc));
  float* lg = (float*)e->lp_logits.p;
  for (int r0 = 0; r0 < R; r0 += chunk) {
    const int m = std::min(chunk, R - r0);
    const GemmOpnd o = pick_operands(sp, e->tok_emb, sp ? e->sw.tok_emb : e->tok_emb, dt, m, vocab_end, 1, e);
    Gemm g = flat(xn + (size_t)r0 * om * dt, o, lg, ldc, m, vocab_end);
    g.out_mode = 1;
    g.site = 3;
    HIPCHK(gemm(e, s, g));
    HIPCHK(launch_token_logprob(lg, ldc, vocab_end, m, tokens_dev, map + r0, sot_len + 1, out, e->err_dev, ERR_TARGET_VOCAB, s));
  }
  return WCA_OK;
}

}  // namespace

extern "C" {

int wca_log_mel(wca_engine* e, const float* pcm_dev, int64_t pcm_stride, const int32_t* n_samples_host, int batch, float* mel_out_dev) {
  if (!e || !pcm_dev || !n_samples_host || !mel_out_dev) return fail(WCA_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(e->device));
  if (int jr = join_phase2(e)) return jr;
  if (batch < 1 || batch > e->max_batch) return fail(WCA_ERR_INVALID, "batch %d outside [1,%d]", batch, e->max_batch);
  for (int b = 0; b < batch; ++b)
    if (n_samples_host[b] < 0 || n_samples_host[b] > 480000 || n_samples_host[b] > pcm_stride)
      return fail(WCA_ERR_INVALID, "n_samples[%d]=%d invalid (pad_or_trim to <= 480000 first)", b, n_samples_host[b]);
  int* rows[4];
  int rc = stage_meta(e, batch, n_samples_host, nullptr, nullptr, nullptr, rows);
  if (rc) return rc;
  return run_logmel(e, pcm_dev, pcm_stride, rows[0], batch, mel_out_dev, false);
}

int wca_log_mel_long(wca_engine* e, const float* pcm_dev, int64_t n_samples, float* mel_out_dev, int64_t ld, int64_t* n_frames_out) {
  if (!e || !mel_out_dev || (!pcm_dev && n_samples > 0)) return fail(WCA_ERR_INVALID, "null argument");
  if (n_samples < 0 || n_samples > INT32_MAX - 480000) return fail(WCA_ERR_INVALID, "n_samples %lld outside [0, 2^31 - 480001]", (long long)n_samples);
  const int64_t T = (n_samples + 480000) / 160;
  if (n_frames_out) *n_frames_out = T;
  if (ld < T) return fail(WCA_ERR_INVALID, "ld %lld < %lld frames of %lld samples + 30 s", (long long)ld, (long long)T, (long long)n_samples);
  if (!e->have_filters) return fail(WCA_ERR_STATE, "mel_filters not loaded (wca_load_weight(\"mel_filters\"))");
  HIPCHK(hipSetDevice(e->device));
  if (int jr = join_phase2(e)) return jr;
  LogMelLongArgs a{};
  a.filters = e->mel_filters;
  a.filt_lo = e->filt_lo;
  a.filt_hi = e->filt_hi;
  a.window = e->window;
  a.twiddle = e->twiddle;
  a.precise = e->split ? 1 : 0;
  a.n_mels = e->dims.n_mels;
  a.pcm = pcm_dev;
  a.n_samples = n_samples;
  a.mel_out = mel_out_dev;
  a.ld = ld;
  a.n_frames = T;
  a.gmax = e->gmax;
  HIPCHK(launch_logmel_long(a, e->stream));
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
  constexpr size_t RS_TABLES_MAX = 8;
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
  HIPCHK(hipSetDevice(e->device));
  if (int jr = join_phase2(e)) return jr;
  ResampleArgs a{};
  a.in = in_dev;
  a.channels = channels;
  a.ld = ld;
  a.n_in = n_in;
  a.out = out_dev;
  a.n_out = n;
  a.max_blocks = 3 * (e->n_cu > 0 ? e->n_cu : 256);
  if (sr_in != RESAMPLE_SR_OUT) {   // the filter is no identity at equal rates, and upstream does nothing there: a copy (the channel mean)
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
    a.plan = &it->plan;
    a.table = it->dev;
  }
  HIPCHK(launch_resample(a, e->stream));
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
  HIPCHK(hipSetDevice(e->device));
  if (int jr = join_phase2(e)) return jr;
  int* rows[4];
  int rc = stage_meta(e, batch, seek_host, size_host, nullptr, nullptr, rows);
  if (rc) return rc;
  HIPCHK(launch_mel_window(mel_long_dev, ld, e->dims.n_mels, rows[0], rows[1], batch, mel_out_dev, e->stream));
  return WCA_OK;
}

int wca_get_attentions(wca_engine* e, const float* mel_dev, const int64_t* tokens_dev, int batch, int n_tok, const int32_t* n_tok_host,
                       const int32_t* max_frames_host, int medfilt_width, float qk_scale, float* weights_out_dev,
                       float* logits_out_dev) {
  int rc = check_ready(e);
  if (rc) return rc;
  if ((rc = join_phase2(e))) return rc;
  if (!mel_dev || !tokens_dev || !max_frames_host || !weights_out_dev) return fail(WCA_ERR_INVALID, "null argument");
  if (batch < 1 || batch > e->max_batch) return fail(WCA_ERR_INVALID, "batch %d outside [1,%d]", batch, e->max_batch);
  if (medfilt_width < 1 || !(medfilt_width & 1) || medfilt_width > 33) return fail(WCA_ERR_INVALID, "medfilt_width must be odd and <= 33");
  int Fmax = 0;
  rc = validate_lengths(batch, n_tok, n_tok_host, max_frames_host, &Fmax);
  if (rc) return rc;
  const wca_model_dims& D = e->dims;
  const int LH = D.n_text_layer * D.n_text_head;
  const int Fpad = (Fmax + 3) & ~3;
  std::vector<int32_t> ntok(batch);
  for (int b = 0; b < batch; ++b) ntok[b] = n_tok_host ? n_tok_host[b] : n_tok;
  int* rows[4];
  rc = stage_meta(e, batch, nullptr, ntok.data(), max_frames_host, nullptr, rows);
  if (rc) return rc;
  if ((rc = mel_to_tm(e, mel_dev, batch))) return rc;
  // cross-K/V go into a slot no queued batch (wca_encode_batch / wca_greedy_decode / an un-fetched alignment) still needs
  const int slot = take_kv_slot(e);
  if (slot < 0) return fail(WCA_ERR_STATE, "both cross-K/V slots hold live batches: fetch or consume one first");
  half_t* kvbuf = slot ? e->kv_alt : e->kv;
  HIPCHK(hipMemsetAsync(e->err_dev, 0, sizeof(int), e->stream));
  rc = run_encoder(e, batch);
  if (rc) return rc;
  rc = run_cross_kv(e, batch, kvbuf);
  if (rc) return rc;
  HIPCHK(e->cap.ensure(sizeof(float) * (size_t)batch * LH * n_tok * Fpad));
  rc = run_decoder(e, tokens_dev, batch, n_tok, (float*)e->cap.p, Fpad, Fmax, logits_out_dev, nullptr, kvbuf);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(e->err_host, e->err_dev, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e->colnorm.ensure(sizeof(float) * (size_t)batch * LH * Fmax));
  HIPCHK(e->scores.ensure(sizeof(float) * (size_t)batch * LH));
  HeadStatsArgs h{};
  h.qk = (const float*)e->cap.p;
  h.qk_bs = (long)LH * n_tok * Fpad;
  h.qk_hs = (long)n_tok * Fpad;
  h.qk_ld = Fpad;
  h.weights = weights_out_dev;
  h.w_bs = (long)LH * n_tok * Fmax;
  h.n_tok = rows[1];
  h.n_frames = rows[2];
  h.n_tok_max = n_tok;
  h.n_frames_max = Fmax;
  h.colnorm = (float*)e->colnorm.p;
  h.scores = (float*)e->scores.p;
  h.LH = LH;
  h.B = batch;
  h.medfilt_width = medfilt_width;
  h.qk_scale = qk_scale;
  h.w_col = 1.f;
  h.w_row = 1.f;
  h.w_cov = 0.f;
  HIPCHK(launch_head_stats(h, e->stream));
  // this entry point is the reference's synchronous per-utterance call: the host learns here whether a token id was
  // outside the vocabulary (the row was embedded as token 0, never read out of bounds)
  HIPCHK(hipStreamSynchronize(e->stream));
  if (e->err_host[0] & 2) return fail(WCA_ERR_HIP, "LayerNorm statistics hand-off timed out inside a GEMM epilogue (a workgroup of a row panel never arrived)");
  if (e->err_host[0]) return fail(WCA_ERR_INVALID, "a token id is outside the model's vocabulary [0, %d) (tokenizer / checkpoint mismatch?)", D.n_vocab);
  return WCA_OK;
}

int wca_median_filter(wca_engine* e, const float* in_dev, float* out_dev, int64_t rows, int F, int width) {
  if (!e || !in_dev || !out_dev) return fail(WCA_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(e->device));
  if (int jr = join_phase2(e)) return jr;
  if (width < 1 || !(width & 1) || width > 33) return fail(WCA_ERR_INVALID, "filter width must be odd and <= 33");
  HIPCHK(launch_median_filter(in_dev, out_dev, rows, F, width, e->stream));
  return WCA_OK;
}

static int stats_on_weights(wca_engine* e, const float* attns_dev, int L, int H, int n, int F, float wc, float wr, float wv, int** rows_out,
                            int dtwN) {
  const int LH = L * H;
  if (L < 1 || H < 1 || n < 1 || n > MAX_TOK) return fail(WCA_ERR_INVALID, "bad shape L=%d H=%d n=%d", L, H, n);
  if (F < 1 || F > N_CTX) return fail(WCA_ERR_TOO_LONG, "F=%d outside [1,%d]", F, N_CTX);
  int32_t nt = n, nf = F, dn = dtwN;
  int rc = stage_meta(e, 1, nullptr, &nt, &nf, &dn, rows_out);
  if (rc) return rc;
  HIPCHK(e->colnorm.ensure(sizeof(float) * (size_t)LH * F));
  HIPCHK(e->scores.ensure(sizeof(float) * (size_t)LH));
  HeadStatsArgs h{};
  h.qk = attns_dev;
  h.qk_bs = 0;
  h.qk_hs = (long)n * F;
  h.qk_ld = F;
  h.weights = nullptr;
  h.n_tok = rows_out[1];
  h.n_frames = rows_out[2];
  h.n_tok_max = n;
  h.n_frames_max = F;
  h.colnorm = (float*)e->colnorm.p;
  h.scores = (float*)e->scores.p;
  h.LH = LH;
  h.B = 1;
  h.medfilt_width = 1;
  h.qk_scale = 1.f;
  h.w_col = wc;
  h.w_row = wr;
  h.w_cov = wv;
  h.input_is_weights = 1;
  HIPCHK(launch_head_stats(h, e->stream));
  return WCA_OK;
}

int wca_filter_attention(wca_engine* e, const float* attns_dev, int L, int H, int n, int F, int topk, float w_colnorm, float w_rownorm,
                         float w_coverage, float* scores_host, int32_t* sel_idx_host, float* sel_score_host) {
  if (!e || !attns_dev) return fail(WCA_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(e->device));
  if (int jr = join_phase2(e)) return jr;
  if (topk < 1) return fail(WCA_ERR_INVALID, "topk must be > 0");
  int* rows[4];
  int rc = stats_on_weights(e, attns_dev, L, H, n, F, w_colnorm, w_rownorm, w_coverage, rows, 0);
  if (rc) return rc;
  const int LH = L * H;
  const int keff = topk < LH ? topk : LH;
  HIPCHK(e->sel.ensure(sizeof(int) * (size_t)topk));
  HIPCHK(e->selsc.ensure(sizeof(float) * (size_t)topk));
  HIPCHK(launch_topk((const float*)e->scores.p, LH, 1, topk, (int*)e->sel.p, (float*)e->selsc.p, e->stream));
  if (scores_host) HIPCHK(hipMemcpyAsync(scores_host, e->scores.p, sizeof(float) * LH, hipMemcpyDeviceToHost, e->stream));
  if (sel_idx_host) HIPCHK(hipMemcpyAsync(sel_idx_host, e->sel.p, sizeof(int) * keff, hipMemcpyDeviceToHost, e->stream));
  if (sel_score_host) HIPCHK(hipMemcpyAsync(sel_score_host, e->selsc.p, sizeof(float) * keff, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return WCA_OK;
}

int wca_force_align(wca_engine* e, const float* ws_dev, int L, int H, int n, int F, const wca_align_opts* o, float* matrix_host,
                    int32_t* text_idx_host, int32_t* time_idx_host, int32_t* path_len_host, int32_t* sel_idx_host,
                    float* sel_score_host) {
  if (!e || !ws_dev || !o || !path_len_host) return fail(WCA_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(e->device));
  if (int jr = join_phase2(e)) return jr;
  if (o->aggregation != WCA_AGGR_MEAN && o->aggregation != WCA_AGGR_TOPK) return fail(WCA_ERR_INVALID, "aggregation %d", o->aggregation);
  if (o->aggregation == WCA_AGGR_TOPK && o->topk < 1) return fail(WCA_ERR_INVALID, "topk must be > 0 (timing.py:92)");
  const int N = n - o->sot_len - 1;
  if (o->sot_len < 0 || N < 1) return fail(WCA_ERR_INVALID, "n=%d leaves no rows after the [sot_len:-1] slice", n);
  int* rows[4];
  int rc = stats_on_weights(e, ws_dev, L, H, n, F, o->w_colnorm, o->w_rownorm, o->w_coverage, rows, N);
  if (rc) return rc;
  rc = run_select_aggregate_dtw(e, ws_dev, 1, L * H, n, F, rows[1], rows[2], rows[3], o, L);
  if (rc) return rc;
  const int cap = N + F + 2;
  std::vector<int> path(2 * (size_t)cap);
  int plen = 0;
  HIPCHK(hipMemcpyAsync(&plen, e->pathlen.p, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(path.data(), e->path.p, sizeof(int) * 2 * cap, hipMemcpyDeviceToHost, e->stream));
  if (matrix_host) HIPCHK(hipMemcpyAsync(matrix_host, e->matrix.p, sizeof(float) * (size_t)N * F, hipMemcpyDeviceToHost, e->stream));
  if (o->aggregation == WCA_AGGR_TOPK) {
    const int keff = o->topk < L * H ? o->topk : L * H;
    if (sel_idx_host) HIPCHK(hipMemcpyAsync(sel_idx_host, e->sel.p, sizeof(int) * keff, hipMemcpyDeviceToHost, e->stream));
    if (sel_score_host) HIPCHK(hipMemcpyAsync(sel_score_host, e->selsc.p, sizeof(float) * keff, hipMemcpyDeviceToHost, e->stream));
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  *path_len_host = plen;
  if (text_idx_host && time_idx_host)
    for (int i = 0; i < plen; ++i) {
      text_idx_host[i] = path[cap - plen + i];
      time_idx_host[i] = path[cap + cap - plen + i];
    }
  return WCA_OK;
}

static int dtw_dev_common(wca_engine* e, const float* matrix_dev, int P, int N, int M, bool want_jump) {
  if (N < 1 || N > 512 || M < 1 || M > 4096) return fail(WCA_ERR_INVALID, "DTW shape N=%d M=%d unsupported (N<=512, M<=4096)", N, M);
  const int wpr = (M + 15) / 16, cap = N + M + 2;
  HIPCHK(e->trace.ensure(sizeof(uint32_t) * (size_t)P * N * wpr));
  HIPCHK(e->path.ensure(sizeof(int) * (size_t)P * 2 * cap));
  HIPCHK(e->pathlen.ensure(sizeof(int) * (size_t)P));
  if (want_jump) HIPCHK(e->jump.ensure(sizeof(int) * (size_t)P * N));
  DtwArgs dg{};
  dg.matrix = matrix_dev;
  dg.m_bs = (long)N * M;
  dg.ld = M;
  dg.N_all = N;
  dg.M_all = M;
  dg.N_max = N;
  dg.M_max = M;
  dg.trace = (uint32_t*)e->trace.p;
  dg.path = (int*)e->path.p;
  dg.path_len = (int*)e->pathlen.p;
  dg.jump_frame = want_jump ? (int*)e->jump.p : nullptr;
  dg.jump_ld = N;
  dg.P = P;
  HIPCHK(launch_dtw(dg, e->stream));
  return WCA_OK;
}

int wca_dtw(wca_engine* e, const float* matrix_host, int N, int M, int32_t* text_idx_host, int32_t* time_idx_host, int32_t* path_len_host) {
  if (!e || !matrix_host || !text_idx_host || !time_idx_host || !path_len_host) return fail(WCA_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(e->device));
  if (int jr = join_phase2(e)) return jr;
  if (N < 1 || M < 1) return fail(WCA_ERR_INVALID, "empty DTW matrix");
  HIPCHK(e->tmp0.ensure(sizeof(float) * (size_t)N * M));
  HIPCHK(hipMemcpyAsync(e->tmp0.p, matrix_host, sizeof(float) * (size_t)N * M, hipMemcpyHostToDevice, e->stream));
  int rc = dtw_dev_common(e, (const float*)e->tmp0.p, 1, N, M, false);
  if (rc) return rc;
  const int cap = N + M + 2;
  std::vector<int> path(2 * (size_t)cap);
  int plen = 0;
  HIPCHK(hipMemcpyAsync(&plen, e->pathlen.p, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(path.data(), e->path.p, sizeof(int) * 2 * cap, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  *path_len_host = plen;
  for (int i = 0; i < plen; ++i) {
    text_idx_host[i] = path[cap - plen + i];
    time_idx_host[i] = path[cap + cap - plen + i];
  }
  return WCA_OK;
}

int wca_dtw_batch_dev(wca_engine* e, const float* matrix_dev, int P, int N, int M, int32_t* jump_frame_host) {
  if (!e || !matrix_dev || !jump_frame_host) return fail(WCA_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(e->device));
  if (int jr = join_phase2(e)) return jr;
  if (P < 1) return fail(WCA_ERR_INVALID, "P < 1");
  int rc = dtw_dev_common(e, matrix_dev, P, N, M, true);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(jump_frame_host, e->jump.p, sizeof(int) * (size_t)P * N, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return WCA_OK;
}

int wca_probe_heads(wca_engine* e, const float* ws_dev, int L, int H, int n, int F, int sot_len, float* scores_host,
                    int32_t* jump_frame_host) {
  if (!e || !ws_dev || !jump_frame_host) return fail(WCA_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(e->device));
  if (int jr = join_phase2(e)) return jr;
  const int LH = L * H, N = n - sot_len - 1;
  if (sot_len < 0 || N < 1) return fail(WCA_ERR_INVALID, "n=%d leaves no rows after the [sot_len:-1] slice", n);
  int* rows[4];
  int rc = stats_on_weights(e, ws_dev, L, H, n, F, 1.f, 1.f, 0.f, rows, N);
  if (rc) return rc;
  // every head becomes its own "utterance": matrix_h = ws_h / ||ws_h||_col  (timing.py:84-89 with L = H = 1)
  HIPCHK(e->tmp1.ensure(sizeof(int) * 2 * (size_t)LH));
  std::vector<int> meta(2 * (size_t)LH);
  for (int i = 0; i < LH; ++i) {
    meta[i] = n;
    meta[LH + i] = F;
  }
  HIPCHK(hipMemcpyAsync(e->tmp1.p, meta.data(), sizeof(int) * 2 * LH, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));  // meta is a stack-lifetime host buffer
  HIPCHK(e->matrix.ensure(sizeof(float) * (size_t)LH * n * F));
  AggregateArgs g{};
  g.weights = ws_dev;
  g.w_bs = (long)n * F;
  g.n_tok_max = n;
  g.n_frames_max = F;
  g.colnorm = (const float*)e->colnorm.p;
  g.sel_idx = nullptr;
  g.head_lo = 0;
  g.LH = 1;
  g.B = LH;
  g.n_tok = (const int*)e->tmp1.p;
  g.n_frames = (const int*)e->tmp1.p + LH;
  g.row_lo = sot_len;
  g.row_hi_trim = 1;
  g.matrix = (float*)e->matrix.p;
  HIPCHK(launch_aggregate(g, e->stream));
  const int wpr = (F + 15) / 16, cap = N + F + 2;
  HIPCHK(e->trace.ensure(sizeof(uint32_t) * (size_t)LH * N * wpr));
  HIPCHK(e->path.ensure(sizeof(int) * (size_t)LH * 2 * cap));
  HIPCHK(e->pathlen.ensure(sizeof(int) * (size_t)LH));
  HIPCHK(e->jump.ensure(sizeof(int) * (size_t)LH * N));
  DtwArgs dg{};
  dg.matrix = (const float*)e->matrix.p;
  dg.m_bs = (long)n * F;
  dg.ld = F;
  dg.N_all = N;
  dg.M_all = F;
  dg.N_max = N;
  dg.M_max = F;
  dg.trace = (uint32_t*)e->trace.p;
  dg.path = (int*)e->path.p;
  dg.path_len = (int*)e->pathlen.p;
  dg.jump_frame = (int*)e->jump.p;
  dg.jump_ld = N;
  dg.P = LH;
  HIPCHK(launch_dtw(dg, e->stream));
  HIPCHK(hipMemcpyAsync(jump_frame_host, e->jump.p, sizeof(int) * (size_t)LH * N, hipMemcpyDeviceToHost, e->stream));
  if (scores_host) HIPCHK(hipMemcpyAsync(scores_host, e->scores.p, sizeof(float) * LH, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e->probe_jump.ensure(sizeof(int) * (size_t)LH * N));
  HIPCHK(hipMemcpyAsync(e->probe_jump.p, e->jump.p, sizeof(int) * (size_t)LH * N, hipMemcpyDeviceToDevice, e->stream));
  e->probe_LH = LH;
  e->probe_N = N;
  HIPCHK(hipStreamSynchronize(e->stream));
  return WCA_OK;
}

int wca_probe_strict_tp(wca_engine* e, int n_heads, const int32_t* word_end_row_host, int n_hyp, const double* ref_times_host, int n_ref,
                        const uint8_t* same_word_host, double tolerance, int32_t* tp_host) {
  if (!e || !tp_host || (n_hyp > 0 && !word_end_row_host) || (n_ref > 0 && !ref_times_host) || (n_hyp > 0 && n_ref > 0 && !same_word_host))
    return fail(WCA_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(e->device));
  if (e->probe_LH <= 0) return fail(WCA_ERR_STATE, "wca_probe_strict_tp needs a preceding wca_probe_heads");
  if (n_heads != e->probe_LH) return fail(WCA_ERR_INVALID, "n_heads %d != the %d heads of the preceding wca_probe_heads", n_heads, e->probe_LH);
  if (n_hyp < 0 || n_ref < 0 || n_ref > 512) return fail(WCA_ERR_INVALID, "n_hyp=%d n_ref=%d outside [0, 512]", n_hyp, n_ref);
  for (int i = 0; i < n_hyp; ++i)
    if (word_end_row_host[i] < 0 || word_end_row_host[i] >= e->probe_N)
      return fail(WCA_ERR_INVALID, "word end row %d = %d outside the %d aligned token rows", i, word_end_row_host[i], e->probe_N);
  const int LH = e->probe_LH;
  const size_t b_wb = align_up(sizeof(int) * (size_t)std::max(n_hyp, 1), 256), b_y = align_up(sizeof(double) * (size_t)std::max(n_ref, 1), 256),
               b_eq = align_up((size_t)std::max(n_hyp * n_ref, 1), 256), b_tp = sizeof(int) * (size_t)LH;
  HIPCHK(e->tmp0.ensure(b_wb + b_y + b_eq + b_tp));
  char* base = (char*)e->tmp0.p;
  if (n_hyp) HIPCHK(hipMemcpyAsync(base, word_end_row_host, sizeof(int) * (size_t)n_hyp, hipMemcpyHostToDevice, e->stream));
  if (n_ref) HIPCHK(hipMemcpyAsync(base + b_wb, ref_times_host, sizeof(double) * (size_t)n_ref, hipMemcpyHostToDevice, e->stream));
  if (n_hyp && n_ref) HIPCHK(hipMemcpyAsync(base + b_wb + b_y, same_word_host, (size_t)n_hyp * n_ref, hipMemcpyHostToDevice, e->stream));
  HIPCHK(launch_probe_strict((const int*)e->probe_jump.p, e->probe_N, LH, (const int*)base, n_hyp, (const double*)(base + b_wb), n_ref,
                             (const unsigned char*)(base + b_wb + b_y), tolerance, (int*)(base + b_wb + b_y + b_eq), e->stream));
  HIPCHK(hipMemcpyAsync(tp_host, base + b_wb + b_y + b_eq, b_tp, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return WCA_OK;
}

int wca_attention_weights(wca_engine* e, const float* qk_dev, int L, int H, int n, int ld, int max_frames, int medfilt_width,
                          float qk_scale, float* weights_out_dev) {
  if (!e || !qk_dev || !weights_out_dev) return fail(WCA_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(e->device));
  if (int jr = join_phase2(e)) return jr;
  const int LH = L * H;
  if (L < 1 || H < 1 || n < 1) return fail(WCA_ERR_INVALID, "bad shape L=%d H=%d n=%d", L, H, n);
  if (n > MAX_TOK) return fail(WCA_ERR_TOO_LONG, "n=%d > %d", n, MAX_TOK);
  if (max_frames < 1 || ld < max_frames) return fail(WCA_ERR_INVALID, "max_frames=%d must be in [1, ld=%d]", max_frames, ld);
  if (max_frames > N_CTX) return fail(WCA_ERR_TOO_LONG, "max_frames=%d > %d", max_frames, N_CTX);
  if (medfilt_width < 1 || !(medfilt_width & 1) || medfilt_width > 33) return fail(WCA_ERR_INVALID, "medfilt_width must be odd and <= 33");
  int32_t nt = n, nf = max_frames;
  int* rows[4];
  int rc = stage_meta(e, 1, nullptr, &nt, &nf, nullptr, rows);
  if (rc) return rc;
  HIPCHK(e->colnorm.ensure(sizeof(float) * (size_t)LH * max_frames));
  HIPCHK(e->scores.ensure(sizeof(float) * (size_t)LH));
  HeadStatsArgs h{};
  h.qk = qk_dev;
  h.qk_bs = 0;
  h.qk_hs = (long)n * ld;
  h.qk_ld = ld;
  h.weights = weights_out_dev;
  h.w_bs = 0;
  h.n_tok = rows[1];
  h.n_frames = rows[2];
  h.n_tok_max = n;
  h.n_frames_max = max_frames;
  h.colnorm = (float*)e->colnorm.p;
  h.scores = (float*)e->scores.p;
  h.LH = LH;
  h.B = 1;
  h.medfilt_width = medfilt_width;
  h.qk_scale = qk_scale;
  h.w_col = 1.f;
  h.w_row = 1.f;
  h.w_cov = 0.f;
  HIPCHK(launch_head_stats(h, e->stream));
  return WCA_OK;
}

int wca_default_find_alignment(wca_engine* e, const float* ws_dev, int L, int H, int n, int F, const int32_t* heads_host, int n_heads,
                                int sot_len, float* weights_norm_out_dev, float* matrix_host, int32_t* text_idx_host,
                                int32_t* time_idx_host, int32_t* path_len_host) {
  if (!e || !ws_dev || !heads_host || !path_len_host) return fail(WCA_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(e->device));
  if (int jr = join_phase2(e)) return jr;
  const int LH = L * H, N = n - sot_len - 1;
  if (n_heads < 1) return fail(WCA_ERR_INVALID, "empty alignment head list");
  if (L < 1 || H < 1 || n < 1 || n > MAX_TOK) return fail(WCA_ERR_INVALID, "bad shape L=%d H=%d n=%d", L, H, n);
  if (F < 1 || F > N_CTX) return fail(WCA_ERR_TOO_LONG, "F=%d outside [1,%d]", F, N_CTX);
  if (sot_len < 0 || N < 1) return fail(WCA_ERR_INVALID, "n=%d leaves no rows after the [sot_len:-1] slice", n);
  for (int i = 0; i < n_heads; ++i)
    if (heads_host[i] < 0 || heads_host[i] >= LH) return fail(WCA_ERR_INVALID, "alignment head %d out of range", heads_host[i]);
  // (w - mean) / std per head and frame over the token axis (two passes, population std), kept for the caller when it
  // asks for it (the reference returns these normalised weights, timing.py:186), then the mean over the heads
  const size_t norm_elems = (size_t)n_heads * n * F;
  HIPCHK(e->tmp1.ensure(sizeof(int) * (size_t)n_heads + (weights_norm_out_dev ? 0 : sizeof(float) * norm_elems) + 256));
  int* sel_dev = reinterpret_cast<int*>(e->tmp1.p);
  float* norm = weights_norm_out_dev ? weights_norm_out_dev
                                     : reinterpret_cast<float*>(reinterpret_cast<char*>(e->tmp1.p) + align_up(sizeof(int) * (size_t)n_heads, 256));
  HIPCHK(hipMemcpyAsync(sel_dev, heads_host, sizeof(int) * n_heads, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));  // heads_host is caller-owned pageable memory
  HIPCHK(launch_stdmean_normalize(ws_dev, sel_dev, n_heads, n, F, norm, e->stream));
  HIPCHK(e->matrix.ensure(sizeof(float) * (size_t)n * F));
  HIPCHK(launch_mean_heads(norm, n_heads, n, F, sot_len, 1, (float*)e->matrix.p, e->stream));
  int rc = dtw_dev_common(e, (const float*)e->matrix.p, 1, N, F, false);
  if (rc) return rc;
  const int cap = N + F + 2;
  std::vector<int> path(2 * (size_t)cap);
  int plen = 0;
  HIPCHK(hipMemcpyAsync(&plen, e->pathlen.p, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(path.data(), e->path.p, sizeof(int) * 2 * cap, hipMemcpyDeviceToHost, e->stream));
  if (matrix_host) HIPCHK(hipMemcpyAsync(matrix_host, e->matrix.p, sizeof(float) * (size_t)N * F, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  *path_len_host = plen;
  if (text_idx_host && time_idx_host)
    for (int i = 0; i < plen; ++i) {
      text_idx_host[i] = path[cap - plen + i];
      time_idx_host[i] = path[cap + cap - plen + i];
    }
  return WCA_OK;
}

int wca_align_batch_enqueue(wca_engine* e, const float* pcm_dev, int64_t pcm_stride, const int32_t* n_samples_host,
                            const int64_t* tokens_dev, int n_tok_max, const int32_t* n_tok_host, const int32_t* max_frames_host,
                            int batch, const wca_align_opts* o) {
  return wca_align_batch_enqueue_ex(e, pcm_dev, pcm_stride, n_samples_host, tokens_dev, n_tok_max, n_tok_host, max_frames_host, batch, o, 0);
}

int wca_align_batch_enqueue_ex(wca_engine* e, const float* pcm_dev, int64_t pcm_stride, const int32_t* n_samples_host,
                               const int64_t* tokens_dev, int n_tok_max, const int32_t* n_tok_host, const int32_t* max_frames_host,
                               int batch, const wca_align_opts* o, int32_t vocab_end) {
  int rc = check_ready(e);
  if (rc) return rc;
  if (!tokens_dev || !n_tok_host || !max_frames_host || !o) return fail(WCA_ERR_INVALID, "null argument");
  if (vocab_end < 0 || vocab_end > e->dims.n_vocab) return fail(WCA_ERR_INVALID, "vocab_end %d outside (0, %d] (0 = no token log-probs)", vocab_end, e->dims.n_vocab);
  const bool want_lp = vocab_end > 0;
  const bool reuse_enc = (pcm_dev == nullptr);  // consume the oldest encoded state (wca_encode_batch / wca_greedy_decode)
  if (reuse_enc && (e->enc_q.empty() || e->enc_q.front().batch != batch))
    return fail(WCA_ERR_STATE, "pcm_dev == NULL re-uses the oldest state left by wca_encode_batch / wca_greedy_decode for the same batch; there is none");
  if (!reuse_enc && !n_samples_host) return fail(WCA_ERR_INVALID, "null argument");
  if (!reuse_enc && !e->enc_q.empty()) {
    // a stand-alone decode may have left a decoded state behind; an undecoded one is still wanted by its owner
    for (auto& st : e->enc_q)
      if (!st.decoded) return fail(WCA_ERR_STATE, "an encoded batch is waiting for wca_greedy_decode / wca_align_batch_enqueue(pcm_dev = NULL)");
    for (auto& st : e->enc_q) e->slot_busy[st.slot] = false;
    e->enc_q.clear();
  }
  if (e->enq_count - e->fetch_count >= 2) return fail(WCA_ERR_STATE, "two batches already in flight: call wca_align_batch_fetch first");
  if (batch < 1 || batch > e->max_batch) return fail(WCA_ERR_INVALID, "batch %d outside [1,%d]", batch, e->max_batch);
  if (o->aggregation != WCA_AGGR_MEAN && o->aggregation != WCA_AGGR_TOPK) return fail(WCA_ERR_INVALID, "aggregation %d", o->aggregation);
  if (o->aggregation == WCA_AGGR_TOPK && o->topk < 1) return fail(WCA_ERR_INVALID, "topk must be > 0 (timing.py:92)");
  if (o->medfilt_width < 1 || !(o->medfilt_width & 1) || o->medfilt_width > 33) return fail(WCA_ERR_INVALID, "medfilt_width must be odd and <= 33");
  int Fmax = 0;
  rc = validate_lengths(batch, n_tok_max, n_tok_host, max_frames_host, &Fmax);
  if (rc) return rc;
  if (!reuse_enc && (rc = check_pcm_lengths(n_samples_host, batch, pcm_stride))) return rc;
  const wca_model_dims& D = e->dims;
  const int LH = D.n_text_layer * D.n_text_head;
  const int Fpad = (Fmax + 3) & ~3;
  std::vector<int32_t> dn(batch);
  for (int b = 0; b < batch; ++b) {
    dn[b] = n_tok_host[b] - o->sot_len - 1;
    if (dn[b] < 0) dn[b] = 0;
  }
  int* rows[4];
  // (re-use: the metadata is only read by phase 2, so it travels on that stream -- `stream` may already hold the next
  // batch's phase 1, and an event recorded behind it would serialise this batch's phase 2 after it)
  hipStream_t s2 = e->overlap ? e->stream2 : e->stream;  // the stream phase 2 runs on
  rc = stage_meta(e, batch, reuse_enc ? nullptr : n_samples_host, n_tok_host, max_frames_host, dn.data(), rows,
                  reuse_enc ? s2 : nullptr);
  if (rc) return rc;
  // token log-probs: the rows that predict text token i of utterance b (row sot_len + i, i < n_text_b = n_tok - sot_len - 2) are compacted;
  // utterance b's first compact row (the prefix sum of n_text) travels through the metadata ring, the row map is built from it on the device
  int* lp_rows[4] = {nullptr, nullptr, nullptr, nullptr};
  int lp_R = 0, lp_nmax = 0;
  if (want_lp) {
    std::vector<int32_t> off(batch);
    for (int b = 0; b < batch; ++b) {
      const int nt = std::max(0, n_tok_host[b] - o->sot_len - 2);
      off[b] = lp_R;
      lp_R += nt;
      lp_nmax = std::max(lp_nmax, nt);
    }
    if ((rc = stage_meta(e, batch, off.data(), nullptr, nullptr, nullptr, lp_rows, reuse_enc ? s2 : nullptr))) return rc;
  }
  // ---- phase 1 on `stream`: log-mel, encoder, cross-K/V of all decoder layers into a free K/V slot (a slot is busy
  // from its encode until the alignment that read it has been fetched; at most 2 alignments are in flight), or the
  // slot of the encoded state this call consumes.
  int bs;
  if (reuse_enc) {
    bs = e->enc_q.front().slot;
    e->enc_q.pop_front();
    record(e, 0);
    record(e, 1);
    record(e, 2);
    record(e, 3);
  } else {
    bs = take_kv_slot(e);
    if (bs < 0) return fail(WCA_ERR_STATE, "both cross-K/V slots hold live batches: fetch or consume one first");
    e->slot_busy[bs] = true;
    // (without token log-probs this path never reads the last layer's cross-attention output: its value projection is skipped)
    rc = run_phase1(e, nullptr, pcm_dev, pcm_stride, rows[0], batch, bs, /*skip_last_v=*/!want_lp);
    if (rc) {
      e->slot_busy[bs] = false;
      return rc;
    }
  }
  half_t* kvbuf = bs ? e->kv_alt : e->kv;
  // ---- phase 2 on `stream2`: decoder with capture, head statistics, top-k, aggregation, DTW, D2H. These are
  // latency-bound kernels with few workgroups; on their own stream they overlap the NEXT batch's phase 1.
  HIPCHK(hipStreamWaitEvent(s2, e->ev_kv[bs], 0));
  HIPCHK(hipMemsetAsync(e->err_dev, 0, sizeof(int), s2));
  HIPCHK(e->cap.ensure(sizeof(float) * (size_t)batch * LH * n_tok_max * Fpad));
  rc = run_decoder(e, tokens_dev, batch, n_tok_max, (float*)e->cap.p, Fpad, Fmax, nullptr, s2, kvbuf, /*finish_last=*/want_lp);
  if (rc) return rc;
  record(e, 4, s2);
  // the softmaxed maps are NOT materialised on this path (53 MB per utterance): head_stats keeps per-row
  // (max, sum) and the aggregation re-derives the values of the few selected heads from the captured logits
  HIPCHK(e->wws.ensure(sizeof(float) * (size_t)batch * LH * n_tok_max * 2));
  HIPCHK(e->colnorm.ensure(sizeof(float) * (size_t)batch * LH * Fmax));
  HIPCHK(e->scores.ensure(sizeof(float) * (size_t)batch * LH));
  HeadStatsArgs h{};
  h.qk = (const float*)e->cap.p;
  h.qk_bs = (long)LH * n_tok_max * Fpad;
  h.qk_hs = (long)n_tok_max * Fpad;
  h.qk_ld = Fpad;
  h.weights = nullptr;
  h.rowstats = (float*)e->wws.p;
  h.n_tok = rows[1];
  h.n_frames = rows[2];
  h.n_tok_max = n_tok_max;
  h.n_frames_max = Fmax;
  h.colnorm = (float*)e->colnorm.p;
  h.scores = (float*)e->scores.p;
  h.LH = LH;
  h.B = batch;
  h.medfilt_width = o->medfilt_width;
  h.qk_scale = o->qk_scale;
  h.w_col = o->w_colnorm;
  h.w_row = o->w_rownorm;
  h.w_cov = o->w_coverage;
  HIPCHK(launch_head_stats(h, s2));
  record(e, 5, s2);
  Remat rm;
  rm.qk = h.qk;
  rm.qk_bs = h.qk_bs;
  rm.qk_hs = h.qk_hs;
  rm.qk_ld = h.qk_ld;
  rm.rowstats = h.rowstats;
  rc = run_select_aggregate_dtw(e, nullptr, batch, LH, n_tok_max, Fmax, rows[1], rows[2], rows[3], o, D.n_text_layer, &rm, s2);
  if (rc) return rc;
  if (want_lp) {
    HIPCHK(e->lp_out.ensure(sizeof(float) * (size_t)batch * n_tok_max));
    rc = run_token_logprobs(e, s2, tokens_dev, batch, n_tok_max, o->sot_len, vocab_end, rows[1], lp_rows[0], lp_R, lp_nmax, (float*)e->lp_out.p);
    if (rc) return rc;
  }
  record(e, 7, s2);
  // results -> pinned staging (ring of 2 so the host can post-process batch i while batch i+1 runs): jump frames [batch][n_tok_max],
  // top-k heads [batch][max(k, 1)], the two flag words, then (token log-probs only) the log-probs [batch][n_tok_max] as f32
  const int k = o->aggregation == WCA_AGGR_TOPK ? o->topk : 0;
  const int rs = (int)(e->enq_count & 1);
  const size_t lp_at = (size_t)batch * n_tok_max + (size_t)batch * (k > 0 ? k : 1) + 2;
  rc = ensure_res_host(e, rs, lp_at + (want_lp ? (size_t)batch * n_tok_max : 0));
  if (rc) return rc;
  if (want_lp)
    HIPCHK(hipMemcpyAsync(e->res_host[rs] + lp_at, e->lp_out.p, sizeof(float) * (size_t)batch * n_tok_max, hipMemcpyDeviceToHost, s2));
  // the flags of this batch travel with its results (last two ints of the staging slot): phase 2's word, and the word phase 1
  // raised for this batch's cross-K/V slot (complete: s2 waited for ev_kv[bs], recorded behind that encoder)
  HIPCHK(hipMemcpyAsync(e->res_host[rs] + (size_t)batch * n_tok_max + (size_t)batch * (k > 0 ? k : 1), e->err_dev, sizeof(int),
                        hipMemcpyDeviceToHost, s2));
  HIPCHK(hipMemcpyAsync(e->res_host[rs] + (size_t)batch * n_tok_max + (size_t)batch * (k > 0 ? k : 1) + 1, e->err_dev + 1 + bs, sizeof(int),
                        hipMemcpyDeviceToHost, s2));
  if (n_tok_max - o->sot_len - 1 >= 1)
    HIPCHK(hipMemcpyAsync(e->res_host[rs], e->jump.p, sizeof(int) * (size_t)batch * n_tok_max, hipMemcpyDeviceToHost, s2));
  if (k > 0)
    HIPCHK(hipMemcpyAsync(e->res_host[rs] + (size_t)batch * n_tok_max, e->sel.p, sizeof(int) * (size_t)batch * k, hipMemcpyDeviceToHost, s2));
  record(e, 8, s2);
  HIPCHK(hipEventRecord(e->res_ev[rs], s2));
  e->res_batch[rs] = batch;
  e->res_ntok[rs] = n_tok_max;
  e->res_topk[rs] = k;
  e->res_lp[rs] = want_lp;
  e->res_kvslot[rs] = bs;
  e->last_batch = batch;
  e->enq_count++;
  return WCA_OK;
}

int wca_encode_batch(wca_engine* e, const float* mel_dev, const float* pcm_dev, int64_t pcm_stride, const int32_t* n_samples_host, int batch) {
  int rc = check_ready(e);
  if (rc) return rc;
  if ((mel_dev == nullptr) == (pcm_dev == nullptr)) return fail(WCA_ERR_INVALID, "pass exactly one of mel_dev / pcm_dev");
  if (pcm_dev && !n_samples_host) return fail(WCA_ERR_INVALID, "null argument");
  if (batch < 1 || batch > e->max_batch) return fail(WCA_ERR_INVALID, "batch %d outside [1,%d]", batch, e->max_batch);
  if (pcm_dev && (rc = check_pcm_lengths(n_samples_host, batch, pcm_stride))) return rc;
  const int slot = take_kv_slot(e);
  if (slot < 0) return fail(WCA_ERR_STATE, "both cross-K/V slots hold live batches: fetch or consume one first");
  int* rows[4] = {nullptr, nullptr, nullptr, nullptr};
  if (pcm_dev) {
    rc = stage_meta(e, batch, n_samples_host, nullptr, nullptr, nullptr, rows);
    if (rc) return rc;
  }
  e->slot_busy[slot] = true;
  rc = run_phase1(e, mel_dev, pcm_dev, pcm_stride, rows[0], batch, slot);
  if (rc) {
    e->slot_busy[slot] = false;
    return rc;
  }
  e->enc_q.push_back({slot, batch, false});
  return WCA_OK;
}

int wca_align_batch_fetch(wca_engine* e, int batch, int n_tok_max, int topk, int32_t* jump_frame_host, int32_t* sel_idx_host) {
  return wca_align_batch_fetch_ex(e, batch, n_tok_max, topk, jump_frame_host, sel_idx_host, nullptr);
}

int wca_align_batch_fetch_ex(wca_engine* e, int batch, int n_tok_max, int topk, int32_t* jump_frame_host, int32_t* sel_idx_host,
                             float* token_logprob_host) {
  if (!e) return fail(WCA_ERR_INVALID, "null engine");
  HIPCHK(hipSetDevice(e->device));
  if (e->fetch_count >= e->enq_count) return fail(WCA_ERR_STATE, "nothing to fetch");
  const int rs = (int)(e->fetch_count & 1);  // oldest un-fetched batch
  if (batch != e->res_batch[rs] || n_tok_max != e->res_ntok[rs]) return fail(WCA_ERR_STATE, "fetch does not match the oldest pending enqueue");
  if (sel_idx_host && e->res_topk[rs] > 0 && topk != e->res_topk[rs]) return fail(WCA_ERR_STATE, "topk does not match the pending enqueue");
  // (checked before anything is consumed: the caller can fetch the same batch again without them)
  if (token_logprob_host && !e->res_lp[rs]) return fail(WCA_ERR_STATE, "token log-probs requested, but the pending batch was enqueued without them (vocab_end = 0)");
  HIPCHK(hipEventSynchronize(e->res_ev[rs]));
  if (jump_frame_host) memcpy(jump_frame_host, e->res_host[rs], sizeof(int) * (size_t)batch * n_tok_max);
  if (sel_idx_host && e->res_topk[rs] > 0)
    memcpy(sel_idx_host, e->res_host[rs] + (size_t)batch * n_tok_max, sizeof(int) * (size_t)batch * topk);
  if (e->res_kvslot[rs] >= 0) e->slot_busy[e->res_kvslot[rs]] = false;
  e->res_kvslot[rs] = -1;
  e->fetch_count++;
  const int kk = e->res_topk[rs];
  const size_t fo = (size_t)batch * n_tok_max + (size_t)batch * (kk > 0 ? kk : 1);
  if (token_logprob_host) memcpy(token_logprob_host, e->res_host[rs] + fo + 2, sizeof(float) * (size_t)batch * n_tok_max);
  const int flag = e->res_host[rs][fo] | (e->res_host[rs][fo + 1] & 2);
  if (flag & 2) return fail(WCA_ERR_HIP, "LayerNorm statistics hand-off timed out inside a GEMM epilogue (a workgroup of a row panel never arrived)");
  if (flag == ERR_TARGET_VOCAB)
    return fail(WCA_ERR_INVALID, "a teacher token is outside the scored vocabulary [0, vocab_end) (its log-prob is NaN)");
  if (flag)
    return fail(WCA_ERR_INVALID, "a token id is outside the model's vocabulary [0, %d) (tokenizer / checkpoint mismatch?)", e->dims.n_vocab);
  return WCA_OK;
}

int wca_align_batch(wca_engine* e, const float* pcm_dev, int64_t pcm_stride, const int32_t* n_samples_host, const int64_t* tokens_dev,
                    int n_tok_max, const int32_t* n_tok_host, const int32_t* max_frames_host, int batch, const wca_align_opts* o,
                    int32_t* jump_frame_host, int32_t* sel_idx_host) {
  int rc = wca_align_batch_enqueue(e, pcm_dev, pcm_stride, n_samples_host, tokens_dev, n_tok_max, n_tok_host, max_frames_host, batch, o);
  if (rc) return rc;
  return wca_align_batch_fetch(e, batch, n_tok_max, o->aggregation == WCA_AGGR_TOPK ? o->topk : 0, jump_frame_host, sel_idx_host);
}

int wca_token_logprobs(wca_engine* e, const float* logits_dev, int rows, int ld, int vocab_end, const int64_t* targets_dev, float* out_dev) {
  if (!e) return fail(WCA_ERR_INVALID, "null engine");
  if (!logits_dev || !targets_dev || !out_dev) return fail(WCA_ERR_INVALID, "null argument");
  if (vocab_end < 1 || vocab_end > e->dims.n_vocab) return fail(WCA_ERR_INVALID, "vocab_end %d outside (0, %d]", vocab_end, e->dims.n_vocab);
  if (rows < 0 || ld < vocab_end) return fail(WCA_ERR_INVALID, "rows %d / ld %d (need rows >= 0, ld >= vocab_end = %d)", rows, ld, vocab_end);
  HIPCHK(hipSetDevice(e->device));
  if (int rc = join_phase2(e)) return rc;
  if (rows == 0) return WCA_OK;
  int* err = e->err_dev + 3;   // (words 0-2 belong to the aligned batches)
  HIPCHK(hipMemsetAsync(err, 0, sizeof(int), e->stream));
  HIPCHK(launch_token_logprob(logits_dev, ld, vocab_end, rows, targets_dev, nullptr, 0, out_dev, err, ERR_TARGET_VOCAB, e->stream));
  HIPCHK(hipMemcpyAsync(e->err_host + 3, err, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (e->err_host[3]) return fail(WCA_ERR_INVALID, "a target token is outside [0, vocab_end = %d) (its log-prob is NaN)", vocab_end);
  return WCA_OK;
}

}  // extern "C"
