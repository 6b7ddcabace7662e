// libwca.so engine: weight residency, activation arena, forward orchestration and the C ABI of
// include/wca.h.  One engine = one MI355X = one host thread; two HIP streams (phase 1: log-mel, encoder, cross-K/V;
// phase 2: decoder / greedy decode loop, post-processing, DTW, D2H) with two cross-K/V slots between them.
//
// Data layout in HBM (per engine, B = max_batch, d = n_state, L = decoder layers):
//   weights   f16 [N][K] row-major (torch Linear layout), q/k/v fused to [3d][d]; the cross-attention
//             key/value projections of ALL decoder layers fused to one [L*2*d][d] matrix so that the
//             encoder output is projected by a single large MFMA GEMM; conv kernels re-ordered to
//             [d][tap*C + c] so the conv stem is a GEMM over overlapping time-major windows.
//   residual  f32 [B*1500][d] (encoder), f32 [B*n][d] (decoder); GEMM operands are f16.
//   capture   f32 [B][L*H][n_max][Fpad]  pre-softmax cross-attention logits (timing.py:50-55)
//   weights_ws f32 [B][L*H][n_max][Fmax] filtered+softmaxed maps (timing.py:63-66; step-by-step API only)
//   decode    f16 self-attention K/V cache [L][2][B][T_max][d], int32 token rows, fp32 logits [B][n_vocab]
//
// This file: engine lifecycle, settings, profiling, the activation arena and the small helpers every entry point uses. The rest of the
// engine is in engine_weights / engine_forward / engine_align / engine_audio / engine_decode / engine_comm / engine_test.hip (engine_internal.h).
#include <cstdarg>

#include "engine_internal.h"

using namespace wca;

namespace {
thread_local std::string g_err;
}

namespace wca {

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

static size_t layout_arena(wca_engine* e, char* base) {
  const wca_model_dims& D = e->dims;
  const size_t B = e->max_batch, d = D.n_audio_state, dt = D.n_text_state, L = D.n_text_layer;
  const size_t om = e->split ? 2 : 1;  // f16 operand buffers hold [hi | lo] rows in split mode
  char* cur = base;
  e->mel_scratch = carve<float>(cur, B * D.n_mels * N_FRAMES);
  e->gmax = carve<unsigned>(cur, B);
  e->mel_f32 = carve<float>(cur, B * D.n_mels * N_FRAMES);
  e->mel_tm = carve<half_t>(cur, om * B * (N_FRAMES + 2) * D.n_mels + 4096);
  e->h1pad = carve<half_t>(cur, om * B * (N_FRAMES + 2) * d + 4096);
  e->x = carve<float>(cur, B * N_CTX * d);
  e->xn = carve<half_t>(cur, om * B * N_CTX * d);
  e->qkv = carve<half_t>(cur, om * B * N_CTX * 3 * d);
  e->att = carve<half_t>(cur, om * B * N_CTX * d);
  e->hid = carve<half_t>(cur, om * B * N_CTX * 4 * d);
  e->kv = carve<half_t>(cur, om * B * N_CTX * L * 2 * dt);
  e->kv_alt = carve<half_t>(cur, om * B * N_CTX * L * 2 * dt);
  e->xd = carve<float>(cur, B * MAX_TOK * dt);
  e->xdn = carve<half_t>(cur, om * B * MAX_TOK * dt);
  e->qkv_d = carve<half_t>(cur, om * B * MAX_TOK * 3 * dt);
  e->att_d = carve<half_t>(cur, om * B * MAX_TOK * dt);
  e->q_d = carve<half_t>(cur, om * B * MAX_TOK * dt);
  e->hid_d = carve<half_t>(cur, om * B * MAX_TOK * 4 * dt);
  e->meta_dev = carve<int>(cur, (size_t)META_SLOTS * 4 * B);
  e->err_dev = carve<int>(cur, 64);
  {
    const size_t mpad = align_up(B * N_CTX, 256);
    e->ln_stats = carve<unsigned long long>(cur, (d / 256 + 1) * mpad);
    e->ln_cnt = carve<unsigned>(cur, mpad / 256 + 16, 256);
  }
  {
    // few-row GEMM, split-K workspace (dec_sk_capacity, gemm_plan.cpp)
    const DecSkCapacity sk = dec_sk_capacity((int)dt);
    e->sk_tiles = sk.tiles;
    e->sk_floats = sk.floats;
    e->sk_part = carve<float>(cur, e->sk_floats);
    e->sk_cnt = carve<unsigned>(cur, e->sk_tiles + 16, 256);
    // 128 x 128 tile GEMM with at most n_cu / 2 = 128 tiles, 4 K slices of f32 partials
    e->sk_big_bytes = (size_t)4 * 128 * 128 * 128 * sizeof(float);
    for (float*& p : e->sk_big) p = carve<float>(cur, e->sk_big_bytes / sizeof(float));
  }
  return (size_t)(cur - base) + 4096;
}

void record(wca_engine* e, int i, hipStream_t s) {
  if (e->profiling && e->ev_valid) (void)hipEventRecord(e->ev[i], s ? s : e->stream);
}

// Entry points other than wca_align_batch* share the phase-2 scratch (capture, norms, DTW buffers) with a batch
// that may still be running on stream2: order them behind it.
int join_phase2(wca_engine* e) {
  if (e->enq_count > e->fetch_count) HIPCHK(hipStreamWaitEvent(e->stream, e->res_ev[(e->enq_count - 1) & 1], 0));
  return WCA_OK;
}

int enter(wca_engine* e) {
  if (!e) return fail(WCA_ERR_INVALID, "null engine");
  HIPCHK(hipSetDevice(e->device));
  return join_phase2(e);
}

int check_ready(wca_engine* e) {
  if (!e) return fail(WCA_ERR_INVALID, "null engine");
  if (!e->finalized) return fail(WCA_ERR_STATE, "weights not finalized (call wca_finalize_weights)");
  HIPCHK(hipSetDevice(e->device));
  return ensure_split_weights(e);  // split mode: the K-doubled weight copies are current (no-op otherwise)
}

// stage per-utterance metadata into the next device slot: rows = {n_samples, n_tok, n_frames, dtwN}
int stage_meta(wca_engine* e, int B, const int32_t* a0, const int32_t* a1, const int32_t* a2, const int32_t* a3, int** dev_rows, hipStream_t s) {
  const int slot = e->meta_slot;
  e->meta_slot = (e->meta_slot + 1) % META_SLOTS;
  int* h = e->meta_host + (size_t)slot * 4 * e->max_batch;
  int* dv = e->meta_dev + (size_t)slot * 4 * e->max_batch;
  const int32_t* src[4] = {a0, a1, a2, a3};
  for (int r = 0; r < 4; ++r)
    for (int b = 0; b < B; ++b) h[r * e->max_batch + b] = src[r] ? src[r][b] : 0;
  HIPCHK(hipMemcpyAsync(dv, h, sizeof(int) * 4 * e->max_batch, hipMemcpyHostToDevice, s ? s : e->stream));
  for (int r = 0; r < 4; ++r) dev_rows[r] = dv + r * e->max_batch;
  return WCA_OK;
}

// K/V slot for a new encode: a free one, else the slot of the oldest state that was decoded but never aligned
// (a stand-alone wca_decode); -1 if both hold data that is still needed.
int take_kv_slot(wca_engine* e) {
  for (int sl = 0; sl < 2; ++sl)
    if (!e->slot_busy[sl]) return sl;
  for (auto it = e->enc_q.begin(); it != e->enc_q.end(); ++it)
    if (it->decoded) {
      const int sl = it->slot;
      e->enc_q.erase(it);
      return sl;
    }
  return -1;
}

}  // namespace wca

// =================================================================================== C ABI
extern "C" {

const char* wca_last_error(void) { return g_err.c_str(); }
int wca_version(void) { return 21; }   // 21: the alignment-heads route of the fused alignment (wca_align_batch*_heads: upstream's find_alignment post-processing; align_heads.hip); 20: windowed DTW (wca_dtw_windows, wca_dtw_batch_dev_windows, wca_align_batch*_windows: every text row has a permitted frame interval); 19: wca_speech_segments (speech activity of a long recording; speech_segments.hip); 18: wca_decode_group (beam search / best_of on grouped decoder rows; beam.hip); 17: one descriptor call each for decode (wca_decode) and the fused alignment (wca_align_batch*) in place of eleven entry points (HISTORY.md); 16: the CU-partition and two-stream decode experiments removed (HISTORY.md; wca_set_decode_mode refuses streams != 1); 15: wca_quiet_cuts (the quietest even frame near each equal share of a long recording); 14: open-end DTW (wca_dtw_open, wca_dtw_batch_dev_open, open-end rows in the fused alignment); 13: wca_detect_language (language identification on the state a decode then takes); 12: wca_resample_plan / wca_resample_table / wca_resample_16k (polyphase resampler to 16 kHz); 11: per-row decode (per-row initial tokens / sample budgets: the rows of a batch at different decoder positions); 10: wca_log_mel_long / wca_mel_window (whole-recording log-mel, window cut); 9: the two diagnostic stamp entry points removed, no switch read from the environment; 8: prompted greedy decode (sot_index, batched prefill); 7: two precision modes only (the per-stage precision mask, its setter / getter and the mixed
                                      // state are gone); 6: teacher-token log-probs (in the fused alignment, and wca_token_logprobs);
                                      // 5: a new engine is in the contract mode; wca_engine_create_ex, W_lo slab, switch table

int wca_engine_create(const wca_model_dims* dims, int device_ordinal, int max_batch, wca_engine** out) {
  return wca_engine_create_ex(dims, device_ordinal, max_batch, WCA_PRECISION_REFERENCE, out);   // the CONTRACT mode is the default (round 5)
}

int wca_engine_create_ex(const wca_model_dims* dims, int device_ordinal, int max_batch, int precision_mode, wca_engine** out) {
  if (!dims || !out) return fail(WCA_ERR_INVALID, "null argument");
  if (precision_mode != WCA_PRECISION_F16 && precision_mode != WCA_PRECISION_REFERENCE) return fail(WCA_ERR_INVALID, "precision mode %d", precision_mode);
  if (max_batch < 1 || max_batch > 256) return fail(WCA_ERR_INVALID, "max_batch %d outside [1,256]", max_batch);
  const wca_model_dims& D = *dims;
  if (D.n_audio_ctx != N_CTX || D.n_text_ctx != MAX_TOK) return fail(WCA_ERR_INVALID, "n_audio_ctx must be 1500 and n_text_ctx 448");
  if (D.n_audio_state % 128 || D.n_text_state % 128 || D.n_audio_state / D.n_audio_head != 64 || D.n_text_state / D.n_text_head != 64 ||
      D.n_audio_state > 1280 || D.n_text_state > 1280)
    return fail(WCA_ERR_INVALID, "unsupported widths: need n_state %% 128 == 0, n_state <= 1280, head_dim == 64");
  if (D.n_audio_state != D.n_text_state) return fail(WCA_ERR_INVALID, "n_audio_state != n_text_state");
  if (D.n_mels % 8 || D.n_mels > 256) return fail(WCA_ERR_INVALID, "n_mels must be a multiple of 8 and <= 256");
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device_ordinal < 0 || device_ordinal >= ndev) return fail(WCA_ERR_INVALID, "device %d not present (%d devices)", device_ordinal, ndev);
  HIPCHK(hipSetDevice(device_ordinal));
  wca_engine* e = new wca_engine();
  e->dims = D;
  e->device = device_ordinal;
  e->max_batch = max_batch;
  HIPCHK(hipDeviceGetAttribute(&e->n_cu, hipDeviceAttributeMultiprocessorCount, device_ordinal));
  HIPCHK(hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking));
  HIPCHK(hipStreamCreateWithFlags(&e->stream2, hipStreamNonBlocking));
  e->stream = e->own_stream;
  for (auto& ev : e->ev_kv) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  e->wslab_bytes = layout_weights(e, nullptr);
  HIPCHK(hipMalloc((void**)&e->wslab, e->wslab_bytes));
  HIPCHK(hipMemset(e->wslab, 0, e->wslab_bytes));
  layout_weights(e, e->wslab);
  if (precision_mode == WCA_PRECISION_REFERENCE) {   // born in the contract mode: the wide arena and the K-doubled weight copies from the start
    e->split = true;
    const size_t wbytes = layout_split_weights(e, nullptr);
    HIPCHK(hipMalloc((void**)&e->wslab2, wbytes));
    HIPCHK(hipMemset(e->wslab2, 0, wbytes));
    layout_split_weights(e, e->wslab2);
    e->sw_dirty = true;
  }
  const size_t abytes = layout_arena(e, nullptr);
  HIPCHK(hipMalloc((void**)&e->aslab, abytes));
  HIPCHK(hipMemset(e->aslab, 0, abytes));  // zero pad rows of mel_tm / h1pad and all slack
  layout_arena(e, e->aslab);
  HIPCHK(hipHostMalloc((void**)&e->meta_host, sizeof(int) * META_SLOTS * 4 * max_batch, hipHostMallocDefault));
  HIPCHK(hipHostMalloc((void**)&e->err_host, sizeof(int) * 4, hipHostMallocDefault));
  e->err_host[0] = 0;
  for (auto& ev : e->ev) HIPCHK(hipEventCreate(&ev));
  for (auto& site : e->kev)
    for (auto& layer : site)
      for (auto& ev : layer) HIPCHK(hipEventCreate(&ev));
  for (auto& ev : e->res_ev) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  e->ev_valid = true;
  // constant tables of the STFT
  {
    std::vector<float> win(N_FFT), tw(2 * N_FFT);
    const double PI = 3.14159265358979323846;
    for (int n = 0; n < N_FFT; ++n) {
      win[n] = (float)(0.5 - 0.5 * std::cos(2.0 * PI * n / N_FFT));  // periodic hann
      tw[2 * n] = (float)std::cos(2.0 * PI * n / N_FFT);
      tw[2 * n + 1] = (float)std::sin(2.0 * PI * n / N_FFT);
    }
    HIPCHK(hipMemcpy(e->window, win.data(), sizeof(float) * N_FFT, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->twiddle, tw.data(), sizeof(float) * 2 * N_FFT, hipMemcpyHostToDevice));
  }
  *out = e;
  return WCA_OK;
}

void wca_engine_destroy(wca_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  (void)hipDeviceSynchronize();
  for (GrowBuf* g : {&e->cap, &e->wws, &e->colnorm, &e->scores, &e->sel, &e->selsc, &e->matrix, &e->trace, &e->path, &e->pathlen,
                     &e->jump, &e->tmp0, &e->tmp1})
    g->release();
  (void)wca_comm_destroy(e);
  e->coll_send.release();
  e->coll_recv.release();
  if (e->wslab) (void)hipFree(e->wslab);
  if (e->wslab2) (void)hipFree(e->wslab2);
  if (e->wslab_lo) (void)hipFree(e->wslab_lo);
  e->wlo_tmp[0].release();
  e->wlo_tmp[1].release();
  if (e->aslab) (void)hipFree(e->aslab);
  if (e->meta_host) (void)hipHostFree(e->meta_host);
  if (e->err_host) (void)hipHostFree(e->err_host);
  if (e->dec_done_host) (void)hipHostFree(e->dec_done_host);
  e->dec_cache.release();
  e->dec_beam.release();
  e->dec_tokens.release();
  e->dec_masks.release();
  e->dec_logits.release();
  e->dec_state.release();
  e->dec_gather.release();
  e->dec_rows.release();
  e->probe_jump.release();
  e->dtw_out.release();
  e->dtw_meta.release();
  for (int i = 0; i < 2; ++i) {
    e->win_dev[i].release();
    if (e->win_host[i]) (void)hipHostFree(e->win_host[i]);
  }
  e->pscore.release();
  e->quiet_out.release();
  e->vad_buf.release();
  for (auto& t : e->rs_tables) (void)hipFree(t.dev);
  for (int i = 0; i < 2; ++i) {
    if (e->res_host[i]) (void)hipHostFree(e->res_host[i]);
    if (e->res_ev[i]) (void)hipEventDestroy(e->res_ev[i]);
  }
  if (e->ev_valid)
  {
    for (auto& ev : e->ev) (void)hipEventDestroy(ev);
    for (auto& site : e->kev)
      for (auto& layer : site)
        for (auto& ev : layer) (void)hipEventDestroy(ev);
  }
  for (auto& ev : e->ev_kv)
    if (ev) (void)hipEventDestroy(ev);
  if (e->stream2) (void)hipStreamDestroy(e->stream2);
  if (e->own_stream) (void)hipStreamDestroy(e->own_stream);
  delete e;
}

int wca_engine_set_stream(wca_engine* e, void* hip_stream) {
  if (!e) return fail(WCA_ERR_INVALID, "null engine");
  e->stream = (hipStream_t)hip_stream;  // NULL is the HIP default (null) stream, which is what torch's default stream is
  return WCA_OK;
}

int wca_engine_synchronize(wca_engine* e) {
  if (!e) return fail(WCA_ERR_INVALID, "null engine");
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipStreamSynchronize(e->stream2));
  return WCA_OK;
}

int wca_set_decode_mode(wca_engine* e, int fused, int streams) {
  if (!e) return fail(WCA_ERR_INVALID, "null engine");
  if (streams != 1) return fail(WCA_ERR_INVALID, "streams must be 1: the two-stream form of the decode loop was removed (it measured no faster)");
  e->dec_fused = fused != 0;
  return WCA_OK;
}

int wca_set_profiling(wca_engine* e, int on) {
  if (!e) return fail(WCA_ERR_INVALID, "null engine");
  e->profiling = on != 0;
  return WCA_OK;
}

int wca_last_stage_ms(wca_engine* e, float* ms8) {
  if (!e || !ms8) return fail(WCA_ERR_INVALID, "null argument");
  if (!e->profiling) return fail(WCA_ERR_STATE, "profiling disabled");
  HIPCHK(hipEventSynchronize(e->ev[8]));
  for (int i = 0; i < 7; ++i) HIPCHK(hipEventElapsedTime(&ms8[i], e->ev[i], e->ev[i + 1]));
  HIPCHK(hipEventElapsedTime(&ms8[7], e->ev[0], e->ev[8]));
  return WCA_OK;
}

int wca_last_kernel_ms(wca_engine* e, int site, int* n_launches, float* total_ms, double* flops_per_launch, double* bytes_per_launch) {
  if (!e || !n_launches || !total_ms || !flops_per_launch || !bytes_per_launch) return fail(WCA_ERR_INVALID, "null argument");
  if (site < 0 || site >= WCA_N_SITES) return fail(WCA_ERR_INVALID, "site %d outside [0,%d)", site, WCA_N_SITES);
  if (!e->profiling) return fail(WCA_ERR_STATE, "profiling disabled");
  HIPCHK(hipEventSynchronize(e->ev[8]));
  int nl = 0;
  float tot = 0.f;
  for (int i = 0; i < 33; ++i) {
    if (!e->kev_set[site][i]) continue;
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e->kev[site][i][0], e->kev[site][i][1]));
    tot += ms;
    ++nl;
  }
  *n_launches = nl;
  *total_ms = tot;
  // algorithmic work of ONE launch at the last batch size (M = batch * 1500 rows, d = n_audio_state). Bytes: operands read once, outputs
  // written once; in split mode every operand / output is an f16 PAIR (4 bytes per element instead of 2), the weights are read once
  const double d = e->dims.n_audio_state, M = (double)e->last_batch * N_CTX, H = e->dims.n_audio_head;
  const double p = e->split ? 2.0 : 1.0;
  const double fused_ln = e->fuse_ln && !e->split ? 2 : 0;   // the fused LayerNorm's f16 output (the f16 mode only)
  double fl = 0, by = 0;
  switch (site) {
    case WCA_SITE_QKV: fl = 2 * M * 3 * d * d; by = 2 * (p * M * d + 3 * d * d + p * M * 3 * d); break;
    case WCA_SITE_ATTN: fl = 4.0 * e->last_batch * H * (double)N_CTX * N_CTX * 64; by = 2 * p * (M * 3 * d + M * d); break;
    case WCA_SITE_OUT: fl = 2 * M * d * d; by = 2 * (p * M * d + d * d) + 8 * M * d + fused_ln * M * d; break;  // f32 residual read + write
    case WCA_SITE_FC1: fl = 2 * M * 4 * d * d; by = 2 * (p * M * d + 4 * d * d + p * M * 4 * d); break;
    case WCA_SITE_FC2: fl = 2 * M * 4 * d * d; by = 2 * (p * M * 4 * d + 4 * d * d) + 8 * M * d + fused_ln * M * d; break;
    case WCA_SITE_LN1:
    case WCA_SITE_LN2: fl = 8 * M * d; by = (4 + 2 * p) * M * d; break;                         // read f32, write f16 (or the f16 pair)
  }
  *flops_per_launch = fl;
  *bytes_per_launch = by;
  return WCA_OK;
}

int wca_set_precision(wca_engine* e, int mode) {
  if (!e) return fail(WCA_ERR_INVALID, "null engine");
  if (mode != WCA_PRECISION_F16 && mode != WCA_PRECISION_SPLIT) return fail(WCA_ERR_INVALID, "precision mode %d", mode);
  const bool want = mode == WCA_PRECISION_SPLIT, was = e->split;
  if (want == was) return WCA_OK;
  if (e->enq_count != e->fetch_count) return fail(WCA_ERR_STATE, "fetch the batches in flight before changing the precision mode");
  for (auto& st : e->enc_q)
    if (!st.decoded) return fail(WCA_ERR_STATE, "an encoded batch is waiting: consume it before changing the precision mode");
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipStreamSynchronize(e->stream2));
  // The activation arena is laid out per mode (operand buffers are twice as wide in split mode) and the K-doubled weight copies
  // exist only then. Allocate the NEW arena (and copies) first; the old ones are released and the engine's state committed only
  // when both allocations succeeded, so a failed switch leaves a working engine in its previous mode.
  e->split = want;
  const size_t abytes = layout_arena(e, nullptr);
  e->split = was;
  char* na = nullptr;
  char* nw = nullptr;
  size_t wbytes = 0;
  hipError_t he = hipMalloc((void**)&na, abytes);
  if (he == hipSuccess && want) {
    wbytes = layout_split_weights(e, nullptr);
    he = hipMalloc((void**)&nw, wbytes);
  }
  if (he == hipSuccess) he = hipMemset(na, 0, abytes);  // zero pad rows of mel_tm / h1pad, counters, flags and all slack
  if (he == hipSuccess && nw) he = hipMemset(nw, 0, wbytes);  // K padding of the conv1 copy stays zero
  if (he == hipSuccess && debug_switch(DBG_FAIL_PRECISION_ALLOC)) he = hipErrorOutOfMemory;  // fault injection (wca_test_set_switch) for the test of the path below
  if (he != hipSuccess) {
    if (na) (void)hipFree(na);
    if (nw) (void)hipFree(nw);
    (void)hipGetLastError();
    layout_arena(e, e->aslab);  // (the sizing pass above moved the arena pointers: restore them)
    if (was) layout_split_weights(e, e->wslab2);
    return fail(WCA_ERR_HIP, "precision switch: allocating the %s arena (%zu + %zu bytes) failed: %s; the engine keeps its previous mode",
                want ? "wide" : "narrow", abytes, wbytes, hipGetErrorString(he));
  }
  (void)hipFree(e->aslab);
  if (e->wslab2) (void)hipFree(e->wslab2);
  e->aslab = na;
  e->wslab2 = nw;
  e->split = want;
  layout_arena(e, e->aslab);
  if (want) {
    layout_split_weights(e, e->wslab2);
    e->sw_dirty = true;  // built on the next entry point that runs the model (after the weights are final)
  }
  e->ln_err = nullptr;
  for (auto& st : e->enc_q) e->slot_busy[st.slot] = false;  // decoded-but-never-aligned states die with the arena
  e->enc_q.clear();
  return WCA_OK;
}

int wca_get_precision(wca_engine* e) { return e && e->split ? WCA_PRECISION_SPLIT : WCA_PRECISION_F16; }

int wca_set_fuse_ln(wca_engine* e, int on) {
  if (!e) return fail(WCA_ERR_INVALID, "null engine");
  e->fuse_ln = on != 0;
  return WCA_OK;
}

int wca_set_overlap(wca_engine* e, int on) {
  if (!e) return fail(WCA_ERR_INVALID, "null engine");
  if (e->enq_count != e->fetch_count) return fail(WCA_ERR_STATE, "fetch the batches in flight before changing the stream layout");
  e->overlap = on != 0;
  return WCA_OK;
}

}  // extern "C"
