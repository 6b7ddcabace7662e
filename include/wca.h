/*
 * wca.h -- C ABI of libwca.so, the MI355X (gfx950) forced-alignment engine.
 *
 * This is the drop-in boundary for the hot path of 30stomercury/whisper-char-alignment.
 * The reference has no FFI layer of its own (it is pure Python calling openai-whisper); the
 * boundary is therefore the set of Python functions below, and each entry point here names the
 * reference interface it replaces (file:line in the reference repository):
 *
 *   wca_log_mel            dataset.py:46-48, dataset.py:107-109, README.md:101-103
 *                          (whisper.pad_or_trim + whisper.log_mel_spectrogram)
 *   wca_log_mel_long       whisper.log_mel_spectrogram(audio, n_mels, padding=N_SAMPLES) of a WHOLE recording, the first step of
 *                          upstream whisper.transcribe (not called by the reference, whose entry points stop at 30 s)
 *   wca_resample_16k       whisper.load_audio's resampling to 16 kHz (upstream pipes every file through ffmpeg; the filter here is the
 *                          default of torchaudio.functional.resample), with wca_resample_plan / wca_resample_table on the host
 *   wca_mel_window         whisper.pad_or_trim(mel[:, seek : seek + segment_size], N_FRAMES), the window cut of whisper.transcribe's loop
 *   wca_quiet_cuts         no counterpart in the reference or upstream: the quietest even frame near each equal share of a long recording,
 *                          where transcribe(pieces=...) cuts it into pieces that are decoded side by side
 *   wca_speech_segments    no counterpart in the reference or upstream (faster-whisper's vad_filter runs a neural detector on the host): the
 *                          frame ranges of a long recording whose smoothed log-mel level stands out of its noise floor, which
 *                          transcribe(vad_filter=True) decodes instead of every window and force_align_long(trim_silence=...) trims words to
 *   wca_get_attentions     timing.py:45-67   get_attentions(): teacher-forced forward with every
 *                          cross-attention QK captured (timing.py:50-58), [:max_frames] slice,
 *                          median_filter, *qk_scale, softmax (timing.py:63-66); logits returned
 *   wca_attention_weights  timing.py:63-66   the same post-processing on caller-supplied captured logits
 *   wca_median_filter      timing.py:65      whisper.timing.median_filter
 *   wca_filter_attention   timing.py:13-43   filter_attention(): head scores + tuple-ordered top-k
 *                          (+ metrics.py:99-111 coverage_penalty)
 *   wca_force_align        timing.py:69-103  force_align() up to and including dtw(-matrix):
 *                          aggregation "mean" (timing.py:84-89) / "topk" (timing.py:91-97), the
 *                          [len(sot_sequence):-1] slice (timing.py:102), DTW + backtrace (timing.py:103)
 *   wca_default_find_alignment  timing.py:116-186 default_find_alignment (std/mean normalised alignment heads)
 *   wca_dtw                timing.py:103     whisper.timing.dtw -> dtw_cpu + backtrace
 *   wca_dtw_open, wca_dtw_batch_dev_open, wca_align_desc.open_end_host
 *                          no counterpart in the reference or upstream (their aligners stop at one 30 s window): the OPEN-END form
 *                          of the same DTW, for a window of a long recording that holds only a prefix of the text it is offered
 *                          (align_long.py: a recording of any length against a given transcript)
 *   wca_dtw_windows, wca_dtw_batch_dev_windows, wca_align_batch_enqueue_windows, wca_align_batch_windows
 *                          no counterpart in the reference or upstream: the WINDOWED form of the same DTW, in which every text row
 *                          has a permitted frame interval (align_long.py force_align_cues: a recording against its subtitles, whose
 *                          cue times bound where each cue's text may lie)
 *   wca_probe_heads        probe_oracle.py:83-90  per-head force_align sweep (one DTW per head)
 *   wca_decode             infer_ali.py:40,60-61, probe_oracle.py:59-60, README.md:107-108:
 *                          whisper.decode(model, mels, DecodingOptions(language="en")) -- the greedy ASR pre-pass
 *                          that produces the teacher text (upstream decoding.py: KV-cached autoregressive
 *                          decoder, SuppressBlank / SuppressTokens / ApplyTimestampRules, GreedyDecoder); through the fields of
 *                          wca_decode_desc also DecodingOptions(prompt=..., prefix=...) (transcribe(initial_prompt=...)), rows with
 *                          prompts and sample budgets of their own (transcribe_batch), and upstream's GreedyDecoder at temperature > 0
 *                          (the rungs of transcribe's temperature fallback ladder)
 *   wca_decode_group       upstream decoding.py BeamSearchDecoder / best_of + MaximumLikelihoodRanker (DecodingOptions(beam_size=..., patience=...,
 *                          best_of=...), what upstream's command line decodes with by default; not called by the reference): wca_decode on
 *                          n_group decoder rows per audio that share its cross-K/V, with the beam step and the cache reorder on the GPU
 *   wca_align_batch       infer_ali.py:93-101 + dataset.py:47-48: the whole per-utterance pipeline
 *                          (log-mel -> forward+capture -> medfilt/softmax -> scores/top-k ->
 *                          aggregate -> DTW) for a micro-batch of utterances, results = the frame
 *                          at which the DTW path enters every token row (timing.py:110-111 `jumps`)
 *   wca_align_desc.vocab_end / wca_align_result.token_logprob_host, wca_token_logprobs
 *                          timing.py:146-150 (`text_token_probs`: softmax of logits[len(sot_sequence):, :eot] at the
 *                          teacher token) and timing.py:181-184 (`word_probabilities`, the per-word mean the host forms):
 *                          the teacher-token log-probabilities, computed and kept on the GPU
 *
 * Conventions
 *   - plain C types only; no torch / HIP types in signatures (streams are passed as void*).
 *   - `_dev` pointers are device (HBM) pointers owned by the caller; `_host` pointers are host memory.
 *   - every function returns 0 on success or a negative wca_status; wca_last_error() gives a
 *     thread-local description. Nothing throws across this boundary.
 *   - one engine <-> one GPU <-> one stream <-> one host thread. Engines are independent.
 *   - limits mirror infer_ali.py:25-26,79: n_tok <= 448, max_frames <= 1500 (WCA_ERR_TOO_LONG).
 */
#ifndef WCA_H_
#define WCA_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wca_engine wca_engine;

typedef enum {
  WCA_OK = 0,
  WCA_ERR_INVALID = -1,   /* bad argument / shape                                  */
  WCA_ERR_TOO_LONG = -2,  /* n_tok > 448 or max_frames > 1500 (infer_ali.py:79)    */
  WCA_ERR_HIP = -3,       /* a HIP runtime call failed                             */
  WCA_ERR_STATE = -4,     /* weights missing / engine not finalized                */
  WCA_ERR_NOMEM = -5
} wca_status;

/* whisper.model.ModelDimensions */
typedef struct {
  int32_t n_mels;
  int32_t n_audio_ctx;    /* 1500 */
  int32_t n_audio_state;
  int32_t n_audio_head;
  int32_t n_audio_layer;
  int32_t n_vocab;
  int32_t n_text_ctx;     /* 448 */
  int32_t n_text_state;
  int32_t n_text_head;
  int32_t n_text_layer;
} wca_model_dims;

enum { WCA_DTYPE_F32 = 0, WCA_DTYPE_F16 = 1 };
enum { WCA_AGGR_MEAN = 0, WCA_AGGR_TOPK = 1 };

/* options of filter_attention / force_align (timing.py:13, timing.py:69-78) */
typedef struct {
  int32_t aggregation;    /* WCA_AGGR_MEAN | WCA_AGGR_TOPK                          */
  int32_t topk;           /* > 0 required for WCA_AGGR_TOPK (timing.py:92)          */
  float w_colnorm;        /* default 1.0                                           */
  float w_rownorm;        /* default 1.0                                           */
  float w_coverage;       /* default 0.0                                           */
  int32_t sot_len;        /* len(tokenizer.sot_sequence): rows dropped at the top   */
  int32_t medfilt_width;  /* odd; used by wca_align_batch / wca_get_attentions      */
  float qk_scale;         /* 1.0 in the reference (infer_ali.py:45)                 */
} wca_align_opts;

const char* wca_last_error(void);
int wca_version(void);   /* 21: wca_align_batch_enqueue_heads / wca_align_batch_heads (openai-whisper's alignment-heads post-processing on the fused path); 20: the windowed DTW (wca_dtw_windows, wca_align_batch*_windows); 19: wca_speech_segments (the speech segments of a long recording: what transcribe(vad_filter=True) decodes); 18: wca_decode_group (beam search and best_of: G decoder rows per audio, a beam step and a cache reorder on the GPU); 17: one descriptor call each for decode (wca_decode, wca_decode_desc) and the fused alignment (wca_align_desc, wca_align_result) in place of the eleven entry points that had grown feature by feature; 16: the CU-partition and two-stream decode experiments are gone; 15: wca_quiet_cuts (where to cut one long recording into pieces decoded side by side); 14: the open-end DTW entry points; 13: wca_detect_language (the language head on the encoded state; the decode that follows re-uses the state); 12: wca_resample_plan, wca_resample_table, wca_resample_16k (any input rate to 16 kHz); 11: per-row prompts and sample budgets in the decode; 10: wca_log_mel_long, wca_mel_window; 9: the diagnostic stamp entry points are gone, switches no longer read the environment; 8: prompt / prefix in the decode (sot_index, batched prefill); 7: exactly two precision modes */

/* ---- engine lifetime ------------------------------------------------------------------------ */
/* A new engine is in the CONTRACT precision mode (WCA_PRECISION_REFERENCE: every stage on (hi, lo) operand pairs = the fp32 forward of
 * /root/reference/timing.py:58 to fp32 summation noise; see wca_set_precision). Since round 5 the fast f16-operand mode is the opt-in:
 * wca_engine_create_ex(..., WCA_PRECISION_F16, ...) builds the engine directly in it (no wide arena is ever allocated), or switch later
 * with wca_set_precision. */
int wca_engine_create(const wca_model_dims* dims, int device_ordinal, int max_batch, wca_engine** out);
int wca_engine_create_ex(const wca_model_dims* dims, int device_ordinal, int max_batch, int precision_mode, wca_engine** out);
void wca_engine_destroy(wca_engine* e);
/* stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = the HIP default (null)
 * stream. Until this is called the engine runs on a private non-blocking stream of its own. */
int wca_engine_set_stream(wca_engine* e, void* hip_stream);
int wca_engine_synchronize(wca_engine* e);

/* Weights in openai-whisper state_dict naming ("encoder.blocks.0.attn.query.weight", ...), host
 * memory, row-major. Also accepts the auxiliary table "mel_filters" [n_mels][201] (whisper's
 * assets/mel_filters.npz). Call wca_finalize_weights once after the last tensor. */
int wca_load_weight(wca_engine* e, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim);
int wca_finalize_weights(wca_engine* e);
/* Weight MATRICES (Linear / Conv1d weights, the token embedding) are stored f16, like every openai checkpoint at rest
 * (/root/reference/infer_ali.py:36-37: whisper.load_model upcasts those f16 values to fp32 parameters); biases, LayerNorm parameters and
 * positional embeddings stay fp32. An fp32 source tensor whose values are NOT f16-representable (a fine-tuned fp32 state dict, which the
 * reference runs in true fp32) is not rounded away: wca_load_weight keeps the remainder lo = f16(w - f16(w)) of every such element in a second
 * slab (w = hi + lo to 2^-22 |w|, the representation the activations travel in) and counts the elements per tensor (wca_weights_inexact:
 * tensors, values, name of the first one). In split mode the GEMMs multiply the extra term A_hi W_lo^T for those
 * matrices (one more f16 pass: an accumulating launch for the residual GEMMs, a pre-activation addend for the others; the embedding adds
 * hi + lo) -- slower, never a narrower model. wca_set_allow_rounded_weights(e, 1) drops the remainders (the engine then computes what the
 * f16-rounded checkpoint computes); the f16 mode (approximate by definition) ignores them. */
int wca_weights_inexact(wca_engine* e, long long* n_tensors_out, long long* n_values_out, char* first_name_out, int first_name_cap);
int wca_set_allow_rounded_weights(wca_engine* e, int on);

/* ---- hot path, one reference function per entry point ---------------------------------------- */

/* pcm_dev: [batch][pcm_stride] f32 (values beyond n_samples are ignored = zero padding to 30 s);
 * mel_out_dev: [batch][n_mels][3000] f32. */
int wca_log_mel(wca_engine* e, const float* pcm_dev, int64_t pcm_stride, const int32_t* n_samples_host, int batch,
                float* mel_out_dev);

/* Log-mel of a whole recording of any length (upstream whisper.transcribe: log_mel_spectrogram(audio, n_mels, padding=N_SAMPLES)).
 * The signal is pcm_dev[0 .. n_samples) followed by 480000 zeros; STFT as wca_log_mel (n_fft 400, hop 160, periodic Hann, centred with
 * reflect padding at both ends of the PADDED signal, last frame dropped): n_frames = (n_samples + 480000) / 160, written to
 * *n_frames_out (may be NULL; it is set before ld is checked, so a call with ld = 0 asks for the size). log10(clamp 1e-10), ONE floor
 * `max - 8` with the maximum over all frames of the recording (not per 30 s window), (x + 4) / 4.
 * mel_out_dev: [n_mels][ld] f32 owned by the CALLER, ld >= n_frames (row m, frame t at m * ld + t; columns beyond n_frames are not
 * touched). The raw log10 values rest in mel_out_dev between the two passes, so the engine keeps no buffer of the recording's size.
 * Precision follows wca_set_precision like wca_log_mel: f64 DFT / filterbank accumulation in WCA_PRECISION_REFERENCE, f32 in the f16
 * mode. n_samples in [0, 2^31 - 480001]; asynchronous on the engine's stream. */
int wca_log_mel_long(wca_engine* e, const float* pcm_dev, int64_t n_samples, float* mel_out_dev, int64_t ld, int64_t* n_frames_out);

/* Sample-rate conversion to 16 kHz, the step upstream whisper.load_audio leaves to ffmpeg. The filter is the default of
 * torchaudio.functional.resample (Hann-windowed sinc, lowpass_filter_width 6, rolloff 0.99) in polyphase form. For an input rate sr_in in
 * [2000, 384000] (anything else: WCA_ERR_INVALID), in integer arithmetic:
 *   g = gcd(sr_in, 16000), L = 16000 / g, M = sr_in / g, W = ceil(600 M / (99 min(L, M))), n_taps = 2 W + 2, n_out = ceil(n_in L / M).
 * Output j reads the inputs k = k0 + i - W for i in [0, n_taps), k0 = floor(j M / L) (64-bit), zero for k outside [0, n_in), against row
 * p = (j M) mod L of the table
 *   h[p][i] = c sinc(t) cos^2(pi t / 12),  c = 0.99 min(L, M) / M,  t = clip((i - W - p / L) c, -6, 6),  sinc(t) = sin(pi t) / (pi t):
 *   y[j] = sum_i h[p][i] x[k], x the mean over the channels.
 * wca_resample_plan and wca_resample_table are host only (no engine, no GPU, like wca_collate_plan): the plan quantities (any output
 * pointer may be NULL) and the table [L][n_taps] in float64 (44101 Hz: 16000 x 36). */
int wca_resample_plan(int sr_in, int32_t* L, int32_t* M, int32_t* W, int32_t* n_taps);
int wca_resample_table(int sr_in, double* table_out);
/* in_dev [channels][ld] f32 (n_in <= ld samples per channel; any 4-byte aligned address, any ld) -> out_dev [*n_out] f32 owned by the
 * CALLER, *n_out = ceil(n_in L / M) <= out_cap (*n_out is set before out_cap is checked, so a call with out_cap = 0 asks for the size).
 * sr_in == 16000 copies (the channel mean): the filter is no identity at equal rates, and upstream does nothing there. The engine rounds
 * the float64 table to f32 once per rate and keeps it on the device (a second call at the same rate uploads nothing); taps accumulate in
 * f32 in ascending order. channels in [1, 8]; *n_out <= 2^31 - 480001 so that the result always fits wca_log_mel_long; n_in = 0 gives
 * *n_out = 0 without a launch. Asynchronous on the engine's stream; the engine keeps no buffer of the recording's size. */
int wca_resample_16k(wca_engine* e, const float* in_dev, int channels, int64_t ld, int64_t n_in, int sr_in, float* out_dev, int64_t out_cap,
                     int64_t* n_out);

/* pad_or_trim(mel[:, seek : seek + size], 3000) for `batch` windows of one long mel (mel_long_dev [n_mels][ld] f32 with n_frames valid
 * frames, as wca_log_mel_long leaves it): mel_out_dev [batch][n_mels][3000] f32 with exact zeros at frames >= size -- the zero padding
 * of the MEL domain that upstream's loop feeds its last, short window (not the log-mel of silence). The result is what
 * wca_decode / wca_encode_batch / wca_get_attentions take as mel_dev. size outside [1, 3000], seek < 0 or seek + size > n_frames
 * is WCA_ERR_INVALID (nothing is read); batch <= max_batch. */
int wca_mel_window(wca_engine* e, const float* mel_long_dev, int64_t ld, int64_t n_frames, const int32_t* seek_host,
                   const int32_t* size_host, int batch, float* mel_out_dev);

/* Where to cut one long recording into n_pieces pieces that can be transcribed side by side: near each equal share, the quietest even
 * frame. mel_long_dev [n_mels][ld] f32 as wca_log_mel_long leaves it, n_mels from the engine; only frames [0, content_frames) are read.
 * Integers from the first sum on, so the summation order cannot matter and the result is exact:
 *   q(x)  = rint(4096 clamp(x, -8, 8)), ties to even; a NaN counts as 8 (loud, never preferred)
 *   e[t]  = sum over the mel rows m of q(mel[m][t])
 *   s[t]  = sum over j in [-half_width, half_width] of e[clamp(t + j, 0, content_frames - 1)]     (inside int32 for n_mels <= 128)
 *   g_k   = floor(k content_frames / n_pieces) in 64-bit, k = 1 .. n_pieces - 1
 *   cuts_host[k] = the EVEN t in [g_k - radius, g_k + radius] with the lexicographically smallest (s[t], |t - g_k|, t): even, so that every
 *   segment time of a piece stays on the 20 ms grid; cuts_host[0] = 0, cuts_host[n_pieces] = content_frames (n_pieces + 1 entries, strictly
 *   increasing); level_host[k - 1] = s[cuts_host[k]] (n_pieces - 1 entries; may be NULL).
 * WCA_ERR_INVALID, with nothing launched and cuts_host untouched, unless 2 <= n_pieces <= 4096, 1 <= radius <= 1500,
 * 0 <= half_width <= 100, content_frames <= ld, content_frames < 2^31 and content_frames / n_pieces >= 2 radius + 2 in integer division
 * (the search ranges are then disjoint and inside (0, content_frames)). Synchronous on the engine's stream: the host needs the cuts. */
int wca_quiet_cuts(wca_engine* e, const float* mel_long_dev, int64_t ld, int64_t content_frames, int n_pieces, int radius, int half_width,
                   int32_t* cuts_host, int32_t* level_host /* nullable */);

/* Speech activity of one long recording: the frame ranges whose level stands out of the recording's own noise floor. An energy detector
 * with an exact definition, not a trained one: the kernels are bit-exact against it (tests/test_speech_segments_gpu.py), the quality of
 * the DEFAULTS on real speech is NOT established (one 2.9 s recording was looked at; no corpus). mel_long_dev [n_mels][ld] f32 as
 * wca_log_mel_long leaves it; with cf = content_frames only frames [0, cf) are read. Integers from the first sum on:
 *   q(x), e[t], s[t]  exactly wca_quiet_cuts' (the frame index of the box sum clamped to [0, cf - 1]); |s| < 2^30 for n_mels <= 128
 *   lo, hi            the r-th smallest (0-based) of the multiset {s[t]}, r = floor((cf - 1) floor_permille / 1000) and
 *                     floor((cf - 1) peak_permille / 1000) in 64-bit
 *   flat              (hi - lo) < min_range n_mels (2 half_width + 1)                                                   (64-bit)
 *   on_thr, off_thr   lo + (((hi - lo) on_share) >> 10), lo + (((hi - lo) off_share) >> 10)      (64-bit product; the result fits int32)
 *   a0[t]             1 if s[t] >= on_thr; 0 if s[t] < off_thr; else a0[t - 1], with a0[-1] = 0                         (hysteresis)
 *   close             a maximal run of 0 shorter than min_silence with a 1 on BOTH sides becomes 1 (leading / trailing silence never)
 *   open              then a maximal run of 1 shorter than min_speech becomes 0
 *   pad               then every run [a, b) becomes [max(0, a - pad), min(cf, b + pad)); runs that overlap OR TOUCH merge
 *   result            the runs in order as (start, stop) pairs; if flat: the one pair (0, cf), whatever the steps above would give
 * Consequences: a NaN frame is loud, so it is never dropped; on_thr <= hi, so a recording that is not flat has at least one active frame
 * before `open`; zero segments is a legal result.
 * segments_host [max_segments][2] receives the first min(n_segments, max_segments) pairs (NULL is allowed with max_segments 0);
 * stats_host [6] = {lo, hi, on_thr, off_thr, flat, n_segments}, n_segments being the TRUE count also where it exceeds max_segments (the
 * call still succeeds; n_segments <= (cf + 1) / 2).
 * WCA_ERR_INVALID, with nothing launched and nothing written, unless 1 <= cf <= ld, cf < 2^31, max_segments >= 0 and the options are in
 * range: half_width 0..100, 0 <= floor_permille <= peak_permille <= 1000, 1 <= on_share <= 1023, 0 <= off_share <= on_share, min_range
 * 0..32768, min_speech and min_silence 1..2^24, pad 0..2^24. The defaults (WCA_VAD_DEFAULTS): 7, 50, 950, 410, 307, 1024 (10 dB averaged
 * over the mel rows), 25, 200, 40 (faster-whisper's 250 ms / 2 s / 400 ms). Synchronous on the engine's stream: the host needs the pairs.
 * Nothing returns to the host between the kernels. */
typedef struct {
  int32_t half_width;
  int32_t floor_permille;
  int32_t peak_permille;
  int32_t on_share;
  int32_t off_share;
  int32_t min_range;
  int32_t min_speech;
  int32_t min_silence;
  int32_t pad;
} wca_vad_opts;
#define WCA_VAD_DEFAULTS {7, 50, 950, 410, 307, 1024, 25, 200, 40}
int wca_speech_segments(wca_engine* e, const float* mel_long_dev, int64_t ld, int64_t content_frames, const wca_vad_opts* opts,
                        int32_t* segments_host /* nullable with max_segments 0 */, int max_segments, int32_t* stats_host);

/* mel_dev [batch][n_mels][3000] f32; tokens_dev [batch][n_tok] int64 (already sot..eot framed,
 * infer_ali.py:69-76; shorter utterances padded with any valid token id, true lengths in n_tok_host,
 * NULL = all n_tok); max_frames_host [batch].
 * weights_out_dev: [batch][L][H][n_tok][F] f32 with F = max over the batch of max_frames (rows/cols
 * beyond an utterance's own n_tok/max_frames are unspecified); logits_out_dev: [batch][n_tok][n_vocab]
 * f32 or NULL. */
int wca_get_attentions(wca_engine* e, const float* mel_dev, const int64_t* tokens_dev, int batch, int n_tok,
                       const int32_t* n_tok_host, const int32_t* max_frames_host, int medfilt_width, float qk_scale,
                       float* weights_out_dev, float* logits_out_dev);

/* The post-capture half of get_attentions (timing.py:63-66) on caller-supplied logits: qk_dev [L][H][n][ld] f32 (what
 * the forward hooks collected, torch.cat'ed over layers; ld = row stride >= max_frames, 1500 in the reference) ->
 * [..., :max_frames] slice, median_filter(medfilt_width), * qk_scale, softmax over frames ->
 * weights_out_dev [L][H][n][max_frames] f32. */
int wca_attention_weights(wca_engine* e, const float* qk_dev, int L, int H, int n, int ld, int max_frames,
                          int medfilt_width, float qk_scale, float* weights_out_dev);

/* in/out [rows][F] f32 device, reflect padding, width odd */
int wca_median_filter(wca_engine* e, const float* in_dev, float* out_dev, int64_t rows, int F, int width);

/* attns_dev [L][H][n][F] f32 (already softmaxed). scores_host [L*H]; sel_idx_host/sel_score_host
 * [min(topk, L*H)] ascending by (score, (l,h)) -- element i is head l = idx / H, h = idx % H. */
int wca_filter_attention(wca_engine* e, const float* attns_dev, int L, int H, int n, int F, int topk, float w_colnorm,
                         float w_rownorm, float w_coverage, float* scores_host, int32_t* sel_idx_host,
                         float* sel_score_host);

/* ws_dev [L][H][n][F] f32. Outputs (host): matrix_host [(n - sot_len - 1)][F] f32 (the sliced,
 * NOT negated matrix, timing.py:102); text_idx_host / time_idx_host [n - sot_len - 1 + F] int32 with
 * *path_len_host valid entries; sel_idx_host / sel_score_host [topk] (topk mode only, may be NULL). */
int wca_force_align(wca_engine* e, const float* ws_dev, int L, int H, int n, int F, const wca_align_opts* opts,
                    float* matrix_host, int32_t* text_idx_host, int32_t* time_idx_host, int32_t* path_len_host,
                    int32_t* sel_idx_host, float* sel_score_host);

/* timing.py:116-186 default_find_alignment (openai-whisper's own aligner, `--default_whisper_timing`), the part after
 * median filter + softmax: weights of the given alignment heads (flat ids l*H + h) are normalised per head and frame
 * over the token axis, (w - mean) / std with population std (timing.py:159-160), averaged over the heads (:162),
 * sliced [sot_len:-1] (:163) and aligned with dtw(-matrix) (:165; the dtw_cpu tie rule is used).
 * ws_dev [L][H][n][F] as returned by wca_get_attentions; heads_host in the order of model.alignment_heads.indices().T
 * (row-major over (l, h)); weights_norm_out_dev [n_heads][n][F] f32 device or NULL: the normalised weights, which
 * the reference returns as its 4th value (timing.py:186); other outputs as in wca_force_align. */
int wca_default_find_alignment(wca_engine* e, const float* ws_dev, int L, int H, int n, int F, const int32_t* heads_host,
                                int n_heads, int sot_len, float* weights_norm_out_dev, float* matrix_host,
                                int32_t* text_idx_host, int32_t* time_idx_host, int32_t* path_len_host);

/* DTW on the NEGATED matrix exactly like `dtw(-matrix)`; matrix_host [N][M] f32 row-major.
 * text_idx_host / time_idx_host capacity N + M. */
int wca_dtw(wca_engine* e, const float* matrix_host, int N, int M, int32_t* text_idx_host, int32_t* time_idx_host,
            int32_t* path_len_host);

/* Same for P independent problems already in HBM (probe_oracle.py:88-90: one DTW per head).
 * matrix_dev [P][N][M]; jump_frame_host [P][N]: frame at which the path enters each row. */
int wca_dtw_batch_dev(wca_engine* e, const float* matrix_dev, int P, int N, int M, int32_t* jump_frame_host);

/* Open-end DTW: the recurrence, tie rule and f64-add / f32-store of wca_dtw, but the path ends in the LAST frame at whichever text row fits
 * best instead of at row N - 1. Every cell carries L, the number of cells on its chosen path (itself included); the end row n* minimises
 * C[i][M-1] / L[i][M-1] (every visited cell adds a non-positive cost, so the unnormalised minimum would always be the last row). The
 * comparison is exact -- row a beats row b iff (double)C_a * L_b < (double)C_b * L_a -- and equal scores go to the lower row.
 * The path is backtraced from (n*, M - 1); *end_row_host = n*, *score_host (nullable) = (float)((double)C / (double)L) at the end cell, for
 * diagnostics only. Limits as wca_dtw (N <= 512, M <= 4096). */
int wca_dtw_open(wca_engine* e, const float* matrix_host, int N, int M, int32_t* text_idx_host, int32_t* time_idx_host,
                 int32_t* path_len_host, int32_t* end_row_host, float* score_host);

/* wca_dtw_batch_dev for P problems of which open_end_host[p] != 0 marks the open-ended ones; one launch may mix open and closed problems.
 * n_rows_host / n_cols_host [P] (each nullable: all N / all M) make the launch ragged: problem p is the n_rows[p] x n_cols[p] top-left
 * corner of its [N][M] slice of matrix_dev. jump_frame_host [P][N]: as wca_dtw_batch_dev for rows i <= end_row[p], -1 for the rows
 * end_row[p] < i < n_rows[p] that the path does not reach, 0 beyond n_rows[p]. end_row_host [P] (N_p - 1 for a closed problem, whose jump
 * frames are exactly wca_dtw_batch_dev's); score_host [P] nullable. */
int wca_dtw_batch_dev_open(wca_engine* e, const float* matrix_dev, int P, int N, int M, const int32_t* n_rows_host,
                           const int32_t* n_cols_host, const int32_t* open_end_host, int32_t* jump_frame_host, int32_t* end_row_host,
                           float* score_host);

/* wca_dtw_batch_dev_open plus the per-row score of each path (a null open_end_host: every problem is closed). For text row i of problem p,
 * path_cells_host[p][i] is the number of cells of the backtraced path in that row and path_mean_host[p][i] the mean of matrix[p][i][j]
 * (NOT negated) over them, added in f64 and rounded once to f32. Within a row the path only moves along the frame axis, so the cells are
 * the frames jump[i] .. last[i]: last = n_cols[p] - 1 for the end row, otherwise jump[i+1] where the path enters row i + 1 vertically (that
 * frame then counts in both rows) and jump[i+1] - 1 where it enters diagonally. Rows the path does not reach (past an open end row, or
 * beyond n_rows[p]) are (0, 0.0). Both outputs are [P][N] like jump_frame_host; the jump frames and end rows are wca_dtw_batch_dev_open's.
 * The score is computed by a kernel of its own behind the DTW; the bits do not depend on P or on a problem's position. Limits as wca_dtw;
 * unlike wca_dtw_batch_dev_open this call also takes an EMPTY problem (n_rows[p] or n_cols[p] = 0): no DTW runs for it, its end row is -1,
 * its jump frames, cells and means are 0. */
int wca_dtw_path_scores(wca_engine* e, const float* matrix_dev, int P, int N, int M, const int32_t* n_rows_host, const int32_t* n_cols_host,
                        const int32_t* open_end_host, int32_t* jump_frame_host, int32_t* end_row_host, float* path_mean_host,
                        int32_t* path_cells_host);

/* Windowed DTW: wca_dtw in which text row i may only sit at the frames row_lo[i] <= j <= row_hi[i]. The recurrence, the f64-add / f32-store
 * and the tie rule are wca_dtw's; a cell outside its row's window costs +inf and the matrix is not modified. One exception to the tie rule:
 * where it chose "left", the left cost is +inf and the diagonal and upper costs are equal and finite (the left edge of a row's window under
 * an exact 0), the move is "up". Without windows that case cannot occur, so full windows [0, M-1] give wca_dtw's path bit for bit.
 * The windows are checked on the host before anything is launched; WCA_ERR_INVALID unless, for every problem (n rows, m columns):
 * 0 <= lo[i] <= hi[i] <= m-1, lo[0] == 0, hi[n-1] == m-1, lo and hi non-decreasing, lo[i+1] <= hi[i] + 1 -- which guarantees a finite path
 * from (0, 0) to (n-1, m-1) inside the windows. row_lo_host / row_hi_host [N] int32. Limits as wca_dtw (N <= 512, M <= 4096). */
int wca_dtw_windows(wca_engine* e, const float* matrix_host, int N, int M, const int32_t* row_lo_host, const int32_t* row_hi_host,
                    int32_t* text_idx_host, int32_t* time_idx_host, int32_t* path_len_host);

/* wca_dtw_batch_dev with windows: P closed problems, ragged through n_rows_host / n_cols_host [P] (each nullable) as in
 * wca_dtw_batch_dev_open. row_lo_host / row_hi_host [P][N] (row stride N): only the first n_rows[p] entries of problem p are read.
 * jump_frame_host [P][N]: the frame at which the path enters each row, 0 beyond n_rows[p]. The result of a problem does not depend on P or
 * on its position. */
int wca_dtw_batch_dev_windows(wca_engine* e, const float* matrix_dev, int P, int N, int M, const int32_t* n_rows_host, const int32_t* n_cols_host,
                              const int32_t* row_lo_host, const int32_t* row_hi_host, int32_t* jump_frame_host);

/* probe_oracle.py:83-90: one alignment PER HEAD (aggregation "mean" on a single head = column
 * normalisation only), all L*H DTWs in one launch. ws_dev [L][H][n][F]; scores_host [L*H] = the
 * filter_attention scores (w_col = w_row = 1); jump_frame_host [L*H][n - sot_len - 1]. */
int wca_probe_heads(wca_engine* e, const float* ws_dev, int L, int H, int n, int F, int sot_len, float* scores_host,
                    int32_t* jump_frame_host);
/* Strict word-boundary scoring of EVERY head of the preceding wca_probe_heads (probe_oracle.py:83-90 calling
 * metrics.py:45-72 eval_n1_strict once per head): head hd's predicted end of hypothesis word i is
 * jump_frame[hd][word_end_row[i]] / 50 s; it is a true positive if an unused reference boundary j with
 * same_word[i * n_ref + j] != 0 lies within `tolerance` (first such j, the reference's loop order). tp_host [n_heads = L*H];
 * fp = n_hyp - tp, fn = n_ref - tp. Times are compared in float64 like the host code: tp is the same integer. */
int wca_probe_strict_tp(wca_engine* e, int n_heads, const int32_t* word_end_row_host, int n_hyp, const double* ref_times_host, int n_ref,
                        const uint8_t* same_word_host, double tolerance, int32_t* tp_host);

/* Fused per-utterance pipeline for a micro-batch (the north-star hot path), and the teacher-token log-probabilities
 * (timing.py:146-150 of the reference: text_token_probs = softmax(logits[len(sot_sequence):, :eot]) at the teacher token, here in log
 * space; the per-word mean of timing.py:181-184 is the caller's). A zero in an optional field means "off". */
typedef struct {
  const float* pcm_dev;             /* [batch][pcm_stride] f32; NULL: consume the oldest encoded state of this batch (wca_encode_batch, or
                                       the one the preceding wca_decode left) instead of running phase 1                                  */
  const int32_t* n_samples_host;    /* [batch]; required with pcm_dev                                                                   */
  const int64_t* tokens_dev;        /* [batch][n_tok_max] int64, each row [*sot_sequence, no_timestamps, *text, eot]                      */
  const int32_t* n_tok_host;        /* [batch]: row b's true length                                                                     */
  const int32_t* max_frames_host;   /* [batch]                                                                                          */
  const wca_align_opts* opts;
  const int32_t* open_end_host;     /* [batch], nullable: row b's DTW is open-ended (wca_dtw_open) where open_end_host[b] != 0; a row with 0
                                       gets exactly the closed result. Everything upstream of the DTW is unchanged.                       */
  int64_t pcm_stride;
  int32_t n_tok_max;
  int32_t batch;
  int32_t vocab_end;                /* in (0, n_vocab] (= tokenizer.eot): also compute the teacher-token log-probs; 0: none. With them the
                                       decoder finishes its last layer and the n_text_b = n_tok[b] - sot_len - 2 text rows of every utterance
                                       go through the final LayerNorm, the vocabulary projection (tok_emb rows [0, vocab_end)) and a
                                       log-sum-exp kernel on the engine's second stream; the [rows][vocab] logits never reach the host. The
                                       jump frames and top-k heads are the same with and without them.                                   */
  int32_t path_scores;              /* != 0: also run the path-score kernel (wca_dtw_path_scores) behind the DTW, on the aggregated matrix
                                       the DTW was given; read with wca_align_batch_path_scores before the fetch. 0: nothing changes.     */
} wca_align_desc;

typedef struct {
  int32_t* jump_frame_host;   /* [batch][n_tok_max]: for utterance b, entries [0, n_tok[b] - sot_len - 1) are the frame index at which the
                                 DTW path enters that text row (jump_times * 50, timing.py:110-111); the remaining entries of a row are 0.
                                 Entries (end_row, n_tok[b] - sot_len - 1) of an open row are -1.                                        */
  int32_t* sel_idx_host;      /* [batch][topk], nullable: the selected heads                                                             */
  float* token_logprob_host;  /* [batch][n_tok_max] f32, nullable: entry i < n_text_b of row b is
                                 log_softmax(logits[b][sot_len + i][0 : vocab_end])[tokens[b][sot_len + 1 + i]], the rest 0; the prediction of
                                 eot is not scored, as in the reference. A teacher token >= vocab_end has no value: NaN, and the fetch returns
                                 WCA_ERR_INVALID.                                                                                        */
  int32_t* end_row_host;      /* [batch], nullable: the last text row of row b's path, counted in DTW rows, i.e. from the first token after
                                 the sot sequence: n_tok[b] - sot_len - 2 for a closed row; -1 where no DTW ran                           */
  float* score_host;          /* [batch], nullable: wca_dtw_open's score of the end cell                                                 */
} wca_align_result;

/* wca_align_batch_enqueue only enqueues the work on the engine stream (no host sync; results stay in the engine's pinned staging ring until
 * wca_align_batch_fetch). Up to TWO batches may be in flight: wca_align_batch_fetch returns the OLDEST pending one (waiting on its HIP event
 * only), so the host can post-process batch i while batch i+1 runs; batch, n_tok_max and topk must be those of that enqueue.
 * WCA_ERR_STATE (and nothing consumed) when token_logprob_host is given but the pending batch was enqueued with vocab_end = 0, or when
 * end_row_host / score_host are given but it was enqueued without open_end_host. wca_align_batch is the enqueue, then the fetch. */
int wca_align_batch_enqueue(wca_engine* e, const wca_align_desc* d);
int wca_align_batch_fetch(wca_engine* e, int batch, int n_tok_max, int topk, const wca_align_result* r);
int wca_align_batch(wca_engine* e, const wca_align_desc* d, const wca_align_result* r);
/* wca_align_batch_enqueue / wca_align_batch with row windows for the DTW (wca_dtw_windows); the entry points above are these with null
 * windows. row_lo_host / row_hi_host [batch][n_tok_max] int32 (row stride n_tok_max; both or neither), counted in DTW rows -- entry 0 of
 * row b belongs to the first token after the sot sequence and no_timestamps, entry n_tok[b] - sot_len - 2 to the eot, later entries are not
 * read -- and in encoder frames of that row's max_frames. They are checked on the host before anything is enqueued (WCA_ERR_INVALID, and
 * nothing is consumed), and a row with open_end_host[b] != 0 takes full windows [0, max_frames[b] - 1] only: one batch may mix open rows and
 * windowed closed ones. path_scores, vocab_end and open_end_host work as without windows; everything upstream of the DTW is unchanged. */
int wca_align_batch_enqueue_windows(wca_engine* e, const wca_align_desc* d, const int32_t* row_lo_host, const int32_t* row_hi_host);
int wca_align_batch_windows(wca_engine* e, const wca_align_desc* d, const int32_t* row_lo_host, const int32_t* row_hi_host,
                            const wca_align_result* r);
/* wca_align_batch_enqueue / wca_align_batch on the ALIGNMENT-HEADS route: openai-whisper's own word aligner (whisper/timing.py
 * find_alignment) in place of head statistics, top-k and aggregation. Phase 1, the teacher-forced decoder with its capture, the ragged DTW,
 * the fetch and the vocab_end log-probabilities are those of wca_align_batch_enqueue. Between them, for the n_heads heads of heads_host
 * (host, layer * n_text_head + head, 1 <= n_heads <= n_text_layer * n_text_head, each in [0, n_text_layer * n_text_head); summed in
 * the order given) and utterance b's
 * n_tok[b] x max_frames[b] corner of the captured logits: softmax over the frames of logits * qk_scale; per head and frame (w - mean) / std
 * over the n_tok[b] token rows (population std, a plain division: a constant column gives NaN, as upstream); the median filter of
 * medfilt_width along the frames (reflect padding; skipped where max_frames[b] <= medfilt_width / 2); the mean over the heads; rows
 * [sot_len, n_tok[b] - 1) go to the DTW, negated. Of d->opts only sot_len, medfilt_width and qk_scale are read. Refused with
 * WCA_ERR_INVALID before anything is enqueued or consumed: a head out of range, n_heads outside that range, d->path_scores != 0 (the score is defined on
 * the [0, 1] aggregation), d->open_end_host != NULL. The results are fetched with wca_align_batch_fetch(..., topk = 0, ...); sel_idx_host
 * is left untouched. */
int wca_align_batch_enqueue_heads(wca_engine* e, const wca_align_desc* d, const int32_t* heads_host, int n_heads);
int wca_align_batch_heads(wca_engine* e, const wca_align_desc* d, const int32_t* heads_host, int n_heads, const wca_align_result* r);
/* The path scores of the OLDEST pending batch, which must have been enqueued with path_scores != 0 (WCA_ERR_STATE otherwise, or when nothing
 * is pending): waits for that batch like the fetch, copies path_mean_host / path_cells_host [batch][n_tok_max] -- laid out like
 * jump_frame_host: entry i of row b belongs to DTW row i, 0 beyond the DTW's rows -- and does NOT consume the batch: the
 * wca_align_batch_fetch that follows does. */
int wca_align_batch_path_scores(wca_engine* e, int batch, int n_tok_max, float* path_mean_host, int32_t* path_cells_host);

/* The filter fields of whisper.DecodingOptions as the reference uses it (infer_ali.py:40: language="en", everything else default:
 * task transcribe, suppress_blank, suppress_tokens "-1", without_timestamps False, max_initial_timestamp 1.0). */
typedef struct {
  int32_t sample_len;                  /* upstream's sample_len (224 = n_text_ctx // 2), kept for the callers' bookkeeping: wca_decode takes
                                          every budget, the shared one of a per_row 0 call too, from sample_len_host and does not read it */
  int32_t eot;                         /* tokenizer.eot                                                       */
  int32_t timestamp_begin;             /* tokenizer.timestamp_begin (<|0.00|>)                                */
  int32_t apply_timestamp_rules;       /* 1 = ApplyTimestampRules (without_timestamps False)                  */
  int32_t max_initial_timestamp_index; /* round(max_initial_timestamp / 0.02) = 50; < 0 = no limit            */
  int32_t no_speech;                   /* tokenizer.no_speech (<|nospeech|>) for no_speech_prob; < 0 = skip   */
} wca_decode_opts;

/* Phase 1 alone (log-mel or a given mel -> encoder -> cross-attention K/V of every decoder layer), enqueued on the
 * engine stream without a host sync. The encoded state is queued: wca_decode without an input decodes
 * the oldest undecoded one, wca_align_batch_enqueue(pcm_dev = NULL) consumes the oldest one. Two K/V slots exist, so
 * the NEXT batch can be encoded while the current one is decoded and aligned (the decode loop and the alignment's
 * phase 2 run on the engine's second stream). */
int wca_encode_batch(wca_engine* e, const float* mel_dev, const float* pcm_dev, int64_t pcm_stride,
                     const int32_t* n_samples_host, int batch);

/* The ASR pre-pass for a micro-batch: whisper.decode at temperature 0 (greedy) or, per row, at a temperature. Pointers first, then 64-bit
 * fields, then 32-bit fields; a zero in an optional field means "off".
 *
 * Input and state. With mel_dev or pcm_dev the batch is encoded first; with neither, the oldest undecoded state of wca_encode_batch (or the
 * one wca_detect_language has read) is decoded. The encoder output and cross-attention K/V stay in the engine: the next
 * wca_align_batch_enqueue for the same batch may pass pcm_dev = NULL to re-use them (the reference runs the encoder twice, infer_ali.py:60
 * and timing.py:58). A state that was decoded but not aligned is dropped when the next wca_decode that is no redecode starts.
 *
 * Rows. Row b holds n_initial[b] initial tokens -- upstream's _get_initial_tokens: [sot_prev, prompt..., ] sot_sequence [, no_timestamps]
 * [, prefix...] -- with <|startoftranscript|> at sot_index[b] (0 without a prompt, 1 + prompt length with one), and samples at most
 * sample_len[b] tokens. The first sampled position, where SuppressBlank and the first-timestamp rules fire, is n_initial[b]. Bounds per row:
 * 1 <= n_initial <= n_text_ctx, sample_len >= 1 and n_initial + sample_len <= n_text_ctx + 1, else WCA_ERR_TOO_LONG (upstream samples until
 * the sequence is longer than n_text_ctx: the last token is sampled, never embedded, so no positional row past n_text_ctx - 1 is read; this
 * is the one length bound of every decode -- the tighter n_initial + sample_len <= n_text_ctx of ABI versions up to 16 belonged to one
 * entry point alone and left with it); 0 <= sot_index < n_initial and every initial token inside the vocabulary, else WCA_ERR_INVALID.
 *
 * Sampling (temperature_host and seed_host, given together; per_row 1 only). A row at temperature 0 is decoded greedily, bit for bit as
 * without the two arrays. A row at T > 0 is upstream's GreedyDecoder.update at temperature > 0: a draw from Categorical(logits = filtered
 * logits / T), sum_logprob accumulating the UNTEMPERED log-softmax of the filtered logits at the drawn token. It draws by Gumbel-max:
 * next = argmax_v (logit[v] * (1.0f / T) + G(v)) over the tokens its filters leave (the lowest index among equals; the "timestamp mass beats
 * every text token" rule is decided on the untempered logits), G(v) = -logf(-logf(u)), u = ((x >> 9) + 0.5) * 2^-23 in fp32, x = word v & 3 of
 * Philox4x32-10 with key (seed low word, seed high word) and counter (v >> 2, c, 0, 0), c = the number of tokens the row has sampled so far.
 * A row's draws therefore follow (seed, c, v, its logits) alone: not the batch row it sits in, not the other rows. The law is upstream's;
 * the draws are not torch's (another generator).
 *
 * Refused with WCA_ERR_INVALID before any work is enqueued: a null engine, descriptor or required field; both inputs given; batch outside
 * [1, max_batch]; per_row, prefill or redecode other than 0 or 1; per_row 0 with a temperature, a seed or redecode; per_row 1 with
 * prefill 0; only one of temperature_host and seed_host; redecode together with an input; a temperature that is negative or not finite.
 * Synchronous (returns with the tokens). wca_last_decode_positions reports the prefill's positions (n_initial, the largest with per_row 1,
 * or 0) and the number of single-position steps. */
typedef struct {
  const float* mel_dev;                /* [batch][n_mels][3000] f32, what whisper.decode takes; at most one of mel_dev / pcm_dev            */
  const float* pcm_dev;                /* [batch][pcm_stride] f32, log-mel computed on the device; needs n_samples_host [batch]             */
  const int32_t* n_samples_host;
  const int32_t* initial_tokens_host;  /* per_row 0: [n_initial]; per_row 1: [batch][n_initial_max], n_initial_max = max_b n_initial[b] (row
                                          b's first n_initial[b] entries count, the rest is ignored)                                       */
  const int32_t* n_initial_host;       /* these three: one entry (per_row 0) or [batch] (per_row 1)                                        */
  const int32_t* sot_index_host;
  const int32_t* sample_len_host;
  const float* temperature_host;       /* [batch] f32, nullable                                                                            */
  const uint64_t* seed_host;           /* [batch], nullable                                                                                */
  const uint8_t* suppress_mask_host;   /* [n_vocab] bytes: 1 = logit forced to -inf at every step (SuppressTokens list and, when the
                                          timestamp rules are on, <|notimestamps|>)                                                        */
  const uint8_t* blank_mask_host;      /* [n_vocab], nullable: 1 = -inf at the first sampled position (SuppressBlank: tokenizer.encode(" ")
                                          + [eot])                                                                                         */
  const wca_decode_opts* opts;
  int32_t* tokens_out_host;            /* [batch][T_max], T_max = max_b (n_initial[b] + sample_len[b]): row b left-aligned, its initial
                                          tokens, then its sampled tokens, eot from its first eot / its budget on                          */
  int32_t* n_tokens_host;              /* [batch]: index of row b's first sampled eot, at most n_initial[b] + sample_len[b]; its sampled
                                          tokens are tokens_out[b][n_initial[b] : n_tokens[b]]                                             */
  float* sum_logprob_host;             /* [batch], nullable: GreedyDecoder's sum of log-probabilities of the sampled tokens                */
  float* no_speech_prob_host;          /* [batch], nullable (needs opts->no_speech >= 0): softmax probability of <|nospeech|> at row b's
                                          sot_index (DecodingResult.no_speech_prob)                                                        */
  int64_t pcm_stride;
  int32_t batch;
  int32_t per_row;                     /* 0: one row description shared by every batch row (the row arrays have one entry), the scalar
                                          kernels run and `prefill` is honoured. 1: the row arrays have `batch` entries, the rows sit at
                                          different decoder positions, the table kernels run, always behind a prefill (rows padded to
                                          n_initial_max with eot; a valid position never attends to a pad), and opts->sample_len is ignored.
                                          A row's tokens do not depend on the other rows' lengths except through the GEMM path the row
                                          COUNT selects (fp32 summation order, as between prefill 0 and 1).                                */
  int32_t prefill;                     /* 0: the initial tokens go through the decoder one position at a time (one decode step each);
                                          1: one batched forward over all of them (causal self-attention, each layer's cross-K/V read
                                          once), upstream's first forward. The two agree up to f16 / fp32 summation order.                 */
  int32_t redecode;                    /* 1 (no input): decode AGAIN the newest state of `batch` rows that is already decoded and not yet
                                          aligned -- the one the previous decode left for wca_align_batch_enqueue(pcm_dev = NULL) --, with
                                          no encoder pass (the rungs of transcribe's temperature fallback ladder); WCA_ERR_STATE if there is
                                          none. Nothing is dropped from the queue and the state is still there for the alignment.          */
} wca_decode_desc;
int wca_decode(wca_engine* e, const wca_decode_desc* d);

/* Beam search and best_of: whisper.decode with DecodingOptions(beam_size=G [, patience]) at temperature 0, or with best_of=G at a
 * temperature. `rows` describes the `batch` audios exactly as for wca_decode (always with prefill = 1; per_row and redecode as there); its
 * four output pointers are not read and may be NULL. Every audio gets n_group decoder rows that share its cross-K/V, decoder row
 * r = b * n_group + g being beam / sample g of audio b, so batch * n_group <= max_batch. The audios go through one prefill; each audio's
 * cache rows and logits are then handed to its rows.
 *
 * mode 0, beam (upstream BeamSearchDecoder, restated; no temperatures): at every choice each live row offers the n_group + 1 most probable
 * tokens of the log-softmax of its FILTERED logits (the filters of wca_decode; the lowest token first among equal logits). The candidates
 * of an audio score sum_logprob[source] + logprob and are walked in the order (score descending, source beam ascending, token
 * ascending): a candidate that ends in eot is newly finished, the others become the next beams, and the walk stops at the n_group-th of
 * those. The newly finished ones join the audio's finished list, best first, while it holds fewer than max_candidates =
 * round(beam_size * patience) (computed by the caller). At the first choice only beam 0 offers candidates (the rows are still identical:
 * upstream's dedup of equal sequences, made deterministic). The self-attention cache rows follow the beams that continue them. The loop
 * stops when every audio's list is full or its budget is used (asked every 4 choices). Then upstream's finalize: a list with fewer than
 * n_group sequences is topped up from the live beams in descending order of sum_logprob (the lower beam among equals).
 * Slots per audio: n_slot = max(n_group, max_candidates) -- with patience > 1 the list may hold more than n_group sequences, and the
 * ranker sees all of them, as upstream's does.
 *
 * mode 1, independent samples (upstream's best_of; temperatures and seeds required): row (b, g) is wca_decode's sampling row at
 * temperature[b] with the seed group_seed(seed[b], g) = seed[b] ^ (g * 0x94D049BB133111EB) mod 2^64, so sample 0 is the plain sampled
 * decode of that seed. n_slot = n_group, slot g = sample g. Nothing selects across rows on the device: the ranking is the caller's.
 *
 * Refused with WCA_ERR_INVALID before any work is enqueued: what wca_decode refuses; a null engine, descriptor or required field;
 * prefill 0; batch * n_group > max_batch; n_group outside [1, 16]; mode 0 with temperatures or max_candidates outside [1, 4096]; mode 1
 * without temperatures. Synchronous. The encoded state stays for the alignment as after wca_decode. */
typedef struct {
  int32_t* tokens_out_host;    /* [batch][n_slot][T_max], T_max as wca_decode: a sequence's initial tokens, its sampled tokens, then eot */
  int32_t* n_tokens_host;      /* [batch][n_slot]: index of the sequence's closing eot (its sampled tokens are [n_initial[b], n_tokens)) */
  float* sum_logprob_host;     /* [batch][n_slot]                                                                                     */
  int32_t* n_out_host;         /* [batch]: how many of the n_slot slots hold a sequence (the first n_out; the others hold eot and 0)    */
  float* no_speech_prob_host;  /* [batch], nullable: as wca_decode, from the audios' <|sot|> rows                                       */
  int32_t n_group;             /* G >= 1                                                                                              */
  int32_t mode;                /* 0 = beam, 1 = independent samples                                                                   */
  int32_t max_candidates;      /* mode 0: round(beam_size * patience) >= 1                                                            */
} wca_group_desc;
int wca_decode_group(wca_engine* e, const wca_decode_desc* rows, const wca_group_desc* g);
/* Language identification, upstream's detect_language(model, mel): which of the language tokens [lang_begin, lang_begin + n_lang)
 * (tokenizer.all_language_tokens: sot + 1 ..., 99 or 100 of them; 1 <= n_lang <= 128) follows <|startoftranscript|> (`sot`) for each row.
 * mel_dev / pcm_dev / pcm_stride / n_samples_host / batch as for wca_decode: at most one input is non-NULL, with both NULL the oldest
 * undecoded state of wca_encode_batch is read. One decoder position (token sot at position 0, the first step of a wca_decode without prefill, f16
 * operands in both precision modes) and the language head: the final LayerNorm and the n_lang rows of the token embedding only, which is
 * upstream's softmax / argmax over logits whose other entries are masked to -inf.
 * lang_token_host [batch] int32: the most probable language token (absolute id; the lowest id among equal logits);
 * probs_host [batch][n_lang] f32: the softmax over the language tokens, entry j for token lang_begin + j.
 * The encoded state stays queued and UNDECODED: a following wca_decode with mel_dev = pcm_dev = NULL decodes it with no second
 * encoder pass (upstream encodes the first window twice), and wca_align_batch_enqueue(pcm_dev = NULL) may consume it. A wca_decode or
 * wca_detect_language that brings an input of its own drops it, as does wca_align_batch_enqueue with a pcm_dev. Synchronous.
 * WCA_ERR_INVALID: null engine / output pointers, both inputs given, batch outside [1, max_batch], sot or the language range outside the
 * vocabulary; WCA_ERR_STATE: no input and no undecoded state of `batch` rows. */
int wca_detect_language(wca_engine* e, const float* mel_dev, const float* pcm_dev, int64_t pcm_stride, const int32_t* n_samples_host,
                        int batch, int sot, int lang_begin, int n_lang, int32_t* lang_token_host, float* probs_host);
/* positions per row that the last wca_decode fed through the batched prefill (n_initial, or 0) and one position at a
 * time (decode steps, the sampling steps after the first included) */
int wca_last_decode_positions(wca_engine* e, int32_t* prefill_positions, int32_t* step_positions);

/* The log-sum-exp kernel of the alignment's token log-probs on caller-supplied logits (timing.py:146-149 on the logits wca_get_attentions returns): logits_dev [rows][ld]
 * f32 (ld >= vocab_end), targets_dev [rows] int64, out_dev [rows] f32 = log_softmax(logits[r][0 : vocab_end])[targets[r]]. Synchronous
 * on the engine stream; a target outside [0, vocab_end) gives NaN there and WCA_ERR_INVALID. */
int wca_token_logprobs(wca_engine* e, const float* logits_dev, int rows, int ld, int vocab_end, const int64_t* targets_dev,
                       float* out_dev);

/* ---- audio I/O on the host (no GPU work, no engine): dataset.py:31,104 read the corpora through torchaudio.load; the
 * LibriSpeech originals are FLAC. buf = the whole .flac file in memory.
 * wca_flac_decode: out [channels][capacity_per_channel] f32 in [-1, 1) (sample / 2^(bits-1), torchaudio's
 * normalisation); out == NULL only counts (*n_decoded = samples per channel: streams whose STREAMINFO has no total).
 * CRC-8 / CRC-16 of every frame are verified; WCA_ERR_INVALID on a malformed / unsupported stream. */
int wca_flac_info(const uint8_t* buf, int64_t nbytes, int32_t* sample_rate, int32_t* channels, int32_t* bits_per_sample,
                  int64_t* total_samples);
int wca_flac_decode(const uint8_t* buf, int64_t nbytes, float* out, int64_t capacity_per_channel, int64_t* n_decoded);

/* ---- collation of the per-rank results over RCCL -----------------------------------------------------
 * The reference is single-process: infer_ali.py:53-56,118-132 accumulates every utterance's result in one dict and three
 * counters. Here utterances shard over one process per GPU; at the end every rank hands its packed records
 * ([utt_index:int32][n:int32][starts:f64 x n][ends:f64 x n] ..., shard.pack_results) to wca_allgather_results: an all-gather
 * of the byte counts, then ONE all-gather of the buffers padded to the largest count (ncclAllGather over xGMI), and
 * wca_allreduce_counters sums the evaluation counters. librccl is resolved at first use (dlopen; the copy already in the
 * process if there is one). The 128-byte unique id is created on rank 0 and reaches the other ranks by the launcher's own
 * side channel (a file, MPI, the torch.distributed store ...). One communicator per engine, on the engine's device and
 * stream. The Python CLI / bench.py collate through torch.distributed (backend "nccl" = the same RCCL) by default;
 * shard.allgather_results(..., engine=model) takes this path. */
#define WCA_COMM_ID_BYTES 128
int wca_comm_unique_id(uint8_t* id_out /* [WCA_COMM_ID_BYTES] */);
int wca_comm_init(wca_engine* e, const uint8_t* id /* [WCA_COMM_ID_BYTES] */, int rank, int world);
int wca_comm_destroy(wca_engine* e);
/* gathered_host [world][capacity_per_rank]: rank r's sizes_host[r] bytes start at r * capacity_per_rank. The first collective
 * gathers every rank's {n_bytes, capacity_per_rank}; WCA_ERR_TOO_LONG is returned ON EVERY RANK ALIKE when the largest n_bytes
 * exceeds the SMALLEST capacity any rank passed (the decision is wca_collate_plan on the gathered pairs, so all ranks issue the
 * same sequence of collectives whatever their own capacity); sizes_host is filled: retry with max(sizes_host) everywhere. */
int wca_allgather_results(wca_engine* e, const uint8_t* packed_host, int64_t n_bytes, uint8_t* gathered_host,
                          int64_t capacity_per_rank, int64_t* sizes_host /* [world] */);
int wca_allreduce_counters(wca_engine* e, int64_t* counters_host /* [n], summed in place */, int n);
/* The fit decision of wca_allgather_results as a pure host function (no GPU, no communicator): WCA_OK and *pad_out = the padded
 * per-rank payload when max(sizes) <= min(capacities), else WCA_ERR_TOO_LONG (pad_out still set). Exported for the protocol tests. */
int wca_collate_plan(const int64_t* sizes /* [world] */, const int64_t* capacities /* [world] */, int world, int64_t* pad_out);

/* ---- kernel-level entry points (used by the parity tests and by bench.py's roofline leg) -------- */
/* C[m][n] = sum_k A[m][k] W[n][k] (+bias) ; A,W f16 device. out_mode low byte: 0 f16 store, 1 f32 store,
 * 2 f32 accumulate, 4 f16 PAIR store (split mode: c_dev is f16 [M][2N], hi = f16(v) at column n, lo = f16(v - hi) at column
 * N + n; GELU is then the erff form); out_mode >> 8: force the tile shape (0 auto, 128, 256). A split-mode GEMM is this call
 * with A = [A_hi | A_lo] ([M][2K]), W = [W | W] ([N][2K]) and K = 2K. */
int wca_test_gemm(wca_engine* e, const void* a_f16_dev, const void* w_f16_dev, const float* bias_dev, void* c_dev, int M,
                  int N, int K, int gelu, int out_mode);
/* The pair product with the W K-tiles staged ONCE (persistent 256 x 256 kernel, SPLITW form): a2 = [A_hi | A_lo] ([M][2K] f16),
 * w = the PLAIN [N][K] matrix, K the algorithmic depth. out_mode as above (0, 1, 2, 4; >> 8: 0 auto, 257, 258).
 * WCA_ERR_INVALID where that kernel does not apply (fewer than 192 256 x 256 tiles, K % 128 != 0): the engine then multiplies
 * the K-doubled operands through wca_test_gemm's path. */
int wca_test_gemm_pairs(wca_engine* e, const void* a2_f16_dev, const void* w_f16_dev, const float* bias_dev, void* c_dev, int M,
                        int N, int K, int gelu, int out_mode);
/* x (f32 [M][N], read-modify-write) += A W^T + bias; xn (f16 [M][N]) = LayerNorm(x; gamma, beta, eps 1e-5): the residual
 * GEMMs of an encoder block with the LayerNorm in their epilogue (gemm_epilogue.h). site 1 / 4 = the out-projection's /
 * fc2's kernel symbol. WCA_ERR_INVALID where the fused form does not apply (N % 256, K % 128, fewer than 192 tiles). */
int wca_test_gemm_ln(wca_engine* e, const void* a_f16_dev, const void* w_f16_dev, const float* bias_dev, float* x_dev,
                     const float* gamma_dev, const float* beta_dev, void* xn_f16_dev, int M, int N, int K, int site);
/* What launch_gemm would do with a GEMM C [M][N] = A [M][K] (rows lda apart) W [N][K]^T on a device of n_cu compute units (csrc/gemm_plan.cpp,
 * plan_gemm): no engine, no GPU, no HIP call. out_mode, gelu, site as GemmArgs; a_lo > 0 = pair operands; force_tile 0 auto / 64 / 128 / 256 /
 * 257 / 258 (GemmForceTile); cu_limit > 0 = a cap on the persistent grid, for tests. flags: 1 an addend, 2 batch-strided A, 4 a positional table, 8 batch-strided
 * C, 16 out_mode 3 WITHOUT its LayerNorm buffers, 32 out_mode 4 WITHOUT c_lo; sk_bytes > 0 = a split-K workspace of that size.
 * WCA_OK and out[10] = {kernel, grid x, grid y, workgroup size, dynamic LDS, splitk, supertile, site instance, a_bytes, w_bytes} with kernel
 * 0 nothing to launch, 1 skinny, 2 128 x 128, 3 256 x 256, 4 persistent 256 x 256, 5 / 6 its pair forms on two-slot rings / three A slots,
 * 7 its residual + LayerNorm form; WCA_ERR_INVALID (reason in wca_last_error) where launch_gemm returns hipErrorInvalidValue. */
int wca_test_gemm_plan(int M, int N, int K, int lda, int out_mode, int gelu, int a_lo, int force_tile, int site, int n_cu, int cu_limit, int flags,
                       int64_t sk_bytes, int32_t* out);
/* wca_test_gemm with every field of the launch description open to the caller -- the strided and batch-strided forms the engine's forward
 * builds (csrc/engine_forward.hip: the conv stem's overlapping windows, the positional table, the pre-activation addend, pair rows,
 * a capped persistent grid). Logical row m = b * rows_per_batch + t of A / C lives at base + b * batch_stride + t * ld (rows_per_batch 0: flat,
 * m * ld); a_lo > 0: A rows are [hi | lo] pairs a_lo elements apart against the plain W; c_lo: out_mode 4's distance from hi to lo;
 * addend [M][ld_addend] f32 is added before the GELU, pos [pos_period][N] f32 after it (row m takes pos[m % pos_period]); force_tile 0 / 64 /
 * 128 / 256 / 257 / 258 and out_mode 0 / 1 / 2 / 3 / 4 as wca_test_gemm_plan. plan_out[2] = {kernel (numbered as in wca_test_gemm_plan), grid x} of
 * the launch. A launch the plan refuses is WCA_ERR_INVALID with the plan's reason and writes nothing. Asynchronous on the engine's stream
 * (out_mode 3 waits for the launch). */
typedef struct wca_test_gemm_desc {
  const void* a;
  const void* w;
  const float* bias;    /* nullable */
  void* c;
  const float* addend;  /* nullable */
  const float* pos;     /* nullable */
  int64_t a_batch_stride, c_batch_stride, a_lo, c_lo;
  int32_t M, N, K;
  int32_t lda, ldw, ldc;
  int32_t a_rows_per_batch, c_rows_per_batch;
  int32_t ld_addend, pos_period;
  int32_t gelu, out_mode, force_tile, site, cu_limit, supertile;
  /* out_mode 3 (c is then x, f32 [M][ldc], read-modify-write): ln_out f16 rows ln_ld apart = LayerNorm(x; ln_gamma, ln_beta, eps 1e-5). The call
   * supplies the statistics workspace and the zeroed error word, waits for the launch and reports a statistics hand-off that timed out. */
  const float* ln_gamma;
  const float* ln_beta;
  void* ln_out;
  int32_t ln_ld;
} wca_test_gemm_desc;
int wca_test_gemm_ex(wca_engine* e, const wca_test_gemm_desc* desc, int32_t* plan_out);
/* wca_test_attention / _split / _rows with every stride open to the caller (element strides; head h of a row at column h * 64; base offsets are
 * applied by the caller to the pointers): split != 0 = pair operands, the lo half of an element *_lo elements after its hi half;
 * cap [b * cap_bs + h * cap_hs + q * cap_ld + key] f32 for key < cap_cols, or NULL; nk_rows device [B] int32 or NULL (one-query f16 form only);
 * causal 0 / 1; variant 0 auto / 1 / 2 as wca_test_attention. Scale 1/8. Asynchronous on the engine's stream. */
typedef struct wca_test_attn_desc {
  const void* q;
  const void* k;
  const void* v;
  void* o;
  float* cap;               /* nullable */
  const int32_t* nk_rows;   /* nullable */
  int64_t q_bs, k_bs, v_bs, o_bs;
  int64_t q_lo, k_lo, v_lo, o_lo;
  int64_t cap_bs, cap_hs;
  int32_t q_rs, k_rs, v_rs, o_rs;
  int32_t cap_ld, cap_cols;
  int32_t split, B, H, nq, nk, causal, variant;
} wca_test_attn_desc;
int wca_test_attention_ex(wca_engine* e, const wca_test_attn_desc* desc);
/* The few-row GEMM of the greedy-decode steps (gemm_rows.hip): C [M][N] = epilogue(A W^T + bias) with A = a_f16_dev [M][K] or,
 * when x_f32_dev != NULL, A = LayerNorm(x_f32_dev [M][K]; gamma, beta, eps 1e-5) computed in the kernel's prologue.
 * out_mode as wca_test_gemm; splitk 0 = smallest split with K / splitk <= 1024, groups 0 = chosen; kv_k / kv_v != NULL
 * (out_mode 0, N = 3 d): columns [d, 3d) go to the caches [M][T_max][d] at position kv_t instead of C. */
int wca_test_gemm_rows(wca_engine* e, const void* a_f16_dev, const float* x_f32_dev, const float* gamma_dev, const float* beta_dev,
                       const void* w_f16_dev, const float* bias_dev, void* c_dev, int M, int N, int K, int gelu, int out_mode, int splitk,
                       int groups, void* kv_k_f16_dev, void* kv_v_f16_dev, int T_max, int kv_t);
/* wca_test_gemm_rows with every field launch_gemm_rows accepts open to the caller (element strides; base offsets are applied by the caller to
 * the pointers). a [M] f16 rows lda apart, or, x != NULL, A = LayerNorm(x rows lda32 floats apart; gamma, beta, eps 1e-5); w [N] rows ldw apart;
 * logical row m of C at c + m * ldc, or, c_rows_per_batch > 0, at c + (m / rows_per_batch) * c_batch_stride + (m % rows_per_batch) * ldc;
 * out_mode 0 f16 / 1 f32 / 2 f32 accumulate; splitk 0 = chosen, groups 0 = chosen; kv_k / kv_v != NULL (out_mode 0, N = 3 d): columns [d, 3d)
 * of row m go to the caches [M][kv_tmax][d] at position kv_t, or, kv_t_rows != NULL (device [M] int32), at kv_t_rows[m] clamped to
 * [0, kv_tmax). The split-K workspace is the engine's scratch; after a split launch the arrival counters must be back at zero
 * (WCA_ERR_HIP otherwise). A launch the launcher refuses is WCA_ERR_INVALID and writes nothing. Returns after the launch has finished. */
typedef struct wca_test_gemm_rows_desc {
  const void* a;              /* nullable when x is given */
  const float* x;             /* nullable */
  const float* gamma;
  const float* beta;
  const void* w;
  const float* bias;          /* nullable */
  void* c;
  void* kv_k;                 /* nullable */
  void* kv_v;
  const int32_t* kv_t_rows;   /* nullable */
  int64_t c_batch_stride;
  int32_t M, N, K;
  int32_t lda, lda32, ldw, ldc;
  int32_t c_rows_per_batch;
  int32_t gelu, out_mode, splitk, groups;
  int32_t kv_tmax, kv_t;
} wca_test_gemm_rows_desc;
int wca_test_gemm_rows_ex(wca_engine* e, const wca_test_gemm_rows_desc* desc);
/* Which path the engine of a model n_text_state wide gives a decoder GEMM C [M][N] = A [M][K] W^T (csrc/gemm_plan.cpp, plan_dec_gemm, the
 * decision of dec_gemm with the few-row kernel enabled): no engine, no GPU, no HIP call. layernorm != 0: A is LayerNorm of the f32 rows;
 * kv_append != 0: the QKV projection of a decode step. out[8] = {few_row (0: the separate LayerNorm / GEMM / kv_append launches, and zeros
 * up to the capacity), splitk, column groups per workgroup, grid x, grid y, dynamic LDS bytes, split-K workspace bytes of the launch,
 * bytes of the engine's split-K workspace}. */
int wca_test_dec_gemm_plan(int n_text_state, int M, int N, int K, int layernorm, int kv_append, int64_t* out);
/* diagnostic, process-wide (the product never calls it; 0 = the contract's three passes per product): leave single MFMA passes out of the
 * encoder's pair attention -- bit 0 K_lo Q_hi, bit 1 K_hi Q_lo, bit 2 V_lo P_hi, bit 3 V_hi P_lo; masks 0, 1, 2, 3, 4, 8, 9, 12, 15 exist.
 * tools/precision_ablation.py --attn-drop: the product-level ablation of timing.py:58's fp32 attention. */
int wca_test_set_attn_split_drop(int mask);
/* test switches of the library, process-wide (csrc/debug_switch.cpp; every switch starts at 0, the shipped choice, and the product never calls
 * this): "attn_split_variant" (1: pair attention on the 16x16x32 kernel everywhere), "head_stats_general" (1: the general head-statistics
 * kernel), "fail_precision_alloc" (1: the next precision switch fails its allocation: the roll-back test), "attn_split_drop" (as
 * wca_test_set_attn_split_drop), "gemm_ring" (1: the pair GEMM on round 4's two-slot rings). No environment variable sets them. */
int wca_test_set_switch(const char* name, int value);
/* the [batch][n_text_layer * n_text_head] head selection scores (timing.py:13-43) of the LAST fused batch, after it was fetched (no batch in
 * flight): tools/precision_ablation.py compares them with the oracle's */
int wca_test_last_scores(wca_engine* e, int batch, float* scores_host);
/* Phase 2's post-processing of wca_align_batch_enqueue on caller-supplied logits (kernel parity test, tests/postproc_ref.py): the metadata
 * staging, the head statistics on logits with the per-row (max, sum) kept, the top-k, the aggregation that re-materialises the selected
 * heads, and the ragged DTW -- the very functions the fused path calls, on the engine's stream, then the copies and one synchronisation.
 * No weights are needed. qk_dev [B][L*H][n_tok_max][ld] f32 with ld >= the largest n_frames[b]; utterance b's n_tok[b] x n_frames[b]
 * corner counts. B in [1, max_batch], lengths as wca_align_desc's (n_tok[b] in [0, n_tok_max], n_frames[b] in [1, 1500]), options as
 * wca_align_batch_enqueue checks them; anything else is WCA_ERR_INVALID / WCA_ERR_TOO_LONG. Every host output is nullable; F = n_frames_max,
 * k = opts->topk: scores [B][L*H], colnorm [B][L*H][F], rowstats [B][L*H][n_tok_max][2] = (max, sum) -- rows [n_tok[b],
 * n_tok_max) of an utterance are not written by this call --, sel_idx [B][k] (top-k only), matrix [B][n_tok_max][F] (rows
 * [0, n_tok[b] - sot_len - 1) x columns [0, n_frames[b]) of utterance b are written by this call), jump [B][n_tok_max] as
 * wca_align_result.jump_frame_host. */
typedef struct {
  const float* qk_dev;
  const int32_t* n_tok_host;
  const int32_t* n_frames_host;
  const int32_t* open_end_host;     /* [B], nullable: as wca_align_desc.open_end_host */
  const wca_align_opts* opts;
  float* scores_host;
  float* colnorm_host;
  float* rowstats_host;
  int32_t* sel_idx_host;
  float* matrix_host;
  int32_t* jump_host;
  int32_t B, L, H, n_tok_max, ld, n_frames_max;   /* n_frames_max: F of the output layouts, largest n_frames[b] <= F <= min(ld, 1500) */
} wca_test_postproc_desc;
int wca_test_align_postproc(wca_engine* e, const wca_test_postproc_desc* desc);
/* wca_test_align_postproc with the path-score kernel behind the DTW, as wca_align_desc.path_scores asks for it (the same function of the
 * fused path): path_mean_host / path_cells_host [B][n_tok_max], laid out like jump_host, both required. */
int wca_test_align_postproc_scores(wca_engine* e, const wca_test_postproc_desc* desc, float* path_mean_host, int32_t* path_cells_host);
/* wca_test_align_postproc's sibling for the alignment-heads route (kernel parity test, tests/align_heads_ref.py): the metadata staging, the
 * three passes of align_heads.hip over the S = n_heads heads of heads_host and the ragged DTW -- the very functions
 * wca_align_batch_enqueue_heads calls, on the engine's stream, then the copies and one synchronisation. No weights are needed. qk_dev, the
 * lengths and B, L, H, n_tok_max, ld, n_frames_max as wca_test_postproc_desc's; of opts only sot_len, medfilt_width and qk_scale are read;
 * heads as wca_align_batch_enqueue_heads checks them. Every host output is nullable; F = n_frames_max: rowstats [B][S][n_tok_max][2] =
 * (max, sum), colstats [B][S][F][2] = (mean, std), matrix [B][n_tok_max][F], jump [B][n_tok_max]. The whole device buffers are copied: only
 * utterance b's own corner of an array is DEFINED (rows [0, n_tok[b]) of rowstats, columns [0, n_frames[b]) of colstats, rows
 * [0, n_tok[b] - sot_len - 1) x columns [0, n_frames[b]) of matrix), the rest holds what a recycled workspace held; the jump rows are whole,
 * 0 past the DTW's rows. */
typedef struct {
  const float* qk_dev;
  const int32_t* n_tok_host;
  const int32_t* n_frames_host;
  const int32_t* heads_host;
  const wca_align_opts* opts;
  float* rowstats_host;
  float* colstats_host;
  float* matrix_host;
  int32_t* jump_host;
  int32_t B, L, H, n_tok_max, ld, n_frames_max, n_heads;
} wca_test_heads_postproc_desc;
int wca_test_align_heads_postproc(wca_engine* e, const wca_test_heads_postproc_desc* desc);
/* the first `count` floats of the column norms [B][L*H][F] that the LAST head-statistics launch on the engine's stream left (after
 * wca_force_align on one utterance: [L*H][F]); reads only, launches nothing */
int wca_test_last_colnorm(wca_engine* e, int64_t count, float* colnorm_host);
/* what the LAST wca_decode call left on the device, after a synchronisation of the decode stream (reads only, launches nothing):
 * logits_host [logits_rows][n_vocab] f32 -- the rows of the last forward, [batch] of them, or [2 batch] after a prefill with no_speech
 * (rows [batch, 2 batch): the <|sot|> position's, which the steps behind the prefill leave alone) -- and cache_f16_host, the self-attention
 * cache [n_text_layer][2][batch][T_max][n_text_state] f16 with T_max = the largest n_initial + sample_len of that call. batch and T_max
 * must be that call's (WCA_ERR_STATE otherwise, also after wca_detect_language, which overwrites the cache); more logits rows than the
 * call left are WCA_ERR_INVALID. */
int wca_test_decode_state(wca_engine* e, int batch, int T_max, int logits_rows, float* logits_host, void* cache_f16_host);
/* One beam step of wca_decode_group (mode 0) on caller-supplied logits and token rows: the per-row candidates, then the per-audio merge
 * (kernel parity test, tests/beam_ref.py). R = batch * n_group decoder rows, all arrays on the device: logits [R][n_vocab] f32;
 * tokens_in / tokens_out [R][T_max] int32, two buffers; cur_len / n_initial / cap [R] int32 (the rows of a group hold equal values; an
 * audio with cur_len - n_initial >= cap is past its budget and copied through); sum_logprob [R] f32, updated in place; src [R] int32;
 * cand_tok [R][n_group + 1] int32 and cand_lp likewise f32 (the candidates, token -1 at -inf where the filters leave fewer); the finished
 * lists fin_n [batch], fin_len / fin_sum [batch][max_candidates], fin_tok [batch][max_candidates][T_max], appended to; trace [R][2] int32 =
 * (source row, token); n_done [1] int32, incremented once per audio whose list is full after the step or that is past its budget.
 * first != 0: only beam 0 of a group offers candidates. Asynchronous on the engine's stream. */
typedef struct {
  const float* logits_dev;
  const int32_t* tokens_in_dev;
  int32_t* tokens_out_dev;
  const int32_t* cur_len_dev;
  const int32_t* n_initial_dev;
  const int32_t* cap_dev;
  const uint8_t* suppress_mask_dev;
  const uint8_t* blank_mask_dev;   /* nullable */
  const wca_decode_opts* opts;
  float* sum_logprob_dev;
  int32_t* src_dev;
  int32_t* cand_tok_dev;
  float* cand_lp_dev;
  int32_t* fin_n_dev;
  int32_t* fin_len_dev;
  float* fin_sum_dev;
  int32_t* fin_tok_dev;
  int32_t* trace_dev;
  int32_t* n_done_dev;
  int32_t batch;
  int32_t n_group;
  int32_t n_vocab;
  int32_t T_max;
  int32_t first;
  int32_t max_candidates;
} wca_test_beam_desc;
int wca_test_beam_step(wca_engine* e, const wca_test_beam_desc* desc);
/* The cache reorder of wca_decode_group alone: for every plane p < n_planes and row r < rows_dst,
 * dst[p][r][0 : n_keep[r]] = src[p][s][0 : n_keep[r]] with s = src_idx_dev[r], or r / div where src_idx_dev is NULL (the broadcast of an
 * audio's prefill to its group). src_dev [n_planes][rows_src][T_max][d] f16, dst_dev [n_planes][rows_dst][T_max][d] f16, two buffers;
 * n_keep_dev [rows_dst] int32 (clamped to [0, T_max]); s is clamped to [0, rows_src); d % 8 == 0. Asynchronous on the engine's stream. */
int wca_test_kv_reorder(wca_engine* e, const void* src_dev, void* dst_dev, int n_planes, int rows_src, int rows_dst, int T_max, int d,
                        const int32_t* src_idx_dev, int div, const int32_t* n_keep_dev);
/* What the LAST wca_decode_group in beam mode chose (reads only): trace_host [steps][rows][2] int32, entry (c, r) = (the row whose beam
 * row r continues after choice c, the token it appended; -1 for a row past its budget). *steps_out / *rows_out (set first, so a call with
 * trace_host = NULL asks for the sizes) = the choices made and batch * n_group; WCA_ERR_STATE if there was no such call, WCA_ERR_INVALID if
 * cap_entries < steps * rows * 2. */
int wca_test_beam_trace(wca_engine* e, int32_t* steps_out, int32_t* rows_out, int32_t* trace_host, int64_t cap_entries);
/* q,k,v [B][n][H*64] f16 device -> o [B][nq][H*64] f16; cap_dev [B][H][nq][cap_ld] f32 or NULL.
 * causal: bit 0 = causal mask; bits 8-9 = kernel variant (0 auto, 1 the 16x16x32-MFMA kernel, 2 the 32x32x16-MFMA
 * kernel that serves the encoder's un-masked self-attention = what auto picks; 3 is WCA_ERR_INVALID) */
int wca_test_attention(wca_engine* e, const void* q_dev, const void* k_dev, const void* v_dev, void* o_dev,
                       float* cap_dev, int cap_ld, int cap_cols, int B, int H, int nq, int nk, int causal);
/* split-mode attention (attention_split.hip): q2,k2,v2 [B][n][2*H*64] f16 rows [hi(H*64) | lo(H*64)] -> o2 [B][nq][2*H*64]
 * likewise; cap_dev as above (the three-pass fp32 logits times scale). causal: bit 0 only. */
int wca_test_attention_split(wca_engine* e, const void* q2_dev, const void* k2_dev, const void* v2_dev, void* o2_dev,
                             float* cap_dev, int cap_ld, int cap_cols, int B, int H, int nq, int nk, int causal);
/* the language head alone (kernel parity test): x_dev [B][n_text_state] f32 rows against the engine's loaded decoder.ln and
 * token_embedding -> probs_dev [B][n_lang] f32, lang_token_dev [B] int32, on the engine's stream (asynchronous) */
int wca_test_language_head(wca_engine* e, const float* x_dev, int B, int lang_begin, int n_lang, float* probs_dev, int32_t* lang_token_dev);
/* one step of the greedy decoder's filters + update on caller-supplied logits (kernel parity test) */
int wca_test_decode_select(wca_engine* e, const float* logits_dev, int batch, int n_vocab, int32_t* tokens_dev, int T_max,
                           int cur_len, int n_initial, const uint8_t* suppress_mask_dev, const uint8_t* blank_mask_dev,
                           const wca_decode_opts* opts, float* sum_logprob_dev, int32_t* n_done_dev);
/* the per-row form of that step (wca_decode with per_row 1): cur_len_dev / n_initial_dev / cap_dev [batch] int32 device arrays; row b holds
 * cur_len[b] tokens of which n_initial[b] are initial, and is a finished row (eot, nothing added to sum_logprob) once
 * cur_len[b] - n_initial[b] >= cap[b]; n_done_dev [n_done_len]: entry n_done_idx counts the rows whose new token is eot */
int wca_test_decode_select_rows(wca_engine* e, const float* logits_dev, int batch, int n_vocab, int32_t* tokens_dev, int T_max,
                                const int32_t* cur_len_dev, const int32_t* n_initial_dev, const int32_t* cap_dev, int n_done_idx,
                                int n_done_len, const uint8_t* suppress_mask_dev, const uint8_t* blank_mask_dev,
                                const wca_decode_opts* opts, float* sum_logprob_dev, int32_t* n_done_dev);
/* that step in its sampling form (wca_decode with temperature_host / seed_host): temperature_dev [batch] f32 and seed_dev [batch] uint64 device arrays; row b
 * draws with the counter cur_len[b] - n_initial[b] and, at temperature 0, takes the argmax exactly as wca_test_decode_select_rows does */
int wca_test_decode_sample_rows(wca_engine* e, const float* logits_dev, int batch, int n_vocab, int32_t* tokens_dev, int T_max,
                                const int32_t* cur_len_dev, const int32_t* n_initial_dev, const int32_t* cap_dev, int n_done_idx,
                                int n_done_len, const uint8_t* suppress_mask_dev, const uint8_t* blank_mask_dev,
                                const wca_decode_opts* opts, float* sum_logprob_dev, int32_t* n_done_dev,
                                const float* temperature_dev, const uint64_t* seed_dev);
/* wca_test_attention (no capture) with per-row key counts: q [B][nq][H*64], k / v [B][nk][H*64] f16, batch row b attends to keys
 * [0, nk_rows_dev[b]) (int32 device, clamped to [1, nk]). Only nq = 1 without a mask exists (the decode step's one-query kernel):
 * anything else is WCA_ERR_INVALID. Row b equals a B = 1 wca_test_attention call with nk = nk_rows[b], bit for bit. */
int wca_test_attention_rows(wca_engine* e, const void* q_dev, const void* k_dev, const void* v_dev, void* o_dev, int B, int H, int nq,
                            int nk, const int32_t* nk_rows_dev, int causal);
int wca_test_layernorm(wca_engine* e, const float* x_dev, const float* g_dev, const float* b_dev, void* out_f16_dev,
                       int rows, int d);
/* split-mode LayerNorm: out2 f16 [rows][2d], hi = f16(y) at column c, lo = f16(y - hi) at column d + c */
int wca_test_layernorm_split(wca_engine* e, const float* x_dev, const float* g_dev, const float* b_dev, void* out2_f16_dev,
                             int rows, int d);
/* encoder only: mel_dev [batch][n_mels][3000] f32 -> xa_out_dev [batch][1500][d] f32 (ln_post output) */
int wca_test_encoder(wca_engine* e, const float* mel_dev, int batch, float* xa_out_dev);

/* timing of the last wca_align_batch* call, milliseconds per stage measured with HIP events on the
 * engine stream: [0] log-mel, [1] encoder, [2] cross K/V projection, [3] decoder, [4] head stats,
 * [5] top-k + aggregate, [6] DTW, [7] total. Valid after a synchronize/fetch. */
int wca_last_stage_ms(wca_engine* e, float* ms8);
/* Per-kernel timing of the encoder layers in the last wca_align_batch* call (profiling enabled): HIP-event pairs around
 * every launch of one kernel site, on the stream the kernel runs on. n_launches = encoder layers; flops / bytes = the
 * ALGORITHMIC work of one launch at the last batch size (M = batch * 1500 rows; bytes: operands read once, outputs
 * written once, f32 residual read + written for the two read-modify-write GEMMs). */
enum {
  WCA_SITE_QKV = 0,   /* encoder self-attention q/k/v projection   gemm256p<0,false,1>  N = 3d, K = d   */
  WCA_SITE_ATTN = 1,  /* encoder self-attention (flash)            attn32_kernel<false>                 */
  WCA_SITE_OUT = 2,   /* attention out-projection + residual: gemm256p<2,false,1> alone (or the fused gemm256p<3,..> + mlp_ln)  */
  WCA_SITE_FC1 = 3,   /* MLP fc1 + GELU                            gemm256p<0,true,1>   N = 4d, K = d   */
  WCA_SITE_FC2 = 4,   /* MLP fc2 + residual: gemm256p<2,false,4> alone (or fused with the next attn_ln / ln_post)                */
  WCA_SITE_LN1 = 5,   /* attn_ln launches (slot li = the layer they feed; slot n_layer = ln_post)                                */
  WCA_SITE_LN2 = 6,   /* mlp_ln launches                                                                                         */
  WCA_N_SITES = 7
};
int wca_last_kernel_ms(wca_engine* e, int site, int* n_launches, float* total_ms, double* flops_per_launch,
                       double* bytes_per_launch);
/* on: the encoder's LayerNorms run in the epilogue of the GEMM that produces their input (attention out-projection ->
 * mlp_ln, fc2 -> the next layer's attn_ln / ln_post) where the shape allows it (>= 192 tiles, N % 256 == 0; otherwise, and
 * always in split mode, the separate launches); off (default): separate LayerNorm launches everywhere. Results agree up to
 * fp32 rounding of the row statistics (a last-bit difference of a few f16 outputs per thousand). Measured at the bench
 * configuration: -0.15 ms per encoder layer at kernel level, +0.9 % end to end; bench.py turns it on.
 * REQUIRES THE GPU TO ITSELF: the N / 256 workgroups of a 256-row panel wait for each other inside the launch, so all of them
 * must be resident together. Kernels of the same engine never prevent that for long (they are short and finite), but a second
 * process or engine running the same kind of launch on the device can hold the CUs its siblings need: the spin is bounded
 * (seconds) and the batch then fails with WCA_ERR_HIP instead of hanging (observed with two bench ranks sharing one GPU). */
int wca_set_fuse_ln(wca_engine* e, int on);
/* Arithmetic of the model forward (reference: timing.py:58, `model(mel.unsqueeze(0), tokens.unsqueeze(0))` -- an fp32
 * forward of a checkpoint whose weights are f16 at rest):
 *   WCA_PRECISION_F16 (opt-in since round 5: wca_engine_create_ex / wca_set_precision): GEMM / attention operands are rounded to f16 once (11 significant bits), accumulation,
 *     residual stream, LayerNorm, softmax and everything downstream fp32. Fastest; attention maps agree with the fp32
 *     reference to ~3e-3, which can move an ill-conditioned DTW path or swap two near-tied heads of the top-k selection.
 *   WCA_PRECISION_SPLIT: reference precision on the f16 matrix pipe. Every activation operand x travels as the pair
 *     hi = f16(x), lo = f16(x - hi) (x = hi + lo to 2^-22 |x|) in one row [hi | lo]; weights are exact in f16, so
 *     A W^T = [A_hi | A_lo] [W | W]^T is a K-doubled call of the same MFMA GEMM kernels (f16 x f16 products are exact in
 *     the fp32 accumulator); attention runs three passes per product (hi.hi + hi.lo + lo.hi), GELU uses erff, the log-mel
 *     DFT accumulates in f64. What is left is fp32 summation-order noise, like between two fp32 BLAS libraries. Costs
 *     ~2.3x the MFMA work, twice the operand memory and a second copy of the weights ([N][2K]).
 *   WCA_PRECISION_REFERENCE = WCA_PRECISION_SPLIT: the CONTRACT mode. A new engine (wca_engine_create), bench.py's `value` and the CLI
 *     run in this mode. Every stage is split: the log-mel DFT, the conv stem, the encoder blocks' GEMMs and self-attention, ln_post and
 *     the cross-attention key / value projection, the teacher-forced decoder and the hooked cross-attention (timing.py:50-55). The
 *     per-stage ablation on the 301-utterance parity leg (profiles/r04_precision_ablation.txt) showed that nothing from the encoder
 *     blocks on can be left on single f16 operands, and that leaving only the log-mel and the conv stem on them moves the head
 *     selection scores by 1e-4 relative (all stages split: 4e-6) and misses two near-tied utterances of a 700-utterance leg
 *     (profiles/r04_parity_leg_700utt.txt).
 * The greedy ASR pre-pass (wca_decode) computes in f16 in both modes, like whisper.decode's fp16 default.
 * Switching re-creates the activation arena: no batch may be in flight, encoded-but-unconsumed states are dropped. */
enum { WCA_PRECISION_F16 = 0, WCA_PRECISION_SPLIT = 1, WCA_PRECISION_REFERENCE = 1 };
int wca_set_precision(wca_engine* e, int mode);   /* F16 or SPLIT (= REFERENCE) */
int wca_get_precision(wca_engine* e);             /* F16 or SPLIT */
/* on (default): phase 2 (decoder, post-processing, DTW) of a batch runs on the engine's second stream beside the next
 * batch's phase 1; off: everything on one stream, so that rocprofv3 per-kernel durations are not inflated by sharing
 * the CUs (profiling aid; throughput drops by the overlap's worth). No batch may be in flight when it is changed. */
int wca_set_overlap(wca_engine* e, int on);
/* Decoder GEMMs on few rows (a decode step of wca_decode: M = batch; batch-1 teacher-forced forwards):
 * fused != 0 (default): for up to 128 rows one few-row kernel per GEMM with the LayerNorm in its prologue, the KV-cache append in its
 * epilogue and deterministic split-K for K = 4 n_state; 0: separate LayerNorm / GEMM / append launches (the round-1 path,
 * kept for A/B tests). streams must be 1: the form that ran the batch as two half-batches on two streams was removed (it measured no
 * faster, HISTORY.md) and any other value is refused with WCA_ERR_INVALID; the argument stays so that existing callers keep their arity.
 * Token choices are independent of `fused` up to fp32 summation order in the split-K GEMM. */
int wca_set_decode_mode(wca_engine* e, int fused, int streams);
/* enable/disable per-stage event recording (default off: no extra events on the stream) */
int wca_set_profiling(wca_engine* e, int on);

#ifdef __cplusplus
}
#endif
#endif /* WCA_H_ */
