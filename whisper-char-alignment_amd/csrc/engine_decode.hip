// libwca.so engine, decode: wca_decode -- every row at the same position with an optional batched prefill, or per-row initial tokens,
// sample budgets, temperatures and seeds, optionally on the state the last decode left -- over one argument check, one loop and one
// read-back; and wca_detect_language (one position and the language head on the state a decode then takes).
#include "engine_internal.h"

using namespace wca;

namespace {

// The rows of a decode as the descriptor gives them. each = per_row = 1: n_initial / sot_index / sample_len are arrays of [batch] and row b's
// initial tokens start at initial + b * n_max; each = 0: one value, one token row, for every row -- the uniform call is `batch` identical
// rows.
struct DecodeRows {
  int batch, each;
  const int32_t *initial, *n_initial, *sot_index, *sample_len;
  int n_max = 0, T_max = 0, S = 0;   // decode_check: the longest initial row, the longest row (initial + budget), the largest budget
  int ni(int b) const { return n_initial[b * each]; }
  int sl(int b) const { return sample_len[b * each]; }
  const int32_t* init(int b) const { return initial + (size_t)b * each * n_max; }
};

// What every decode is refused for, before any work is enqueued: the engine's state, the exclusive mel / pcm inputs, null pointers, the batch
// range, each row's lengths and <|sot|> position, eot / timestamp_begin, the initial tokens. Sets r's sizes.
// need_out: the descriptor's own output arrays are required (wca_decode_group writes its group descriptor's instead).
int decode_check(wca_engine* e, const wca_decode_desc* d, DecodeRows* r, bool need_out = true) {
  const float *mel_dev = d->mel_dev, *pcm_dev = d->pcm_dev;
  const int32_t* n_samples_host = d->n_samples_host;
  const wca_decode_opts* o = d->opts;
  const bool any_null = !d->initial_tokens_host || !d->n_initial_host || !d->sot_index_host || !d->sample_len_host || !d->suppress_mask_host ||
                        !o || (need_out && (!d->tokens_out_host || !d->n_tokens_host));
  const int rc = check_ready(e);
  if (rc) return rc;
  if (mel_dev != nullptr && pcm_dev != nullptr) return fail(WCA_ERR_INVALID, "pass at most one of mel_dev / pcm_dev");
  if (any_null || (pcm_dev && !n_samples_host)) return fail(WCA_ERR_INVALID, "null argument");
  if (r->batch < 1 || r->batch > e->max_batch) return fail(WCA_ERR_INVALID, "batch %d outside [1,%d]", r->batch, e->max_batch);
  const wca_model_dims& D = e->dims;
  const int n_rows = r->each ? r->batch : 1;
  char row[24] = "";
  auto prefix = [&](int b) {   // the row form names the row
    if (r->each) snprintf(row, sizeof(row), "row %d: ", b);
    return row;
  };
  for (int b = 0; b < n_rows; ++b) {
    prefix(b);
    const int ni = r->ni(b), sl = r->sl(b), sot = r->sot_index[b * r->each];
    // upstream samples until the sequence is longer than n_ctx: the (n_text_ctx + 1)-th token is sampled, never embedded
    if (ni < 1 || sl < 1 || ni > D.n_text_ctx || ni + sl > D.n_text_ctx + 1)
      return fail(WCA_ERR_TOO_LONG, "%sn_initial %d + sample_len %d exceeds n_text_ctx + 1 = %d (or n_initial exceeds n_text_ctx)", row, ni, sl,
                  D.n_text_ctx + 1);
    if (sot < 0 || sot >= ni) return fail(WCA_ERR_INVALID, "%ssot_index %d outside [0,%d)", row, sot, ni);
    r->n_max = std::max(r->n_max, ni);
    r->T_max = std::max(r->T_max, ni + sl);
    r->S = std::max(r->S, sl);
  }
  if (o->eot < 0 || o->eot >= D.n_vocab || o->timestamp_begin < 0 || o->timestamp_begin > D.n_vocab)
    return fail(WCA_ERR_INVALID, "eot / timestamp_begin outside the vocabulary");
  for (int b = 0; b < n_rows; ++b)
    for (int i = 0; i < r->ni(b); ++i)
      if (r->init(b)[i] < 0 || r->init(b)[i] >= D.n_vocab) return fail(WCA_ERR_INVALID, "%sinitial token %d outside the vocabulary", prefix(b), i);
  return WCA_OK;
}

// What the uniform and the per-row decode share around the loop.
// Phase 1 on `stream` (unless an encoded state is waiting: wca_encode_batch) and the state to decode; the state stays queued for the
// alignment (wca_align_batch_enqueue with pcm_dev = NULL). A state that was decoded but never aligned is stale once another decode
// starts (stand-alone whisper.decode use). The autoregressive loop runs on `stream2` (it shares the decoder scratch with phase 2 of
// the alignment, which is ordered before it on that stream; phase 1 of the NEXT batch may run beside it on `stream`): stream2 is made
// to wait for the state's cross-K/V here.
// redecode (no input of its own): the state is the NEWEST one that is already decoded and not yet aligned -- what
// the previous decode left for the alignment -- and nothing is dropped: it stays queued, decoded, for that alignment.
int decode_take_state(wca_engine* e, const float* mel_dev, const float* pcm_dev, int64_t pcm_stride, const int32_t* n_samples_host, int batch,
                      wca_engine::EncState** out, bool redecode = false) {
  if (redecode) {
    wca_engine::EncState* st = nullptr;
    for (auto it = e->enc_q.rbegin(); it != e->enc_q.rend() && !st; ++it)
      if (it->decoded) st = &*it;
    if (!st || st->batch != batch) return fail(WCA_ERR_STATE, "no decoded batch of %d utterances is waiting to be decoded again", batch);
    HIPCHK(hipStreamWaitEvent(e->stream2, e->ev_kv[st->slot], 0));
    *out = st;
    return WCA_OK;
  }
  // (a state that wca_detect_language has read waits for the decode of that same state; a call that brings its own input drops it)
  const bool fresh = mel_dev != nullptr || pcm_dev != nullptr;
  for (auto it = e->enc_q.begin(); it != e->enc_q.end();) {
    if (it->decoded || (fresh && it->detected)) {
      e->slot_busy[it->slot] = false;
      it = e->enc_q.erase(it);
    } else {
      ++it;
    }
  }
  if (mel_dev != nullptr || pcm_dev != nullptr) {
    const int rc = wca_encode_batch(e, mel_dev, pcm_dev, pcm_stride, n_samples_host, batch);
    if (rc) return rc;
  }
  wca_engine::EncState* st = nullptr;
  for (auto& q : e->enc_q)
    if (!q.decoded) {
      st = &q;
      break;
    }
  if (!st || st->batch != batch) return fail(WCA_ERR_STATE, "no encoded batch of %d utterances is waiting to be decoded", batch);
  HIPCHK(hipStreamWaitEvent(e->stream2, e->ev_kv[st->slot], 0));
  *out = st;
  return WCA_OK;
}

// The token rows, sum_logprob and no_speech_prob of a loop that made `steps` choices to the host. Row b holds its initial tokens and has
// written positions [0, n_have) with n_have = n_initial + min(steps, its budget); n_tokens[b] = its first sampled EOT (or n_have):
// tokens_out[b][n_initial : n_tokens[b]] are the sampled tokens, and positions never reached hold EOT. Marks the state decoded.
int decode_read_back(wca_engine* e, hipStream_t s2, wca_engine::EncState* st, const DecodeRows& r, int steps, const wca_decode_desc* d,
                     bool want_nsp) {
  const int batch = r.batch, T_max = r.T_max, eot = d->opts->eot;
  int32_t *tokens_out_host = d->tokens_out_host, *n_tokens_host = d->n_tokens_host;
  float *sum_logprob_host = d->sum_logprob_host, *no_speech_prob_host = want_nsp ? d->no_speech_prob_host : nullptr;
  std::vector<int32_t> toks((size_t)batch * T_max);
  HIPCHK(hipMemcpyAsync(toks.data(), e->dec_tokens.p, sizeof(int) * toks.size(), hipMemcpyDeviceToHost, s2));
  std::vector<float> lp(2 * (size_t)batch);  // sum_logprob [batch], no_speech_prob [batch] at the head of dec_state
  HIPCHK(hipMemcpyAsync(lp.data(), e->dec_state.p, sizeof(float) * 2 * batch, hipMemcpyDeviceToHost, s2));
  HIPCHK(hipStreamSynchronize(s2));
  for (int b = 0; b < batch; ++b) {
    const int n_have = r.ni(b) + std::min(steps, r.sl(b));
    int n = n_have;
    for (int i = r.ni(b); i < n_have; ++i)
      if (toks[(size_t)b * T_max + i] == eot) {
        n = i;
        break;
      }
    n_tokens_host[b] = n;
    for (int i = 0; i < T_max; ++i) tokens_out_host[(size_t)b * T_max + i] = (i < n_have) ? toks[(size_t)b * T_max + i] : eot;
    if (sum_logprob_host) sum_logprob_host[b] = lp[b];
    if (no_speech_prob_host) no_speech_prob_host[b] = lp[batch + b];
  }
  st->decoded = true;
  e->last_batch = batch;
  return WCA_OK;
}

// What the loop works on, set up by decode_begin: the state to decode, the device buffers and the select arguments every step starts
// from. Rows never interact (per-row kernels, per-row cache planes); n_done is an atomic counter.
struct DecodeLoop {
  wca_engine* e = nullptr;
  wca_engine::EncState* st = nullptr;
  const half_t* kvbuf = nullptr;
  hipStream_t s2 = nullptr;
  int batch = 0, T_max = 0, V = 0;
  bool want_nsp = false;
  int no_speech = -1;        // the <|nospeech|> token (want_nsp)
  int* tokens_dev = nullptr;
  float* nsp = nullptr;      // no_speech_prob [batch]
  int* n_done = nullptr;     // completion counters
  DecodeSelectArgs sel{};    // whole batch; the per-step fields (cur_len ...) are the loop's
  // whisper's loop ends when every row has produced EOT: the counter of this step, read back (a host sync; the loop asks every 4 steps:
  // a late stop only costs time, finished rows keep emitting EOT)
  int all_done(const int* counter, bool* done) const {
    HIPCHK(hipMemcpyAsync(e->dec_done_host, counter, sizeof(int), hipMemcpyDeviceToHost, s2));
    HIPCHK(hipStreamSynchronize(s2));
    *done = e->dec_done_host[0] >= batch;
    return WCA_OK;
  }
};

// Takes the state to decode (phase 1 first where a mel / PCM is given), sizes the decode buffers, uploads the token rows [batch][T_max]
// (row b's initial tokens, then eot), the per-row tables `tab` (nullable -> e->dec_rows) and the masks, zeroes sum_logprob / no_speech_prob
// and the n_done_len completion counters. A prefill also leaves the <|sot|> logits (rows [batch, 2 batch)) and needs the gather scratch.
int decode_begin(wca_engine* e, const wca_decode_desc* d, const DecodeRows& r, int n_done_len, const std::vector<int32_t>* tab, DecodeLoop* out) {
  const wca_decode_opts* o = d->opts;
  const uint8_t *suppress_mask_host = d->suppress_mask_host, *blank_mask_host = d->blank_mask_host;
  const bool prefill = d->prefill == 1;
  const wca_model_dims& D = e->dims;
  const int V = D.n_vocab, dt = D.n_text_state, L = D.n_text_layer, batch = r.batch, T_max = r.T_max;
  std::vector<int32_t> init((size_t)batch * T_max, o->eot);
  for (int b = 0; b < batch; ++b) std::copy(r.init(b), r.init(b) + r.ni(b), init.begin() + (size_t)b * T_max);
  DecodeLoop& lp = *out;
  lp.e = e;
  lp.batch = batch;
  lp.T_max = T_max;
  lp.V = V;
  WCA_TRY(decode_take_state(e, d->mel_dev, d->pcm_dev, d->pcm_stride, d->n_samples_host, batch, &lp.st, d->redecode == 1));
  lp.kvbuf = lp.st->slot ? e->kv_alt : e->kv;
  hipStream_t s2 = lp.s2 = e->stream2;
  e->dec_cache_off = 0;
  HIPCHK(e->dec_cache.ensure(sizeof(half_t) * (size_t)L * 2 * batch * T_max * dt));
  HIPCHK(e->dec_tokens.ensure(sizeof(int) * (size_t)batch * T_max));
  HIPCHK(e->dec_masks.ensure((size_t)2 * V));
  lp.want_nsp = d->no_speech_prob_host && o->no_speech >= 0 && o->no_speech < V;
  lp.no_speech = o->no_speech;
  // the prefill's logits: rows [0, B) at the last initial position, rows [B, 2B) at <|sot|>
  HIPCHK(e->dec_logits.ensure(sizeof(float) * (size_t)((prefill && lp.want_nsp) ? 2 : 1) * batch * V));
  const size_t state_bytes = sizeof(float) * 2 * batch + sizeof(int) * (size_t)n_done_len;
  HIPCHK(e->dec_state.ensure(state_bytes));
  if (prefill) HIPCHK(e->dec_gather.ensure(sizeof(float) * 2 * (size_t)batch * dt));
  if (tab) HIPCHK(e->dec_rows.ensure(sizeof(int) * tab->size()));
  if (!e->dec_done_host) HIPCHK(hipHostMalloc((void**)&e->dec_done_host, sizeof(int) * 4, hipHostMallocDefault));
  lp.tokens_dev = (int*)e->dec_tokens.p;
  unsigned char* masks = (unsigned char*)e->dec_masks.p;
  float* sum_lp = (float*)e->dec_state.p;
  lp.nsp = sum_lp + batch;
  lp.n_done = (int*)((char*)e->dec_state.p + sizeof(float) * 2 * batch);
  HIPCHK(hipMemcpyAsync(lp.tokens_dev, init.data(), sizeof(int) * init.size(), hipMemcpyHostToDevice, s2));
  if (tab) HIPCHK(hipMemcpyAsync(e->dec_rows.p, tab->data(), sizeof(int) * tab->size(), hipMemcpyHostToDevice, s2));
  HIPCHK(hipMemcpyAsync(masks, suppress_mask_host, V, hipMemcpyHostToDevice, s2));
  if (blank_mask_host) HIPCHK(hipMemcpyAsync(masks + V, blank_mask_host, V, hipMemcpyHostToDevice, s2));
  HIPCHK(hipMemsetAsync(e->dec_state.p, 0, state_bytes, s2));
  HIPCHK(hipStreamSynchronize(s2));  // `init` / `tab` are pageable host memory
  DecodeSelectArgs& sel = lp.sel;
  sel.logits = (const float*)e->dec_logits.p;
  sel.ld = V;
  sel.n_vocab = V;
  sel.tokens = lp.tokens_dev;
  sel.T_max = T_max;
  sel.suppress_mask = masks;
  sel.blank_mask = blank_mask_host ? masks + V : nullptr;
  sel.eot = o->eot;
  sel.timestamp_begin = o->timestamp_begin;
  sel.apply_timestamp_rules = o->apply_timestamp_rules;
  sel.max_initial_timestamp_index = o->max_initial_timestamp_index;
  sel.sum_logprob = sum_lp;
  sel.n_done = lp.n_done;
  return WCA_OK;
}

// What the loop does for a call. The first choice comes from one batched forward over n_prefill (padded) initial positions on s2 for the
// whole batch (run_decode_prefill), and the step loop continues behind it; or (n_prefill = 0) the initial tokens are fed
// one position at a time, n_warm of them before the first choice (the plain start is 3 tokens: sot, language, task). At most `budget`
// choices. Uniform rows (tab == nullptr): every row holds n_initial tokens, choice c reads the forward of position n_initial - 1 + c, and
// no_speech_prob is taken at position sot_index. Per-row (tab, device): the tables of decode_per_row say where each row is.
struct DecodePlan {
  int n_prefill, n_warm, budget;
  int n_initial, sot_index;
  const int* tab;
};

// The loop over forwards: forward f feeds one position of every row (or, the prefill, all initial ones) and, from f = n_warm on, makes
// choice c = f - n_warm. Ends after `budget` choices or when every row has produced EOT (or used its own budget), asked every 4 choices.
// The uniform form launches the scalar kernels with n_done indexed by cur_len, the per-row form the table kernels with n_done indexed by c.
// Then the results to the host (decode_read_back) and the positions wca_last_decode_positions reports.
int decode_run(const DecodeLoop& lp, const DecodePlan& pl, const DecodeRows& r, const wca_decode_desc* d) {
  wca_engine* e = lp.e;
  const int B = lp.batch, V = lp.V;
  const float* logits = (const float*)e->dec_logits.p;
  int steps = 0, step_positions = 0;
  for (int f = 0; f < pl.n_warm + pl.budget; ++f) {
    const int c = f - pl.n_warm;
    const int t = pl.n_initial - 1 - pl.n_warm + f;                                        // uniform: the position fed
    const int* row = pl.tab ? pl.tab + (size_t)(4 + 3 * c) * B : nullptr;                  // per-row: fed position, key count, cur_len of choice c
    const bool sot_logits = lp.want_nsp && !pl.n_prefill && t == pl.sot_index;             // probs_at_sot of DecodingTask._main_loop
    DecodeSelectArgs sel = lp.sel;
    if (row) {
      sel.cur_len_rows = row + 2 * (size_t)B;
      sel.n_done_idx = c;
    } else {
      sel.cur_len = t + 1;
    }
    if (pl.n_prefill && c == 0) {
      const StepPos last{pl.n_prefill - 1, pl.tab}, sot{lp.want_nsp ? pl.sot_index : -1, lp.want_nsp && pl.tab ? pl.tab + B : nullptr};
      WCA_TRY(run_decode_prefill(e, lp.s2, lp.kvbuf, lp.tokens_dev, B, pl.n_prefill, lp.T_max, last, sot));
      if (lp.want_nsp) HIPCHK(launch_token_prob(logits + (size_t)B * V, V, V, lp.no_speech, lp.nsp, B, lp.s2));
      HIPCHK(launch_decode_select(sel, B, lp.s2));
    } else {
      ++step_positions;
      WCA_TRY(run_decode_step(e, lp.s2, lp.kvbuf, lp.tokens_dev, B, StepPos{t, row}, lp.T_max, c >= 0 || sot_logits));
      if (sot_logits) HIPCHK(launch_token_prob(logits, V, V, lp.no_speech, lp.nsp, B, lp.s2));
      if (c >= 0) HIPCHK(launch_decode_select(sel, B, lp.s2));
    }
    if (c < 0) continue;
    steps = c + 1;
    if ((steps & 3) == 0 && steps < pl.budget) {
      bool done = false;
      WCA_TRY(lp.all_done(lp.n_done + (row ? c : t + 1), &done));
      if (done) break;
    }
  }
  WCA_TRY(decode_read_back(e, lp.s2, lp.st, r, steps, d, lp.want_nsp));
  e->dec_prefill_positions = pl.n_prefill;
  e->dec_step_positions = step_positions;
  e->dec_batch = B;
  e->dec_T_max = lp.T_max;
  e->dec_logits_rows = (pl.n_prefill && lp.want_nsp ? 2 : 1) * B;   // a prefill leaves the <|sot|> rows behind the last position's
  return WCA_OK;
}

// The uniform decode (per_row 0): every row holds the same n_initial tokens; the scalar kernels, with or without a prefill.
int decode_uniform(wca_engine* e, const wca_decode_desc* d, const DecodeRows& r) {
  const int n_initial = r.ni(0);
  const bool prefill = d->prefill == 1;
  DecodeLoop lp;
  WCA_TRY(decode_begin(e, d, r, r.T_max, nullptr, &lp));
  lp.sel.n_initial = n_initial;
  // sampling starts after the last initial token
  const DecodePlan pl{prefill ? n_initial : 0, prefill ? 0 : n_initial - 1, r.S, n_initial, r.sot_index[0], nullptr};
  return decode_run(lp, pl, r, d);
}

// The decode of a batch whose rows carry initial tokens of their own (per_row 1; transcribe_batch: every recording's prompt is its own
// previous text). Row b holds n_initial[b] tokens and samples at most sample_len[b]; at loop step s (0 = the prefill's choice) it is at
// cur_len = n_initial[b] + s. Prefill: every row padded with eot to n_max = max n_initial (a valid query never sees a later position,
// and the K/V that the pad positions leave in cache slots >= n_initial[b] are overwritten by the step loop before they are read);
// steps: the per-row forms of embed_step / KV append / one-query attention / decode_select, fed from small device tables built here.
// A row past its budget keeps going through the kernels as a finished row at a clamped position (<= T_max - 2, so no positional row
// past n_text_ctx - 1 and no cache slot past T_max - 1 is touched); what it computes is never read.
//
// Sampling (temperature_host / seed_host [batch], else both null): the tables gain the rows' Philox seeds and temperatures, and the select
// step takes its sampling form (upstream GreedyDecoder.update at temperature > 0; decode.hip); everything else is the greedy call.
// redecode: see decode_take_state.
int decode_per_row(wca_engine* e, const wca_decode_desc* d, const DecodeRows& r) {
  const int batch = r.batch, T_max = r.T_max, S = r.S;
  const float* temperature_host = d->temperature_host;
  // the int tables: [0] n_initial - 1, [1] sot_index, [2] n_initial, [3] sample cap; then per choice c in [0, S): fed position
  // min(n_initial + c - 1, T_max - 2), key count = fed position + 1, cur_len = n_initial + c  ([batch] each)
  // sampling: behind them (at an even index: 8-byte aligned) the seeds [batch] uint64, then the temperatures [batch] f32
  const size_t n_int = (size_t)(4 + 3 * S) * batch, seed_at = (n_int + 1) & ~(size_t)1, temp_at = seed_at + 2 * (size_t)batch;
  std::vector<int32_t> tab(temperature_host ? temp_at + batch : n_int);
  if (temperature_host) {
    memcpy(tab.data() + seed_at, d->seed_host, sizeof(uint64_t) * batch);
    memcpy(tab.data() + temp_at, temperature_host, sizeof(float) * batch);
  }
  for (int b = 0; b < batch; ++b) {
    const int ni = r.ni(b);
    tab[0 * (size_t)batch + b] = ni - 1;
    tab[1 * (size_t)batch + b] = r.sot_index[b];
    tab[2 * (size_t)batch + b] = ni;
    tab[3 * (size_t)batch + b] = r.sl(b);
    for (int c = 0; c < S; ++c) {
      const int pos = std::max(0, std::min(ni + c - 1, T_max - 2));
      tab[(size_t)(4 + 3 * c + 0) * batch + b] = pos;
      tab[(size_t)(4 + 3 * c + 1) * batch + b] = pos + 1;
      tab[(size_t)(4 + 3 * c + 2) * batch + b] = ni + c;
    }
  }
  DecodeLoop lp;
  WCA_TRY(decode_begin(e, d, r, S, &tab, &lp));
  const int* tab_dev = (const int*)e->dec_rows.p;
  lp.sel.n_initial_rows = tab_dev + 2 * (size_t)batch;
  lp.sel.cap_rows = tab_dev + 3 * (size_t)batch;
  if (temperature_host) {
    lp.sel.seed_rows = (const unsigned long long*)(tab_dev + seed_at);
    lp.sel.temperature_rows = (const float*)(tab_dev + temp_at);
  }
  const DecodePlan pl{r.n_max, 0, S, 0, -1, tab_dev};
  return decode_run(lp, pl, r, d);
}

// The Philox seed of sample g of a row whose seed is s (include/wca.h): g = 0 keeps s.
inline uint64_t group_seed(uint64_t s, int g) { return s ^ ((uint64_t)g * 0x94D049BB133111EBull); }

// wca_decode_group: G decoder rows per audio, row b * G + g = beam or sample g of audio b. The B audios go through today's prefill; each
// audio's cache rows and logits are then handed to its G rows, and the step loop is decode_per_row's on R = B G rows whose cross-attention
// reads the audio's K/V (run_decode_step, kv_group). The rows of a group hold their audio's initial tokens, positions and budget.
//   mode 0 (beam): each choice is beam_topk + beam_merge between two token buffers, and from the second choice on the cache rows follow
//     their beams into the other half of dec_cache (kv_reorder; at the first choice every beam continues beam 0, whose cache all G rows
//     already hold). The loop stops when every audio's finished list holds max_candidates sequences or is past its budget. Upstream's
//     finalize runs on the host: a list shorter than G is topped up from the live beams, which the merge leaves in descending order of
//     sum_logprob.
//   mode 1 (samples): decode_select's sampling form on the R rows, row (b, g) drawing with group_seed(seed[b], g); nothing is reordered.
int decode_group(wca_engine* e, const wca_decode_desc* d, const wca_group_desc* gd, const DecodeRows& r) {
  const wca_decode_opts* o = d->opts;
  const wca_model_dims& D = e->dims;
  const int B = r.batch, G = gd->n_group, R = B * G, T_max = r.T_max, S = r.S, K = G + 1;
  const int V = D.n_vocab, dt = D.n_text_state, L = D.n_text_layer;
  const bool beam = gd->mode == 0;
  const int MC = beam ? gd->max_candidates : 1, n_slot = beam ? std::max(G, MC) : G;
  // the int tables of decode_per_row on R rows; behind them the prefill's [B] last initial positions and [B] <|sot|> positions; sampling:
  // behind those (8-byte aligned) the rows' seeds [R] uint64 and temperatures [R] f32
  const size_t n_int = (size_t)(4 + 3 * S) * R, pre_at = n_int, seed_at = (pre_at + 2 * (size_t)B + 1) & ~(size_t)1, temp_at = seed_at + 2 * (size_t)R;
  std::vector<int32_t> tab(beam ? pre_at + 2 * (size_t)B : temp_at + R);
  for (int row = 0; row < R; ++row) {
    const int b = row / G, ni = r.ni(b);
    tab[0 * (size_t)R + row] = ni - 1;
    tab[1 * (size_t)R + row] = r.sot_index[b * r.each];
    tab[2 * (size_t)R + row] = ni;
    tab[3 * (size_t)R + row] = r.sl(b);
    for (int c = 0; c < S; ++c) {
      const int pos = std::max(0, std::min(ni + c - 1, T_max - 2));
      tab[(size_t)(4 + 3 * c + 0) * R + row] = pos;
      tab[(size_t)(4 + 3 * c + 1) * R + row] = pos + 1;
      tab[(size_t)(4 + 3 * c + 2) * R + row] = ni + c;
    }
    if (!beam) {
      const uint64_t seed = group_seed(d->seed_host[b], row - b * G);
      memcpy(tab.data() + seed_at + 2 * (size_t)row, &seed, sizeof(seed));
      memcpy(tab.data() + temp_at + row, d->temperature_host + b, sizeof(float));
    }
  }
  for (int b = 0; b < B; ++b) {
    tab[pre_at + b] = r.ni(b) - 1;
    tab[pre_at + B + b] = r.sot_index[b * r.each];
  }
  // token rows: two buffers [R][T_max] (the beam step gathers from one into the other), then the prefill's [B][T_max]
  std::vector<int32_t> init((size_t)(2 * R + B) * T_max, o->eot);
  for (int row = 0; row < 2 * R + B; ++row) {
    const int b = row < 2 * R ? (row % R) / G : row - 2 * R;
    std::copy(r.init(b), r.init(b) + r.ni(b), init.begin() + (size_t)row * T_max);
  }

  wca_engine::EncState* st = nullptr;
  WCA_TRY(decode_take_state(e, d->mel_dev, d->pcm_dev, d->pcm_stride, d->n_samples_host, B, &st, d->redecode == 1));
  const half_t* kvbuf = st->slot ? e->kv_alt : e->kv;
  hipStream_t s2 = e->stream2;
  const size_t half_elems = (size_t)L * 2 * R * T_max * dt;   // one of the two caches
  const bool want_nsp = gd->no_speech_prob_host && o->no_speech >= 0 && o->no_speech < V;
  e->dec_cache_off = 0;
  e->dec_batch = e->dec_T_max = e->dec_logits_rows = 0;
  e->grp_steps = e->grp_rows = 0;
  HIPCHK(e->dec_cache.ensure(sizeof(half_t) * 2 * half_elems));
  HIPCHK(e->dec_tokens.ensure(sizeof(int) * init.size()));
  HIPCHK(e->dec_masks.ensure((size_t)2 * V));
  HIPCHK(e->dec_logits.ensure(sizeof(float) * (size_t)std::max(R, 2 * B) * V));
  const size_t state_bytes = sizeof(float) * (R + B) + sizeof(int) * (size_t)S;
  HIPCHK(e->dec_state.ensure(state_bytes));
  HIPCHK(e->dec_gather.ensure(sizeof(float) * 2 * (size_t)B * dt));
  HIPCHK(e->dec_rows.ensure(sizeof(int) * tab.size()));
  // the beam step's arrays, 4-byte entries: candidates [R][K] tokens and log-probabilities, sources [R], the finished lists (counts [B],
  // lengths and sums [B][MC], token rows [B][MC][T_max]), the trace [S][R][2]
  const size_t cand_at = 0, lp_at = cand_at + (size_t)R * K, src_at = lp_at + (size_t)R * K, finn_at = src_at + R, finlen_at = finn_at + B,
               finsum_at = finlen_at + (size_t)B * MC, fintok_at = finsum_at + (size_t)B * MC, trace_at = fintok_at + (size_t)B * MC * T_max,
               beam_words = trace_at + (size_t)S * R * 2;
  if (beam) {
    HIPCHK(e->dec_beam.ensure(sizeof(int) * beam_words));
    HIPCHK(hipMemsetAsync(e->dec_beam.p, 0, sizeof(int) * beam_words, s2));
  }
  if (!e->dec_done_host) HIPCHK(hipHostMalloc((void**)&e->dec_done_host, sizeof(int) * 4, hipHostMallocDefault));
  int* tok_buf[2] = {(int*)e->dec_tokens.p, (int*)e->dec_tokens.p + (size_t)R * T_max};
  int* tok_pre = (int*)e->dec_tokens.p + 2 * (size_t)R * T_max;
  unsigned char* masks = (unsigned char*)e->dec_masks.p;
  float* sum_lp = (float*)e->dec_state.p;
  float* nsp = sum_lp + R;
  int* n_done = (int*)(nsp + B);
  int* bw = (int*)e->dec_beam.p;
  float* logits = (float*)e->dec_logits.p;
  half_t* cache = (half_t*)e->dec_cache.p;
  const int* tab_dev = (const int*)e->dec_rows.p;
  HIPCHK(hipMemcpyAsync(tok_buf[0], init.data(), sizeof(int) * init.size(), hipMemcpyHostToDevice, s2));
  HIPCHK(hipMemcpyAsync(e->dec_rows.p, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice, s2));
  HIPCHK(hipMemcpyAsync(masks, d->suppress_mask_host, V, hipMemcpyHostToDevice, s2));
  if (d->blank_mask_host) HIPCHK(hipMemcpyAsync(masks + V, d->blank_mask_host, V, hipMemcpyHostToDevice, s2));
  HIPCHK(hipMemsetAsync(e->dec_state.p, 0, state_bytes, s2));
  HIPCHK(hipStreamSynchronize(s2));  // `init` / `tab` are pageable host memory

  DecodeSelectArgs sel{};
  sel.logits = logits;
  sel.ld = V;
  sel.n_vocab = V;
  sel.T_max = T_max;
  sel.suppress_mask = masks;
  sel.blank_mask = d->blank_mask_host ? masks + V : nullptr;
  sel.eot = o->eot;
  sel.timestamp_begin = o->timestamp_begin;
  sel.apply_timestamp_rules = o->apply_timestamp_rules;
  sel.max_initial_timestamp_index = o->max_initial_timestamp_index;
  sel.sum_logprob = sum_lp;
  sel.n_done = n_done;
  sel.n_initial_rows = tab_dev + 2 * (size_t)R;
  sel.cap_rows = tab_dev + 3 * (size_t)R;
  if (!beam) {
    sel.seed_rows = (const unsigned long long*)(tab_dev + seed_at);
    sel.temperature_rows = (const float*)(tab_dev + temp_at);
  }

  int cur_tok = 0, cur_cache = 0, steps = 0, step_positions = 0;
  for (int c = 0; c < S; ++c) {
    const int* row = tab_dev + (size_t)(4 + 3 * c) * R;   // fed position, key count, cur_len of choice c
    if (c == 0) {
      const StepPos last{r.n_max - 1, tab_dev + pre_at}, sot{-1, want_nsp ? tab_dev + pre_at + B : nullptr};
      WCA_TRY(run_decode_prefill(e, s2, kvbuf, tok_pre, B, r.n_max, T_max, last, sot));   // into the first half, as planes of B rows
      if (want_nsp) HIPCHK(launch_token_prob(logits + (size_t)B * V, V, V, o->no_speech, nsp, B, s2));
      // every row of a group starts from its audio's logits and cache: logits row b to rows [b G, (b + 1) G), from the back so that no
      // source row is overwritten before it is read; the cache rows [0, n_initial) into the second half, as planes of R rows
      for (int dst = R - 1; dst > 0; --dst)
        if (dst != dst / G)
          HIPCHK(hipMemcpyAsync(logits + (size_t)dst * V, logits + (size_t)(dst / G) * V, sizeof(float) * V, hipMemcpyDeviceToDevice, s2));
      HIPCHK(launch_kv_reorder(cache, cache + half_elems, 2 * L, B, R, T_max, dt, nullptr, G, tab_dev + 2 * (size_t)R, s2));
      cur_cache = 1;
    } else {
      ++step_positions;
      e->dec_cache_off = cur_cache * half_elems;
      WCA_TRY(run_decode_step(e, s2, kvbuf, tok_buf[cur_tok], R, StepPos{0, row}, T_max, true, G));
    }
    sel.tokens = tok_buf[cur_tok];
    sel.cur_len_rows = row + 2 * (size_t)R;
    sel.n_done_idx = c;
    if (beam) {
      BeamTopkArgs tk{sel, K, bw + cand_at, (float*)(bw + lp_at)};
      HIPCHK(launch_beam_topk(tk, R, s2));
      BeamMergeArgs m{};
      m.cand_tok = bw + cand_at;
      m.cand_lp = (const float*)(bw + lp_at);
      m.K = K;
      m.G = G;
      m.tok_in = tok_buf[cur_tok];
      m.tok_out = tok_buf[cur_tok ^ 1];
      m.T_max = T_max;
      m.sum_logprob = sum_lp;
      m.src = bw + src_at;
      m.cur_len_rows = sel.cur_len_rows;
      m.n_initial_rows = sel.n_initial_rows;
      m.cap_rows = sel.cap_rows;
      m.first = c == 0;
      m.eot = o->eot;
      m.max_candidates = MC;
      m.fin_n = bw + finn_at;
      m.fin_len = bw + finlen_at;
      m.fin_sum = (float*)(bw + finsum_at);
      m.fin_tok = bw + fintok_at;
      m.trace = bw + trace_at + (size_t)c * R * 2;
      m.n_done = n_done + c;
      HIPCHK(launch_beam_merge(m, B, s2));
      cur_tok ^= 1;
      if (c > 0) {   // the cache rows follow their beams: key count of this step's forward
        HIPCHK(launch_kv_reorder(cache + cur_cache * half_elems, cache + (cur_cache ^ 1) * half_elems, 2 * L, R, R, T_max, dt, bw + src_at, 1,
                                 row + R, s2));
        cur_cache ^= 1;
      }
    } else {
      HIPCHK(launch_decode_select(sel, R, s2));
    }
    steps = c + 1;
    if ((steps & 3) == 0 && steps < S) {
      HIPCHK(hipMemcpyAsync(e->dec_done_host, n_done + c, sizeof(int), hipMemcpyDeviceToHost, s2));
      HIPCHK(hipStreamSynchronize(s2));
      if (e->dec_done_host[0] >= (beam ? B : R)) break;
    }
  }
  e->dec_cache_off = cur_cache * half_elems;

  // read-back and, for the beams, upstream's finalize
  std::vector<int32_t> toks((size_t)R * T_max), fin(beam ? trace_at - finn_at : 0);
  std::vector<float> lp((size_t)R + B);
  HIPCHK(hipMemcpyAsync(toks.data(), tok_buf[cur_tok], sizeof(int) * toks.size(), hipMemcpyDeviceToHost, s2));
  HIPCHK(hipMemcpyAsync(lp.data(), sum_lp, sizeof(float) * lp.size(), hipMemcpyDeviceToHost, s2));
  if (beam) HIPCHK(hipMemcpyAsync(fin.data(), bw + finn_at, sizeof(int) * fin.size(), hipMemcpyDeviceToHost, s2));
  HIPCHK(hipStreamSynchronize(s2));
  const int32_t *fin_n = fin.data(), *fin_len = fin_n + B, *fin_tok = fin_len + 2 * (size_t)B * MC;
  const float* fin_sum = (const float*)(fin_len + (size_t)B * MC);
  const int eot = o->eot;
  std::fill(gd->tokens_out_host, gd->tokens_out_host + (size_t)B * n_slot * T_max, eot);
  for (int b = 0; b < B; ++b) {
    const int ni = r.ni(b), n_have = ni + std::min(steps, r.sl(b));
    int n_out = 0;
    auto put = [&](const int32_t* row, int n_tok, float sum) {
      const size_t slot = (size_t)b * n_slot + n_out++;
      std::copy(row, row + n_tok, gd->tokens_out_host + slot * T_max);
      gd->n_tokens_host[slot] = n_tok;
      gd->sum_logprob_host[slot] = sum;
    };
    if (beam) {
      for (int q = 0; q < fin_n[b]; ++q) put(fin_tok + ((size_t)b * MC + q) * T_max, fin_len[(size_t)b * MC + q], fin_sum[(size_t)b * MC + q]);
      for (int g = 0; g < G && n_out < G; ++g)   // the live beams, best first; a dead beam (-inf) is no sequence
        if (std::isfinite(lp[(size_t)b * G + g])) put(toks.data() + ((size_t)b * G + g) * T_max, n_have, lp[(size_t)b * G + g]);
    } else {
      for (int g = 0; g < G; ++g) {
        const int32_t* row = toks.data() + ((size_t)b * G + g) * T_max;
        int n = n_have;
        for (int i = ni; i < n_have; ++i)
          if (row[i] == eot) {
            n = i;
            break;
          }
        put(row, n, lp[(size_t)b * G + g]);
      }
    }
    for (int q = n_out; q < n_slot; ++q) {
      gd->n_tokens_host[(size_t)b * n_slot + q] = 0;
      gd->sum_logprob_host[(size_t)b * n_slot + q] = 0.f;
    }
    gd->n_out_host[b] = n_out;
    if (want_nsp) gd->no_speech_prob_host[b] = lp[(size_t)R + b];
  }
  st->decoded = true;
  e->last_batch = B;
  e->dec_prefill_positions = r.n_max;
  e->dec_step_positions = step_positions;
  e->dec_batch = R;
  e->dec_T_max = T_max;
  e->dec_logits_rows = R;
  if (beam) {
    e->grp_steps = steps;
    e->grp_rows = R;
    e->grp_trace_off = sizeof(int) * trace_at;
  }
  return WCA_OK;
}

}  // namespace

extern "C" {

int wca_decode(wca_engine* e, const wca_decode_desc* d) {
  if (!e) return fail(WCA_ERR_INVALID, "null engine");
  if (!d) return fail(WCA_ERR_INVALID, "null descriptor");
  if ((d->per_row | d->prefill | d->redecode) & ~1) return fail(WCA_ERR_INVALID, "per_row, prefill and redecode must each be 0 or 1");
  if (!d->temperature_host != !d->seed_host) return fail(WCA_ERR_INVALID, "temperature_host and seed_host are given together or not at all");
  if (!d->per_row && (d->temperature_host || d->redecode)) return fail(WCA_ERR_INVALID, "temperatures, seeds and redecode need per_row = 1");
  if (d->per_row && !d->prefill) return fail(WCA_ERR_INVALID, "per_row = 1 always runs the batched prefill: pass prefill = 1");
  if (d->redecode && (d->mel_dev || d->pcm_dev)) return fail(WCA_ERR_INVALID, "redecode takes no input: pass mel_dev = pcm_dev = NULL");
  DecodeRows r{d->batch, d->per_row, d->initial_tokens_host, d->n_initial_host, d->sot_index_host, d->sample_len_host};
  WCA_TRY(decode_check(e, d, &r));
  for (int b = 0; d->temperature_host && b < d->batch; ++b)
    if (!(d->temperature_host[b] >= 0.f) || !std::isfinite(d->temperature_host[b]))
      return fail(WCA_ERR_INVALID, "row %d: temperature %g is negative or not finite", b, (double)d->temperature_host[b]);
  return d->per_row ? decode_per_row(e, d, r) : decode_uniform(e, d, r);
}

int wca_decode_group(wca_engine* e, const wca_decode_desc* d, const wca_group_desc* g) {
  if (!e) return fail(WCA_ERR_INVALID, "null engine");
  if (!d || !g) return fail(WCA_ERR_INVALID, "null descriptor");
  if (!g->tokens_out_host || !g->n_tokens_host || !g->sum_logprob_host || !g->n_out_host) return fail(WCA_ERR_INVALID, "null argument");
  if ((d->per_row | d->prefill | d->redecode) & ~1) return fail(WCA_ERR_INVALID, "per_row, prefill and redecode must each be 0 or 1");
  if (!d->prefill) return fail(WCA_ERR_INVALID, "a group decode always runs the batched prefill: pass prefill = 1");
  if (!d->temperature_host != !d->seed_host) return fail(WCA_ERR_INVALID, "temperature_host and seed_host are given together or not at all");
  if (!d->per_row && (d->temperature_host || d->redecode)) return fail(WCA_ERR_INVALID, "temperatures, seeds and redecode need per_row = 1");
  if (d->redecode && (d->mel_dev || d->pcm_dev)) return fail(WCA_ERR_INVALID, "redecode takes no input: pass mel_dev = pcm_dev = NULL");
  if (g->mode != 0 && g->mode != 1) return fail(WCA_ERR_INVALID, "mode %d is neither 0 (beam) nor 1 (samples)", g->mode);
  if (g->n_group < 1 || g->n_group > BEAM_GROUP_MAX) return fail(WCA_ERR_INVALID, "n_group %d outside [1,%d]", g->n_group, BEAM_GROUP_MAX);
  if (g->mode == 0 && d->temperature_host) return fail(WCA_ERR_INVALID, "beam search runs at temperature 0: pass no temperatures");
  if (g->mode == 1 && !d->temperature_host) return fail(WCA_ERR_INVALID, "independent samples need temperature_host and seed_host");
  if (g->mode == 0 && (g->max_candidates < 1 || g->max_candidates > 4096)) return fail(WCA_ERR_INVALID, "max_candidates %d outside [1,4096]", g->max_candidates);
  if (d->batch < 1 || (long)d->batch * g->n_group > e->max_batch)
    return fail(WCA_ERR_INVALID, "batch %d x n_group %d outside [1, max_batch = %d] decoder rows", d->batch, g->n_group, e->max_batch);
  DecodeRows r{d->batch, d->per_row, d->initial_tokens_host, d->n_initial_host, d->sot_index_host, d->sample_len_host};
  WCA_TRY(decode_check(e, d, &r, false));
  for (int b = 0; d->temperature_host && b < d->batch; ++b)
    if (!(d->temperature_host[b] >= 0.f) || !std::isfinite(d->temperature_host[b]))
      return fail(WCA_ERR_INVALID, "row %d: temperature %g is negative or not finite", b, (double)d->temperature_host[b]);
  return decode_group(e, d, g, r);
}

// Language identification (upstream detect_language): phase 1 as a decode takes it, ONE decoder position (t = 0, token sot) for every
// row -- the first warm step of a wca_decode without prefill up to the final residual stream, no vocabulary projection --, the language head on
// e->xd (language_head.hip: final LayerNorm and the n_lang rows of the token embedding), one read-back. f16 operands in both precision
// modes, like the greedy pre-pass. The state stays queued and UNDECODED: the decode that follows with mel_dev = pcm_dev = NULL runs on it
// with no second encoder pass (decode_begin sets up dec_tokens, dec_state and the cache again; nothing of the detection is read).
int wca_detect_language(wca_engine* e, const float* mel_dev, const float* pcm_dev, int64_t pcm_stride, const int32_t* n_samples_host, int batch,
                        int sot, int lang_begin, int n_lang, int32_t* lang_token_host, float* probs_host) {
  const int rc = check_ready(e);
  if (rc) return rc;
  if (mel_dev != nullptr && pcm_dev != nullptr) return fail(WCA_ERR_INVALID, "pass at most one of mel_dev / pcm_dev");
  if (!lang_token_host || !probs_host || (pcm_dev && !n_samples_host)) return fail(WCA_ERR_INVALID, "null argument");
  if (batch < 1 || batch > e->max_batch) return fail(WCA_ERR_INVALID, "batch %d outside [1,%d]", batch, e->max_batch);
  const wca_model_dims& D = e->dims;
  const int V = D.n_vocab, dt = D.n_text_state, L = D.n_text_layer;
  if (sot < 0 || sot >= V) return fail(WCA_ERR_INVALID, "sot %d outside the vocabulary", sot);
  if (n_lang < 1 || n_lang > 128) return fail(WCA_ERR_INVALID, "n_lang %d outside [1,128]", n_lang);
  if (lang_begin < 0 || lang_begin > V - n_lang) return fail(WCA_ERR_INVALID, "language tokens [%d,%d) outside the vocabulary", lang_begin, lang_begin + n_lang);
  wca_engine::EncState* st = nullptr;
  WCA_TRY(decode_take_state(e, mel_dev, pcm_dev, pcm_stride, n_samples_host, batch, &st));
  const half_t* kvbuf = st->slot ? e->kv_alt : e->kv;
  hipStream_t s2 = e->stream2;
  const int T_max = 1;   // a one-slot self-attention cache: position 0 attends to itself
  e->dec_batch = e->dec_T_max = e->dec_logits_rows = 0;   // the last decode's cache is overwritten
  e->dec_cache_off = 0;
  HIPCHK(e->dec_cache.ensure(sizeof(half_t) * (size_t)L * 2 * batch * T_max * dt));
  HIPCHK(e->dec_tokens.ensure(sizeof(int) * (size_t)batch * T_max));
  HIPCHK(e->dec_state.ensure((sizeof(float) * n_lang + sizeof(int)) * (size_t)batch));
  int* tokens_dev = (int*)e->dec_tokens.p;
  float* probs_dev = (float*)e->dec_state.p;
  int* lang_dev = (int*)(probs_dev + (size_t)batch * n_lang);
  const std::vector<int32_t> init((size_t)batch, sot);
  HIPCHK(hipMemcpyAsync(tokens_dev, init.data(), sizeof(int) * init.size(), hipMemcpyHostToDevice, s2));
  HIPCHK(hipStreamSynchronize(s2));  // `init` is pageable host memory
  WCA_TRY(run_decode_step(e, s2, kvbuf, tokens_dev, batch, StepPos{0, nullptr}, T_max, false));
  HIPCHK(launch_language_head(e->xd, e->lnf_g, e->lnf_b, e->tok_emb, batch, dt, V, lang_begin, n_lang, probs_dev, lang_dev, s2));
  // probs [batch][n_lang] f32 and lang_token [batch] int32 sit back to back: one copy
  std::vector<float> out((size_t)batch * (n_lang + 1));
  HIPCHK(hipMemcpyAsync(out.data(), probs_dev, sizeof(float) * out.size(), hipMemcpyDeviceToHost, s2));
  HIPCHK(hipStreamSynchronize(s2));
  memcpy(probs_host, out.data(), sizeof(float) * (size_t)batch * n_lang);
  memcpy(lang_token_host, out.data() + (size_t)batch * n_lang, sizeof(int32_t) * (size_t)batch);
  st->detected = true;
  return WCA_OK;
}

int wca_last_decode_positions(wca_engine* e, int32_t* prefill_positions, int32_t* step_positions) {
  if (!e || !prefill_positions || !step_positions) return fail(WCA_ERR_INVALID, "null argument");
  *prefill_positions = e->dec_prefill_positions;
  *step_positions = e->dec_step_positions;
  return WCA_OK;
}

}  // extern "C"
