// libwca.so engine, decode: wca_decode -- every row at the same position with an optional batched prefill, or per-row initial tokens,
// sample budgets, temperatures and seeds, optionally on the state the last decode left -- and wca_decode_group -- G decoder rows per
// audio, the beams of a beam search or independent samples -- over one argument check, one table builder, one loop and one read-back;
// and wca_detect_language (one position and the language head on the state a decode then takes).
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
  int sot(int b) const { return sot_index[b * each]; }
  const int32_t* init(int b) const { return initial + (size_t)b * each * n_max; }
};

// What every decode is refused for, before any work is enqueued: flag combinations no call can mean, the engine's state, the exclusive
// mel / pcm inputs, null pointers, the batch range, each row's lengths and <|sot|> position, eot / timestamp_begin, the initial tokens, the
// temperatures. Sets r's sizes.
// need_out: the descriptor's own output arrays are required (wca_decode_group writes its group descriptor's instead).
int decode_check(wca_engine* e, const wca_decode_desc* d, DecodeRows* r, bool need_out = true) {
  if ((d->per_row | d->prefill | d->redecode) & ~1) return fail(WCA_ERR_INVALID, "per_row, prefill and redecode must each be 0 or 1");
  if (!d->temperature_host != !d->seed_host) return fail(WCA_ERR_INVALID, "temperature_host and seed_host are given together or not at all");
  if (!d->per_row && (d->temperature_host || d->redecode)) return fail(WCA_ERR_INVALID, "temperatures, seeds and redecode need per_row = 1");
  if (d->redecode && (d->mel_dev || d->pcm_dev)) return fail(WCA_ERR_INVALID, "redecode takes no input: pass mel_dev = pcm_dev = NULL");
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
    const int ni = r->ni(b), sl = r->sl(b), sot = r->sot(b);
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
  for (int b = 0; d->temperature_host && b < d->batch; ++b)
    if (!(d->temperature_host[b] >= 0.f) || !std::isfinite(d->temperature_host[b]))
      return fail(WCA_ERR_INVALID, "row %d: temperature %g is negative or not finite", b, (double)d->temperature_host[b]);
  return WCA_OK;
}

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

// The Philox seed of sample g of a row whose seed is s (include/wca.h): g = 0 keeps s.
inline uint64_t group_seed(uint64_t s, int g) { return s ^ ((uint64_t)g * 0x94D049BB133111EBull); }

// The tables of a per-row decode on R = batch G decoder rows, row b G + g = beam or sample g of audio b (G = 1: the rows are the audios).
// int rows of [R]: [0] n_initial - 1 and [1] sot_index, which only the prefill reads, per AUDIO: entries [0, batch); [2] n_initial,
// [3] sample cap; then per choice c in [0, S): the fed position n_initial + c - 1, clamped to the last slot but one, key count = fed
// position + 1, cur_len = n_initial + c. The rows of a group hold their audio's values.
// sampled: behind them (at an even index: 8-byte aligned) the seeds [R] uint64, row (b, g) drawing with group_seed(seed[b], g), then the
// temperatures [R] f32.
struct DecodeTab {
  int R = 0;
  bool sampled = false;
  size_t seed_at = 0, temp_at = 0;
  std::vector<int32_t> host;
  size_t choice(int c) const { return (size_t)(4 + 3 * c) * R; }   // where choice c's three rows start; choice(S): the end of the int rows
};

DecodeTab decode_tables(const DecodeRows& r, int G, const uint64_t* seed_host, const float* temperature_host) {
  DecodeTab t;
  const int R = t.R = r.batch * G;
  t.sampled = temperature_host != nullptr;
  t.seed_at = (t.choice(r.S) + 1) & ~(size_t)1;
  t.temp_at = t.seed_at + 2 * (size_t)R;
  t.host.resize(t.sampled ? t.temp_at + R : t.choice(r.S));
  int32_t* tab = t.host.data();
  for (int b = 0; b < r.batch; ++b) {
    tab[b] = r.ni(b) - 1;
    tab[(size_t)R + b] = r.sot(b);
  }
  for (int row = 0; row < R; ++row) {
    const int b = row / G, ni = r.ni(b);
    tab[2 * (size_t)R + row] = ni;
    tab[3 * (size_t)R + row] = r.sl(b);
    for (int c = 0; c < r.S; ++c) {
      const int pos = std::max(0, std::min(ni + c - 1, r.T_max - 2));
      tab[t.choice(c) + row] = pos;
      tab[t.choice(c) + R + row] = pos + 1;
      tab[t.choice(c) + 2 * (size_t)R + row] = ni + c;
    }
    if (t.sampled) {
      const uint64_t seed = group_seed(seed_host[b], row - b * G);
      memcpy(tab + t.seed_at + 2 * (size_t)row, &seed, sizeof(seed));
      memcpy(tab + t.temp_at + row, temperature_host + b, sizeof(float));
    }
  }
  return t;
}

// What the loop does for a call. The first choice comes from one batched forward over n_prefill (padded) initial positions on s2 for the
// whole batch (run_decode_prefill), and the step loop continues behind it; or (n_prefill = 0) the initial tokens are fed
// one position at a time, n_warm of them before the first choice (the plain start is 3 tokens: sot, language, task). At most `budget`
// choices. Uniform rows (tab == nullptr): every row holds n_initial tokens, choice c reads the forward of position n_initial - 1 + c, and
// no_speech_prob is taken at position sot_index. Per-row (tab): the tables say where each row is.
// gd (wca_decode_group, per-row only): G decoder rows per audio. The B audios go through the prefill; each audio's logits and cache rows
// are then handed to its G rows, whose cross-attention reads the audio's K/V (run_decode_step, kv_group).
//   mode 0 (beam): each choice is beam_topk + beam_merge between two token buffers, and from the second choice on the cache rows follow
//     their beams into the other half of dec_cache (kv_reorder; at the first choice every beam continues beam 0, whose cache all G rows
//     already hold). The loop stops when every audio's finished list holds max_candidates sequences or is past its budget.
//   mode 1 (samples): decode_select's sampling form on the R rows; nothing is reordered.
struct DecodePlan {
  int n_prefill, n_warm, budget;
  int n_initial, sot_index;
  const DecodeTab* tab;
  const wca_group_desc* gd;
  int G() const { return gd ? gd->n_group : 1; }
  bool beam() const { return gd && gd->mode == 0; }
};

// dec_beam as the beam step uses it, offsets in 4-byte entries: candidates [R][K] tokens and log-probabilities, sources [R]; the finished
// lists, which the finalize reads back as one block: counts [B], lengths and sums [B][MC], token rows [B][MC][T_max]; the trace [S][R][2].
struct BeamScratch {
  size_t cand_tok, cand_lp, src, fin_n, fin_len, fin_sum, fin_tok, trace, words;
};

BeamScratch beam_scratch(int R, int B, int K, int MC, int T_max, int S) {
  BeamScratch s{};
  s.cand_lp = s.cand_tok + (size_t)R * K;
  s.src = s.cand_lp + (size_t)R * K;
  s.fin_n = s.src + R;
  s.fin_len = s.fin_n + B;
  s.fin_sum = s.fin_len + (size_t)B * MC;
  s.fin_tok = s.fin_sum + (size_t)B * MC;
  s.trace = s.fin_tok + (size_t)B * MC * T_max;
  s.words = s.trace + (size_t)S * R * 2;
  return s;
}

// What the loop works on, set up by decode_begin: the state to decode, the device buffers and the select arguments every step starts
// from. Rows interact only in the beam step (per-row kernels, per-row cache planes); n_done is an atomic counter.
struct DecodeLoop {
  wca_engine* e = nullptr;
  wca_engine::EncState* st = nullptr;
  const half_t* kvbuf = nullptr;
  hipStream_t s2 = nullptr;
  int batch = 0, B = 0;      // decoder rows (B G) and audios: the prefill's rows
  int T_max = 0, V = 0;
  bool want_nsp = false;
  int no_speech = -1;        // the <|nospeech|> token (want_nsp)
  int* tok[2] = {};          // the steps' token rows [batch][T_max]; a group decode has two (the beam step gathers from one into the other)
  int* tok_pre = nullptr;    // the prefill's token rows [B][T_max]: tok[0], or, a group decode, rows of their own behind the two buffers
  size_t half_elems = 0;     // halfs in one self-attention cache [L][2][batch][T_max][d]; a group decode has two
  float* nsp = nullptr;      // no_speech_prob [B]
  int* n_done = nullptr;     // completion counters
  DecodeSelectArgs sel{};    // whole batch; the per-step fields (tokens, cur_len ...) are the loop's
  BeamScratch bs{};
  // whisper's loop ends when every row has produced EOT (`need` rows; the beam step counts audios): the counter of this step, read back (a
  // host sync; the loop asks every 4 steps: a late stop only costs time, finished rows keep emitting EOT)
  int all_done(const int* counter, int need, bool* done) const {
    HIPCHK(hipMemcpyAsync(e->dec_done_host, counter, sizeof(int), hipMemcpyDeviceToHost, s2));
    HIPCHK(hipStreamSynchronize(s2));
    *done = e->dec_done_host[0] >= need;
    return WCA_OK;
  }
};

// Takes the state to decode (phase 1 first where a mel / PCM is given), sizes the decode buffers, uploads the token rows (row b's initial
// tokens, then eot), the per-row tables (-> e->dec_rows) and the masks, zeroes sum_logprob [batch] / no_speech_prob [B], the completion
// counters behind them (one per position of a uniform call, else one per choice) and the beam's scratch. A prefill also leaves the <|sot|>
// logits (rows [B, 2 B)) and needs the gather scratch.
int decode_begin(wca_engine* e, const wca_decode_desc* d, const DecodeRows& r, const DecodePlan& pl, DecodeLoop* out) {
  const wca_decode_opts* o = d->opts;
  const uint8_t *suppress_mask_host = d->suppress_mask_host, *blank_mask_host = d->blank_mask_host;
  const wca_model_dims& D = e->dims;
  const int V = D.n_vocab, dt = D.n_text_state, L = D.n_text_layer, B = r.batch, G = pl.G(), R = B * G, T_max = r.T_max;
  const bool grouped = pl.gd != nullptr;
  const int n_buf = grouped ? 2 : 1;   // token buffers and cache halves
  // token rows: the n_buf buffers of [R][T_max], then, for a group, the prefill's [B][T_max]
  std::vector<int32_t> init((size_t)(grouped ? 2 * R + B : R) * T_max, o->eot);
  for (size_t row = 0; row < init.size() / T_max; ++row) {
    const int b = row < (size_t)n_buf * R ? (int)(row % R) / G : (int)row - n_buf * R;
    std::copy(r.init(b), r.init(b) + r.ni(b), init.begin() + row * T_max);
  }
  DecodeLoop& lp = *out;
  lp.e = e;
  lp.batch = R;
  lp.B = B;
  lp.T_max = T_max;
  lp.V = V;
  WCA_TRY(decode_take_state(e, d->mel_dev, d->pcm_dev, d->pcm_stride, d->n_samples_host, B, &lp.st, d->redecode == 1));
  lp.kvbuf = lp.st->slot ? e->kv_alt : e->kv;
  hipStream_t s2 = lp.s2 = e->stream2;
  lp.half_elems = (size_t)L * 2 * R * T_max * dt;
  e->dec_cache_off = 0;
  e->dec_batch = e->dec_T_max = e->dec_logits_rows = 0;
  if (grouped) e->grp_steps = e->grp_rows = 0;
  HIPCHK(e->dec_cache.ensure(sizeof(half_t) * n_buf * lp.half_elems));
  HIPCHK(e->dec_tokens.ensure(sizeof(int) * init.size()));
  HIPCHK(e->dec_masks.ensure((size_t)2 * V));
  const float* nsp_host = grouped ? pl.gd->no_speech_prob_host : d->no_speech_prob_host;
  lp.want_nsp = nsp_host && o->no_speech >= 0 && o->no_speech < V;
  lp.no_speech = o->no_speech;
  // the prefill's logits: rows [0, B) at the last initial position, rows [B, 2B) at <|sot|>; a group's steps: R rows
  const int logits_rows = grouped ? std::max(R, 2 * B) : ((pl.n_prefill && lp.want_nsp) ? 2 : 1) * B;
  HIPCHK(e->dec_logits.ensure(sizeof(float) * (size_t)logits_rows * V));
  const size_t state_bytes = sizeof(float) * (R + B) + sizeof(int) * (size_t)(pl.tab ? r.S : T_max);
  HIPCHK(e->dec_state.ensure(state_bytes));
  if (pl.n_prefill) HIPCHK(e->dec_gather.ensure(sizeof(float) * 2 * (size_t)B * dt));
  if (pl.tab) HIPCHK(e->dec_rows.ensure(sizeof(int) * pl.tab->host.size()));
  if (pl.beam()) {
    lp.bs = beam_scratch(R, B, G + 1, pl.gd->max_candidates, T_max, r.S);
    HIPCHK(e->dec_beam.ensure(sizeof(int) * lp.bs.words));
    HIPCHK(hipMemsetAsync(e->dec_beam.p, 0, sizeof(int) * lp.bs.words, s2));
  }
  if (!e->dec_done_host) HIPCHK(hipHostMalloc((void**)&e->dec_done_host, sizeof(int) * 4, hipHostMallocDefault));
  lp.tok[0] = (int*)e->dec_tokens.p;
  lp.tok[1] = grouped ? lp.tok[0] + (size_t)R * T_max : nullptr;
  lp.tok_pre = lp.tok[0] + (size_t)(grouped ? 2 * R : 0) * T_max;
  unsigned char* masks = (unsigned char*)e->dec_masks.p;
  float* sum_lp = (float*)e->dec_state.p;
  lp.nsp = sum_lp + R;
  lp.n_done = (int*)(lp.nsp + B);
  HIPCHK(hipMemcpyAsync(lp.tok[0], init.data(), sizeof(int) * init.size(), hipMemcpyHostToDevice, s2));
  if (pl.tab) HIPCHK(hipMemcpyAsync(e->dec_rows.p, pl.tab->host.data(), sizeof(int) * pl.tab->host.size(), hipMemcpyHostToDevice, s2));
  HIPCHK(hipMemcpyAsync(masks, suppress_mask_host, V, hipMemcpyHostToDevice, s2));
  if (blank_mask_host) HIPCHK(hipMemcpyAsync(masks + V, blank_mask_host, V, hipMemcpyHostToDevice, s2));
  HIPCHK(hipMemsetAsync(e->dec_state.p, 0, state_bytes, s2));
  HIPCHK(hipStreamSynchronize(s2));  // `init` / the tables are pageable host memory
  DecodeSelectArgs& sel = lp.sel;
  sel.logits = (const float*)e->dec_logits.p;
  sel.ld = V;
  sel.n_vocab = V;
  sel.T_max = T_max;
  sel.n_initial = pl.n_initial;
  sel.suppress_mask = masks;
  sel.blank_mask = blank_mask_host ? masks + V : nullptr;
  sel.eot = o->eot;
  sel.timestamp_begin = o->timestamp_begin;
  sel.apply_timestamp_rules = o->apply_timestamp_rules;
  sel.max_initial_timestamp_index = o->max_initial_timestamp_index;
  sel.sum_logprob = sum_lp;
  sel.n_done = lp.n_done;
  if (pl.tab) {
    const int* tab_dev = (const int*)e->dec_rows.p;
    sel.n_initial_rows = tab_dev + 2 * (size_t)R;
    sel.cap_rows = tab_dev + 3 * (size_t)R;
    if (pl.tab->sampled) {
      sel.seed_rows = (const unsigned long long*)(tab_dev + pl.tab->seed_at);
      sel.temperature_rows = (const float*)(tab_dev + pl.tab->temp_at);
    }
  }
  return WCA_OK;
}

// The beam step's merge at choice c, from buffer cur_tok into the other one; sel: that choice's select arguments.
BeamMergeArgs beam_merge_args(const DecodeLoop& lp, const DecodePlan& pl, const DecodeSelectArgs& sel, int c, int cur_tok) {
  int* bw = (int*)lp.e->dec_beam.p;
  const BeamScratch& bs = lp.bs;
  BeamMergeArgs m{};
  m.cand_tok = bw + bs.cand_tok;
  m.cand_lp = (const float*)(bw + bs.cand_lp);
  m.K = pl.G() + 1;
  m.G = pl.G();
  m.tok_in = lp.tok[cur_tok];
  m.tok_out = lp.tok[cur_tok ^ 1];
  m.T_max = lp.T_max;
  m.sum_logprob = sel.sum_logprob;
  m.src = bw + bs.src;
  m.cur_len_rows = sel.cur_len_rows;
  m.n_initial_rows = sel.n_initial_rows;
  m.cap_rows = sel.cap_rows;
  m.first = c == 0;
  m.eot = sel.eot;
  m.max_candidates = pl.gd->max_candidates;
  m.fin_n = bw + bs.fin_n;
  m.fin_len = bw + bs.fin_len;
  m.fin_sum = (float*)(bw + bs.fin_sum);
  m.fin_tok = bw + bs.fin_tok;
  m.trace = bw + bs.trace + (size_t)c * lp.batch * 2;
  m.n_done = sel.n_done + c;
  return m;
}

// The token rows (buffer `tok`), sum_logprob and no_speech_prob of a loop that made `steps` choices to the host. Decoder row (b, g) holds
// its audio's initial tokens and has written positions [0, n_have) with n_have = n_initial + min(steps, its budget). It goes to a slot of
// audio b: slot g of G (samples), the one slot of wca_decode's [B][T_max], or, beam search, upstream's finalize: the finished list in the
// order it filled, topped up to G from the live beams, which the merge leaves in descending order of sum_logprob. n_tokens of a slot = the
// row's first sampled EOT (or n_have), or the finished sequence's length: tokens_out[slot][n_initial : n_tokens] are the sampled tokens,
// and positions behind them hold EOT. Marks the state decoded and records what the test accessors report.
int decode_read_back(const DecodeLoop& lp, const DecodePlan& pl, const DecodeRows& r, int steps, int step_positions, const int* tok,
                     const wca_decode_desc* d) {
  wca_engine* e = lp.e;
  const wca_group_desc* gd = pl.gd;
  const int R = lp.batch, B = lp.B, G = pl.G(), T_max = lp.T_max, eot = d->opts->eot, MC = pl.beam() ? gd->max_candidates : 1;
  const int n_slot = pl.beam() ? std::max(G, MC) : G;
  int32_t *tokens_out = gd ? gd->tokens_out_host : d->tokens_out_host, *n_tokens = gd ? gd->n_tokens_host : d->n_tokens_host;
  float *sum_out = gd ? gd->sum_logprob_host : d->sum_logprob_host, *nsp_out = gd ? gd->no_speech_prob_host : d->no_speech_prob_host;
  const BeamScratch& bs = lp.bs;
  std::vector<int32_t> toks((size_t)R * T_max), fin(bs.trace - bs.fin_n);
  std::vector<float> sums((size_t)R + B);   // sum_logprob [R], no_speech_prob [B] at the head of dec_state
  HIPCHK(hipMemcpyAsync(toks.data(), tok, sizeof(int) * toks.size(), hipMemcpyDeviceToHost, lp.s2));
  HIPCHK(hipMemcpyAsync(sums.data(), e->dec_state.p, sizeof(float) * sums.size(), hipMemcpyDeviceToHost, lp.s2));
  if (pl.beam()) HIPCHK(hipMemcpyAsync(fin.data(), (const int*)e->dec_beam.p + bs.fin_n, sizeof(int) * fin.size(), hipMemcpyDeviceToHost, lp.s2));
  HIPCHK(hipStreamSynchronize(lp.s2));
  const int32_t *fin_n = fin.data(), *fin_len = fin_n + (bs.fin_len - bs.fin_n), *fin_tok = fin_n + (bs.fin_tok - bs.fin_n);
  const float* fin_sum = (const float*)(fin_n + (bs.fin_sum - bs.fin_n));
  std::fill(tokens_out, tokens_out + (size_t)B * n_slot * T_max, eot);
  for (int b = 0; b < B; ++b) {
    const int ni = r.ni(b), n_have = ni + std::min(steps, r.sl(b));
    int n_out = 0;
    auto put = [&](const int32_t* row, int n_tok, float sum) {
      const size_t slot = (size_t)b * n_slot + n_out++;
      std::copy(row, row + n_tok, tokens_out + slot * T_max);
      n_tokens[slot] = n_tok;
      if (sum_out) sum_out[slot] = sum;
    };
    if (pl.beam()) {
      for (int q = 0; q < fin_n[b]; ++q) put(fin_tok + ((size_t)b * MC + q) * T_max, fin_len[(size_t)b * MC + q], fin_sum[(size_t)b * MC + q]);
      for (int g = 0; g < G && n_out < G; ++g)   // the live beams, best first; a dead beam (-inf) is no sequence
        if (std::isfinite(sums[(size_t)b * G + g])) put(toks.data() + ((size_t)b * G + g) * T_max, n_have, sums[(size_t)b * G + g]);
    } else {
      for (int g = 0; g < G; ++g) {
        const int32_t* row = toks.data() + ((size_t)b * G + g) * T_max;
        int n = n_have;
        for (int i = ni; i < n_have; ++i)   // a finished row keeps emitting EOT: nothing but EOT lies behind the first one
          if (row[i] == eot) {
            n = i;
            break;
          }
        put(row, n, sums[(size_t)b * G + g]);
      }
    }
    for (int q = n_out; q < n_slot; ++q) {
      n_tokens[(size_t)b * n_slot + q] = 0;
      sum_out[(size_t)b * n_slot + q] = 0.f;
    }
    if (gd) gd->n_out_host[b] = n_out;
    if (lp.want_nsp) nsp_out[b] = sums[(size_t)R + b];
  }
  lp.st->decoded = true;
  e->last_batch = B;
  e->dec_prefill_positions = pl.n_prefill;
  e->dec_step_positions = step_positions;
  e->dec_batch = R;
  e->dec_T_max = T_max;
  // a prefill leaves the <|sot|> rows behind the last position's; a group's steps leave their R rows
  e->dec_logits_rows = gd ? R : (pl.n_prefill && lp.want_nsp ? 2 : 1) * B;
  if (pl.beam()) {
    e->grp_steps = steps;
    e->grp_rows = R;
    e->grp_trace_off = sizeof(int) * bs.trace;
  }
  return WCA_OK;
}

// The loop over forwards: forward f feeds one position of every row (or, the prefill, all initial ones of every audio) and, from f = n_warm
// on, makes choice c = f - n_warm: decode_select, or the beam step. Ends after `budget` choices or when every row has produced EOT (or used
// its own budget; beam search: every audio's finished list is full), asked every 4 choices. The uniform form launches the scalar kernels
// with n_done indexed by cur_len, the per-row form the table kernels with n_done indexed by c. Then the results to the host
// (decode_read_back).
int decode_run(wca_engine* e, const wca_decode_desc* d, const DecodeRows& r, const DecodePlan& pl) {
  DecodeLoop lp;
  WCA_TRY(decode_begin(e, d, r, pl, &lp));
  const int R = lp.batch, B = lp.B, G = pl.G(), V = lp.V, T_max = lp.T_max, L = e->dims.n_text_layer, dt = e->dims.n_text_state;
  int* bw = (int*)e->dec_beam.p;
  float* logits = (float*)e->dec_logits.p;
  half_t* cache = (half_t*)e->dec_cache.p;
  const int* tab = pl.tab ? (const int*)e->dec_rows.p : nullptr;
  int steps = 0, step_positions = 0, cur_tok = 0, cur_cache = 0;   // the token buffer and the cache half the next step reads
  for (int f = 0; f < pl.n_warm + pl.budget; ++f) {
    const int c = f - pl.n_warm;
    const int t = pl.n_initial - 1 - pl.n_warm + f;                                        // uniform: the position fed
    const int* row = tab ? tab + pl.tab->choice(c) : nullptr;                              // per-row: fed position, key count, cur_len of choice c
    const bool sot_logits = lp.want_nsp && !pl.n_prefill && t == pl.sot_index;             // probs_at_sot of DecodingTask._main_loop
    DecodeSelectArgs sel = lp.sel;
    sel.tokens = lp.tok[cur_tok];
    if (row) {
      sel.cur_len_rows = row + 2 * (size_t)R;
      sel.n_done_idx = c;
    } else {
      sel.cur_len = t + 1;
    }
    if (pl.n_prefill && c == 0) {
      const StepPos last{pl.n_prefill - 1, tab}, sot{lp.want_nsp ? pl.sot_index : -1, lp.want_nsp && tab ? tab + R : nullptr};
      WCA_TRY(run_decode_prefill(e, lp.s2, lp.kvbuf, lp.tok_pre, B, pl.n_prefill, T_max, last, sot));   // a group: into the first half, as planes of B rows
      if (lp.want_nsp) HIPCHK(launch_token_prob(logits + (size_t)B * V, V, V, lp.no_speech, lp.nsp, B, lp.s2));
      if (pl.gd) {
        // every row of a group starts from its audio's logits and cache: logits row b to rows [b G, (b + 1) G), from the back so that no
        // source row is overwritten before it is read; the cache rows [0, n_initial) into the second half, as planes of R rows
        for (int dst = R - 1; dst > 0; --dst)
          if (dst != dst / G)
            HIPCHK(hipMemcpyAsync(logits + (size_t)dst * V, logits + (size_t)(dst / G) * V, sizeof(float) * V, hipMemcpyDeviceToDevice, lp.s2));
        HIPCHK(launch_kv_reorder(cache, cache + lp.half_elems, 2 * L, B, R, T_max, dt, nullptr, G, lp.sel.n_initial_rows, lp.s2));
        cur_cache = 1;
      }
    } else {
      ++step_positions;
      e->dec_cache_off = cur_cache * lp.half_elems;
      WCA_TRY(run_decode_step(e, lp.s2, lp.kvbuf, lp.tok[cur_tok], R, StepPos{t, row}, T_max, c >= 0 || sot_logits, G));
      if (sot_logits) HIPCHK(launch_token_prob(logits, V, V, lp.no_speech, lp.nsp, B, lp.s2));
    }
    if (c < 0) continue;
    if (pl.beam()) {
      const BeamMergeArgs m = beam_merge_args(lp, pl, sel, c, cur_tok);
      HIPCHK(launch_beam_topk(BeamTopkArgs{sel, m.K, bw + lp.bs.cand_tok, (float*)(bw + lp.bs.cand_lp)}, R, lp.s2));
      HIPCHK(launch_beam_merge(m, B, lp.s2));
      cur_tok ^= 1;
      if (c > 0) {   // the cache rows follow their beams: key count of this step's forward
        HIPCHK(launch_kv_reorder(cache + cur_cache * lp.half_elems, cache + (cur_cache ^ 1) * lp.half_elems, 2 * L, R, R, T_max, dt, m.src, 1,
                                 row + R, lp.s2));
        cur_cache ^= 1;
      }
    } else {
      HIPCHK(launch_decode_select(sel, R, lp.s2));
    }
    steps = c + 1;
    if ((steps & 3) == 0 && steps < pl.budget) {
      bool done = false;
      WCA_TRY(lp.all_done(lp.n_done + (row ? c : t + 1), pl.beam() ? B : R, &done));
      if (done) break;
    }
  }
  e->dec_cache_off = cur_cache * lp.half_elems;
  return decode_read_back(lp, pl, r, steps, step_positions, lp.tok[cur_tok], d);
}

// The uniform decode (per_row 0): every row holds the same n_initial tokens; the scalar kernels, with or without a prefill.
int decode_uniform(wca_engine* e, const wca_decode_desc* d, const DecodeRows& r) {
  const int n_initial = r.ni(0);
  const bool prefill = d->prefill == 1;
  // sampling starts after the last initial token
  return decode_run(e, d, r, DecodePlan{prefill ? n_initial : 0, prefill ? 0 : n_initial - 1, r.S, n_initial, r.sot(0), nullptr, nullptr});
}

// The decode of a batch whose rows carry initial tokens of their own (per_row 1; transcribe_batch: every recording's prompt is its own
// previous text), and, gd, every group decode. Row b holds n_initial[b] tokens and samples at most sample_len[b]; at loop step s (0 = the
// prefill's choice) it is at cur_len = n_initial[b] + s. Prefill: every row padded with eot to n_max = max n_initial (a valid query never
// sees a later position, and the K/V that the pad positions leave in cache slots >= n_initial[b] are overwritten by the step loop before
// they are read); steps: the per-row forms of embed_step / KV append / one-query attention / decode_select, fed from the small device
// tables of decode_tables. A row past its budget keeps going through the kernels as a finished row at a clamped position (so no positional
// row past n_text_ctx - 1 and no cache slot past T_max - 1 is touched); what it computes is never read.
//
// Sampling (temperature_host / seed_host [batch], else both null): the tables gain the rows' Philox seeds and temperatures, and the select
// step takes its sampling form (upstream GreedyDecoder.update at temperature > 0; decode.hip); everything else is the greedy call.
// redecode: see decode_take_state.
int decode_per_row(wca_engine* e, const wca_decode_desc* d, const DecodeRows& r, const wca_group_desc* gd = nullptr) {
  const DecodeTab tab = decode_tables(r, gd ? gd->n_group : 1, d->seed_host, d->temperature_host);
  return decode_run(e, d, r, DecodePlan{r.n_max, 0, r.S, 0, -1, &tab, gd});
}

}  // namespace

extern "C" {

int wca_decode(wca_engine* e, const wca_decode_desc* d) {
  if (!e) return fail(WCA_ERR_INVALID, "null engine");
  if (!d) return fail(WCA_ERR_INVALID, "null descriptor");
  if (d->per_row == 1 && !d->prefill) return fail(WCA_ERR_INVALID, "per_row = 1 always runs the batched prefill: pass prefill = 1");
  DecodeRows r{d->batch, d->per_row, d->initial_tokens_host, d->n_initial_host, d->sot_index_host, d->sample_len_host};
  WCA_TRY(decode_check(e, d, &r));
  return d->per_row ? decode_per_row(e, d, r) : decode_uniform(e, d, r);
}

int wca_decode_group(wca_engine* e, const wca_decode_desc* d, const wca_group_desc* g) {
  if (!e) return fail(WCA_ERR_INVALID, "null engine");
  if (!d || !g) return fail(WCA_ERR_INVALID, "null descriptor");
  if (!g->tokens_out_host || !g->n_tokens_host || !g->sum_logprob_host || !g->n_out_host) return fail(WCA_ERR_INVALID, "null argument");
  if (!d->prefill) return fail(WCA_ERR_INVALID, "a group decode always runs the batched prefill: pass prefill = 1");
  if (g->mode != 0 && g->mode != 1) return fail(WCA_ERR_INVALID, "mode %d is neither 0 (beam) nor 1 (samples)", g->mode);
  if (g->n_group < 1 || g->n_group > BEAM_GROUP_MAX) return fail(WCA_ERR_INVALID, "n_group %d outside [1,%d]", g->n_group, BEAM_GROUP_MAX);
  if (g->mode == 0 && d->temperature_host) return fail(WCA_ERR_INVALID, "beam search runs at temperature 0: pass no temperatures");
  if (g->mode == 1 && !d->temperature_host) return fail(WCA_ERR_INVALID, "independent samples need temperature_host and seed_host");
  if (g->mode == 0 && (g->max_candidates < 1 || g->max_candidates > 4096)) return fail(WCA_ERR_INVALID, "max_candidates %d outside [1,4096]", g->max_candidates);
  if (d->batch < 1 || (long)d->batch * g->n_group > e->max_batch)
    return fail(WCA_ERR_INVALID, "batch %d x n_group %d outside [1, max_batch = %d] decoder rows", d->batch, g->n_group, e->max_batch);
  DecodeRows r{d->batch, d->per_row, d->initial_tokens_host, d->n_initial_host, d->sot_index_host, d->sample_len_host};
  WCA_TRY(decode_check(e, d, &r, false));
  return decode_per_row(e, d, r, g);
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
