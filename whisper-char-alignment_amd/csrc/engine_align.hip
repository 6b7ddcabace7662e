// libwca.so engine, alignment: the step-by-step API (attentions, filters, DTW, probes), the batched path wca_align_batch_enqueue / _fetch
// with its two phases, wca_encode_batch and the teacher-token log-probs. Each post-processing launch is filled in one place: run_head_stats,
// run_dtw, read_path (the path's way to the host) and res_layout (the pinned results slot, shared by enqueue and fetch).
#include "engine_internal.h"

using namespace wca;

int wca::check_medfilt(int width) {
  if (width < 1 || !(width & 1) || width > 33) return fail(WCA_ERR_INVALID, "median filter width %d must be odd and in [1, 33]", width);
  return WCA_OK;
}

int wca::check_aggregation(const wca_align_opts* o) {
  if (o->aggregation != WCA_AGGR_MEAN && o->aggregation != WCA_AGGR_TOPK) return fail(WCA_ERR_INVALID, "aggregation %d", o->aggregation);
  if (o->aggregation == WCA_AGGR_TOPK && o->topk < 1) return fail(WCA_ERR_INVALID, "topk must be > 0 (timing.py:92)");
  return WCA_OK;
}

int wca::validate_lengths(int B, int n_tok_max, const int32_t* n_tok, const int32_t* max_frames, int* Fmax_out) {
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

namespace {

// attention maps [L][H][n][F] handed in by the caller
int check_maps(int L, int H, int n, int F) {
  if (L < 1 || H < 1 || n < 1 || n > MAX_TOK) return fail(WCA_ERR_INVALID, "bad shape L=%d H=%d n=%d", L, H, n);
  if (F < 1 || F > N_CTX) return fail(WCA_ERR_TOO_LONG, "F=%d outside [1,%d]", F, N_CTX);
  return WCA_OK;
}

// a cross-K/V slot no queued batch (wca_encode_batch / wca_decode / an un-fetched alignment) still needs
int kv_slot_or_fail(wca_engine* e, int* slot) {
  *slot = take_kv_slot(e);
  return *slot < 0 ? fail(WCA_ERR_STATE, "both cross-K/V slots hold live batches: fetch or consume one first") : WCA_OK;
}

}  // namespace

// One head_stats launch on s over qk [B][LH][n_max][ld]: captured logits, or (input_is_weights) softmaxed maps, of which utterance b's
// n_tok[b] x n_frames[b] corner counts. Column norms go to e->colnorm and scores to e->scores; want_rowstats keeps the per-row (max, sum)
// in e->wws for a later re-materialisation, weights_out takes the dense maps [B][LH][n_max][Fmax]. *h: what was launched.
int wca::run_head_stats(wca_engine* e, hipStream_t s, HeadStatsArgs* h, const float* qk, int ld, bool input_is_weights, float* weights_out,
                        bool want_rowstats, const int* n_tok_dev, const int* n_frames_dev, int n_max, int Fmax, int LH, int B, int medfilt_width,
                        float qk_scale, float w_col, float w_row, float w_cov) {
  HIPCHK(e->colnorm.ensure(sizeof(float) * (size_t)B * LH * Fmax));
  HIPCHK(e->scores.ensure(sizeof(float) * (size_t)B * LH));
  if (want_rowstats) HIPCHK(e->wws.ensure(sizeof(float) * (size_t)B * LH * n_max * 2));
  *h = HeadStatsArgs{};
  h->qk = qk;
  h->qk_bs = (long)LH * n_max * ld;
  h->qk_hs = (long)n_max * ld;
  h->qk_ld = ld;
  h->weights = weights_out;
  h->w_bs = (long)LH * n_max * Fmax;
  h->n_tok = n_tok_dev;
  h->n_frames = n_frames_dev;
  h->n_tok_max = n_max;
  h->n_frames_max = Fmax;
  h->colnorm = (float*)e->colnorm.p;
  h->scores = (float*)e->scores.p;
  h->rowstats = want_rowstats ? (float*)e->wws.p : nullptr;
  h->LH = LH;
  h->B = B;
  h->medfilt_width = medfilt_width;
  h->qk_scale = qk_scale;
  h->w_col = w_col;
  h->w_row = w_row;
  h->w_cov = w_cov;
  h->input_is_weights = input_is_weights ? 1 : 0;
  HIPCHK(launch_head_stats(*h, s));
  return WCA_OK;
}

namespace {

// One DTW launch on s over P problems (matrix + p * m_bs, rows ld apart): N_dev[p] x M_dev[p] each, within N_max x M_max, or (both null) all
// N_max x M_max. Trace, path and path length go to e->trace / e->path / e->pathlen; jump_ld > 0 also asks for the jump frames in e->jump, rows
// jump_ld apart. open_dev ([P] device flags, 1 = open end) or open_all asks for the open-end kernel: the end rows [P] and then the scores [P]
// land in e->dtw_out, and a closed problem of such a launch gets what the closed kernel gives it (end row N - 1).
// launched (nullable): the arguments of that launch, for run_path_score behind it. win_lo_dev / win_hi_dev ([P][win_ld] device, both or
// neither): the windowed kernel, on windows the caller has checked (check_windows).
int run_dtw(wca_engine* e, hipStream_t s, const float* matrix, long m_bs, int ld, int P, int N_max, int M_max, const int* N_dev, const int* M_dev,
            int jump_ld, const int* open_dev = nullptr, bool open_all = false, DtwArgs* launched = nullptr, const int* win_lo_dev = nullptr,
            const int* win_hi_dev = nullptr, int win_ld = 0) {
  const int wpr = (M_max + 15) / 16, cap = N_max + M_max + 2;
  HIPCHK(e->trace.ensure(sizeof(uint32_t) * (size_t)P * N_max * wpr));
  HIPCHK(e->path.ensure(sizeof(int) * (size_t)P * 2 * cap));
  HIPCHK(e->pathlen.ensure(sizeof(int) * (size_t)P));
  if (jump_ld) HIPCHK(e->jump.ensure(sizeof(int) * (size_t)P * jump_ld));
  DtwArgs dg{};
  dg.matrix = matrix;
  dg.m_bs = m_bs;
  dg.ld = ld;
  dg.N = N_dev;
  dg.M = M_dev;
  if (!N_dev) dg.N_all = N_max;
  if (!M_dev) dg.M_all = M_max;
  dg.N_max = N_max;
  dg.M_max = M_max;
  dg.trace = (uint32_t*)e->trace.p;
  dg.path = (int*)e->path.p;
  dg.path_len = (int*)e->pathlen.p;
  dg.jump_frame = jump_ld ? (int*)e->jump.p : nullptr;
  dg.jump_ld = jump_ld;
  dg.P = P;
  if (open_dev || open_all) {
    HIPCHK(e->dtw_out.ensure(2 * sizeof(int) * (size_t)P));
    dg.open_end = open_dev;
    dg.open_all = open_all ? 1 : 0;
    dg.end_row = (int*)e->dtw_out.p;
    dg.score = (float*)e->dtw_out.p + P;
  }
  dg.row_lo = win_lo_dev;
  dg.row_hi = win_hi_dev;
  dg.win_ld = win_ld;
  HIPCHK(launch_dtw(dg, s));
  if (launched) *launched = dg;
  return WCA_OK;
}

// The host check of the row windows lo / hi [P][ld] before anything is launched: problem p is n[p] x m[p] (a null n / m: n_all / m_all), and
// only its first n[p] entries are read; a problem without rows has none to check. The windows of an open problem (open[p] != 0, nullable)
// must be full, [0, m - 1] in every row: end-row selection among infinite cells is not defined.
int check_windows(const int32_t* lo, const int32_t* hi, int ld, int P, const int32_t* n, int n_all, const int32_t* m, int m_all, const int32_t* open) {
  for (int p = 0; p < P; ++p) {
    const int np = n ? n[p] : n_all, mp = m ? m[p] : m_all;
    if (np < 1) continue;
    const int32_t *l = lo + (size_t)p * ld, *h = hi + (size_t)p * ld;
    int row = 0;
    if (const char* why = dtw_windows_invalid(l, h, np, mp, &row))
      return fail(WCA_ERR_INVALID, "row windows of problem %d (%d x %d), row %d [%d, %d]: %s", p, np, mp, row, l[row], h[row], why);
    if (open && open[p])
      for (int i = 0; i < np; ++i)
        if (l[i] != 0 || h[i] != mp - 1)
          return fail(WCA_ERR_INVALID, "problem %d is open-ended and row %d has the window [%d, %d]: an open end takes full windows [0, %d] only", p, i,
                      l[i], h[i], mp - 1);
  }
  return WCA_OK;
}

// The per-row path scores of the DTW launch dg (run_dtw's `launched`, which asked for jump frames) on s behind it: e->pscore holds the means
// [P][out_ld] f32 and then the cell counts [P][out_ld], both 0 wherever the kernel writes nothing (columns past dg.N_max).
int run_path_score(wca_engine* e, hipStream_t s, const DtwArgs& dg, int out_ld) {
  const size_t n = (size_t)dg.P * out_ld;
  HIPCHK(e->pscore.ensure(2 * sizeof(int) * n));
  HIPCHK(hipMemsetAsync(e->pscore.p, 0, 2 * sizeof(int) * n, s));
  PathScoreArgs ps{};
  ps.d = dg;
  ps.mean = (float*)e->pscore.p;
  ps.cells = (int*)e->pscore.p + n;
  ps.out_ld = out_ld;
  HIPCHK(launch_path_score(ps, s));
  return WCA_OK;
}

// The ragged DTW on s behind an aggregation that left e->matrix [B][n_max][Fmax] (rows [0, dtwN[b]) x columns [0, n_frames[b]) of utterance b):
// the jump frames land in e->jump [B][n_max]; open_dev, path_scores and the row windows as run_select_aggregate_dtw describes them.
int run_matrix_dtw(wca_engine* e, hipStream_t s, int B, int n_max, int Fmax, int sot_len, const int* dtwN_dev, const int* n_frames_dev,
                   const int* open_dev, bool path_scores, const int* win_lo_dev, const int* win_hi_dev) {
  const int Nmax = n_max - sot_len - 1;
  if (Nmax >= 1) {
    // the DTW writes n_tok[b] - sot_len - 1 entries per utterance; the rest of a row is defined as 0 (the buffer is recycled memory, and a
    // caller that compares or stores whole rows must not see what an earlier allocation left there)
    HIPCHK(e->jump.ensure(sizeof(int) * (size_t)B * n_max));
    HIPCHK(hipMemsetAsync(e->jump.p, 0, sizeof(int) * (size_t)B * n_max, s));
    DtwArgs dg;
    WCA_TRY(run_dtw(e, s, (const float*)e->matrix.p, (long)n_max * Fmax, Fmax, B, Nmax, Fmax, dtwN_dev, n_frames_dev, n_max, open_dev, false, &dg,
                    win_lo_dev, win_hi_dev, n_max));
    if (path_scores) WCA_TRY(run_path_score(e, s, dg, n_max));
  } else {
    if (open_dev) {
      HIPCHK(e->dtw_out.ensure(2 * sizeof(int) * (size_t)B));
      HIPCHK(hipMemsetAsync(e->dtw_out.p, 0xFF, 2 * sizeof(int) * (size_t)B, s));
    }
    if (path_scores) {
      HIPCHK(e->pscore.ensure(2 * sizeof(int) * (size_t)B * n_max));
      HIPCHK(hipMemsetAsync(e->pscore.p, 0, 2 * sizeof(int) * (size_t)B * n_max, s));
    }
  }
  return WCA_OK;
}

// The path of the N x M DTW that `stream` ran last on one problem, to the host: path_len entries of (text_idx, time_idx), which the kernel
// leaves right-aligned in rows of N + M + 2. The copies a caller wants with it share the one synchronisation: the first N rows of e->matrix
// (matrix_host), the keff selected heads and their scores (sel_idx_host / sel_score_host).
int read_path(wca_engine* e, int N, int M, int32_t* text_idx_host, int32_t* time_idx_host, int32_t* path_len_host, float* matrix_host = nullptr,
              int keff = 0, int32_t* sel_idx_host = nullptr, float* sel_score_host = nullptr) {
  const int cap = N + M + 2;
  std::vector<int> path(2 * (size_t)cap);
  int plen = 0;
  HIPCHK(hipMemcpyAsync(&plen, e->pathlen.p, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(path.data(), e->path.p, sizeof(int) * 2 * cap, hipMemcpyDeviceToHost, e->stream));
  if (matrix_host) HIPCHK(hipMemcpyAsync(matrix_host, e->matrix.p, sizeof(float) * (size_t)N * M, hipMemcpyDeviceToHost, e->stream));
  if (sel_idx_host) HIPCHK(hipMemcpyAsync(sel_idx_host, e->sel.p, sizeof(int) * keff, hipMemcpyDeviceToHost, e->stream));
  if (sel_score_host) HIPCHK(hipMemcpyAsync(sel_score_host, e->selsc.p, sizeof(float) * keff, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  *path_len_host = plen;
  if (text_idx_host && time_idx_host)
    for (int i = 0; i < plen; ++i) {
      text_idx_host[i] = path[cap - plen + i];
      time_idx_host[i] = path[cap + cap - plen + i];
    }
  return WCA_OK;
}

}  // namespace

// top-k / aggregate / DTW on s behind the head statistics h of run_head_stats: on the dense maps h read (input_is_weights), or re-derived
// from the captured logits and row statistics h kept. The jump frames land in e->jump [B][n_tok_max]. open_dev: run_dtw's per-utterance
// open-end flags (end rows and scores in e->dtw_out; -1 / NaN where no DTW ran). path_scores: run_path_score behind the DTW, rows n_tok_max
// apart like the jump frames (all 0 where no DTW ran).
int wca::run_select_aggregate_dtw(wca_engine* e, hipStream_t s, const HeadStatsArgs& h, const int* dtwN_dev, const wca_align_opts* o,
                                  int L_layers, const int* open_dev, bool path_scores, const int* win_lo_dev, const int* win_hi_dev) {
  const int B = h.B, LH = h.LH, n_max = h.n_tok_max, Fmax = h.n_frames_max;
  const int k = o->aggregation == WCA_AGGR_TOPK ? o->topk : 0;
  if (o->aggregation == WCA_AGGR_TOPK) {
    HIPCHK(e->sel.ensure(sizeof(int) * (size_t)B * k));
    HIPCHK(e->selsc.ensure(sizeof(float) * (size_t)B * k));
    HIPCHK(launch_topk(h.scores, LH, B, k, (int*)e->sel.p, (float*)e->selsc.p, s));
  }
  HIPCHK(e->matrix.ensure(sizeof(float) * (size_t)B * n_max * Fmax));
  AggregateArgs g{};
  g.w_bs = (long)LH * n_max * Fmax;
  g.n_tok_max = n_max;
  g.n_frames_max = Fmax;
  g.colnorm = h.colnorm;
  g.LH = LH;
  g.B = B;
  g.n_tok = h.n_tok;
  g.n_frames = h.n_frames;
  g.row_lo = o->sot_len;
  g.row_hi_trim = 1;
  g.matrix = (float*)e->matrix.p;
  if (h.input_is_weights) {
    g.weights = h.qk;
  } else {
    g.qk = h.qk;
    g.qk_bs = h.qk_bs;
    g.qk_hs = h.qk_hs;
    g.qk_ld = h.qk_ld;
    g.rowstats = h.rowstats;
    g.medfilt_width = h.medfilt_width;
    g.qk_scale = h.qk_scale;
  }
  if (o->aggregation == WCA_AGGR_TOPK) {
    g.sel_idx = (const int*)e->sel.p;
    g.n_sel = k;
  } else {
    const int H = LH / L_layers;
    g.head_lo = (L_layers / 2) * H;  // ws[n_layers//2:]  (timing.py:88)
  }
  HIPCHK(launch_aggregate(g, s));
  record(e, 6, s);

  return run_matrix_dtw(e, s, B, n_max, Fmax, o->sot_len, dtwN_dev, h.n_frames, open_dev, path_scores, win_lo_dev, win_hi_dev);
}

int wca::check_heads(const int32_t* heads_host, int n_heads, int LH) {
  if (n_heads < 1) return fail(WCA_ERR_INVALID, "empty alignment head list");
  if (n_heads > LH) return fail(WCA_ERR_INVALID, "%d alignment heads for a model of %d", n_heads, LH);
  for (int i = 0; i < n_heads; ++i)
    if (heads_host[i] < 0 || heads_host[i] >= LH) return fail(WCA_ERR_INVALID, "alignment head %d outside [0, %d)", heads_host[i], LH);
  return WCA_OK;
}

// upstream's post-processing (align_heads.hip) of the S heads heads_dev on s over qk [B][LH][n_max][ld], in place of head statistics, top-k
// and aggregation: the row statistics land in e->wws [B][S][n_max][2], the column statistics in e->colnorm [B][S][Fmax][2], the matrix in
// e->matrix, and the ragged closed DTW behind it leaves the jump frames in e->jump. Of o only sot_len, medfilt_width and qk_scale are read.
int wca::run_align_heads(wca_engine* e, hipStream_t s, const float* qk, int ld, const int* heads_dev, int S, const int* n_tok_dev,
                         const int* n_frames_dev, const int* dtwN_dev, int n_max, int Fmax, int LH, int B, const wca_align_opts* o) {
  HIPCHK(e->wws.ensure(sizeof(float) * (size_t)B * S * n_max * 2));
  HIPCHK(e->colnorm.ensure(sizeof(float) * (size_t)B * S * Fmax * 2));
  HIPCHK(e->matrix.ensure(sizeof(float) * (size_t)B * n_max * Fmax));
  AlignHeadsArgs a{};
  a.qk = qk;
  a.qk_bs = (long)LH * n_max * ld;
  a.qk_hs = (long)n_max * ld;
  a.qk_ld = ld;
  a.heads = heads_dev;
  a.S = S;
  a.n_tok = n_tok_dev;
  a.n_frames = n_frames_dev;
  a.n_tok_max = n_max;
  a.n_frames_max = Fmax;
  a.B = B;
  a.sot_len = o->sot_len;
  a.medfilt_width = o->medfilt_width;
  a.qk_scale = o->qk_scale;
  a.rowstats = (float*)e->wws.p;
  a.colstats = (float*)e->colnorm.p;
  a.matrix = (float*)e->matrix.p;
  HIPCHK(launch_align_heads(a, s));
  record(e, 5, s);   // (profiling: the head-statistics stage holds the three passes, the aggregation stage nothing)
  record(e, 6, s);
  return run_matrix_dtw(e, s, B, n_max, Fmax, o->sot_len, dtwN_dev, n_frames_dev, nullptr, false, nullptr, nullptr);
}

namespace {

// The pinned results slot of one enqueued batch, in ints: jump frames [batch][n_tok_max], top-k heads [batch][max(k, 1)], two flag words
// (phase 2's, and the one phase 1 raised for the batch's cross-K/V slot), then (token log-probs only) the log-probs [batch][n_tok_max] as f32,
// then (open-end batches only) the end rows [batch] and the scores [batch] as f32, then (path-score batches only) the per-row means
// [batch][n_tok_max] as f32 and the cell counts [batch][n_tok_max].
struct ResLayout {
  size_t jump, sel, flags, lp, open, ps, ints;
};
ResLayout res_layout(int batch, int n_tok_max, int k, bool want_lp, bool want_open = false, bool want_ps = false) {
  ResLayout r;
  r.jump = 0;
  r.sel = r.jump + (size_t)batch * n_tok_max;
  r.flags = r.sel + (size_t)batch * (k > 0 ? k : 1);
  r.lp = r.flags + 2;
  r.open = r.lp + (want_lp ? (size_t)batch * n_tok_max : 0);
  r.ps = r.open + (want_open ? 2 * (size_t)batch : 0);
  r.ints = r.ps + (want_ps ? 2 * (size_t)batch * n_tok_max : 0);
  return r;
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

// One batch's int table that is too long for the metadata ring -- a [na], then b [nb] (nullable) behind it -- to the device on s without a
// synchronisation: through the pinned mirror and device buffer of this enqueue's parity, whose previous batch has been fetched (at most two
// are in flight). A batch has row windows (lo, then hi) or a head list, never both, so the two share the slot. *dev: where a starts.
int stage_table(wca_engine* e, const int32_t* a, size_t na, const int32_t* b, size_t nb, hipStream_t s, const int** dev) {
  const int ws = (int)(e->enq_count & 1);
  const size_t total = na + nb;
  if (e->win_host_ints[ws] < total) {
    if (e->win_host[ws]) (void)hipHostFree(e->win_host[ws]);
    e->win_host[ws] = nullptr;
    e->win_host_ints[ws] = 0;
    HIPCHK(hipHostMalloc((void**)&e->win_host[ws], total * sizeof(int), hipHostMallocDefault));
    e->win_host_ints[ws] = total;
  }
  HIPCHK(e->win_dev[ws].ensure(total * sizeof(int)));
  memcpy(e->win_host[ws], a, na * sizeof(int));
  if (nb) memcpy(e->win_host[ws] + na, b, nb * sizeof(int));
  HIPCHK(hipMemcpyAsync(e->win_dev[ws].p, e->win_host[ws], total * sizeof(int), hipMemcpyHostToDevice, s));
  *dev = (const int*)e->win_dev[ws].p;
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
    Gemm g = flat(xn + (size_t)r0 * om * dt, sp, e->tok_emb, e->sw.tok_emb, dt, lg, ldc, m, vocab_end);
    g.out_mode = 1;
    g.site = 3;
    HIPCHK(gemm(e, s, g));
    HIPCHK(launch_token_logprob(lg, ldc, vocab_end, m, tokens_dev, map + r0, sot_len + 1, out, e->err_dev, ERR_TARGET_VOCAB, s));
  }
  return WCA_OK;
}

}  // namespace

// the DTW of the step-by-step entry points: P problems of N x M on `stream`
static int dtw_dev_common(wca_engine* e, const float* matrix_dev, int P, int N, int M, bool want_jump, const int* open_dev = nullptr,
                          bool open_all = false) {
  if (N < 1 || N > 512 || M < 1 || M > 4096) return fail(WCA_ERR_INVALID, "DTW shape N=%d M=%d unsupported (N<=512, M<=4096)", N, M);
  return run_dtw(e, e->stream, matrix_dev, (long)N * M, M, P, N, M, nullptr, nullptr, want_jump ? N : 0, open_dev, open_all);
}

// head statistics of one utterance's given maps attns_dev [L*H][n][F] (wca_filter_attention's scores); dtwN travels as metadata row 3
static int stats_on_weights(wca_engine* e, const float* attns_dev, int LH, int n, int F, float wc, float wr, float wv, int dtwN, int** rows,
                            HeadStatsArgs* h) {
  int32_t nt = n, nf = F, dn = dtwN;
  WCA_TRY(stage_meta(e, 1, nullptr, &nt, &nf, &dn, rows));
  return run_head_stats(e, e->stream, h, attns_dev, F, true, nullptr, false, rows[1], rows[2], n, F, LH, 1, 1, 1.f, wc, wr, wv);
}

extern "C" {

int wca_get_attentions(wca_engine* e, const float* mel_dev, const int64_t* tokens_dev, int batch, int n_tok, const int32_t* n_tok_host,
                       const int32_t* max_frames_host, int medfilt_width, float qk_scale, float* weights_out_dev,
                       float* logits_out_dev) {
  if (!e || !mel_dev || !tokens_dev || !max_frames_host || !weights_out_dev) return fail(WCA_ERR_INVALID, "null argument");
  if (batch < 1 || batch > e->max_batch) return fail(WCA_ERR_INVALID, "batch %d outside [1,%d]", batch, e->max_batch);
  WCA_TRY(check_medfilt(medfilt_width));
  int Fmax = 0;
  WCA_TRY(validate_lengths(batch, n_tok, n_tok_host, max_frames_host, &Fmax));
  WCA_TRY(check_ready(e));
  WCA_TRY(join_phase2(e));
  const wca_model_dims& D = e->dims;
  const int LH = D.n_text_layer * D.n_text_head;
  const int Fpad = (Fmax + 3) & ~3;
  std::vector<int32_t> ntok(batch);
  for (int b = 0; b < batch; ++b) ntok[b] = n_tok_host ? n_tok_host[b] : n_tok;
  int* rows[4];
  WCA_TRY(stage_meta(e, batch, nullptr, ntok.data(), max_frames_host, nullptr, rows));
  WCA_TRY(mel_to_tm(e, mel_dev, batch));
  int slot;
  WCA_TRY(kv_slot_or_fail(e, &slot));
  half_t* kvbuf = slot ? e->kv_alt : e->kv;
  HIPCHK(hipMemsetAsync(e->err_dev, 0, sizeof(int), e->stream));
  WCA_TRY(run_encoder(e, batch));
  WCA_TRY(run_cross_kv(e, batch, kvbuf));
  HIPCHK(e->cap.ensure(sizeof(float) * (size_t)batch * LH * n_tok * Fpad));
  WCA_TRY(run_decoder(e, tokens_dev, batch, n_tok, (float*)e->cap.p, Fpad, Fmax, logits_out_dev, nullptr, kvbuf));
  HIPCHK(hipMemcpyAsync(e->err_host, e->err_dev, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HeadStatsArgs h;
  WCA_TRY(run_head_stats(e, e->stream, &h, (const float*)e->cap.p, Fpad, false, weights_out_dev, false, rows[1], rows[2], n_tok, Fmax, LH, batch,
                         medfilt_width, qk_scale, 1.f, 1.f, 0.f));
  // this entry point is the reference's synchronous per-utterance call: the host learns here whether a token id was
  // outside the vocabulary (the row was embedded as token 0, never read out of bounds)
  HIPCHK(hipStreamSynchronize(e->stream));
  if (e->err_host[0] & 2) return fail(WCA_ERR_HIP, "LayerNorm statistics hand-off timed out inside a GEMM epilogue (a workgroup of a row panel never arrived)");
  if (e->err_host[0]) return fail(WCA_ERR_INVALID, "a token id is outside the model's vocabulary [0, %d) (tokenizer / checkpoint mismatch?)", D.n_vocab);
  return WCA_OK;
}

int wca_median_filter(wca_engine* e, const float* in_dev, float* out_dev, int64_t rows, int F, int width) {
  if (!e || !in_dev || !out_dev) return fail(WCA_ERR_INVALID, "null argument");
  WCA_TRY(check_medfilt(width));
  WCA_TRY(enter(e));
  HIPCHK(launch_median_filter(in_dev, out_dev, rows, F, width, e->stream));
  return WCA_OK;
}

int wca_filter_attention(wca_engine* e, const float* attns_dev, int L, int H, int n, int F, int topk, float w_colnorm, float w_rownorm,
                         float w_coverage, float* scores_host, int32_t* sel_idx_host, float* sel_score_host) {
  if (!e || !attns_dev) return fail(WCA_ERR_INVALID, "null argument");
  if (topk < 1) return fail(WCA_ERR_INVALID, "topk must be > 0");
  WCA_TRY(check_maps(L, H, n, F));
  WCA_TRY(enter(e));
  const int LH = L * H;
  int* rows[4];
  HeadStatsArgs h;
  WCA_TRY(stats_on_weights(e, attns_dev, LH, n, F, w_colnorm, w_rownorm, w_coverage, 0, rows, &h));
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
  WCA_TRY(check_aggregation(o));
  const int LH = L * H, N = n - o->sot_len - 1;
  if (o->sot_len < 0 || N < 1) return fail(WCA_ERR_INVALID, "n=%d leaves no rows after the [sot_len:-1] slice", n);
  WCA_TRY(check_maps(L, H, n, F));
  WCA_TRY(enter(e));
  int* rows[4];
  HeadStatsArgs h;
  WCA_TRY(stats_on_weights(e, ws_dev, LH, n, F, o->w_colnorm, o->w_rownorm, o->w_coverage, N, rows, &h));
  WCA_TRY(run_select_aggregate_dtw(e, e->stream, h, rows[3], o, L));
  const bool topk = o->aggregation == WCA_AGGR_TOPK;
  return read_path(e, N, F, text_idx_host, time_idx_host, path_len_host, matrix_host, std::min(o->topk, LH), topk ? sel_idx_host : nullptr,
                   topk ? sel_score_host : nullptr);
}

int wca_dtw(wca_engine* e, const float* matrix_host, int N, int M, int32_t* text_idx_host, int32_t* time_idx_host, int32_t* path_len_host) {
  if (!e || !matrix_host || !text_idx_host || !time_idx_host || !path_len_host) return fail(WCA_ERR_INVALID, "null argument");
  if (N < 1 || M < 1) return fail(WCA_ERR_INVALID, "empty DTW matrix");
  WCA_TRY(enter(e));
  HIPCHK(e->tmp0.ensure(sizeof(float) * (size_t)N * M));
  HIPCHK(hipMemcpyAsync(e->tmp0.p, matrix_host, sizeof(float) * (size_t)N * M, hipMemcpyHostToDevice, e->stream));
  WCA_TRY(dtw_dev_common(e, (const float*)e->tmp0.p, 1, N, M, false));
  return read_path(e, N, M, text_idx_host, time_idx_host, path_len_host);
}

int wca_dtw_batch_dev(wca_engine* e, const float* matrix_dev, int P, int N, int M, int32_t* jump_frame_host) {
  if (!e || !matrix_dev || !jump_frame_host) return fail(WCA_ERR_INVALID, "null argument");
  if (P < 1) return fail(WCA_ERR_INVALID, "P < 1");
  WCA_TRY(enter(e));
  WCA_TRY(dtw_dev_common(e, matrix_dev, P, N, M, true));
  HIPCHK(hipMemcpyAsync(jump_frame_host, e->jump.p, sizeof(int) * (size_t)P * N, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return WCA_OK;
}

int wca_dtw_windows(wca_engine* e, const float* matrix_host, int N, int M, const int32_t* row_lo_host, const int32_t* row_hi_host,
                    int32_t* text_idx_host, int32_t* time_idx_host, int32_t* path_len_host) {
  if (!e || !matrix_host || !row_lo_host || !row_hi_host || !text_idx_host || !time_idx_host || !path_len_host) return fail(WCA_ERR_INVALID, "null argument");
  if (N < 1 || N > 512 || M < 1 || M > 4096) return fail(WCA_ERR_INVALID, "DTW shape N=%d M=%d unsupported (N<=512, M<=4096)", N, M);
  WCA_TRY(check_windows(row_lo_host, row_hi_host, N, 1, nullptr, N, nullptr, M, nullptr));
  WCA_TRY(enter(e));
  HIPCHK(e->tmp0.ensure(sizeof(float) * (size_t)N * M));
  HIPCHK(e->dtw_meta.ensure(sizeof(int) * 2 * (size_t)N));
  int* wd = (int*)e->dtw_meta.p;
  HIPCHK(hipMemcpyAsync(e->tmp0.p, matrix_host, sizeof(float) * (size_t)N * M, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(wd, row_lo_host, sizeof(int) * (size_t)N, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(wd + N, row_hi_host, sizeof(int) * (size_t)N, hipMemcpyHostToDevice, e->stream));
  WCA_TRY(run_dtw(e, e->stream, (const float*)e->tmp0.p, (long)N * M, M, 1, N, M, nullptr, nullptr, 0, nullptr, false, nullptr, wd, wd + N, N));
  return read_path(e, N, M, text_idx_host, time_idx_host, path_len_host);   // (synchronises: the caller's pageable buffers are read by then)
}

int wca_dtw_batch_dev_windows(wca_engine* e, const float* matrix_dev, int P, int N, int M, const int32_t* n_rows_host, const int32_t* n_cols_host,
                              const int32_t* row_lo_host, const int32_t* row_hi_host, int32_t* jump_frame_host) {
  if (!e || !matrix_dev || !row_lo_host || !row_hi_host || !jump_frame_host) return fail(WCA_ERR_INVALID, "null argument");
  if (P < 1) return fail(WCA_ERR_INVALID, "P < 1");
  if (N < 1 || N > 512 || M < 1 || M > 4096) return fail(WCA_ERR_INVALID, "DTW shape N=%d M=%d unsupported (N<=512, M<=4096)", N, M);
  // the per-problem tables travel as one block: the row and column counts [P] each, then the windows lo [P][N] and hi [P][N]
  const size_t PN = (size_t)P * N;
  std::vector<int32_t> meta(2 * (size_t)P + 2 * PN);
  for (int p = 0; p < P; ++p) {
    const int n = n_rows_host ? n_rows_host[p] : N, m = n_cols_host ? n_cols_host[p] : M;
    if (n < 1 || n > N || m < 1 || m > M) return fail(WCA_ERR_INVALID, "problem %d is %d x %d, outside [1,%d] x [1,%d]", p, n, m, N, M);
    meta[p] = n;
    meta[(size_t)P + p] = m;
    for (int i = 0; i < N; ++i) {   // (entries past a problem's rows are not read by anyone: defined as 0)
      meta[2 * (size_t)P + (size_t)p * N + i] = i < n ? row_lo_host[(size_t)p * N + i] : 0;
      meta[2 * (size_t)P + PN + (size_t)p * N + i] = i < n ? row_hi_host[(size_t)p * N + i] : 0;
    }
  }
  WCA_TRY(check_windows(row_lo_host, row_hi_host, N, P, meta.data(), N, meta.data() + P, M, nullptr));
  WCA_TRY(enter(e));
  HIPCHK(e->dtw_meta.ensure(sizeof(int) * meta.size()));
  const int* md = (const int*)e->dtw_meta.p;
  HIPCHK(hipMemcpyAsync(e->dtw_meta.p, meta.data(), sizeof(int) * meta.size(), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e->jump.ensure(sizeof(int) * PN));
  HIPCHK(hipMemsetAsync(e->jump.p, 0, sizeof(int) * PN, e->stream));
  WCA_TRY(run_dtw(e, e->stream, matrix_dev, (long)N * M, M, P, N, M, md, md + P, N, nullptr, false, nullptr, md + 2 * (size_t)P, md + 2 * (size_t)P + PN, N));
  HIPCHK(hipMemcpyAsync(jump_frame_host, e->jump.p, sizeof(int) * PN, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));   // (meta is a stack-lifetime host buffer)
  return WCA_OK;
}

int wca_dtw_open(wca_engine* e, const float* matrix_host, int N, int M, int32_t* text_idx_host, int32_t* time_idx_host, int32_t* path_len_host,
                 int32_t* end_row_host, float* score_host) {
  if (!e || !matrix_host || !text_idx_host || !time_idx_host || !path_len_host || !end_row_host) return fail(WCA_ERR_INVALID, "null argument");
  if (N < 1 || M < 1) return fail(WCA_ERR_INVALID, "empty DTW matrix");
  if (N > 512 || M > 4096) return fail(WCA_ERR_INVALID, "DTW shape N=%d M=%d unsupported (N<=512, M<=4096)", N, M);
  WCA_TRY(enter(e));
  HIPCHK(e->tmp0.ensure(sizeof(float) * (size_t)N * M));
  HIPCHK(hipMemcpyAsync(e->tmp0.p, matrix_host, sizeof(float) * (size_t)N * M, hipMemcpyHostToDevice, e->stream));
  WCA_TRY(dtw_dev_common(e, (const float*)e->tmp0.p, 1, N, M, false, nullptr, true));
  HIPCHK(hipMemcpyAsync(end_row_host, e->dtw_out.p, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  if (score_host) HIPCHK(hipMemcpyAsync(score_host, (const float*)e->dtw_out.p + 1, sizeof(float), hipMemcpyDeviceToHost, e->stream));
  return read_path(e, N, M, text_idx_host, time_idx_host, path_len_host);
}

// wca_dtw_batch_dev_open and wca_dtw_path_scores: the ragged, mixed open / closed DTW on `stream`, with the path-score kernel behind it where the
// two score outputs are given
static int dtw_batch_open_common(wca_engine* e, const float* matrix_dev, int P, int N, int M, const int32_t* n_rows_host, const int32_t* n_cols_host,
                                 const int32_t* open_end_host, int32_t* jump_frame_host, int32_t* end_row_host, float* score_host,
                                 float* path_mean_host, int32_t* path_cells_host) {
  const int least = path_mean_host ? 0 : 1;   // (the score entry also takes an empty problem: no path, end row -1, every row (0, 0.0))
  if (P < 1) return fail(WCA_ERR_INVALID, "P < 1");
  if (N < 1 || N > 512 || M < 1 || M > 4096) return fail(WCA_ERR_INVALID, "DTW shape N=%d M=%d unsupported (N<=512, M<=4096)", N, M);
  // the per-problem tables travel as one block: open flags, then (ragged launches) the row and column counts
  std::vector<int32_t> meta(3 * (size_t)P);
  for (int p = 0; p < P; ++p) {
    const int n = n_rows_host ? n_rows_host[p] : N, m = n_cols_host ? n_cols_host[p] : M;
    if (n < least || n > N || m < least || m > M)
      return fail(WCA_ERR_INVALID, "problem %d is %d x %d, outside [%d,%d] x [%d,%d]", p, n, m, least, N, least, M);
    meta[p] = open_end_host && open_end_host[p] ? 1 : 0;
    meta[(size_t)P + p] = n;
    meta[2 * (size_t)P + p] = m;
  }
  WCA_TRY(enter(e));
  HIPCHK(e->dtw_meta.ensure(sizeof(int) * 3 * (size_t)P));
  const int* md = (const int*)e->dtw_meta.p;
  HIPCHK(hipMemcpyAsync(e->dtw_meta.p, meta.data(), sizeof(int) * 3 * (size_t)P, hipMemcpyHostToDevice, e->stream));
  // rows of a problem that the DTW does not write (beyond its own row count) are defined as 0, as on the fused path
  HIPCHK(e->jump.ensure(sizeof(int) * (size_t)P * N));
  HIPCHK(hipMemsetAsync(e->jump.p, 0, sizeof(int) * (size_t)P * N, e->stream));
  DtwArgs dg;
  WCA_TRY(run_dtw(e, e->stream, matrix_dev, (long)N * M, M, P, N, M, md + P, md + 2 * (size_t)P, N, md, false, &dg));
  HIPCHK(hipMemcpyAsync(jump_frame_host, e->jump.p, sizeof(int) * (size_t)P * N, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(end_row_host, e->dtw_out.p, sizeof(int) * (size_t)P, hipMemcpyDeviceToHost, e->stream));
  if (score_host) HIPCHK(hipMemcpyAsync(score_host, (const float*)e->dtw_out.p + P, sizeof(float) * (size_t)P, hipMemcpyDeviceToHost, e->stream));
  if (path_mean_host) {
    WCA_TRY(run_path_score(e, e->stream, dg, N));
    HIPCHK(hipMemcpyAsync(path_mean_host, e->pscore.p, sizeof(float) * (size_t)P * N, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(path_cells_host, (const int*)e->pscore.p + (size_t)P * N, sizeof(int) * (size_t)P * N, hipMemcpyDeviceToHost, e->stream));
  }
  HIPCHK(hipStreamSynchronize(e->stream));   // (meta is a stack-lifetime host buffer)
  return WCA_OK;
}

int wca_dtw_batch_dev_open(wca_engine* e, const float* matrix_dev, int P, int N, int M, const int32_t* n_rows_host, const int32_t* n_cols_host,
                           const int32_t* open_end_host, int32_t* jump_frame_host, int32_t* end_row_host, float* score_host) {
  if (!e || !matrix_dev || !open_end_host || !jump_frame_host || !end_row_host) return fail(WCA_ERR_INVALID, "null argument");
  return dtw_batch_open_common(e, matrix_dev, P, N, M, n_rows_host, n_cols_host, open_end_host, jump_frame_host, end_row_host, score_host, nullptr,
                               nullptr);
}

int wca_dtw_path_scores(wca_engine* e, const float* matrix_dev, int P, int N, int M, const int32_t* n_rows_host, const int32_t* n_cols_host,
                        const int32_t* open_end_host, int32_t* jump_frame_host, int32_t* end_row_host, float* path_mean_host,
                        int32_t* path_cells_host) {
  if (!e || !matrix_dev || !jump_frame_host || !end_row_host || !path_mean_host || !path_cells_host) return fail(WCA_ERR_INVALID, "null argument");
  return dtw_batch_open_common(e, matrix_dev, P, N, M, n_rows_host, n_cols_host, open_end_host, jump_frame_host, end_row_host, nullptr,
                               path_mean_host, path_cells_host);
}

int wca_probe_heads(wca_engine* e, const float* ws_dev, int L, int H, int n, int F, int sot_len, float* scores_host,
                    int32_t* jump_frame_host) {
  if (!e || !ws_dev || !jump_frame_host) return fail(WCA_ERR_INVALID, "null argument");
  const int LH = L * H, N = n - sot_len - 1;
  if (sot_len < 0 || N < 1) return fail(WCA_ERR_INVALID, "n=%d leaves no rows after the [sot_len:-1] slice", n);
  WCA_TRY(check_maps(L, H, n, F));
  WCA_TRY(enter(e));
  int* rows[4];
  HeadStatsArgs h;
  WCA_TRY(stats_on_weights(e, ws_dev, LH, n, F, 1.f, 1.f, 0.f, N, rows, &h));
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
  WCA_TRY(run_dtw(e, e->stream, (const float*)e->matrix.p, (long)n * F, F, LH, N, F, nullptr, nullptr, N));
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
  if (e->probe_LH <= 0) return fail(WCA_ERR_STATE, "wca_probe_strict_tp needs a preceding wca_probe_heads");
  if (n_heads != e->probe_LH) return fail(WCA_ERR_INVALID, "n_heads %d != the %d heads of the preceding wca_probe_heads", n_heads, e->probe_LH);
  if (n_hyp < 0 || n_ref < 0 || n_ref > 512) return fail(WCA_ERR_INVALID, "n_hyp=%d n_ref=%d outside [0, 512]", n_hyp, n_ref);
  for (int i = 0; i < n_hyp; ++i)
    if (word_end_row_host[i] < 0 || word_end_row_host[i] >= e->probe_N)
      return fail(WCA_ERR_INVALID, "word end row %d = %d outside the %d aligned token rows", i, word_end_row_host[i], e->probe_N);
  HIPCHK(hipSetDevice(e->device));
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
  if (L < 1 || H < 1 || n < 1) return fail(WCA_ERR_INVALID, "bad shape L=%d H=%d n=%d", L, H, n);
  if (n > MAX_TOK) return fail(WCA_ERR_TOO_LONG, "n=%d > %d", n, MAX_TOK);
  if (max_frames < 1 || ld < max_frames) return fail(WCA_ERR_INVALID, "max_frames=%d must be in [1, ld=%d]", max_frames, ld);
  if (max_frames > N_CTX) return fail(WCA_ERR_TOO_LONG, "max_frames=%d > %d", max_frames, N_CTX);
  WCA_TRY(check_medfilt(medfilt_width));
  WCA_TRY(enter(e));
  int32_t nt = n, nf = max_frames;
  int* rows[4];
  WCA_TRY(stage_meta(e, 1, nullptr, &nt, &nf, nullptr, rows));
  HeadStatsArgs h;
  return run_head_stats(e, e->stream, &h, qk_dev, ld, false, weights_out_dev, false, rows[1], rows[2], n, max_frames, L * H, 1, medfilt_width,
                        qk_scale, 1.f, 1.f, 0.f);
}

int wca_default_find_alignment(wca_engine* e, const float* ws_dev, int L, int H, int n, int F, const int32_t* heads_host, int n_heads,
                                int sot_len, float* weights_norm_out_dev, float* matrix_host, int32_t* text_idx_host,
                                int32_t* time_idx_host, int32_t* path_len_host) {
  if (!e || !ws_dev || !heads_host || !path_len_host) return fail(WCA_ERR_INVALID, "null argument");
  const int LH = L * H, N = n - sot_len - 1;
  if (n_heads < 1) return fail(WCA_ERR_INVALID, "empty alignment head list");
  WCA_TRY(check_maps(L, H, n, F));
  if (sot_len < 0 || N < 1) return fail(WCA_ERR_INVALID, "n=%d leaves no rows after the [sot_len:-1] slice", n);
  for (int i = 0; i < n_heads; ++i)
    if (heads_host[i] < 0 || heads_host[i] >= LH) return fail(WCA_ERR_INVALID, "alignment head %d out of range", heads_host[i]);
  WCA_TRY(enter(e));
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
  WCA_TRY(dtw_dev_common(e, (const float*)e->matrix.p, 1, N, F, false));
  return read_path(e, N, F, text_idx_host, time_idx_host, path_len_host, matrix_host);
}

// the fused pipeline, enqueued: d->open_end_host [batch] (nullable) makes the DTW of the flagged rows open-ended; row_lo_host / row_hi_host
// [batch][n_tok_max] (both or neither) give every DTW row its permitted frame interval; heads_host [n_heads] (nullable, and then without
// windows) takes the alignment-heads route: upstream's post-processing of those heads in place of head statistics, top-k and aggregation
static int enqueue_batch(wca_engine* e, const wca_align_desc* d, const int32_t* row_lo_host, const int32_t* row_hi_host, const int32_t* heads_host,
                         int n_heads) {
  if (!e || !d || !d->tokens_dev || !d->n_tok_host || !d->max_frames_host || !d->opts) return fail(WCA_ERR_INVALID, "null argument");
  if ((row_lo_host == nullptr) != (row_hi_host == nullptr)) return fail(WCA_ERR_INVALID, "row_lo_host and row_hi_host go together");
  const bool want_win = row_lo_host != nullptr;
  const bool by_heads = heads_host != nullptr;
  if (by_heads) {   // (refused before anything is consumed or enqueued)
    if (d->path_scores) return fail(WCA_ERR_INVALID, "path scores are defined on the [0, 1] aggregation, not on the alignment-heads matrix");
    if (d->open_end_host) return fail(WCA_ERR_INVALID, "the alignment-heads route has no open-ended DTW");
    WCA_TRY(check_heads(heads_host, n_heads, e->dims.n_text_layer * e->dims.n_text_head));
  }
  const float* pcm_dev = d->pcm_dev;
  const int64_t pcm_stride = d->pcm_stride;
  const int64_t* tokens_dev = d->tokens_dev;
  const int32_t *n_samples_host = d->n_samples_host, *n_tok_host = d->n_tok_host, *max_frames_host = d->max_frames_host,
                *open_end_host = d->open_end_host;
  const int n_tok_max = d->n_tok_max, batch = d->batch, vocab_end = d->vocab_end;
  const wca_align_opts* o = d->opts;
  const bool want_open = open_end_host != nullptr;
  const bool want_ps = d->path_scores != 0;
  if (vocab_end < 0 || vocab_end > e->dims.n_vocab) return fail(WCA_ERR_INVALID, "vocab_end %d outside (0, %d] (0 = no token log-probs)", vocab_end, e->dims.n_vocab);
  const bool want_lp = vocab_end > 0;
  const bool reuse_enc = (pcm_dev == nullptr);  // consume the oldest encoded state (wca_encode_batch / wca_decode)
  if (reuse_enc && (e->enc_q.empty() || e->enc_q.front().batch != batch))
    return fail(WCA_ERR_STATE, "pcm_dev == NULL re-uses the oldest state left by wca_encode_batch / wca_decode for the same batch; there is none");
  if (!reuse_enc && !n_samples_host) return fail(WCA_ERR_INVALID, "null argument");
  if (!reuse_enc && !e->enc_q.empty()) {
    // a stand-alone decode (or language detection) may have left its state behind; any other undecoded one is still wanted by its owner
    for (auto& st : e->enc_q)
      if (!st.decoded && !st.detected) return fail(WCA_ERR_STATE, "an encoded batch is waiting for wca_decode / wca_align_batch_enqueue(pcm_dev = NULL)");
    for (auto& st : e->enc_q) e->slot_busy[st.slot] = false;
    e->enc_q.clear();
  }
  if (e->enq_count - e->fetch_count >= 2) return fail(WCA_ERR_STATE, "two batches already in flight: call wca_align_batch_fetch first");
  if (batch < 1 || batch > e->max_batch) return fail(WCA_ERR_INVALID, "batch %d outside [1,%d]", batch, e->max_batch);
  if (!by_heads) WCA_TRY(check_aggregation(o));
  if (by_heads && o->sot_len < 0) return fail(WCA_ERR_INVALID, "sot_len %d < 0", o->sot_len);
  WCA_TRY(check_medfilt(o->medfilt_width));
  int Fmax = 0;
  WCA_TRY(validate_lengths(batch, n_tok_max, n_tok_host, max_frames_host, &Fmax));
  if (!reuse_enc) WCA_TRY(check_pcm_lengths(n_samples_host, batch, pcm_stride));
  WCA_TRY(check_ready(e));
  const wca_model_dims& D = e->dims;
  const int LH = D.n_text_layer * D.n_text_head;
  const int Fpad = (Fmax + 3) & ~3;
  std::vector<int32_t> dn(batch);
  for (int b = 0; b < batch; ++b) {
    dn[b] = n_tok_host[b] - o->sot_len - 1;
    if (dn[b] < 0) dn[b] = 0;
  }
  // (before anything is staged or launched; validate_lengths has bounded n_tok and max_frames)
  if (want_win) WCA_TRY(check_windows(row_lo_host, row_hi_host, n_tok_max, batch, dn.data(), 0, max_frames_host, 0, open_end_host));
  int* rows[4];
  // (re-use: the metadata is only read by phase 2, so it travels on that stream -- `stream` may already hold the next
  // batch's phase 1, and an event recorded behind it would serialise this batch's phase 2 after it)
  hipStream_t s2 = e->overlap ? e->stream2 : e->stream;  // the stream phase 2 runs on
  WCA_TRY(stage_meta(e, batch, reuse_enc ? nullptr : n_samples_host, n_tok_host, max_frames_host, dn.data(), rows, reuse_enc ? s2 : nullptr));
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
    WCA_TRY(stage_meta(e, batch, off.data(), nullptr, nullptr, nullptr, lp_rows, reuse_enc ? s2 : nullptr));
  }
  int* open_rows[4] = {nullptr, nullptr, nullptr, nullptr};
  if (want_open) {
    std::vector<int32_t> flags(batch);
    for (int b = 0; b < batch; ++b) flags[b] = open_end_host[b] ? 1 : 0;
    WCA_TRY(stage_meta(e, batch, flags.data(), nullptr, nullptr, nullptr, open_rows, reuse_enc ? s2 : nullptr));
  }
  // the row windows ([batch][n_tok_max] each, not [batch]) and the head list [n_heads] travel like the metadata, through stage_table
  const int *win_lo_dev = nullptr, *win_hi_dev = nullptr, *heads_dev = nullptr;
  hipStream_t ts = reuse_enc ? s2 : e->stream;
  if (want_win) {
    const size_t n = (size_t)batch * n_tok_max;
    WCA_TRY(stage_table(e, row_lo_host, n, row_hi_host, n, ts, &win_lo_dev));
    win_hi_dev = win_lo_dev + n;
  } else if (by_heads) {
    WCA_TRY(stage_table(e, heads_host, (size_t)n_heads, nullptr, 0, ts, &heads_dev));
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
    WCA_TRY(kv_slot_or_fail(e, &bs));
    e->slot_busy[bs] = true;
    // (without token log-probs this path never reads the last layer's cross-attention output: its value projection is skipped)
    if (int rc = run_phase1(e, nullptr, pcm_dev, pcm_stride, rows[0], batch, bs, /*skip_last_v=*/!want_lp)) {
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
  WCA_TRY(run_decoder(e, tokens_dev, batch, n_tok_max, (float*)e->cap.p, Fpad, Fmax, nullptr, s2, kvbuf, /*finish_last=*/want_lp));
  record(e, 4, s2);
  // the softmaxed maps are NOT materialised on this path (53 MB per utterance): head_stats keeps per-row
  // (max, sum) and the aggregation re-derives the values of the few selected heads from the captured logits
  if (by_heads) {
    WCA_TRY(run_align_heads(e, s2, (const float*)e->cap.p, Fpad, heads_dev, n_heads, rows[1], rows[2], rows[3], n_tok_max, Fmax, LH, batch, o));
  } else {
    HeadStatsArgs h;
    WCA_TRY(run_head_stats(e, s2, &h, (const float*)e->cap.p, Fpad, false, nullptr, true, rows[1], rows[2], n_tok_max, Fmax, LH, batch,
                           o->medfilt_width, o->qk_scale, o->w_colnorm, o->w_rownorm, o->w_coverage));
    record(e, 5, s2);
    WCA_TRY(run_select_aggregate_dtw(e, s2, h, rows[3], o, D.n_text_layer, open_rows[0], want_ps, win_lo_dev, win_hi_dev));
  }
  if (want_lp) {
    HIPCHK(e->lp_out.ensure(sizeof(float) * (size_t)batch * n_tok_max));
    WCA_TRY(run_token_logprobs(e, s2, tokens_dev, batch, n_tok_max, o->sot_len, vocab_end, rows[1], lp_rows[0], lp_R, lp_nmax, (float*)e->lp_out.p));
  }
  record(e, 7, s2);
  // results -> pinned staging (ring of 2 so the host can post-process batch i while batch i+1 runs). The flags of this batch travel with
  // its results: phase 2's word, and the word phase 1 raised for this batch's cross-K/V slot (complete: s2 waited for ev_kv[bs], recorded
  // behind that encoder)
  const int k = !by_heads && o->aggregation == WCA_AGGR_TOPK ? o->topk : 0;
  const int rs = (int)(e->enq_count & 1);
  const ResLayout at = res_layout(batch, n_tok_max, k, want_lp, want_open, want_ps);
  WCA_TRY(ensure_res_host(e, rs, at.ints));
  int* res = e->res_host[rs];
  if (want_lp) HIPCHK(hipMemcpyAsync(res + at.lp, e->lp_out.p, sizeof(float) * (size_t)batch * n_tok_max, hipMemcpyDeviceToHost, s2));
  HIPCHK(hipMemcpyAsync(res + at.flags, e->err_dev, sizeof(int), hipMemcpyDeviceToHost, s2));
  HIPCHK(hipMemcpyAsync(res + at.flags + 1, e->err_dev + 1 + bs, sizeof(int), hipMemcpyDeviceToHost, s2));
  if (n_tok_max - o->sot_len - 1 >= 1) HIPCHK(hipMemcpyAsync(res + at.jump, e->jump.p, sizeof(int) * (size_t)batch * n_tok_max, hipMemcpyDeviceToHost, s2));
  if (k > 0) HIPCHK(hipMemcpyAsync(res + at.sel, e->sel.p, sizeof(int) * (size_t)batch * k, hipMemcpyDeviceToHost, s2));
  if (want_open) HIPCHK(hipMemcpyAsync(res + at.open, e->dtw_out.p, 2 * sizeof(int) * (size_t)batch, hipMemcpyDeviceToHost, s2));
  if (want_ps) HIPCHK(hipMemcpyAsync(res + at.ps, e->pscore.p, 2 * sizeof(int) * (size_t)batch * n_tok_max, hipMemcpyDeviceToHost, s2));
  record(e, 8, s2);
  HIPCHK(hipEventRecord(e->res_ev[rs], s2));
  e->res_batch[rs] = batch;
  e->res_ntok[rs] = n_tok_max;
  e->res_topk[rs] = k;
  e->res_lp[rs] = want_lp;
  e->res_open[rs] = want_open;
  e->res_ps[rs] = want_ps;
  e->res_kvslot[rs] = bs;
  e->last_batch = batch;
  e->enq_count++;
  return WCA_OK;
}

int wca_encode_batch(wca_engine* e, const float* mel_dev, const float* pcm_dev, int64_t pcm_stride, const int32_t* n_samples_host, int batch) {
  if (!e) return fail(WCA_ERR_INVALID, "null engine");
  if ((mel_dev == nullptr) == (pcm_dev == nullptr)) return fail(WCA_ERR_INVALID, "pass exactly one of mel_dev / pcm_dev");
  if (pcm_dev && !n_samples_host) return fail(WCA_ERR_INVALID, "null argument");
  if (batch < 1 || batch > e->max_batch) return fail(WCA_ERR_INVALID, "batch %d outside [1,%d]", batch, e->max_batch);
  if (pcm_dev) WCA_TRY(check_pcm_lengths(n_samples_host, batch, pcm_stride));
  WCA_TRY(check_ready(e));
  int slot;
  WCA_TRY(kv_slot_or_fail(e, &slot));
  int* rows[4] = {nullptr, nullptr, nullptr, nullptr};
  if (pcm_dev) WCA_TRY(stage_meta(e, batch, n_samples_host, nullptr, nullptr, nullptr, rows));
  e->slot_busy[slot] = true;
  if (int rc = run_phase1(e, mel_dev, pcm_dev, pcm_stride, rows[0], batch, slot)) {
    e->slot_busy[slot] = false;
    return rc;
  }
  e->enc_q.push_back({slot, batch, false});
  return WCA_OK;
}

int wca_align_batch_fetch(wca_engine* e, int batch, int n_tok_max, int topk, const wca_align_result* r) {
  if (!e) return fail(WCA_ERR_INVALID, "null engine");
  if (!r) return fail(WCA_ERR_INVALID, "null argument");
  int32_t *jump_frame_host = r->jump_frame_host, *sel_idx_host = r->sel_idx_host, *end_row_host = r->end_row_host;
  float *token_logprob_host = r->token_logprob_host, *score_host = r->score_host;
  if (e->fetch_count >= e->enq_count) return fail(WCA_ERR_STATE, "nothing to fetch");
  const int rs = (int)(e->fetch_count & 1);  // oldest un-fetched batch
  if (batch != e->res_batch[rs] || n_tok_max != e->res_ntok[rs]) return fail(WCA_ERR_STATE, "fetch does not match the oldest pending enqueue");
  if (sel_idx_host && e->res_topk[rs] > 0 && topk != e->res_topk[rs]) return fail(WCA_ERR_STATE, "topk does not match the pending enqueue");
  // (checked before anything is consumed: the caller can fetch the same batch again without them)
  if (token_logprob_host && !e->res_lp[rs]) return fail(WCA_ERR_STATE, "token log-probs requested, but the pending batch was enqueued without them (vocab_end = 0)");
  if ((end_row_host || score_host) && !e->res_open[rs])
    return fail(WCA_ERR_STATE, "end rows requested, but the pending batch was enqueued without open_end_host");
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipEventSynchronize(e->res_ev[rs]));
  const ResLayout at = res_layout(batch, n_tok_max, e->res_topk[rs], e->res_lp[rs], e->res_open[rs], e->res_ps[rs]);
  const int* res = e->res_host[rs];
  if (jump_frame_host) memcpy(jump_frame_host, res + at.jump, sizeof(int) * (size_t)batch * n_tok_max);
  if (sel_idx_host && e->res_topk[rs] > 0) memcpy(sel_idx_host, res + at.sel, sizeof(int) * (size_t)batch * topk);
  if (e->res_kvslot[rs] >= 0) e->slot_busy[e->res_kvslot[rs]] = false;
  e->res_kvslot[rs] = -1;
  e->fetch_count++;
  if (token_logprob_host) memcpy(token_logprob_host, res + at.lp, sizeof(float) * (size_t)batch * n_tok_max);
  if (end_row_host) memcpy(end_row_host, res + at.open, sizeof(int) * (size_t)batch);
  if (score_host) memcpy(score_host, res + at.open + batch, sizeof(float) * (size_t)batch);
  const int flag = res[at.flags] | (res[at.flags + 1] & 2);
  if (flag & 2) return fail(WCA_ERR_HIP, "LayerNorm statistics hand-off timed out inside a GEMM epilogue (a workgroup of a row panel never arrived)");
  if (flag == ERR_TARGET_VOCAB)
    return fail(WCA_ERR_INVALID, "a teacher token is outside the scored vocabulary [0, vocab_end) (its log-prob is NaN)");
  if (flag)
    return fail(WCA_ERR_INVALID, "a token id is outside the model's vocabulary [0, %d) (tokenizer / checkpoint mismatch?)", e->dims.n_vocab);
  return WCA_OK;
}

int wca_align_batch_path_scores(wca_engine* e, int batch, int n_tok_max, float* path_mean_host, int32_t* path_cells_host) {
  if (!e || !path_mean_host || !path_cells_host) return fail(WCA_ERR_INVALID, "null argument");
  if (e->fetch_count >= e->enq_count) return fail(WCA_ERR_STATE, "nothing to fetch");
  const int rs = (int)(e->fetch_count & 1);  // oldest un-fetched batch, which stays pending
  if (batch != e->res_batch[rs] || n_tok_max != e->res_ntok[rs]) return fail(WCA_ERR_STATE, "call does not match the oldest pending enqueue");
  if (!e->res_ps[rs]) return fail(WCA_ERR_STATE, "path scores requested, but the pending batch was enqueued without them (path_scores = 0)");
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipEventSynchronize(e->res_ev[rs]));
  const ResLayout at = res_layout(batch, n_tok_max, e->res_topk[rs], e->res_lp[rs], e->res_open[rs], true);
  const int* res = e->res_host[rs];
  const size_t n = (size_t)batch * n_tok_max;
  memcpy(path_mean_host, res + at.ps, sizeof(float) * n);
  memcpy(path_cells_host, res + at.ps + n, sizeof(int) * n);
  return WCA_OK;
}

int wca_align_batch_enqueue_windows(wca_engine* e, const wca_align_desc* d, const int32_t* row_lo_host, const int32_t* row_hi_host) {
  return enqueue_batch(e, d, row_lo_host, row_hi_host, nullptr, 0);
}

int wca_align_batch_enqueue(wca_engine* e, const wca_align_desc* d) { return enqueue_batch(e, d, nullptr, nullptr, nullptr, 0); }

int wca_align_batch_enqueue_heads(wca_engine* e, const wca_align_desc* d, const int32_t* heads_host, int n_heads) {
  if (!e || !d || !heads_host) return fail(WCA_ERR_INVALID, "null argument");
  return enqueue_batch(e, d, nullptr, nullptr, heads_host, n_heads);
}

int wca_align_batch_heads(wca_engine* e, const wca_align_desc* d, const int32_t* heads_host, int n_heads, const wca_align_result* r) {
  if (!e || !d || !heads_host || !r) return fail(WCA_ERR_INVALID, "null argument");
  WCA_TRY(wca_align_batch_enqueue_heads(e, d, heads_host, n_heads));
  return wca_align_batch_fetch(e, d->batch, d->n_tok_max, 0, r);
}

int wca_align_batch_windows(wca_engine* e, const wca_align_desc* d, const int32_t* row_lo_host, const int32_t* row_hi_host, const wca_align_result* r) {
  if (!e || !d || !r) return fail(WCA_ERR_INVALID, "null argument");
  WCA_TRY(wca_align_batch_enqueue_windows(e, d, row_lo_host, row_hi_host));
  return wca_align_batch_fetch(e, d->batch, d->n_tok_max, d->opts->aggregation == WCA_AGGR_TOPK ? d->opts->topk : 0, r);
}

int wca_align_batch(wca_engine* e, const wca_align_desc* d, const wca_align_result* r) {
  if (!e || !d || !r) return fail(WCA_ERR_INVALID, "null argument");
  WCA_TRY(wca_align_batch_enqueue(e, d));
  return wca_align_batch_fetch(e, d->batch, d->n_tok_max, d->opts->aggregation == WCA_AGGR_TOPK ? d->opts->topk : 0, r);
}

int wca_token_logprobs(wca_engine* e, const float* logits_dev, int rows, int ld, int vocab_end, const int64_t* targets_dev, float* out_dev) {
  if (!e || !logits_dev || !targets_dev || !out_dev) return fail(WCA_ERR_INVALID, "null argument");
  if (vocab_end < 1 || vocab_end > e->dims.n_vocab) return fail(WCA_ERR_INVALID, "vocab_end %d outside (0, %d]", vocab_end, e->dims.n_vocab);
  if (rows < 0 || ld < vocab_end) return fail(WCA_ERR_INVALID, "rows %d / ld %d (need rows >= 0, ld >= vocab_end = %d)", rows, ld, vocab_end);
  WCA_TRY(enter(e));
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
