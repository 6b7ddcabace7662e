// libwca.so engine, forward passes: the GEMM helpers, the encoder, the cross-K/V projection, the decoder (one layer walk and the
// four passes that drive it: teacher-forced in both precision modes, the greedy decode step, the prompted decode's prefill),
// the mel layout change and phase 1 of a micro-batch.
#include "engine_internal.h"

using namespace wca;

namespace wca {

// c_lo > 0 (split mode, f16 output): the value is stored as the pair hi at C, lo at C + c_lo (out_mode 4).
// w_plain / k_plain (pair products only): when the engine holds a W_lo slab and this matrix has non-zero lo elements (an fp32 checkpoint that
// is not exact in f16), the product gets its third term A_hi W_lo^T -- the A_lo W_lo^T term is below 2^-22 of the result like every dropped
// lo.lo term: an accumulating launch for the read-modify-write mode, an f32 scratch added before the activation (GemmArgs.addend) for the others.
// a_lo > 0 is a candidate: plan_gemm says whether the launch as it now stands (the addend included, which the pair kernels do not take)
// gets a pair kernel; where not, the product is the K-doubled call on w_pair.
hipError_t gemm(wca_engine* e, hipStream_t s, Gemm g) {
  if (g.c_lo > 0 && g.out_mode == 0) g.out_mode = 4;
  if (g.w_plain != nullptr && use_wlo(e) && e->wlo_bases.count(g.w_plain)) {
    // A_hi (the hi halves of the pair rows: same row and batch strides, k_plain columns) x W_lo^T ([N][k_plain])
    GemmArgs x = flat(g.A, g.lda, g.w_lo ? g.w_lo : wlo_of(e, g.w_plain), g.k_plain, g.C, g.ldc, g.M, g.N, g.k_plain);
    x.a_rows_per_batch = g.a_rows_per_batch;
    x.a_batch_stride = g.a_batch_stride;
    x.site = g.site;
    x.out_mode = 2;
    if (g.out_mode != 2) {
      GrowBuf& tmp = e->wlo_tmp[s == e->stream ? 0 : 1];
      if (hipError_t he = tmp.ensure((size_t)g.M * g.N * sizeof(float)); he != hipSuccess) return he;
      x.C = tmp.p;
      x.ldc = g.N;
      x.out_mode = 1;
      g.addend = (const float*)tmp.p;
      g.ld_addend = g.N;
    }
    if (hipError_t he = launch_gemm(x, s); he != hipSuccess) return he;
  }
  if (g.a_lo > 0 && !plan_gemm(g, e->n_cu).pair()) {
    g.W = g.w_pair;
    g.K = g.ldw = 2 * g.k_plain;
    g.a_lo = 0;
  }
  return launch_gemm(g, s);
}

namespace {

// profiling: the start (which = 0) / stop (1) event of encoder site `site` (WCA_SITE_*, < 0 = none), layer slot li
void mark_site(wca_engine* e, hipStream_t s, int site, int li, int which) {
  if (e->profiling && site >= 0 && li >= 0 && li < 33) {
    (void)hipEventRecord(e->kev[site][li][which], s);
    e->kev_set[site][li] = true;
  }
}

// One GEMM of the decoder on few rows (a greedy-decode step: M = batch; batch-1 teacher-forced forwards: M = n tokens), on single f16
// operands. g.A32 != nullptr: the A operand is LayerNorm(A32 rows; ln_gamma, ln_beta), xn_scratch its f16 rows where that is a launch
// of its own. g.kv_k != nullptr (QKV projection of a decode step, N = 3 d): the k / v columns go to the self-attention cache
// ([.][kv_tmax][d] planes) at position kv_t, or, kv_t_rows (device [M]) given, row m at its own position (StepPos{kv_t, kv_t_rows}).
// M <= DEC_ROWS_MAX and a shape the few-row kernel takes: one launch (gemm_rows.hip); otherwise the separate LayerNorm / GEMM /
// kv_append launches.
int dec_gemm(wca_engine* e, hipStream_t s, Gemm g, half_t* xn_scratch = nullptr) {
  const bool ln = g.A32 != nullptr;
  const int M = g.M, N = g.N, K = g.K, T_max = g.kv_tmax;
  const DecGemmPlan plan = plan_dec_gemm(M, N, K, ln, g.kv_k != nullptr, DecSkCapacity{e->sk_tiles, e->sk_floats});
  if (e->dec_fused && plan.few_row) {
    g.lda32 = K;
    g.ln_eps = 1e-5f;
    g.splitk = plan.splitk;
    g.sk_part = e->sk_part;
    g.sk_cnt = e->sk_cnt;
    g.kv_bs = (long)T_max * K;
    g.kv_d = g.kv_k ? N / 3 : 0;
    if (!g.kv_k) g.kv_t_rows = nullptr;
    HIPCHK(launch_gemm_rows(g, s));
    return WCA_OK;
  }
  Gemm t = flat(g.A, g.lda, g.W, g.ldw, g.C, g.ldc, M, N, K);
  if (ln) {
    HIPCHK(launch_layernorm_f16(g.A32, g.ln_gamma, g.ln_beta, xn_scratch, M, K, 1e-5f, s));
    t.A = xn_scratch;
    t.lda = K;
  }
  t.bias = g.bias;
  t.gelu = g.gelu;
  t.out_mode = g.out_mode;
  t.site = g.site;
  t.sk_part = e->sk_big[1];
  t.sk_bytes = e->sk_big_bytes;
  HIPCHK(gemm(e, s, t));
  if (g.kv_k) HIPCHK(launch_kv_append(reinterpret_cast<const half_t*>(g.C), g.kv_k, g.kv_v, M, T_max, StepPos{g.kv_t, g.kv_t_rows}, N / 3, s));
  return WCA_OK;
}

// x (f32 residual stream, g.C [M][N]) += A W^T + bias, then xn (f16) = LayerNorm(x) with (gamma, beta): ONE kernel where the
// persistent GEMM can exchange the row statistics between the workgroups of a 256-row panel (gemm_epilogue.h, out_mode 3);
// otherwise (few tiles: small batches) the read-modify-write GEMM followed by the LayerNorm kernel.
// Split mode never fuses: no fused form writes the [hi(N) | lo(N)] rows its consumer reads, and only the separate GEMM adds the
// A_hi W_lo^T term of an inexact checkpoint; the f16 mode has no W_lo term.
// ev (profiling): event slots {site, layer} for the GEMM and for the LayerNorm launch; the fused kernel is timed as the GEMM's site alone.
struct EvSlots {
  int gemm_site, gemm_li, ln_site, ln_li;
};
int gemm_residual_ln(wca_engine* e, hipStream_t s, Gemm g, const float* gamma, const float* beta, half_t* xn, bool allow_fused, const EvSlots& slots) {
  mark_site(e, s, slots.gemm_site, slots.gemm_li, 0);
  GemmArgs f = g;
  f.out_mode = 3;
  f.ln_gamma = gamma;
  f.ln_beta = beta;
  f.ln_out = xn;
  f.ln_ld = g.N;
  f.ln_eps = 1e-5f;
  f.ln_stats = e->ln_stats;
  f.ln_cnt = e->ln_cnt;
  f.ln_err = e->ln_err ? e->ln_err : e->err_dev;
  if (allow_fused && !e->split && plan_gemm(f, e->n_cu).kernel == GemmKernel::Persist256LN) {
    HIPCHK(launch_gemm(f, s));
    mark_site(e, s, slots.gemm_site, slots.gemm_li, 1);
    return WCA_OK;
  }
  g.out_mode = 2;
  g.sk_part = e->sk_big[0];
  g.sk_bytes = e->sk_big_bytes;
  HIPCHK(gemm(e, s, g));
  mark_site(e, s, slots.gemm_site, slots.gemm_li, 1);
  mark_site(e, s, slots.ln_site, slots.ln_li, 0);
  HIPCHK(launch_layernorm_f16(reinterpret_cast<const float*>(g.C), gamma, beta, xn, g.M, g.N, 1e-5f, s, (e->split ? 2 : 1) * g.N, e->split ? g.N : 0));
  mark_site(e, s, slots.ln_site, slots.ln_li, 1);
  return WCA_OK;
}

}  // namespace

// ---- encoder: mel_tm (f16 time-major) -> xn = ln_post(x) (f16) and optionally x (f32)
// Split mode runs the same launches on [hi | lo] operand rows (row width 2 * width, lo half `width` elements after the hi half)
// against the K-doubled weight copies; every producer stores pairs (out_mode 4 / the LayerNorm's lo_off); the fp32 residual
// stream is the same in both modes.
int run_encoder(wca_engine* e, int B) {
  const wca_model_dims& D = e->dims;
  const int d = D.n_audio_state, H = D.n_audio_head;
  const bool sp = e->split;
  const int om = sp ? 2 : 1;  // f16 operand rows: [hi | lo] pairs in split mode
  hipStream_t s = e->stream;
  {
    const int k1 = sp ? e->sw.k1pad : e->k1pad;
    // output frame t lands in padded row t + 1
    Gemm g = flat(e->mel_tm, om * D.n_mels, sp ? e->sw.conv1_w : e->conv1_w, k1, e->h1pad + om * d, om * d, B * N_FRAMES, d, k1);
    g.a_rows_per_batch = N_FRAMES;
    g.a_batch_stride = (long)(N_FRAMES + 2) * om * D.n_mels;
    g.bias = e->conv1_b;
    g.c_rows_per_batch = N_FRAMES;
    g.c_batch_stride = (long)(N_FRAMES + 2) * om * d;
    g.c_lo = sp ? d : 0;
    g.gelu = 1;
    g.site = 3;
    if (sp) {   // inexact conv1 weights: the A_hi W_lo^T term, added before the GELU
      g.w_plain = e->conv1_w;
      g.k_plain = k1;
      g.w_lo = e->sw.conv1_wlo;
    }
    HIPCHK(gemm(e, s, g));
  }
  {
    // stride 2: every other padded frame row
    Gemm g = flat(e->h1pad, 2 * om * d, sp ? e->sw.conv2_w : e->conv2_w, 3 * om * d, e->x, d, B * N_CTX, d, 3 * om * d);
    g.a_rows_per_batch = N_CTX;
    g.a_batch_stride = (long)(N_FRAMES + 2) * om * d;
    g.bias = e->conv2_b;
    g.pos = e->enc_pos;
    g.pos_period = N_CTX;
    g.gelu = 1;
    g.out_mode = 1;
    g.site = 3;
    if (sp) {
      g.w_plain = e->conv2_w;
      g.k_plain = 3 * om * d;
      g.w_lo = e->sw.conv2_wlo;
    }
    HIPCHK(gemm(e, s, g));
  }
  const int M = B * N_CTX;
  const float scale = 1.0f / std::sqrt((float)(d / H));
  memset(e->kev_set, 0, sizeof(e->kev_set));
  auto mark = [&](int site, int li, int which) { mark_site(e, s, site, li, which); };
  // LayerNorms ride in the epilogue of the GEMM that produces their input (gemm_residual_ln) where wca_set_fuse_ln allows it and
  // the mode is f16: mlp_ln in the attention out-projection, the NEXT layer's attn_ln (ln_post after the last layer) in fc2;
  // only layer 0's attn_ln is always a launch
  mark(WCA_SITE_LN1, 0, 0);
  HIPCHK(launch_layernorm_f16(e->x, e->enc[0].ln1_g, e->enc[0].ln1_b, e->xn, M, d, 1e-5f, s, om * d, sp ? d : 0));
  mark(WCA_SITE_LN1, 0, 1);
  for (int li = 0; li < D.n_audio_layer; ++li) {
    const LayerW& l = e->enc[li];
    const LayerW& w2 = sp ? e->sw.enc[li] : l;  // the K-doubled copies [N][2K] = [W | W] (present in split mode)
    mark(WCA_SITE_QKV, li, 0);
    Gemm gq = flat(e->xn, sp, l.qkv_w, w2.qkv_w, d, e->qkv, om * 3 * d, M, 3 * d);
    gq.bias = l.qkv_b;
    gq.c_lo = sp ? 3 * d : 0;
    gq.site = 1;
    HIPCHK(gemm(e, s, gq));
    mark(WCA_SITE_QKV, li, 1);
    AttnArgs a{};
    a.Q = e->qkv;
    a.K = e->qkv + d;
    a.V = e->qkv + 2 * d;
    a.q_bs = a.k_bs = a.v_bs = (long)N_CTX * om * 3 * d;
    a.q_rs = a.k_rs = a.v_rs = om * 3 * d;
    a.O = e->att;
    a.o_bs = (long)N_CTX * om * d;
    a.o_rs = om * d;
    a.split = sp ? 1 : 0;
    a.q_lo = a.k_lo = a.v_lo = 3 * d;
    a.o_lo = d;
    a.nq = N_CTX;
    a.nk = N_CTX;
    a.H = H;
    a.B = B;
    a.scale = scale;
    a.causal = 0;
    mark(WCA_SITE_ATTN, li, 0);
    HIPCHK(launch_attention(a, s));
    mark(WCA_SITE_ATTN, li, 1);
    // sites OUT / FC2 = the GEMM alone (or the fused GEMM + LayerNorm kernel); the LayerNorm launches: mlp_ln = LN2[li], the next
    // layer's attn_ln / ln_post = LN1[li + 1]
    Gemm go = flat(e->att, sp, l.out_w, w2.out_w, d, e->x, d, M, d);
    go.bias = l.out_b;
    go.site = 1;
    WCA_TRY(gemm_residual_ln(e, s, go, l.ln2_g, l.ln2_b, e->xn, e->fuse_ln, {WCA_SITE_OUT, li, WCA_SITE_LN2, li}));
    mark(WCA_SITE_FC1, li, 0);
    Gemm g1 = flat(e->xn, sp, l.fc1_w, w2.fc1_w, d, e->hid, om * 4 * d, M, 4 * d);
    g1.bias = l.fc1_b;
    g1.gelu = 1;
    g1.c_lo = sp ? 4 * d : 0;
    g1.site = 1;
    HIPCHK(gemm(e, s, g1));
    mark(WCA_SITE_FC1, li, 1);
    const bool last = li + 1 == D.n_audio_layer;
    // the LayerNorm behind fc2 feeds the next layer's q / k / v projection, or (ln_post) the cross-K/V projection
    Gemm g2 = flat(e->hid, sp, l.fc2_w, w2.fc2_w, 4 * d, e->x, d, M, d);
    g2.bias = l.fc2_b;
    g2.site = 4;
    WCA_TRY(gemm_residual_ln(e, s, g2, last ? e->lnpost_g : e->enc[li + 1].ln1_g, last ? e->lnpost_b : e->enc[li + 1].ln1_b, e->xn, e->fuse_ln,
                             {WCA_SITE_FC2, li, WCA_SITE_LN1, li + 1}));
  }
  return WCA_OK;
}

// cross-attention K/V of every decoder layer in one GEMM: kv[b*1500 + t][(2l + {0,1})*dt + c]
// skip_last_v: the value projection of the LAST decoder layer (the final dt columns) is only read by that layer's
// P.V product, whose result nobody uses when the caller wants the captured logits but no output logits.
// The rows are pairs [hi(L*2*dt) | lo(L*2*dt)] in split mode.
int run_cross_kv(wca_engine* e, int B, half_t* kvbuf, bool skip_last_v) {
  if (!kvbuf) kvbuf = e->kv;
  const wca_model_dims& D = e->dims;
  const int d = D.n_audio_state, dt = D.n_text_state, L = D.n_text_layer;
  const int n_cols = L * 2 * dt - (skip_last_v ? dt : 0);
  const bool sp = e->split;
  Gemm g = flat(e->xn, sp, e->kv_w, e->sw.kv_w, d, kvbuf, (sp ? 2 : 1) * L * 2 * dt, B * N_CTX, n_cols);
  g.bias = e->kv_b;
  g.c_lo = sp ? (long)L * 2 * dt : 0;
  g.site = 3;
  HIPCHK(gemm(e, e->stream, g));
  return WCA_OK;
}

// ---- decoder
// One pass over decoder layers [l0, l1): what the teacher-forced decoder (both precision modes), the greedy decode step and the
// prompted decode's prefill differ in. Each layer is the same launches: [LN1 + QKV (+ K/V append)], (K/V scatter,) self-attention,
// [out-projection + residual], [LNc + cross query], cross-attention (+ capture), [cross out + residual], [LN2 + fc1 + GELU],
// [fc2 + residual]. The embedding before layer 0 and the final LayerNorm + logits stay with the caller.
struct DecPass {
  hipStream_t s;
  int B, nq;             // B batch rows of nq queries each
  bool pair;             // operands are [hi | lo] rows against the K-doubled weights (the teacher-forced decoder in split mode); otherwise
                         // single f16 operands on plain weights -- in split mode too (prefill and step: whisper.decode runs in fp16)
  const half_t* kv;      // cross-K/V of the batch (rows [hi | lo] in split mode; single operands read the hi halves)
  int kv_group;          // > 1: row b reads the cross-K/V of audio b / kv_group (the beams of wca_decode_group; one-query steps only)
  // self-attention keys: the QKV buffer itself under the causal mask (cache == nullptr), or the cache planes [L][2][B][T_max][d], to
  // which the QKV projection appends position pos and whose first pos + 1 slots the one query attends to. With per-row positions the key
  // counts are the table behind the positions: a step's tables are [B] fed positions, then [B] key counts (the per-row wca_decode)
  half_t* cache;
  int T_max;
  StepPos pos;
  const int* nk_rows() const { return pos.rows ? pos.rows + B : nullptr; }
  half_t* scatter;       // prefill: the cache planes that take each layer's K/V at positions [0, nq) (self-attention stays in place)
  float* cap;            // capture of the cross-attention logits [B][L*H][nq][Fpad] (first Fcap keys), nullable
  int Fpad, Fcap;
  int l0, l1;
  bool stop_at_capture;  // the last layer ends behind its cross-attention: its logits are captured and nothing downstream is read
};

namespace {

// C = act(A W^T + bias), or C += ... (out_mode 2), with A = LayerNorm(g.A32) where given: g describes the product on single operands
// (dec_gemm); pair operands get the LayerNorm launch with a lo half, the pair form of flat() (W2 = the [W | W] copy) and an
// f16 result as a pair
int dec_linear(wca_engine* e, const DecPass& p, Gemm g, const half_t* W2, half_t* xn) {
  if (!p.pair) return dec_gemm(e, p.s, g, xn);
  const bool f16_out = g.out_mode == 0;
  if (g.A32) {
    HIPCHK(launch_layernorm_f16(g.A32, g.ln_gamma, g.ln_beta, xn, g.M, g.K, 1e-5f, p.s, 2 * g.K, g.K));
    g.A = xn;
  }
  Gemm m = flat(g.A, true, g.W, W2, g.K, g.C, (f16_out ? 2 : 1) * g.ldc, g.M, g.N);
  m.bias = g.bias;
  m.gelu = g.gelu;
  m.out_mode = g.out_mode;
  m.site = g.site;
  m.c_lo = f16_out ? g.N : 0;
  m.sk_part = e->sk_big[1];
  m.sk_bytes = e->sk_big_bytes;
  HIPCHK(gemm(e, p.s, m));
  return WCA_OK;
}

// the product of a decoder Linear on single operands: C [M][N] = A [M][K] W [N][K]^T + bias, every row dense
Gemm dec_flat(const half_t* A, const half_t* W, const float* bias, void* C, int M, int N, int K) {
  Gemm g = flat(A, K, W, K, C, N, M, N, K);
  g.bias = bias;
  g.site = 2;
  return g;
}
// the same on A = LayerNorm(x; gamma, beta)
Gemm dec_flat_ln(const float* x, const float* gamma, const float* beta, const half_t* W, const float* bias, void* C, int M, int N, int K) {
  Gemm g = flat(nullptr, 0, W, K, C, N, M, N, K);
  g.A32 = x;
  g.ln_gamma = gamma;
  g.ln_beta = beta;
  g.bias = bias;
  g.site = 2;
  return g;
}

AttnArgs attn_common(const wca_engine* e, const DecPass& p, const half_t* q, int q_rs, half_t* o) {
  const int dt = e->dims.n_text_state, H = e->dims.n_text_head, om = p.pair ? 2 : 1;
  AttnArgs a{};
  a.Q = q;
  a.q_bs = (long)p.nq * q_rs;
  a.q_rs = q_rs;
  a.O = o;
  a.o_bs = (long)p.nq * om * dt;
  a.o_rs = om * dt;
  if (p.pair) {
    a.split = 1;
    a.o_lo = dt;
  }
  a.nq = p.nq;
  a.H = H;
  a.B = p.B;
  a.scale = 1.0f / std::sqrt((float)(dt / H));
  return a;
}

// self-attention of layer li: causal inside the QKV buffer, or the one query of a step against the cached prefix (kc / vc)
AttnArgs self_attn_args(const wca_engine* e, const DecPass& p, const half_t* qkv, half_t* o, const half_t* kc, const half_t* vc) {
  const int dt = e->dims.n_text_state, om = p.pair ? 2 : 1;
  AttnArgs a = attn_common(e, p, qkv, om * 3 * dt, o);
  if (p.cache) {
    a.K = kc;
    a.V = vc;
    a.k_bs = a.v_bs = (long)p.T_max * dt;
    a.k_rs = a.v_rs = dt;
    a.nk = p.pos.rows ? p.T_max : p.pos.t + 1;  // the cache holds exactly the causal prefix (per row: nk_rows[b] of the T_max cached rows)
    a.nk_rows = p.nk_rows();
    return a;
  }
  a.K = qkv + dt;
  a.V = qkv + 2 * dt;
  a.k_bs = a.v_bs = a.q_bs;
  a.k_rs = a.v_rs = a.q_rs;
  if (p.pair) a.q_lo = a.k_lo = a.v_lo = 3 * dt;
  a.nk = p.nq;
  a.causal = 1;
  return a;
}

// cross-attention of layer li over this batch's cross-K/V ([b][1500][L][2][dt], pairs in split mode), with the capture where asked
AttnArgs cross_attn_args(const wca_engine* e, const DecPass& p, int li, const half_t* q, half_t* o) {
  const int dt = e->dims.n_text_state, H = e->dims.n_text_head, L = e->dims.n_text_layer, om = p.pair ? 2 : 1;
  const int kv_ld = (e->split ? 2 : 1) * L * 2 * dt;
  AttnArgs a = attn_common(e, p, q, om * dt, o);
  a.K = p.kv + (size_t)(2 * li) * dt;
  a.V = p.kv + (size_t)(2 * li + 1) * dt;
  a.k_bs = a.v_bs = (long)N_CTX * kv_ld;
  a.k_rs = a.v_rs = kv_ld;
  if (p.pair) {
    a.q_lo = dt;
    a.k_lo = a.v_lo = (long)L * 2 * dt;
  }
  a.cap = p.cap ? p.cap + (size_t)li * H * p.nq * p.Fpad : nullptr;
  a.cap_bs = (long)L * H * p.nq * p.Fpad;
  a.cap_hs = (long)p.nq * p.Fpad;
  a.cap_ld = p.Fpad;
  a.cap_cols = p.Fcap;
  a.nk = N_CTX;
  a.kv_group = p.kv_group;
  return a;
}

int run_decoder_layers(wca_engine* e, const DecPass& p) {
  const int dt = e->dims.n_text_state, L = e->dims.n_text_layer;
  const int M = p.B * p.nq;
  float* xd = e->xd;
  half_t *xdn = e->xdn, *qkv_d = e->qkv_d, *att_d = e->att_d, *q_d = e->q_d, *hid_d = e->hid_d;
  half_t* planes = p.cache ? p.cache : p.scatter;
  const size_t plane = (size_t)p.B * p.T_max * dt;  // one layer's K (or V) cache
  for (int li = p.l0; li < p.l1; ++li) {
    const LayerW& l = e->dec[li];
    const LayerW& w2 = p.pair ? e->sw.dec[li] : l;   // the [W | W] copies
    half_t* kc = planes ? planes + (size_t)(2 * li) * plane : nullptr;
    half_t* vc = planes ? kc + plane : nullptr;
    Gemm g = dec_flat_ln(xd, l.ln1_g, l.ln1_b, l.qkv_w, l.qkv_b, qkv_d, M, 3 * dt, dt);
    if (p.cache) {
      g.kv_k = kc;
      g.kv_v = vc;
      g.kv_tmax = p.T_max;
      g.kv_t = p.pos.t;
      g.kv_t_rows = p.pos.rows;
    }
    WCA_TRY(dec_linear(e, p, g, w2.qkv_w, xdn));
    if (p.scatter) HIPCHK(launch_kv_scatter(qkv_d, kc, vc, p.B, p.nq, p.T_max, dt, p.s));
    HIPCHK(launch_attention(self_attn_args(e, p, qkv_d, att_d, kc, vc), p.s));
    g = dec_flat(att_d, l.out_w, l.out_b, xd, M, dt, dt);
    g.out_mode = 2;
    WCA_TRY(dec_linear(e, p, g, w2.out_w, xdn));
    WCA_TRY(dec_linear(e, p, dec_flat_ln(xd, l.lnc_g, l.lnc_b, l.cq_w, l.cq_b, q_d, M, dt, dt), w2.cq_w, xdn));
    HIPCHK(launch_attention(cross_attn_args(e, p, li, q_d, att_d), p.s));
    if (li == L - 1 && p.stop_at_capture) break;
    g = dec_flat(att_d, l.co_w, l.co_b, xd, M, dt, dt);
    g.out_mode = 2;
    WCA_TRY(dec_linear(e, p, g, w2.co_w, xdn));
    g = dec_flat_ln(xd, l.ln2_g, l.ln2_b, l.fc1_w, l.fc1_b, hid_d, M, 4 * dt, dt);
    g.gelu = 1;
    WCA_TRY(dec_linear(e, p, g, w2.fc1_w, xdn));
    g = dec_flat(hid_d, l.fc2_w, l.fc2_b, xd, M, dt, 4 * dt);
    g.out_mode = 2;
    WCA_TRY(dec_linear(e, p, g, w2.fc2_w, xdn));
  }
  return WCA_OK;
}

// the final LayerNorm and the vocabulary projection of M rows of x -> fp32 logits [M][n_vocab]
int dec_logits(wca_engine* e, const DecPass& p, const float* x, half_t* xn, int M, float* logits) {
  const wca_model_dims& D = e->dims;
  Gemm g = dec_flat_ln(x, e->lnf_g, e->lnf_b, e->tok_emb, nullptr, logits, M, D.n_vocab, D.n_text_state);
  g.out_mode = 1;
  g.site = 3;
  return dec_linear(e, p, g, e->sw.tok_emb, xn);
}

}  // namespace

// The teacher-forced decoder with capture. tokens_dev [B][n]; capture -> cap [B][L*H][n][Fpad] (first Fcap keys).
// Split mode: LayerNorms, GEMMs, causal self-attention and the hooked cross-attention on pairs -- separate LayerNorm launches, the tile
// GEMMs (the few-row kernel of gemm_rows.hip has no pair output), attn_split_kernel; the captured logits are the three-pass fp32 sums and
// every f16 operand row is [hi | lo], twice as wide as in the f16 mode.
// finish_last: the last layer runs to its end (cross-out, ln2, MLP) also without logits_out: e->xd then holds the final residual stream
// (the token log-probs of wca_align_batch_enqueue with vocab_end take it from there)
int run_decoder(wca_engine* e, const int64_t* tokens_dev, int B, int n, float* cap, int Fpad, int Fcap, float* logits_out, hipStream_t s,
                const half_t* kvbuf, bool finish_last) {
  const wca_model_dims& D = e->dims;
  DecPass p{};
  p.s = s ? s : e->stream;
  p.B = B;
  p.nq = n;
  p.pair = e->split;
  p.kv = kvbuf ? kvbuf : e->kv;
  p.cap = cap;
  p.Fpad = Fpad;
  p.Fcap = Fcap;
  p.l1 = D.n_text_layer;
  p.stop_at_capture = !logits_out && !finish_last;
  HIPCHK(launch_embed(tokens_dev, e->tok_emb, e->dec_pos, e->xd, B, n, D.n_text_state, D.n_vocab, e->err_dev, p.s,
                      (e->split && use_wlo(e) && e->wlo_bases.count(e->tok_emb)) ? wlo_of(e, e->tok_emb) : nullptr));
  WCA_TRY(run_decoder_layers(e, p));
  if (logits_out) WCA_TRY(dec_logits(e, p, e->xd, e->xdn, B * n, logits_out));
  return WCA_OK;
}

// One autoregressive step of the greedy ASR pre-pass: position pos of every row (token tokens[b][pos]) through the decoder with the
// self-attention K/V cache (positions 0..pos), cross-attention over this batch's cross-K/V; want_logits: the logits of that position
// -> e->dec_logits (otherwise the step ends with the final residual stream in e->xd).
// pos.rows (a step's tables): row b feeds the token at its OWN position and attends to the cached keys up to it (DecPass::nk_rows).
int run_decode_step(wca_engine* e, hipStream_t s, const half_t* kvbuf, const int* tokens, int B, StepPos pos, int T_max, bool want_logits,
                    int kv_group) {
  const wca_model_dims& D = e->dims;
  DecPass p{};
  p.s = s;
  p.B = B;
  p.nq = 1;
  p.kv = kvbuf;   // split mode: the cross-K/V rows are [hi | lo]; the greedy pre-pass (whisper.decode runs in fp16 itself) reads the hi halves
  p.kv_group = kv_group;
  p.cache = (half_t*)e->dec_cache.p + e->dec_cache_off;
  p.T_max = T_max;
  p.pos = pos;
  p.l1 = D.n_text_layer;
  HIPCHK(launch_embed_step(tokens, T_max, pos, e->tok_emb, e->dec_pos, e->xd, B, D.n_text_state, D.n_vocab, s));
  WCA_TRY(run_decoder_layers(e, p));
  if (want_logits) WCA_TRY(dec_logits(e, p, e->xd, e->xdn, B, (float*)e->dec_logits.p));
  return WCA_OK;
}

// Prefill of a prompted greedy decode (upstream DecodingTask._main_loop, i == 0: the first forward runs every initial token):
// positions [0, n) of all B rows in one teacher-forced pass on M = B n rows, with the f16 decoder's structure but the step
// path's operands -- plain f16 weights and f16 activations in both precision modes (whisper.decode runs in fp16), the
// cross-K/V hi halves in split mode. Each layer's self-attention K/V go into the cache at positions [0, n) ([L][2][B][T_max][d],
// the step loop continues at t = n); each layer's cross-K/V is read once for all n queries of a row. Only the rows whose logits
// are needed get the final LayerNorm and the vocabulary projection: position `last` (the first choice is read there) -> e->dec_logits
// rows [0, B), and, where given, position `sot` -> rows [B, 2B). Scalars (last.t = n - 1; sot.t < 0: no sot logits), or per row where the
// rows hold different numbers of initial tokens, padded to n (the per-row wca_decode: last.rows[b] = n_initial[b] - 1; sot.rows nullable).
int run_decode_prefill(wca_engine* e, hipStream_t s, const half_t* kvbuf, const int* tokens, int B, int n, int T_max, StepPos last, StepPos sot) {
  const int dt = e->dims.n_text_state;
  // the scratch is carved for max_batch x n_text_ctx rows; the GEMMs on more than DEC_ROWS_MAX rows take dec_gemm's separate
  // LayerNorm + gemm() launches, which are given no lo operands, so the products stay single f16 ones in split mode too
  DecPass p{};
  p.s = s;
  p.B = B;
  p.nq = n;
  p.kv = kvbuf;
  p.scatter = (half_t*)e->dec_cache.p + e->dec_cache_off;
  p.T_max = T_max;
  p.l1 = e->dims.n_text_layer;
  HIPCHK(launch_embed_prefix(tokens, T_max, n, e->tok_emb, e->dec_pos, e->xd, B, dt, e->dims.n_vocab, s));
  WCA_TRY(run_decoder_layers(e, p));
  const int R = ((last.rows ? sot.rows != nullptr : sot.t >= 0) ? 2 : 1) * B;
  float* xg = (float*)e->dec_gather.p;
  HIPCHK(launch_gather_rows(e->xd, xg, B, n, last, sot, dt, s));
  return dec_logits(e, p, xg, e->xdn, R, (float*)e->dec_logits.p);
}

}  // namespace wca

namespace {

// mel f32 [B][n_mels][3000] -> time-major f16 image used by the conv GEMM
// row = row length of the image (n_mels, or 2 n_mels in split mode: lo = f16(v - hi) at column lo_off + m)
__global__ void mel_to_tm_kernel(const float* __restrict__ mel, half_t* __restrict__ tm, int n_mels, int B, int row, int lo_off) {
  const int b = blockIdx.y;
  const long e0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e0 >= (long)n_mels * N_FRAMES) return;
  const int t = (int)(e0 / n_mels), m = (int)(e0 - (long)t * n_mels);
  const float v = mel[((long)b * n_mels + m) * N_FRAMES + t];
  const half_t hv = (half_t)v;
  half_t* o = tm + ((long)b * (N_FRAMES + 2) + t + 1) * row + m;
  o[0] = hv;
  if (lo_off) o[lo_off] = (half_t)(v - (float)hv);  // (v is a loaded value: nothing to contract into either conversion)
}

}  // namespace

namespace wca {

int mel_to_tm(wca_engine* e, const float* mel_dev, int batch) {
  const wca_model_dims& D = e->dims;
  const size_t nel = (size_t)D.n_mels * N_FRAMES;
  dim3 grid((unsigned)((nel + 255) / 256), batch);
  hipLaunchKernelGGL(mel_to_tm_kernel, grid, dim3(256), 0, e->stream, mel_dev, e->mel_tm, D.n_mels, batch, (e->split ? 2 : 1) * D.n_mels, e->split ? D.n_mels : 0);
  HIPCHK(hipGetLastError());
  return WCA_OK;
}

// Phase 1 on `stream` for one micro-batch: log-mel (from PCM) or layout change (from a given mel), encoder, cross-K/V of
// every decoder layer into K/V slot `slot`; records ev_kv[slot]. n_samples_dev is only needed with pcm_dev.
int run_phase1(wca_engine* e, const float* mel_dev, const float* pcm_dev, int64_t pcm_stride, const int* n_samples_dev, int batch, int slot,
               bool skip_last_v) {
  half_t* kvbuf = slot ? e->kv_alt : e->kv;
  record(e, 0);
  if (pcm_dev) {
    int rc = run_logmel(e, pcm_dev, pcm_stride, n_samples_dev, batch, nullptr, true);
    if (rc) return rc;
  } else {
    if (int mr = mel_to_tm(e, mel_dev, batch)) return mr;
  }
  record(e, 1);
  e->ln_err = e->err_dev + 1 + slot;
  HIPCHK(hipMemsetAsync(e->ln_err, 0, sizeof(int), e->stream));
  int rc = run_encoder(e, batch);
  e->ln_err = e->err_dev;
  if (!rc) {
    record(e, 2);
    rc = run_cross_kv(e, batch, kvbuf, skip_last_v);
  }
  if (rc) return rc;
  record(e, 3);
  HIPCHK(hipEventRecord(e->ev_kv[slot], e->stream));
  return WCA_OK;
}

}  // namespace wca
