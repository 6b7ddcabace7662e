// libwca.so engine, kernel-level test entry points (wca_test_*): single kernels and the encoder alone, for tests/ and tools/.
#include "engine_internal.h"

using namespace wca;

namespace {

// out[r][c] = hi + lo of a split row [hi(d) | lo(d)]
__global__ void widen_split_kernel(const half_t* __restrict__ in, float* __restrict__ out, size_t rows, int d) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t st = (size_t)gridDim.x * blockDim.x;
  for (; i < rows * d; i += st) {
    const size_t r = i / d, c = i - r * d;
    out[i] = (float)in[r * 2 * d + c] + (float)in[r * 2 * d + d + c];
  }
}

__global__ void widen_kernel(const half_t* __restrict__ in, float* __restrict__ out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t st = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += st) out[i] = (float)in[i];
}

// dense q / o [B][nq][w], k / v [B][nk][w] with rows of w elements (H * 64, or twice that for [hi | lo] pairs)
AttnArgs dense_attn(const void* q, const void* k, const void* v, void* o, int w, int B, int H, int nq, int nk, int causal) {
  AttnArgs a{};
  a.Q = (const half_t*)q;
  a.K = (const half_t*)k;
  a.V = (const half_t*)v;
  a.O = (half_t*)o;
  a.q_bs = a.o_bs = (long)nq * w;
  a.k_bs = a.v_bs = (long)nk * w;
  a.q_rs = a.k_rs = a.v_rs = a.o_rs = w;
  a.nq = nq;
  a.nk = nk;
  a.H = H;
  a.B = B;
  a.scale = 0.125f;
  a.causal = causal & 1;
  return a;
}

// what both forms of decode_select take
DecodeSelectArgs select_args(const float* logits_dev, int n_vocab, int32_t* tokens_dev, int T_max, const uint8_t* suppress_mask_dev,
                             const uint8_t* blank_mask_dev, const wca_decode_opts* o, float* sum_logprob_dev, int32_t* n_done_dev) {
  DecodeSelectArgs a{};
  a.logits = logits_dev;
  a.ld = n_vocab;
  a.n_vocab = n_vocab;
  a.tokens = tokens_dev;
  a.T_max = T_max;
  a.suppress_mask = suppress_mask_dev;
  a.blank_mask = blank_mask_dev;
  a.eot = o->eot;
  a.timestamp_begin = o->timestamp_begin;
  a.apply_timestamp_rules = o->apply_timestamp_rules;
  a.max_initial_timestamp_index = o->max_initial_timestamp_index;
  a.sum_logprob = sum_logprob_dev;
  a.n_done = n_done_dev;
  return a;
}

}  // namespace

extern "C" {

int wca_test_gemm(wca_engine* e, const void* a, const void* w, const float* bias, void* c, int M, int N, int K, int gelu, int out_mode) {
  if (!e) return fail(WCA_ERR_INVALID, "null engine");
  HIPCHK(hipSetDevice(e->device));
  GemmArgs g = flat((const half_t*)a, K, (const half_t*)w, K, c, N, M, N, K);
  g.bias = bias;
  g.gelu = gelu;
  g.out_mode = out_mode & 0xff;
  if (g.out_mode == 4) {  // f16 pair output: c [M][2N], hi at column n, lo at column N + n
    g.ldc = 2 * N;
    g.c_lo = N;
  }
  g.force_tile = (out_mode >> 8) & 0xfff;  // 0 auto / 128 / 256 / 257 (persistent) / 258 (one tile per workgroup)
  g.supertile = out_mode >> 20;             // 0 = launch_gemm's choice (tools: tile-order experiments)
  g.sk_part = e->sk_big[0];                  // few tiles, K >= 2048, out_mode 2: split-K with the engine's workspace, as the encoder does
  g.sk_bytes = e->sk_big_bytes;
  HIPCHK(launch_gemm(g, e->stream));
  return WCA_OK;
}

int wca_test_gemm_pairs(wca_engine* e, const void* a2, const void* w, const float* bias, void* c, int M, int N, int K, int gelu, int out_mode) {
  if (!e || !a2 || !w || !c) return fail(WCA_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(e->device));
  const int om = out_mode & 0xff;
  GemmArgs g = flat((const half_t*)a2, 2 * K, (const half_t*)w, K, c, N, M, N, K);
  g.a_lo = K;
  g.bias = bias;
  g.gelu = gelu;
  g.out_mode = om;
  if (om == 4) {
    g.ldc = 2 * N;
    g.c_lo = N;
  }
  g.force_tile = (out_mode >> 8) & 0xfff;
  g.site = 1;
  if (!plan_gemm(g, e->n_cu).pair()) return fail(WCA_ERR_INVALID, "the pair-operand kernel does not take M=%d N=%d K=%d out_mode %d", M, N, K, om);
  HIPCHK(launch_gemm(g, e->stream));
  return WCA_OK;
}

int wca_test_gemm_ln(wca_engine* e, const void* a, const void* w, const float* bias, float* x, const float* gamma, const float* beta,
                     void* xn, int M, int N, int K, int site) {
  if (!e || !a || !w || !x || !gamma || !beta || !xn) return fail(WCA_ERR_INVALID, "null argument");
  wca_test_gemm_desc d{};
  d.a = a;
  d.w = w;
  d.bias = bias;
  d.c = x;
  d.M = M;
  d.N = N;
  d.K = K;
  d.lda = d.ldw = K;
  d.ldc = d.ln_ld = N;
  d.out_mode = 3;
  d.site = site;
  d.ln_gamma = gamma;
  d.ln_beta = beta;
  d.ln_out = xn;
  int32_t plan[2];
  return wca_test_gemm_ex(e, &d, plan);
}

int wca_test_gemm_plan(int M, int N, int K, int lda, int out_mode, int gelu, int a_lo, int force_tile, int site, int n_cu, int cu_limit, int flags,
                       int64_t sk_bytes, int32_t* out) {
  if (!out) return fail(WCA_ERR_INVALID, "null argument");
  static float buf;   // what the pointers of the description point to: the plan looks at null or not
  GemmArgs g = flat(nullptr, lda, nullptr, K, nullptr, N, M, N, K);
  g.out_mode = out_mode;
  g.gelu = gelu;
  g.a_lo = a_lo;
  g.force_tile = force_tile;
  g.site = site;
  g.cu_limit = cu_limit;
  if (flags & 1) g.addend = &buf;
  if (flags & 2) g.a_rows_per_batch = 1;
  if (flags & 4) g.pos = &buf;
  if (flags & 8) g.c_rows_per_batch = 1;
  if (out_mode == 3 && !(flags & 16)) {
    g.ln_gamma = g.ln_beta = &buf;
    g.ln_out = (half_t*)&buf;
    g.ln_stats = (unsigned long long*)&buf;
    g.ln_cnt = (unsigned*)&buf;
    g.ln_ld = N;
  }
  if (out_mode == 4 && !(flags & 32)) g.c_lo = N;
  if (sk_bytes > 0) {
    g.sk_part = &buf;
    g.sk_bytes = (size_t)sk_bytes;
  }
  const GemmPlan p = plan_gemm(g, n_cu);
  if (p.refused) return fail(WCA_ERR_INVALID, "GEMM refused: %s", p.refused);
  const int32_t v[10] = {(int32_t)p.kernel, (int32_t)p.grid_x, (int32_t)p.grid_y, (int32_t)p.block, (int32_t)p.lds,
                         p.splitk,          p.supertile,       p.site_used,       (int32_t)p.a_bytes, (int32_t)p.w_bytes};
  memcpy(out, v, sizeof(v));
  return WCA_OK;
}

int wca_test_dec_gemm_plan(int n_text_state, int M, int N, int K, int layernorm, int kv_append, int64_t* out) {
  if (!out) return fail(WCA_ERR_INVALID, "null argument");
  if (n_text_state < 1 || M < 1 || N < 1 || K < 1) return fail(WCA_ERR_INVALID, "bad shape n_text_state=%d M=%d N=%d K=%d", n_text_state, M, N, K);
  const DecSkCapacity cap = dec_sk_capacity(n_text_state);
  const DecGemmPlan p = plan_dec_gemm(M, N, K, layernorm != 0, kv_append != 0, cap);
  const int64_t v[8] = {p.few_row ? 1 : 0,    p.splitk,          p.groups, (int64_t)p.grid_x, (int64_t)p.grid_y, (int64_t)p.lds,
                        (int64_t)p.ws_bytes, (int64_t)(cap.floats * sizeof(float))};
  memcpy(out, v, sizeof(v));
  return WCA_OK;
}

int wca_test_gemm_ex(wca_engine* e, const wca_test_gemm_desc* d, int32_t* plan_out) {
  if (!e || !d || !plan_out || !d->a || !d->w || !d->c) return fail(WCA_ERR_INVALID, "null argument");
  GemmArgs g = flat((const half_t*)d->a, d->lda, (const half_t*)d->w, d->ldw, d->c, d->ldc, d->M, d->N, d->K);
  g.bias = d->bias;
  g.addend = d->addend;
  g.ld_addend = d->ld_addend;
  g.pos = d->pos;
  g.pos_period = d->pos_period;
  g.a_rows_per_batch = d->a_rows_per_batch;
  g.a_batch_stride = (long)d->a_batch_stride;
  g.c_rows_per_batch = d->c_rows_per_batch;
  g.c_batch_stride = (long)d->c_batch_stride;
  g.a_lo = (long)d->a_lo;
  g.c_lo = (long)d->c_lo;
  g.gelu = d->gelu;
  g.out_mode = d->out_mode;
  g.force_tile = d->force_tile;
  g.site = d->site;
  g.cu_limit = d->cu_limit;
  g.supertile = d->supertile;
  g.sk_part = e->sk_big[0];
  g.sk_bytes = e->sk_big_bytes;
  if (g.pos != nullptr && g.pos_period <= 0) return fail(WCA_ERR_INVALID, "a positional table needs pos_period > 0");
  if (g.addend != nullptr && g.ld_addend < g.N) return fail(WCA_ERR_INVALID, "ld_addend < N");
  const bool ln = g.out_mode == 3;
  if (ln) {
    // residual + LayerNorm epilogue: the statistics workspace of the engine's scratch buffers and its error word
    if (!d->ln_gamma || !d->ln_beta || !d->ln_out) return fail(WCA_ERR_INVALID, "null argument");
    if (g.M <= 0 || g.N <= 0) return fail(WCA_ERR_INVALID, "residual + LayerNorm epilogue not available for M=%d N=%d K=%d", g.M, g.N, g.K);
    HIPCHK(hipSetDevice(e->device));
    const size_t mpad = align_up((size_t)g.M, 256);
    HIPCHK(e->tmp0.ensure(sizeof(unsigned long long) * (size_t)((g.N + 255) / 256) * mpad));
    HIPCHK(e->tmp1.ensure(sizeof(unsigned) * (mpad / 256 + 16)));
    g.ln_gamma = d->ln_gamma;
    g.ln_beta = d->ln_beta;
    g.ln_out = (half_t*)d->ln_out;
    g.ln_ld = d->ln_ld;
    g.ln_eps = 1e-5f;
    g.ln_stats = (unsigned long long*)e->tmp0.p;
    g.ln_cnt = (unsigned*)e->tmp1.p;
    g.ln_err = e->err_dev;
  }
  const GemmPlan p = plan_gemm(g, e->n_cu);
  if (p.refused) return fail(WCA_ERR_INVALID, "GEMM refused: %s", p.refused);
  if (ln && p.kernel != GemmKernel::Persist256LN) return fail(WCA_ERR_INVALID, "residual + LayerNorm epilogue not available for M=%d N=%d K=%d", g.M, g.N, g.K);
  plan_out[0] = (int32_t)p.kernel;
  plan_out[1] = (int32_t)p.grid_x;
  HIPCHK(hipSetDevice(e->device));
  if (ln) HIPCHK(hipMemsetAsync(e->err_dev, 0, sizeof(int), e->stream));
  HIPCHK(launch_gemm(g, e->stream));
  if (ln) {
    HIPCHK(hipMemcpyAsync(e->err_host, e->err_dev, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (e->err_host[0] & 2) return fail(WCA_ERR_HIP, "LayerNorm statistics hand-off timed out");
  }
  return WCA_OK;
}

int wca_test_attention_ex(wca_engine* e, const wca_test_attn_desc* d) {
  if (!e || !d || !d->q || !d->k || !d->v || !d->o) return fail(WCA_ERR_INVALID, "null argument");
  if (d->B < 1 || d->H < 1 || d->nq < 1 || d->nk < 1) return fail(WCA_ERR_INVALID, "bad shape");
  if (d->variant < 0 || d->variant > 2) return fail(WCA_ERR_INVALID, "attention variant %d does not exist", d->variant);
  AttnArgs a{};
  a.Q = (const half_t*)d->q;
  a.K = (const half_t*)d->k;
  a.V = (const half_t*)d->v;
  a.O = (half_t*)d->o;
  a.q_bs = (long)d->q_bs;
  a.k_bs = (long)d->k_bs;
  a.v_bs = (long)d->v_bs;
  a.o_bs = (long)d->o_bs;
  a.q_rs = d->q_rs;
  a.k_rs = d->k_rs;
  a.v_rs = d->v_rs;
  a.o_rs = d->o_rs;
  a.split = d->split;
  a.q_lo = (long)d->q_lo;
  a.k_lo = (long)d->k_lo;
  a.v_lo = (long)d->v_lo;
  a.o_lo = (long)d->o_lo;
  a.cap = d->cap;
  a.cap_bs = (long)d->cap_bs;
  a.cap_hs = (long)d->cap_hs;
  a.cap_ld = d->cap_ld;
  a.cap_cols = d->cap_cols;
  a.nk_rows = d->nk_rows;
  a.B = d->B;
  a.H = d->H;
  a.nq = d->nq;
  a.nk = d->nk;
  a.scale = 0.125f;
  a.causal = d->causal & 1;
  a.variant = d->variant;
  HIPCHK(hipSetDevice(e->device));
  if (launch_attention(a, e->stream) != hipSuccess) return fail(WCA_ERR_INVALID, "the attention launcher refused these arguments");
  return WCA_OK;
}

int wca_test_gemm_rows(wca_engine* e, const void* a_f16, const float* x_f32, const float* gamma, const float* beta, const void* w,
                       const float* bias, void* c, int M, int N, int K, int gelu, int out_mode, int splitk, int groups, void* kv_k, void* kv_v,
                       int T_max, int kv_t) {
  wca_test_gemm_rows_desc d{};
  d.a = a_f16;
  d.x = x_f32;
  d.gamma = gamma;
  d.beta = beta;
  d.w = w;
  d.bias = bias;
  d.c = c;
  d.kv_k = kv_k;
  d.kv_v = kv_v;
  d.M = M;
  d.N = N;
  d.K = K;
  d.lda = d.lda32 = d.ldw = K;
  d.ldc = N;
  d.gelu = gelu;
  d.out_mode = out_mode;
  d.splitk = splitk;
  d.groups = groups;
  d.kv_tmax = T_max;
  d.kv_t = kv_t;
  return wca_test_gemm_rows_ex(e, &d);
}

int wca_test_gemm_rows_ex(wca_engine* e, const wca_test_gemm_rows_desc* d) {
  if (!e || !d || !d->w || !d->c || (!d->a && !d->x) || (d->x && (!d->gamma || !d->beta))) return fail(WCA_ERR_INVALID, "null argument");
  const int M = d->M, N = d->N, K = d->K;
  if (M < 1 || N < 1 || K < 1) return fail(WCA_ERR_INVALID, "bad shape M=%d N=%d K=%d", M, N, K);
  HIPCHK(hipSetDevice(e->device));
  int splitk = d->splitk;
  if (splitk <= 0) splitk = gemm_rows_pick_splitk(K);
  if (splitk <= 0) return fail(WCA_ERR_INVALID, "no split of K=%d fits the few-row kernel", K);
  const size_t tiles = (size_t)((M + 63) / 64) * ((N + 15) / 16);
  if (splitk > 1) {
    HIPCHK(e->tmp0.ensure(gemm_rows_workspace_bytes(M, N, splitk)));
    HIPCHK(e->tmp1.ensure(sizeof(unsigned) * tiles));
    HIPCHK(hipMemsetAsync(e->tmp1.p, 0, sizeof(unsigned) * tiles, e->stream));
  }
  GemmArgs g = flat((const half_t*)d->a, d->lda, (const half_t*)d->w, d->ldw, d->c, d->ldc, M, N, K);
  g.c_rows_per_batch = d->c_rows_per_batch;
  g.c_batch_stride = (long)d->c_batch_stride;
  g.A32 = d->x;
  g.lda32 = d->lda32;
  g.ln_gamma = d->gamma;
  g.ln_beta = d->beta;
  g.ln_eps = 1e-5f;
  g.bias = d->bias;
  g.gelu = d->gelu;
  g.out_mode = d->out_mode;
  g.splitk = splitk;
  g.groups = d->groups;
  g.sk_part = (float*)e->tmp0.p;
  g.sk_cnt = (unsigned*)e->tmp1.p;
  g.kv_k = (half_t*)d->kv_k;
  g.kv_v = (half_t*)d->kv_v;
  g.kv_bs = (long)d->kv_tmax * (N / 3);
  g.kv_t = d->kv_t;
  g.kv_d = d->kv_k ? N / 3 : 0;
  g.kv_t_rows = d->kv_t_rows;
  g.kv_tmax = d->kv_tmax;
  // the launcher trusts kv_t and the strides of C (the engine derives them): an entry point for tests checks what would leave the buffers
  if (d->kv_k && !d->kv_t_rows && (d->kv_t < 0 || d->kv_t >= d->kv_tmax)) return fail(WCA_ERR_INVALID, "kv_t %d outside [0,%d)", d->kv_t, d->kv_tmax);
  if (d->ldc < (d->kv_k ? N / 3 : N) || (d->c_rows_per_batch > 0 && d->c_batch_stride < (int64_t)d->c_rows_per_batch * d->ldc))
    return fail(WCA_ERR_INVALID, "rows of C overlap (ldc %d, c_batch_stride %lld)", d->ldc, (long long)d->c_batch_stride);
  const hipError_t he = launch_gemm_rows(g, e->stream);
  if (he == hipErrorInvalidValue) {
    (void)hipGetLastError();
    return fail(WCA_ERR_INVALID, "the few-row GEMM's launcher refused M=%d N=%d K=%d splitk %d out_mode %d", M, N, K, splitk, d->out_mode);
  }
  HIPCHK(he);
  if (splitk > 1) {
    // the counters must be back at zero (self-cleaning): a second launch on the same workspace has to give the same result
    std::vector<unsigned> cnt(tiles);
    HIPCHK(hipMemcpyAsync(cnt.data(), e->tmp1.p, sizeof(unsigned) * tiles, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (unsigned v : cnt)
      if (v != 0) return fail(WCA_ERR_HIP, "split-K arrival counter left at %u", v);
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  return WCA_OK;
}

int wca_test_set_attn_split_drop(int mask) {
  if (mask != 0 && mask != 1 && mask != 2 && mask != 3 && mask != 4 && mask != 8 && mask != 9 && mask != 12 && mask != 15)
    return fail(WCA_ERR_INVALID, "attention pass mask %d is not instantiated", mask);
  set_debug_switch("attn_split_drop", mask);
  return WCA_OK;
}

int wca_test_set_switch(const char* name, int value) {
  if (!name) return fail(WCA_ERR_INVALID, "null argument");
  if (set_debug_switch(name, value) != 0) return fail(WCA_ERR_INVALID, "unknown switch %s", name);
  return WCA_OK;
}

int wca_test_last_scores(wca_engine* e, int batch, float* scores_host) {
  if (!e || !scores_host) return fail(WCA_ERR_INVALID, "null argument");
  if (e->enq_count != e->fetch_count) return fail(WCA_ERR_STATE, "fetch the batches in flight first");
  HIPCHK(hipSetDevice(e->device));
  const size_t n = (size_t)batch * e->dims.n_text_layer * e->dims.n_text_head;
  if (batch < 1 || e->scores.bytes < n * sizeof(float)) return fail(WCA_ERR_INVALID, "no head scores of a batch of %d are held", batch);
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipStreamSynchronize(e->stream2));
  HIPCHK(hipMemcpy(scores_host, e->scores.p, n * sizeof(float), hipMemcpyDeviceToHost));
  return WCA_OK;
}

static int align_postproc(wca_engine* e, const wca_test_postproc_desc* d, float* path_mean_host, int32_t* path_cells_host);

int wca_test_align_postproc(wca_engine* e, const wca_test_postproc_desc* d) { return align_postproc(e, d, nullptr, nullptr); }

int wca_test_align_postproc_scores(wca_engine* e, const wca_test_postproc_desc* d, float* path_mean_host, int32_t* path_cells_host) {
  if (!path_mean_host || !path_cells_host) return fail(WCA_ERR_INVALID, "null argument");
  return align_postproc(e, d, path_mean_host, path_cells_host);
}

static int align_postproc(wca_engine* e, const wca_test_postproc_desc* d, float* path_mean_host, int32_t* path_cells_host) {
  if (!e || !d || !d->qk_dev || !d->n_tok_host || !d->n_frames_host || !d->opts) return fail(WCA_ERR_INVALID, "null argument");
  const wca_align_opts* o = d->opts;
  const int B = d->B, LH = d->L * d->H, n_max = d->n_tok_max, F = d->n_frames_max;
  if (B < 1 || B > e->max_batch) return fail(WCA_ERR_INVALID, "batch %d outside [1,%d]", B, e->max_batch);
  if (d->L < 1 || d->H < 1 || LH > 8192) return fail(WCA_ERR_INVALID, "bad shape L=%d H=%d", d->L, d->H);
  if (o->sot_len < 0) return fail(WCA_ERR_INVALID, "sot_len %d < 0", o->sot_len);
  WCA_TRY(check_aggregation(o));
  WCA_TRY(check_medfilt(o->medfilt_width));
  int Fmax = 0;
  WCA_TRY(validate_lengths(B, n_max, d->n_tok_host, d->n_frames_host, &Fmax));
  if (F > N_CTX) return fail(WCA_ERR_TOO_LONG, "n_frames_max=%d > %d", F, N_CTX);
  if (F < Fmax || d->ld < F) return fail(WCA_ERR_INVALID, "need the largest n_frames %d <= n_frames_max %d <= ld %d", Fmax, F, d->ld);
  WCA_TRY(enter(e));
  std::vector<int32_t> dn(B), flags(B);
  for (int b = 0; b < B; ++b) {
    dn[b] = std::max(0, d->n_tok_host[b] - o->sot_len - 1);
    flags[b] = d->open_end_host && d->open_end_host[b] ? 1 : 0;
  }
  int* rows[4];
  int* open_rows[4] = {nullptr, nullptr, nullptr, nullptr};
  WCA_TRY(stage_meta(e, B, nullptr, d->n_tok_host, d->n_frames_host, dn.data(), rows));
  if (d->open_end_host) WCA_TRY(stage_meta(e, B, flags.data(), nullptr, nullptr, nullptr, open_rows));
  hipStream_t s = e->stream;
  HeadStatsArgs h;
  WCA_TRY(run_head_stats(e, s, &h, d->qk_dev, d->ld, false, nullptr, true, rows[1], rows[2], n_max, F, LH, B, o->medfilt_width, o->qk_scale,
                         o->w_colnorm, o->w_rownorm, o->w_coverage));
  WCA_TRY(run_select_aggregate_dtw(e, s, h, rows[3], o, d->L, open_rows[0], path_mean_host != nullptr));
  const bool topk = o->aggregation == WCA_AGGR_TOPK;
  const size_t BLH = (size_t)B * LH;
  if (d->scores_host) HIPCHK(hipMemcpyAsync(d->scores_host, e->scores.p, sizeof(float) * BLH, hipMemcpyDeviceToHost, s));
  if (d->colnorm_host) HIPCHK(hipMemcpyAsync(d->colnorm_host, e->colnorm.p, sizeof(float) * BLH * F, hipMemcpyDeviceToHost, s));
  if (d->rowstats_host) HIPCHK(hipMemcpyAsync(d->rowstats_host, e->wws.p, sizeof(float) * BLH * n_max * 2, hipMemcpyDeviceToHost, s));
  if (d->sel_idx_host && topk) HIPCHK(hipMemcpyAsync(d->sel_idx_host, e->sel.p, sizeof(int) * (size_t)B * o->topk, hipMemcpyDeviceToHost, s));
  if (d->matrix_host) HIPCHK(hipMemcpyAsync(d->matrix_host, e->matrix.p, sizeof(float) * (size_t)B * n_max * F, hipMemcpyDeviceToHost, s));
  if (d->jump_host) {
    if (n_max - o->sot_len - 1 >= 1)   // (otherwise no DTW ran and nothing wrote e->jump: the rows are 0 by definition)
      HIPCHK(hipMemcpyAsync(d->jump_host, e->jump.p, sizeof(int) * (size_t)B * n_max, hipMemcpyDeviceToHost, s));
    else
      memset(d->jump_host, 0, sizeof(int) * (size_t)B * n_max);
  }
  if (path_mean_host) {
    const size_t n = (size_t)B * n_max;
    HIPCHK(hipMemcpyAsync(path_mean_host, e->pscore.p, sizeof(float) * n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(path_cells_host, (const int*)e->pscore.p + n, sizeof(int) * n, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  return WCA_OK;
}

int wca_test_align_heads_postproc(wca_engine* e, const wca_test_heads_postproc_desc* d) {
  if (!e || !d || !d->qk_dev || !d->n_tok_host || !d->n_frames_host || !d->heads_host || !d->opts) return fail(WCA_ERR_INVALID, "null argument");
  const wca_align_opts* o = d->opts;
  const int B = d->B, LH = d->L * d->H, n_max = d->n_tok_max, F = d->n_frames_max, S = d->n_heads;
  if (B < 1 || B > e->max_batch) return fail(WCA_ERR_INVALID, "batch %d outside [1,%d]", B, e->max_batch);
  if (d->L < 1 || d->H < 1 || LH > 8192) return fail(WCA_ERR_INVALID, "bad shape L=%d H=%d", d->L, d->H);
  if (o->sot_len < 0) return fail(WCA_ERR_INVALID, "sot_len %d < 0", o->sot_len);
  WCA_TRY(check_heads(d->heads_host, S, LH));
  WCA_TRY(check_medfilt(o->medfilt_width));
  int Fmax = 0;
  WCA_TRY(validate_lengths(B, n_max, d->n_tok_host, d->n_frames_host, &Fmax));
  if (F > N_CTX) return fail(WCA_ERR_TOO_LONG, "n_frames_max=%d > %d", F, N_CTX);
  if (F < Fmax || d->ld < F) return fail(WCA_ERR_INVALID, "need the largest n_frames %d <= n_frames_max %d <= ld %d", Fmax, F, d->ld);
  WCA_TRY(enter(e));
  std::vector<int32_t> dn(B);
  for (int b = 0; b < B; ++b) dn[b] = std::max(0, d->n_tok_host[b] - o->sot_len - 1);
  int* rows[4];
  WCA_TRY(stage_meta(e, B, nullptr, d->n_tok_host, d->n_frames_host, dn.data(), rows));
  hipStream_t s = e->stream;
  HIPCHK(e->tmp1.ensure(sizeof(int) * (size_t)S));
  HIPCHK(hipMemcpyAsync(e->tmp1.p, d->heads_host, sizeof(int) * (size_t)S, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));   // heads_host is caller-owned pageable memory
  WCA_TRY(run_align_heads(e, s, d->qk_dev, d->ld, (const int*)e->tmp1.p, S, rows[1], rows[2], rows[3], n_max, F, LH, B, o));
  const size_t BS = (size_t)B * S;
  if (d->rowstats_host) HIPCHK(hipMemcpyAsync(d->rowstats_host, e->wws.p, sizeof(float) * BS * n_max * 2, hipMemcpyDeviceToHost, s));
  if (d->colstats_host) HIPCHK(hipMemcpyAsync(d->colstats_host, e->colnorm.p, sizeof(float) * BS * F * 2, hipMemcpyDeviceToHost, s));
  if (d->matrix_host) HIPCHK(hipMemcpyAsync(d->matrix_host, e->matrix.p, sizeof(float) * (size_t)B * n_max * F, hipMemcpyDeviceToHost, s));
  if (d->jump_host) {
    if (n_max - o->sot_len - 1 >= 1)   // (otherwise no DTW ran and nothing wrote e->jump: the rows are 0 by definition)
      HIPCHK(hipMemcpyAsync(d->jump_host, e->jump.p, sizeof(int) * (size_t)B * n_max, hipMemcpyDeviceToHost, s));
    else
      memset(d->jump_host, 0, sizeof(int) * (size_t)B * n_max);
  }
  HIPCHK(hipStreamSynchronize(s));
  return WCA_OK;
}

int wca_test_last_colnorm(wca_engine* e, int64_t count, float* colnorm_host) {
  if (!e || !colnorm_host) return fail(WCA_ERR_INVALID, "null argument");
  if (count < 1 || (size_t)count * sizeof(float) > e->colnorm.bytes) return fail(WCA_ERR_INVALID, "%lld column norms are not held", (long long)count);
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(colnorm_host, e->colnorm.p, sizeof(float) * (size_t)count, hipMemcpyDeviceToHost));
  return WCA_OK;
}

int wca_test_decode_state(wca_engine* e, int batch, int T_max, int logits_rows, float* logits_host, void* cache_f16_host) {
  if (!e || !logits_host || !cache_f16_host) return fail(WCA_ERR_INVALID, "null argument");
  const wca_model_dims& D = e->dims;
  if (batch < 1 || batch != e->dec_batch || T_max != e->dec_T_max)
    return fail(WCA_ERR_STATE, "the last decode ran batch %d with T_max %d, not batch %d with T_max %d", e->dec_batch, e->dec_T_max, batch, T_max);
  if (logits_rows < 1 || logits_rows > e->dec_logits_rows)
    return fail(WCA_ERR_INVALID, "the last decode left %d logits rows, not %d", e->dec_logits_rows, logits_rows);
  const size_t logits_bytes = sizeof(float) * (size_t)logits_rows * D.n_vocab;
  const size_t cache_bytes = sizeof(half_t) * (size_t)D.n_text_layer * 2 * batch * T_max * D.n_text_state;
  const size_t cache_off = sizeof(half_t) * e->dec_cache_off;   // a group decode: the half its last step wrote
  if (logits_bytes > e->dec_logits.bytes || cache_off + cache_bytes > e->dec_cache.bytes) return fail(WCA_ERR_INVALID, "the decode buffers hold less than was asked for");
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipStreamSynchronize(e->stream2));
  HIPCHK(hipMemcpy(logits_host, e->dec_logits.p, logits_bytes, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(cache_f16_host, (const char*)e->dec_cache.p + cache_off, cache_bytes, hipMemcpyDeviceToHost));
  return WCA_OK;
}

int wca_test_beam_step(wca_engine* e, const wca_test_beam_desc* d) {
  if (!e || !d) return fail(WCA_ERR_INVALID, "null argument");
  if (!d->logits_dev || !d->tokens_in_dev || !d->tokens_out_dev || !d->cur_len_dev || !d->n_initial_dev || !d->cap_dev || !d->suppress_mask_dev ||
      !d->opts || !d->sum_logprob_dev || !d->src_dev || !d->cand_tok_dev || !d->cand_lp_dev || !d->fin_n_dev || !d->fin_len_dev || !d->fin_sum_dev ||
      !d->fin_tok_dev || !d->trace_dev || !d->n_done_dev)
    return fail(WCA_ERR_INVALID, "null argument");
  const wca_decode_opts* o = d->opts;
  if (d->batch < 1 || d->n_group < 1 || d->n_group > BEAM_GROUP_MAX || d->n_vocab < 1 || d->T_max < 2 || d->max_candidates < 1)
    return fail(WCA_ERR_INVALID, "bad shape");
  if (d->tokens_in_dev == d->tokens_out_dev) return fail(WCA_ERR_INVALID, "tokens_in_dev and tokens_out_dev are two buffers");
  if (o->eot < 0 || o->eot >= d->n_vocab || o->timestamp_begin < 0 || o->timestamp_begin > d->n_vocab)
    return fail(WCA_ERR_INVALID, "eot / timestamp_begin outside the vocabulary");
  HIPCHK(hipSetDevice(e->device));
  const int R = d->batch * d->n_group;
  BeamTopkArgs tk{};
  tk.sel = select_args(d->logits_dev, d->n_vocab, const_cast<int32_t*>(d->tokens_in_dev), d->T_max, d->suppress_mask_dev, d->blank_mask_dev, o,
                       d->sum_logprob_dev, d->n_done_dev);
  tk.sel.cur_len_rows = d->cur_len_dev;
  tk.sel.n_initial_rows = d->n_initial_dev;
  tk.sel.cap_rows = d->cap_dev;
  tk.K = d->n_group + 1;
  tk.cand_tok = d->cand_tok_dev;
  tk.cand_lp = d->cand_lp_dev;
  HIPCHK(launch_beam_topk(tk, R, e->stream));
  BeamMergeArgs m{};
  m.cand_tok = d->cand_tok_dev;
  m.cand_lp = d->cand_lp_dev;
  m.K = tk.K;
  m.G = d->n_group;
  m.tok_in = d->tokens_in_dev;
  m.tok_out = d->tokens_out_dev;
  m.T_max = d->T_max;
  m.sum_logprob = d->sum_logprob_dev;
  m.src = d->src_dev;
  m.cur_len_rows = d->cur_len_dev;
  m.n_initial_rows = d->n_initial_dev;
  m.cap_rows = d->cap_dev;
  m.first = d->first != 0;
  m.eot = o->eot;
  m.max_candidates = d->max_candidates;
  m.fin_n = d->fin_n_dev;
  m.fin_len = d->fin_len_dev;
  m.fin_sum = d->fin_sum_dev;
  m.fin_tok = d->fin_tok_dev;
  m.trace = d->trace_dev;
  m.n_done = d->n_done_dev;
  HIPCHK(launch_beam_merge(m, d->batch, e->stream));
  return WCA_OK;
}

int wca_test_kv_reorder(wca_engine* e, const void* src_dev, void* dst_dev, int n_planes, int rows_src, int rows_dst, int T_max, int d,
                        const int32_t* src_idx_dev, int div, const int32_t* n_keep_dev) {
  if (!e || !src_dev || !dst_dev || !n_keep_dev) return fail(WCA_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(e->device));
  if (launch_kv_reorder((const half_t*)src_dev, (half_t*)dst_dev, n_planes, rows_src, rows_dst, T_max, d, src_idx_dev, div, n_keep_dev, e->stream) !=
      hipSuccess)
    return fail(WCA_ERR_INVALID, "the cache reorder refused these arguments");
  return WCA_OK;
}

int wca_test_beam_trace(wca_engine* e, int32_t* steps_out, int32_t* rows_out, int32_t* trace_host, int64_t cap_entries) {
  if (!e || !steps_out || !rows_out) return fail(WCA_ERR_INVALID, "null argument");
  if (e->grp_rows < 1) return fail(WCA_ERR_STATE, "the last decode was no beam search");
  *steps_out = e->grp_steps;
  *rows_out = e->grp_rows;
  if (!trace_host) return WCA_OK;
  const size_t n = (size_t)e->grp_steps * e->grp_rows * 2;
  if (cap_entries < 0 || (size_t)cap_entries < n) return fail(WCA_ERR_INVALID, "the trace holds %zu entries, more than the %lld offered", n, (long long)cap_entries);
  if (e->grp_trace_off + sizeof(int) * n > e->dec_beam.bytes) return fail(WCA_ERR_STATE, "the beam buffers hold less than the trace");
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipStreamSynchronize(e->stream2));
  HIPCHK(hipMemcpy(trace_host, (const char*)e->dec_beam.p + e->grp_trace_off, sizeof(int) * n, hipMemcpyDeviceToHost));
  return WCA_OK;
}

int wca_test_attention(wca_engine* e, const void* q, const void* k, const void* v, void* o, float* cap_dev, int cap_ld, int cap_cols,
                       int B, int H, int nq, int nk, int causal) {
  if (!e) return fail(WCA_ERR_INVALID, "null engine");
  const int variant = (causal >> 8) & 3;  // 0 auto, 1 the 16x16x32 kernel, 2 the 32x32x16 kernel (attention.hip)
  if (variant == 3) return fail(WCA_ERR_INVALID, "attention variant 3 does not exist");
  HIPCHK(hipSetDevice(e->device));
  AttnArgs a = dense_attn(q, k, v, o, H * 64, B, H, nq, nk, causal);
  a.cap = cap_dev;
  a.cap_bs = (long)H * nq * cap_ld;
  a.cap_hs = (long)nq * cap_ld;
  a.cap_ld = cap_ld;
  a.cap_cols = cap_cols;
  a.variant = variant;
  HIPCHK(launch_attention(a, e->stream));
  return WCA_OK;
}

int wca_test_attention_split(wca_engine* e, const void* q2, const void* k2, const void* v2, void* o2, float* cap_dev, int cap_ld, int cap_cols,
                             int B, int H, int nq, int nk, int causal) {
  if (!e || !q2 || !k2 || !v2 || !o2) return fail(WCA_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(e->device));
  AttnArgs a = dense_attn(q2, k2, v2, o2, 2 * H * 64, B, H, nq, nk, causal);
  a.split = 1;
  a.q_lo = a.k_lo = a.v_lo = a.o_lo = H * 64;
  a.cap = cap_dev;
  a.cap_bs = (long)H * nq * cap_ld;
  a.cap_hs = (long)nq * cap_ld;
  a.cap_ld = cap_ld;
  a.cap_cols = cap_cols;
  HIPCHK(launch_attention(a, e->stream));
  return WCA_OK;
}

int wca_test_decode_select(wca_engine* e, const float* logits_dev, int batch, int n_vocab, int32_t* tokens_dev, int T_max, int cur_len,
                           int n_initial, const uint8_t* suppress_mask_dev, const uint8_t* blank_mask_dev, const wca_decode_opts* o,
                           float* sum_logprob_dev, int32_t* n_done_dev) {
  if (!e || !logits_dev || !tokens_dev || !suppress_mask_dev || !o || !sum_logprob_dev || !n_done_dev) return fail(WCA_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(e->device));
  DecodeSelectArgs a = select_args(logits_dev, n_vocab, tokens_dev, T_max, suppress_mask_dev, blank_mask_dev, o, sum_logprob_dev, n_done_dev);
  a.cur_len = cur_len;
  a.n_initial = n_initial;
  HIPCHK(launch_decode_select(a, batch, e->stream));
  return WCA_OK;
}

int wca_test_decode_select_rows(wca_engine* e, const float* logits_dev, int batch, int n_vocab, int32_t* tokens_dev, int T_max,
                                const int32_t* cur_len_dev, const int32_t* n_initial_dev, const int32_t* cap_dev, int n_done_idx, int n_done_len,
                                const uint8_t* suppress_mask_dev, const uint8_t* blank_mask_dev, const wca_decode_opts* o, float* sum_logprob_dev,
                                int32_t* n_done_dev) {
  if (!e || !logits_dev || !tokens_dev || !cur_len_dev || !n_initial_dev || !cap_dev || !suppress_mask_dev || !o || !sum_logprob_dev || !n_done_dev)
    return fail(WCA_ERR_INVALID, "null argument");
  if (batch < 1 || n_vocab < 1 || T_max < 2 || n_done_idx < 0 || n_done_idx >= n_done_len) return fail(WCA_ERR_INVALID, "bad shape");
  if (o->eot < 0 || o->eot >= n_vocab || o->timestamp_begin < 0 || o->timestamp_begin > n_vocab)
    return fail(WCA_ERR_INVALID, "eot / timestamp_begin outside the vocabulary");
  HIPCHK(hipSetDevice(e->device));
  DecodeSelectArgs a = select_args(logits_dev, n_vocab, tokens_dev, T_max, suppress_mask_dev, blank_mask_dev, o, sum_logprob_dev, n_done_dev);
  a.cur_len_rows = cur_len_dev;
  a.n_initial_rows = n_initial_dev;
  a.cap_rows = cap_dev;
  a.n_done_idx = n_done_idx;
  HIPCHK(launch_decode_select(a, batch, e->stream));
  return WCA_OK;
}

int wca_test_decode_sample_rows(wca_engine* e, const float* logits_dev, int batch, int n_vocab, int32_t* tokens_dev, int T_max,
                                const int32_t* cur_len_dev, const int32_t* n_initial_dev, const int32_t* cap_dev, int n_done_idx, int n_done_len,
                                const uint8_t* suppress_mask_dev, const uint8_t* blank_mask_dev, const wca_decode_opts* o, float* sum_logprob_dev,
                                int32_t* n_done_dev, const float* temperature_dev, const uint64_t* seed_dev) {
  if (!e || !logits_dev || !tokens_dev || !cur_len_dev || !n_initial_dev || !cap_dev || !suppress_mask_dev || !o || !sum_logprob_dev ||
      !n_done_dev || !temperature_dev || !seed_dev)
    return fail(WCA_ERR_INVALID, "null argument");
  if (batch < 1 || n_vocab < 1 || T_max < 2 || n_done_idx < 0 || n_done_idx >= n_done_len) return fail(WCA_ERR_INVALID, "bad shape");
  if (o->eot < 0 || o->eot >= n_vocab || o->timestamp_begin < 0 || o->timestamp_begin > n_vocab)
    return fail(WCA_ERR_INVALID, "eot / timestamp_begin outside the vocabulary");
  HIPCHK(hipSetDevice(e->device));
  DecodeSelectArgs a = select_args(logits_dev, n_vocab, tokens_dev, T_max, suppress_mask_dev, blank_mask_dev, o, sum_logprob_dev, n_done_dev);
  a.cur_len_rows = cur_len_dev;
  a.n_initial_rows = n_initial_dev;
  a.cap_rows = cap_dev;
  a.n_done_idx = n_done_idx;
  a.temperature_rows = temperature_dev;
  a.seed_rows = (const unsigned long long*)seed_dev;
  HIPCHK(launch_decode_select(a, batch, e->stream));
  return WCA_OK;
}

int wca_test_language_head(wca_engine* e, const float* x_dev, int B, int lang_begin, int n_lang, float* probs_dev, int32_t* lang_token_dev) {
  if (!e || !x_dev || !probs_dev || !lang_token_dev) return fail(WCA_ERR_INVALID, "null argument");
  if (!e->finalized) return fail(WCA_ERR_STATE, "weights not finalized (call wca_finalize_weights)");
  HIPCHK(hipSetDevice(e->device));
  if (launch_language_head(x_dev, e->lnf_g, e->lnf_b, e->tok_emb, B, e->dims.n_text_state, e->dims.n_vocab, lang_begin, n_lang, probs_dev,
                           lang_token_dev, e->stream) != hipSuccess)
    return fail(WCA_ERR_INVALID, "the language head takes B >= 1, 1 <= n_lang <= 128 and language tokens [%d,%d) inside the vocabulary", lang_begin,
                lang_begin + n_lang);
  return WCA_OK;
}

int wca_test_attention_rows(wca_engine* e, const void* q, const void* k, const void* v, void* o, int B, int H, int nq, int nk,
                            const int32_t* nk_rows_dev, int causal) {
  if (!e || !q || !k || !v || !o || !nk_rows_dev) return fail(WCA_ERR_INVALID, "null argument");
  if (B < 1 || H < 1 || nq < 1 || nk < 1) return fail(WCA_ERR_INVALID, "bad shape");
  HIPCHK(hipSetDevice(e->device));
  AttnArgs a = dense_attn(q, k, v, o, H * 64, B, H, nq, nk, causal);
  a.nk_rows = nk_rows_dev;
  if (launch_attention(a, e->stream) != hipSuccess)
    return fail(WCA_ERR_INVALID, "per-row key counts are taken by the one-query f16 attention only (nq = 1, no mask)");
  return WCA_OK;
}

int wca_test_layernorm(wca_engine* e, const float* x, const float* g, const float* b, void* out, int rows, int d) {
  if (!e) return fail(WCA_ERR_INVALID, "null engine");
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(launch_layernorm_f16(x, g, b, (half_t*)out, rows, d, 1e-5f, e->stream));
  return WCA_OK;
}

int wca_test_layernorm_split(wca_engine* e, const float* x, const float* g, const float* b, void* out2, int rows, int d) {
  if (!e) return fail(WCA_ERR_INVALID, "null engine");
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(launch_layernorm_f16(x, g, b, (half_t*)out2, rows, d, 1e-5f, e->stream, 2 * d, d));
  return WCA_OK;
}

int wca_test_encoder(wca_engine* e, const float* mel_dev, int batch, float* xa_out_dev) {
  int rc = check_ready(e);
  if (rc) return rc;
  if ((rc = join_phase2(e))) return rc;
  if (batch < 1 || batch > e->max_batch) return fail(WCA_ERR_INVALID, "batch %d outside [1,%d]", batch, e->max_batch);
  const wca_model_dims& D = e->dims;
  if ((rc = ensure_split_weights(e))) return rc;
  if ((rc = mel_to_tm(e, mel_dev, batch))) return rc;
  rc = run_encoder(e, batch);
  if (rc) return rc;
  // xn holds ln_post(x) in f16 (split mode: hi + lo pairs); widen for the caller
  const size_t n = (size_t)batch * N_CTX * D.n_audio_state;
  if (e->split)
    hipLaunchKernelGGL(widen_split_kernel, dim3(2048), dim3(256), 0, e->stream, e->xn, xa_out_dev, (size_t)batch * N_CTX, D.n_audio_state);
  else
    hipLaunchKernelGGL(widen_kernel, dim3(2048), dim3(256), 0, e->stream, e->xn, xa_out_dev, n);
  HIPCHK(hipGetLastError());
  return WCA_OK;
}

}  // extern "C"
