// Host-side launch interface of the HIP kernels (internal to libwca.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wca {

typedef _Float16 half_t;

// ---------------------------------------------------------------- test switches (debug_switch.cpp; wca_test_set_switch)
enum { DBG_ATTN_SPLIT_VARIANT = 0, DBG_HEAD_STATS_GENERAL, DBG_FAIL_PRECISION_ALLOC, DBG_ATTN_SPLIT_DROP, DBG_GEMM_RING, DBG_SWITCH_COUNT };
int debug_switch(int id);                            // current value (0 until set)
int set_debug_switch(const char* name, int value);   // 0, or -1 for an unknown name

// ---------------------------------------------------------------- GEMM (gemm.hip)
// C[m][n] = epilogue( sum_k A[m][k] * W[n][k] ),  A/W f16, fp32 accumulate on MFMA.
// Rows of A and C may be "batch strided": logical row m = b * rows_per_batch + t lives at
// base + b * batch_stride + t * ld  (this is how the conv stem reads overlapping windows).
struct GemmArgs {
  const half_t* A;
  long a_lo;               // > 0: A rows are [hi(K) | lo(K)] pairs, lo half a_lo elements after the hi half, and W is the PLAIN [N][K]
                           // matrix: C = (A_hi + A_lo) W^T with each W K-tile staged once (gemm256p SPLITW; only where
                           // plan_gemm() takes it -- elsewhere the caller passes K-doubled operands [A_hi | A_lo], [W | W])
  int lda;                 // elements between consecutive A rows inside a batch
  int a_rows_per_batch;    // 0 => flat
  long a_batch_stride;     // elements
  const half_t* W;         // [N][ldw]
  int ldw;
  const float* bias;       // [N] or nullptr
  void* C;                 // f16 or f32, see `out_mode`
  int ldc;
  int c_rows_per_batch;    // 0 => flat
  long c_batch_stride;     // elements
  long c_lo;               // out_mode 4: elements from a value's hi half to its lo half (a multiple of 8)
  const float* addend;     // optional PRE-activation addend addend[m * ld_addend + n] (f32): added to the accumulator (with the bias) before GELU / the store --
                           // the A_hi W_lo^T term of a weight matrix that is not exact in f16 (engine_weights.hip, W_lo slab); out_mode 0 / 1 / 4 of the tile kernels
  int ld_addend;
  const float* pos;        // optional additive table pos[(m % pos_period)][N] (f32), or nullptr
  int pos_period;
  int M, N, K;             // K % 64 == 0
  int gelu;                // apply exact (erf) GELU after bias
  int out_mode;            // 0: store f16, 1: store f32, 2: f32 accumulate (C += result),
                           // 4: store the value as an f16 PAIR hi = f16(v) at C, lo = f16(v - hi) at C + c_lo (reference-precision
                           //    "split" mode, see wca_set_precision; GELU is then the erff form, not the 1.5e-7 polynomial),
                           // 3: f32 accumulate + LayerNorm of the updated row -> ln_out (f16); the row statistics are
                           //    exchanged between the N/256 workgroups that share a 256-row panel (gemm_epilogue.h)
  unsigned a_bytes, w_bytes; // valid bytes behind A / W (buffer-descriptor bounds); 0 => derived for flat layouts
  int force_tile;          // GemmForceTile (tests, tools)
  // out_mode 3 only (the residual GEMMs of a transformer block, N = n_state <= 2048, a multiple of 256):
  const float* ln_gamma;   // [N]
  const float* ln_beta;    // [N]
  half_t* ln_out;          // [M][ln_ld] f16: LayerNorm(C) with C the updated residual row
  int ln_ld;
  float ln_eps;
  unsigned long long* ln_stats;  // workspace [N/256][ceil(M/256)*256] x {mean, M2} f32 pairs (written + read inside the launch)
  unsigned* ln_cnt;        // workspace [ceil(M/256)] arrival counters, ZEROED by launch_gemm before the launch
  int* ln_err;             // device int: bit 1 is raised if a workgroup gave up waiting for its panel's statistics
  int site;                // 0 generic, 1 encoder block (QKV / out-projection / fc1), 2 decoder, 3 conv stem / cross-KV / logits,
                           // 4 encoder fc2: selects a distinct kernel symbol per call site so rocprofv3 --stats separates them
  int supertile;           // 256x256 persistent kernel: m-panels per supertile of the tile order (0 = chosen by launch_gemm)
  int cu_limit;            // > 0: a cap on the persistent grid, for tests (one workgroup walks many tiles of a small shape); the engine leaves it 0
  // ---- few-row kernel only (gemm_rows.hip, launch_gemm_rows):
  const float* A32;        // non-null: the A operand is LayerNorm(A32 rows; ln_gamma, ln_beta, ln_eps) computed in the prologue
  int lda32;               // floats between A32 rows (K == row length)
  half_t* kv_k;            // non-null (out_mode 0, N == 3 kv_d): columns [kv_d, 2 kv_d) of row m go to kv_k + m * kv_bs + kv_t * kv_d,
  half_t* kv_v;            // columns [2 kv_d, 3 kv_d) to kv_v + ... (the step's KV-cache append); columns [0, kv_d) to C as usual
  long kv_bs;              // elements between batch rows of a cache plane (T_max * d)
  int kv_t, kv_d;
  size_t sk_bytes;         // launch_gemm (128 x 128 tile kernel, out_mode 2, few tiles and K >= 2048): bytes behind sk_part; it then
                           // splits K over up to 4 workgroups per tile ([slice][M][N] f32 partials + an ordered reduce kernel)
  float* sk_part;          // split-K workspace (gemm_rows_workspace_bytes) and
  unsigned* sk_cnt;        // one arrival counter per (64-row block, 16-column group), zero before the first launch (self-cleaning)
  int splitk;              // workgroups sharing K (0 = chosen by launch_gemm_rows: smallest with K / splitk <= 1024)
  int groups;              // 16-column groups per workgroup (0 = chosen: grid.x <= 256)
  const int* kv_t_rows;    // few-row kernel, with kv_k: non-null = row m appends at position kv_t_rows[m] (device [M], clamped to [0, kv_tmax))
  int kv_tmax;             // instead of kv_t: the rows of the per-row wca_decode sit at different positions
};
// Forced kernel choices: tests and tools pack the value into bits 8-19 of the out_mode they hand to wca_test_gemm*
enum GemmForceTile {
  GEMM_TILE_AUTO = 0,
  GEMM_TILE_SKINNY = 64,        // the skinny kernel, or nothing
  GEMM_TILE_128 = 128,
  GEMM_TILE_256 = 256,          // the two-barrier 256 x 256 kernel
  GEMM_TILE_PERSIST = 257,      // the persistent 256 x 256 kernel
  GEMM_TILE_PERSIST_ONE = 258,  // ... with one tile per workgroup
};
// dynamic LDS of the tile kernels: what a launch asks for, and the limit its kernel symbol is given (launch.h)
constexpr int GEMM_LDS_128 = 2 * 2 * 128 * 64 * (int)sizeof(half_t);                       // gemm_f16_kernel: two slots of A | W, 64 KiB
constexpr int GEMM_LDS_256 = 2 * 2 * 256 * 64 * (int)sizeof(half_t);                       // gemm256_f16_kernel: 128 KiB
constexpr int GEMM_LDS_256P = GEMM_LDS_256 + 2 * 256 * (int)sizeof(float);                 // gemm256p_f16_kernel: + the tile's bias values, double buffered
constexpr int GEMM_LDS_256P_LN = GEMM_LDS_256P + (2 * 512 + 2560) * (int)sizeof(float);    // ... out_mode 3: + gamma | beta (double buffered) + the statistics exchange area
constexpr long GEMM_MIN_TILES_256 = 192;   // fewer 256 x 256 tiles go to the 128 x 128 kernel: the 256 x 256 kernels run one workgroup per CU

// What launch_gemm does with a GemmArgs, decided on the host without a HIP call (gemm_plan.cpp): every argument check and every choice
// of kernel, grid and LDS. Callers that must know the outcome beforehand (pair operands or K-doubled ones, the fused LayerNorm or a
// launch of its own) plan the launch they would make and look.
enum class GemmKernel { None /* M or N is 0: nothing to launch */, Skinny, Tile128, Tile256, Persist256, Persist256Pair2, Persist256Pair3, Persist256LN };
struct GemmPlan {
  GemmKernel kernel;
  unsigned grid_x, grid_y, block;
  unsigned lds;            // dynamic LDS of the launch
  int splitk;              // 128 x 128 kernel only, else 1
  int supertile;           // GemmArgs.supertile of the launch
  unsigned a_bytes, w_bytes;
  int site_used;           // the SITE instance that is launched: the pair forms exist for sites 1 and 4 (two-slot rings) or 1-4, out_mode 3 for 1 and 4
  const char* refused;     // null, or why the arguments are not taken (launch_gemm: hipErrorInvalidValue)
  bool pair() const { return kernel == GemmKernel::Persist256Pair2 || kernel == GemmKernel::Persist256Pair3; }
};
GemmPlan plan_gemm(const GemmArgs& a, int n_cu);
hipError_t launch_gemm(const GemmArgs& a, hipStream_t s);
// Few-row GEMM (M <= a few hundred rows: greedy-decode steps, batch-1 decoder forwards) with optional LayerNorm prologue,
// KV-cache append and deterministic split-K; returns hipErrorInvalidValue for shapes it does not take (gemm_rows_supported)
hipError_t launch_gemm_rows(const GemmArgs& a, hipStream_t s);
bool gemm_rows_supported(int M, int N, int K, bool layernorm_a);
int gemm_rows_pick_splitk(int K);
size_t gemm_rows_workspace_bytes(int M, int N, int splitk);
// Which path a decoder GEMM on M rows takes (engine_forward.hip dec_gemm), decided on the host without a HIP call (gemm_plan.cpp;
// wca_test_dec_gemm_plan pins it on the CPU): the few-row kernel for M <= DEC_ROWS_MAX rows of a shape it takes whose split-K workspace
// fits the engine's (a split-K launch takes no KV append), otherwise the separate LayerNorm / GEMM / kv_append launches.
constexpr int DEC_ROWS_MAX = 128;
struct DecSkCapacity {
  size_t tiles, floats;    // arrival counters and f32 partials of the engine's few-row split-K workspace
};
DecSkCapacity dec_sk_capacity(int n_text_state);
struct DecGemmPlan {
  bool few_row;
  int splitk, groups;      // what launch_gemm_rows runs with (groups as it chooses them); 0 where few_row is false, as everything below
  unsigned grid_x, grid_y;
  size_t lds;              // dynamic LDS of the launch
  size_t ws_bytes;         // split-K partials of the launch
};
DecGemmPlan plan_dec_gemm(int M, int N, int K, bool layernorm_a, bool kv_append, const DecSkCapacity& cap);

// ---------------------------------------------------------------- attention (attention.hip)
// Flash-style multi-head attention with head_dim == 64 (every Whisper size).
// Optionally writes the pre-softmax logits q.k*scale (f32) of the first `cap_cols` keys.
struct AttnArgs {
  const half_t* Q; long q_bs; int q_rs;   // element strides: batch, row
  const half_t* K; long k_bs; int k_rs;
  const half_t* V; long v_bs; int v_rs;
  half_t* O; long o_bs; int o_rs;
  float* cap;                              // nullptr => no capture
  long cap_bs; long cap_hs; int cap_ld;    // cap[b*cap_bs + h*cap_hs + q*cap_ld + key]
  int cap_cols;                            // keys [0, cap_cols) are captured, and nothing past them is written (cap_ld % 4 == 0, cap_ld >= roundup4(cap_cols))
  int nq, nk, H, B;
  float scale;                             // applied to q.k (head_dim^-0.5)
  int causal;
  int variant;                             // 0 auto, 1 force the 16x16x32 kernel, 2 force the 32x32x16 kernel (tests)
  // split-f16 operands (reference-precision mode): every value x is carried as hi = f16(x), lo = f16(x - hi). The pointers above
  // address the hi halves; the lo half of an element lives `*_lo` elements further (same strides). split != 0 selects
  // attn_split_kernel: S = Qhi.Khi + Qhi.Klo + Qlo.Khi, O = Phi.Vhi + Phi.Vlo + Plo.Vhi, fp32 softmax on the exact logits.
  int split;
  long q_lo, k_lo, v_lo, o_lo;
  // per-row key counts (device [B], nullable): batch row b attends to keys [0, min(nk_rows[b], nk)). Only the one-query f16 kernel
  // of the decode step takes it (nq == 1, no capture, no mask, not split): anything else is hipErrorInvalidValue. Row b gets the key
  // partition and summation order of a uniform call with nk = nk_rows[b].
  const int* nk_rows;
  // rows of a group share one K / V (wca_decode_group: decoder row b is a beam of audio b / kv_group and attends to that audio's
  // cross-K/V): kv_group > 1 indexes K and V by b / kv_group. Only the one-query f16 kernel with uniform key counts takes it, as its own
  // instance; 0 and 1 mean the plain form, whose instances hold none of this.
  int kv_group;
};
hipError_t launch_attention(const AttnArgs& a, hipStream_t s);
hipError_t launch_attention_split(const AttnArgs& a, hipStream_t s);  // attention_split.hip (launch_attention forwards a.split != 0 here)
// (diagnostic switch DBG_ATTN_SPLIT_DROP, 0 in the product: leaves single passes out of the encoder's three-pass attention -- bit 0 K_lo Q_hi,
// bit 1 K_hi Q_lo, bit 2 V_lo P_hi, bit 3 V_hi P_lo; masks 0, 1, 2, 3, 4, 8, 9, 12, 15 are instantiated)

// ---------------------------------------------------------------- small ops (elementwise.hip)
// ld_out: elements between output rows (0 = d). lo_off != 0: split output, hi = f16(y) at out, lo = f16(y - hi) at out + lo_off
hipError_t launch_layernorm_f16(const float* x, const float* gamma, const float* beta, half_t* out,
                                int rows, int d, float eps, hipStream_t s, int ld_out = 0, long lo_off = 0);
// x[b*n + i][:] = tok_emb[tokens[b*n+i]][:] + pos_emb[i][:]
// ids outside [0, n_vocab) are embedded as token 0 and raise *err (device int, nullable)
// tok_emb_lo (nullable): the lo halves of an embedding table that is not exact in f16 (value = hi + lo)
hipError_t launch_embed(const int64_t* tokens, const half_t* tok_emb, const float* pos_emb, float* x,
                        int B, int n, int d, int n_vocab, int* err, hipStream_t s, const half_t* tok_emb_lo = nullptr);
hipError_t launch_fill_f16(half_t* p, size_t n, float v, hipStream_t s);

// ---------------------------------------------------------------- greedy ASR decode steps (decode.hip)
// Where the rows of a decode step are: every row at position t (rows == nullptr), or row b at rows[b] (device [B], clamped to the slots the launch
// addresses; the per-row wca_decode). Host side only: each launcher picks the scalar or the table form of its kernel and runs that form's checks.
// The engine reads rows (and AttnArgs.nk_rows, DecodeSelectArgs.cur_len_rows) from per-step tables it builds once per call on the host
// instead of adding a scalar step to row_pos[b] in every kernel: a row past its sample budget stays in the batch at a CLAMPED position
// (<= T_max - 2: no positional row past n_text_ctx - 1, no cache slot past T_max - 1), the attention needs a plain count array anyway, and
// the clamp then lives in one place. 3 * steps * B ints per call.
struct StepPos {
  int t;
  const int* rows;
};
// x[b][:] = tok_emb[tokens[b*T_max + pos_b]][:] + pos_emb[pos_b][:]
hipError_t launch_embed_step(const int* tokens, int T_max, StepPos pos, const half_t* tok_emb, const float* pos_emb, float* x, int B, int d,
                             int n_vocab, hipStream_t s);
// k / v columns of qkv [B][3d] -> kc / vc [B][T_max][d] at position pos_b
hipError_t launch_kv_append(const half_t* qkv, half_t* kc, half_t* vc, int B, int T_max, StepPos pos, int d, hipStream_t s);
// prefill of a prompted decode (all n initial positions of every row in one forward):
// x[b*n + i][:] = tok_emb[tokens[b*T_max + i]][:] + pos_emb[i][:] for i < n
hipError_t launch_embed_prefix(const int* tokens, int T_max, int n, const half_t* tok_emb, const float* pos_emb, float* x, int B, int d,
                               int n_vocab, hipStream_t s);
// k / v columns of qkv [B*n][3d] -> kc / vc [B][T_max][d] at positions [0, n)
hipError_t launch_kv_scatter(const half_t* qkv, half_t* kc, half_t* vc, int B, int n, int T_max, int d, hipStream_t s);
// out [B][d] = rows (b, p0) of x [B*n][d] f32, and out [B..2B) = rows (b, p1) where p1 is given (p1.t >= 0; with p0.rows: p1.rows non-null).
// p0 decides the form; the per-row positions are clamped to [0, n)
hipError_t launch_gather_rows(const float* x, float* out, int B, int n, StepPos p0, StepPos p1, int d, hipStream_t s);
// logit filters + greedy update of one decoding step (upstream decoding.py: SuppressBlank, SuppressTokens,
// ApplyTimestampRules, GreedyDecoder.update at temperature 0, or -- per-row form, temperature_rows -- at a temperature per row); one
// workgroup per batch row
struct DecodeSelectArgs {
  const float* logits;                 // [B] rows, ld apart: the last position's fp32 logits
  int ld, n_vocab;
  int* tokens;                         // [B][T_max]; row b holds cur_len tokens, the new one is written at [cur_len]
  int T_max, cur_len, n_initial;
  const unsigned char* suppress_mask;  // [n_vocab] 1 = always -inf (SuppressTokens, <|notimestamps|>)
  const unsigned char* blank_mask;     // [n_vocab] 1 = -inf on the first sampled position (SuppressBlank); nullable
  int eot, timestamp_begin;
  int apply_timestamp_rules, max_initial_timestamp_index;  // index < 0: no limit
  float* sum_logprob;                  // [B] accumulated log-probability of the sampled tokens
  int* n_done;                         // [T_max] n_done[cur_len] += 1 for every row whose new token is EOT
  // the per-row form (device [B] each; cur_len_rows != nullptr selects it, cur_len / n_initial above are then unused):
  const int* cur_len_rows;             // tokens row b holds; SuppressBlank / the first-timestamp rules fire at cur_len_rows[b] == n_initial_rows[b]
  const int* n_initial_rows;           // the timestamp history is tokens[b][n_initial_rows[b] : cur_len_rows[b]]
  const int* cap_rows;                 // sample budget: a row with cur_len - n_initial >= cap is a finished row (EOT, nothing added)
  int n_done_idx;                      // n_done[n_done_idx] += 1 per row whose new token is EOT (the step, not cur_len)
  // the sampling form (per-row form only; temperature_rows != nullptr selects it; device [B] each): GreedyDecoder.update at temperature > 0,
  // drawn by Gumbel-max over the filtered logits. A row at temperature 0 takes the argmax as the greedy form does, bit for bit.
  const float* temperature_rows;            // T: next = argmax_v (lg[v] * (1 / T) + G(v)); sum_logprob still adds the UNTEMPERED log-softmax
  const unsigned long long* seed_rows;      // Philox4x32-10 key (low word, high word); counter (v >> 2, cur_len - n_initial, 0, 0), word v & 3
};
hipError_t launch_decode_select(const DecodeSelectArgs& a, int B, hipStream_t s);
// out[b] = softmax(logits[b])[token]  (no_speech_prob: the <|nospeech|> probability at the <|sot|> position)
hipError_t launch_token_prob(const float* logits, int ld, int n_vocab, int token, float* out, int B, hipStream_t s);
hipError_t launch_f32_to_f16(const float* in, half_t* out, size_t n, hipStream_t s);
// ---------------------------------------------------------------- beam step and cache reorder (beam.hip)
// Decoder row r = b * G + g is beam g of audio b (wca_decode_group). A step is two launches: the per-row candidates, then the per-audio merge.
constexpr int BEAM_GROUP_MAX = 16;
// (a) one workgroup per row: the filters of decode_select (the per-row form of `sel`: cur_len_rows / n_initial_rows / cap_rows), the fp32
// log-softmax of the filtered logits, the top K = G + 1 entries -- the lowest token first among equal logits -- into cand_tok / cand_lp
// [R][K]. Entries past the tokens the filters leave, and every entry of a row that is past its budget, are token -1 at -inf.
struct BeamTopkArgs {
  DecodeSelectArgs sel;   // logits, masks, options and the CURRENT token rows; sum_logprob / n_done are not used
  int K;
  int* cand_tok;
  float* cand_lp;
};
hipError_t launch_beam_topk(const BeamTopkArgs& a, int R, hipStream_t s);
// (b) one wave per audio, upstream's BeamSearchDecoder.update: the G K candidates score sum_logprob[source] + logprob and are walked in the
// order (score descending, source beam ascending, token ascending); a candidate ending in eot is newly finished, the others become the G
// next beams and the walk stops at the G-th. The newly finished ones join the audio's finished list, best first, while it holds fewer than
// max_candidates. tok_out row b * G + g = tok_in row src, its first cur_len tokens, then the new token (tok_in and tok_out are two
// buffers); sum_logprob is updated in place, src[r] is the ABSOLUTE source row, trace[r] = (src[r], token). first != 0: only beam 0 of a
// group offers candidates (the beams are still identical). An audio past its budget is copied through (src[r] = r, trace token -1). *n_done
// counts the audios whose finished list is full after this step or that are past their budget.
struct BeamMergeArgs {
  const int* cand_tok;
  const float* cand_lp;
  int K, G;
  const int* tok_in;
  int* tok_out;
  int T_max;
  float* sum_logprob;                                  // [R]
  int* src;                                            // [R]
  const int *cur_len_rows, *n_initial_rows, *cap_rows;  // [R]: the rows of a group hold their audio's values
  int first, eot, max_candidates;
  int* fin_n;      // [B] sequences in the audio's finished list
  int* fin_len;    // [B][max_candidates] tokens before the closing eot
  float* fin_sum;  // [B][max_candidates]
  int* fin_tok;    // [B][max_candidates][T_max]
  int* trace;      // [R][2] of this step
  int* n_done;
};
hipError_t launch_beam_merge(const BeamMergeArgs& a, int B, hipStream_t s);
// For every plane p < n_planes (a decoder layer's K or V cache) and row r < rows_dst: dst[p][r][0 : n_keep[r]] = src[p][s][0 : n_keep[r]]
// with s = src_idx[r], or r / div where src_idx is null (the broadcast of an audio's prefill to its group); planes are [rows][T_max][d] f16,
// copied 8 halfs at a time (d % 8 == 0). s is clamped to [0, rows_src) and n_keep[r] to [0, T_max]; src and dst must not overlap.
hipError_t launch_kv_reorder(const half_t* src, half_t* dst, int n_planes, int rows_src, int rows_dst, int T_max, int d, const int* src_idx,
                             int div, const int* n_keep, hipStream_t s);
// ---------------------------------------------------------------- language identification head (language_head.hip)
// x [B][d] f32: the final residual stream at the <|sot|> position. Per row: xn = f16(LayerNorm(x; gamma, beta)), logit_j = xn . tok_emb[lang_begin + j]
// (fp32 accumulation) for j < n_lang, probs [B][n_lang] = softmax(logit), lang_token [B] = lang_begin + argmax (lowest index among equals).
// hipErrorInvalidValue: d % 8 != 0 (or d > 1280), n_lang outside [1, 128], [lang_begin, lang_begin + n_lang) not inside [0, n_vocab).
hipError_t launch_language_head(const float* x, const float* gamma, const float* beta, const half_t* tok_emb, int B, int d, int n_vocab,
                                int lang_begin, int n_lang, float* probs, int* lang_token, hipStream_t s);
// ---------------------------------------------------------------- teacher-token log-probabilities (token_prob.hip)
// the f32 rows that predict a text token: row (b, sot_len + i) of x [B * n_tok_max][d] for i < n_tok[b] - sot_len - 2 -> out [row_off[b] + i][d],
// row_map[row_off[b] + i] = b * n_tok_max + i (n_tok, row_off: device [B]; n_text_max >= every n_text)
hipError_t launch_gather_text_rows(const float* x, int n_tok_max, int d, int sot_len, const int* n_tok, const int* row_off, int B, int n_text_max,
                                   float* out, int* row_map, hipStream_t s);
// out[idx] = log_softmax(logits[r][0 : vocab_end])[targets[idx + tgt_off]] for r < rows, idx = row_map ? row_map[r] : r (logits rows ld floats
// apart); a target outside [0, vocab_end) gives NaN and raises err_bit in *err
hipError_t launch_token_logprob(const float* logits, long ld, int vocab_end, int rows, const int64_t* targets, const int* row_map, int tgt_off,
                                float* out, int* err, int err_bit, hipStream_t s);

// ---------------------------------------------------------------- log-mel (logmel.hip)
struct LogMelTables {      // what pass 1 of every log-mel form reads
  const float* filters;    // [n_mels][201]
  const int* filt_lo;      // [n_mels] first non-zero bin of each filter (device)
  const int* filt_hi;      // [n_mels] one past the last non-zero bin (device)
  const float* window;     // [400] periodic hann
  const float* twiddle;    // [400][2] cos,sin(2*pi*m/400)
  int precise;             // != 0: the DFT and the filterbank sums accumulate in f64 (reference-precision mode)
  int n_mels;
};
struct LogMelArgs : LogMelTables {
  const float* pcm;        // [B][pcm_stride] f32 16 kHz, already trimmed/padded by the caller or shorter
  long pcm_stride;
  const int* n_samples;    // [B] valid samples per utterance (<= 480000); device pointer
  float* mel_out;          // [B][n_mels][3000] f32 (may be nullptr)
  half_t* mel_tm;          // [B][3002][n_mels_pad] f16 time-major, rows 0 and 3001 zero (may be nullptr)
  int n_mels_pad;          // row length of mel_tm
  int tm_lo;               // != 0: mel_tm carries split values, hi at column m, lo = f16(v - hi) at column tm_lo + m
  float* scratch;          // [B][n_mels][3000] raw log10 values (required)
  unsigned* gmax;          // [B] ordered-int encoded running max (required)
  int B;
};
hipError_t launch_logmel(const LogMelArgs& a, hipStream_t s);

// whisper.log_mel_spectrogram(audio, n_mels, padding=480000) of a recording of any length: n_samples of pcm followed by 480000 zeros,
// n_frames = (n_samples + 480000) / 160 frames, ONE floor (max over the whole recording) - 8. mel_out [n_mels][ld] f32 (ld >= n_frames)
// holds the raw log10 values between the two passes, so there is no scratch; gmax is one ordered-int word.
struct LogMelLongArgs : LogMelTables {
  const float* pcm;        // [n_samples] f32 16 kHz
  long n_samples;
  float* mel_out;          // [n_mels][ld]
  long ld;
  long n_frames;           // (n_samples + 480000) / 160
  unsigned* gmax;
};
hipError_t launch_logmel_long(const LogMelLongArgs& a, hipStream_t s);

// pad_or_trim(mel[:, seek : seek + size], 3000) for B windows of one long mel: out [B][n_mels][3000] f32, exact zeros at t >= size[b].
// seek / size are device arrays; the caller has checked 0 <= seek, 1 <= size <= 3000, seek + size <= the long mel's frames.
hipError_t launch_mel_window(const float* mel_long, long ld, int n_mels, const int* seek, const int* size, int B, float* out, hipStream_t s);

// ---------------------------------------------------------------- quiet cuts of a long recording (quiet_cuts.hip)
constexpr int QUIET_PIECES_MAX = 4096, QUIET_RADIUS_MAX = 1500, QUIET_HALF_WIDTH_MAX = 100;
// The interior cuts of wca_quiet_cuts (include/wca.h has the definition): cuts [n_pieces - 1] and level [n_pieces - 1] are device arrays,
// entry k - 1 for target g_k. Only frames [0, content_frames) of mel_long [n_mels][ld] are read. The caller has checked the ranges of
// include/wca.h (the launcher refuses what would leave the kernel's LDS or let two search ranges meet).
hipError_t launch_quiet_cuts(const float* mel_long, long ld, int n_mels, long content_frames, int n_pieces, int radius, int half_width,
                             int* cuts, int* level, hipStream_t s);

// ---------------------------------------------------------------- speech segments of a long recording (speech_segments.hip)
// The options of wca_speech_segments, in the order of wca_vad_opts (include/wca.h has the definition and the ranges).
struct VadOpts {
  int half_width, floor_permille, peak_permille, on_share, off_share, min_range, min_speech, min_silence, pad;
};
// The device scratch of one call, carved out of one allocation: vad_scratch(nullptr, ...) gives the size in `bytes`, a second call with
// the allocation's base the pointers. cap = the (start, stop) pairs `segs` holds.
struct VadScratch {
  int *e, *s;                    // [cf] frame levels and smoothed levels
  unsigned char *f0, *f1;        // [cf] the activity flags of the stages, ping-pong
  int *agg_last, *agg_first;     // [tiles] per tile of VAD_TILE frames: the last / first frame the next stage's scan starts from
  int *carry_f, *carry_b;        // [tiles + 1] what enters a tile from the tiles before / after it
  unsigned *hist, *sel;          // [2][256] radix histograms of both ranks; {prefix lo, prefix hi, rank lo, rank hi}
  int *stats, *segs;             // [6] as stats_host; [cap][2]
  size_t bytes;
};
constexpr int VAD_TILE = 1024;
VadScratch vad_scratch(void* base, long content_frames, long cap);
// Everything of wca_speech_segments on the device, with no return to the host in between: sc.stats and sc.segs hold the result.
// The caller has checked the ranges of include/wca.h, n_mels <= 128 and 1 <= content_frames <= ld.
hipError_t launch_speech_segments(const float* mel_long, long ld, int n_mels, long content_frames, const VadOpts& o, long cap,
                                  const VadScratch& sc, hipStream_t s);

// ---------------------------------------------------------------- resampler to 16 kHz (resample.hip)
constexpr int RESAMPLE_SR_OUT = 16000, RESAMPLE_SR_MIN = 2000, RESAMPLE_SR_MAX = 384000;
enum { RESAMPLE_HOME_UNIFORM = 0, RESAMPLE_HOME_LDS = 1, RESAMPLE_HOME_GLOBAL = 2 };   // where the kernel reads the polyphase table from
struct ResamplePlan {
  int L, M, W, n_taps;     // 16000 / g, sr_in / g, half width in input samples, 2 W + 2
  int home;                // RESAMPLE_HOME_*
  int tile, span_max;      // outputs per tile, input samples a tile stages at most
};
int resample_plan(int sr_in, ResamplePlan* pl);          // host only; -1 for sr_in outside [RESAMPLE_SR_MIN, RESAMPLE_SR_MAX]
void resample_table(const ResamplePlan& pl, double* h);  // host only: h [L][n_taps] f64
struct ResampleArgs {
  const float* in;         // [channels][ld] f32, n_in <= ld samples per channel, any 4-byte aligned address and any ld
  int channels;
  long ld, n_in;
  float* out;              // [n_out] f32 16 kHz: the filtered mean over channels
  long n_out;              // ceil(n_in L / M) (n_in when plan is null)
  const ResamplePlan* plan;  // null: the input is at 16 kHz already (copy / channel mean)
  const float* table;      // device f32: [n_taps][L] for RESAMPLE_HOME_LDS, [L][n_taps] otherwise
  int max_blocks;          // grid cap: the workgroups stride over the tiles
};
hipError_t launch_resample(const ResampleArgs& a, hipStream_t s);

// ---------------------------------------------------------------- post-processing (postproc.hip)
struct HeadStatsArgs {
  const float* qk;         // captured logits: qk[b*qk_bs + head*qk_hs + t*qk_ld + f]
  long qk_bs; long qk_hs; int qk_ld;
  float* weights;          // optional dense out: weights[b*w_bs + head*n*F... ] see w_* (nullptr => skip)
  long w_bs;               // elements between utterances
  const int* n_tok;        // [B] decoder rows per utterance (device)
  const int* n_frames;     // [B] F per utterance (device)
  int n_tok_max, n_frames_max;  // strides of the dense `weights` layout: [head][n_tok_max][n_frames_max]
  float* colnorm;          // [B][LH][n_frames_max] per-head column L2 norms
  float* scores;           // [B][LH]
  float* rowstats;         // optional [B][LH][n_tok_max][2] = (row max of med*scale, sum of exp) so that selected
                           // heads can be re-materialised later without storing `weights`
  int LH, B, medfilt_width;
  float qk_scale, w_col, w_row, w_cov;
  int input_is_weights;    // 1: `qk` already holds softmaxed weights (filter_attention on a given tensor): no median/softmax
};
hipError_t launch_head_stats(const HeadStatsArgs& a, hipStream_t s);

// ascending top-k (python tuple order: score, then flat head index); k_eff = min(k, LH)
hipError_t launch_topk(const float* scores, int LH, int B, int k, int* sel_idx /*[B][k]*/,
                       float* sel_score /*[B][k]*/, hipStream_t s);

struct AggregateArgs {
  const float* weights; long w_bs; int n_tok_max, n_frames_max;
  const float* colnorm;    // [B][LH][n_frames_max]
  const int* sel_idx;      // [B][n_sel] head ids (or nullptr => heads [head_lo, LH))
  int n_sel, head_lo, LH, B;
  const int* n_tok; const int* n_frames;
  int row_lo, row_hi_trim; // output rows [row_lo, n_tok - row_hi_trim)
  float* matrix;           // [B][n_tok_max][n_frames_max]
  // recompute mode (weights == nullptr): re-derive the softmaxed value from the captured logits + rowstats
  const float* qk; long qk_bs; long qk_hs; int qk_ld;
  const float* rowstats;   // [B][LH][n_tok_max][2]
  int medfilt_width; float qk_scale;
};
hipError_t launch_aggregate(const AggregateArgs& a, hipStream_t s);

// default_find_alignment (timing.py:159-163): out[s][t][f] = (ws[sel[s]][t][f] - mean_t) / std_t (population std over
// the n token rows), then matrix = mean over s of rows [row_lo, n - row_hi_trim). ws [LH][n][F], out [n_sel][n][F].
hipError_t launch_stdmean_normalize(const float* ws, const int* sel_dev, int n_sel, int n, int F, float* out, hipStream_t s);
hipError_t launch_mean_heads(const float* x, int n_sel, int n, int F, int row_lo, int row_hi_trim, float* matrix, hipStream_t s);

// per-head strict word-boundary scoring of the probe (metrics.py:45-72 over every head of probe_oracle.py:83-90): tp_out[hd]
hipError_t launch_probe_strict(const int* jump, int jump_ld, int LH, const int* wb_end, int n_hyp, const double* y, int n_ref,
                               const unsigned char* eq, double tol, int* tp_out, hipStream_t s);

// standalone median filter along the last axis with reflect padding (whisper.timing.median_filter)
hipError_t launch_median_filter(const float* in, float* out, long rows, int F, int width, hipStream_t s);

// ---------------------------------------------------------------- alignment-heads post-processing (align_heads.hip)
// openai-whisper's find_alignment on the captured logits of a ragged batch, over a fixed list of S heads: softmax over the frames, then
// (w - mean) / std per head and frame over the token axis, then the median filter, then the mean over the heads, for the rows
// [sot_len, n_tok - 1) the DTW is given. Three launches; the S maps are never written out, only their row and column statistics.
struct AlignHeadsArgs {
  const float* qk;         // captured logits: qk[b*qk_bs + head*qk_hs + t*qk_ld + f], as HeadStatsArgs
  long qk_bs; long qk_hs; int qk_ld;
  const int* heads;        // [S] device: layer * H + head, summed in this order
  int S;
  const int* n_tok;        // [B] decoder rows per utterance (device)
  const int* n_frames;     // [B] F per utterance (device)
  int n_tok_max, n_frames_max, B;
  int sot_len, medfilt_width;
  float qk_scale;
  float* rowstats;         // [B][S][n_tok_max][2] = (row max of qk*scale, sum of exp)
  float* colstats;         // [B][S][n_frames_max][2] = (mean, population std) of the softmaxed column over the n_tok rows
  float* matrix;           // [B][n_tok_max][n_frames_max], rows [0, n_tok - sot_len - 1) of an utterance, as AggregateArgs::matrix
};
hipError_t launch_align_heads(const AlignHeadsArgs& a, hipStream_t s);

// ---------------------------------------------------------------- DTW (dtw.hip)
struct DtwArgs {
  const float* matrix;     // P problems: matrix + p*m_bs, rows ld apart; DTW runs on the NEGATED matrix
  long m_bs; int ld;
  const int* N;            // [P] rows per problem (device)   (or nullptr => N_all)
  const int* M;            // [P] cols per problem (device)   (or nullptr => M_all)
  int N_all, M_all;
  int N_max, M_max;
  uint32_t* trace;         // workspace: P * N_max * ceil(M_max/16) words
  int* path;               // [P][2][cap] text idx row then time idx row, right-aligned; cap = N_max + M_max + 2
  int* path_len;           // [P]
  int* jump_frame;         // [P][jump_ld] first frame of each text row (or nullptr)
  int jump_ld;             // row stride of jump_frame (>= N_max)
  int P;
  // open-end form (either of the first two set: the launch takes the open-end kernel, which also serves its closed problems): the path
  // of an open problem ends in the last frame at the row n* of the smallest cost per path cell; jump_frame[i] = -1 for n* < i < N
  const int* open_end;     // [P] 1 = open, 0 = closed (device)   (or nullptr => open_all)
  int open_all;
  int* end_row;            // [P] n* (N - 1 for a closed problem, -1 for a refused one), or nullptr
  float* score;            // [P] C / L at the end cell, for diagnostics (no decision reads it), or nullptr
  // windowed form (both set, or both null): cell (i, j) of problem p is allowed iff row_lo[p*win_ld + i] <= j <= row_hi[p*win_ld + i]; the
  // launch takes the windowed kernel. The windows must be valid (dtw_windows_invalid), and an open problem's must be full ([0, M-1]).
  const int* row_lo;       // [P][win_ld] device, entries [0, N[p]) of a problem are read
  const int* row_hi;
  int win_ld;              // row stride of row_lo / row_hi (>= N_max)
};
hipError_t launch_dtw(const DtwArgs& a, hipStream_t s);
// host check of one n x m problem's windows: nullptr if valid, else the failed condition (*row: where)
const char* dtw_windows_invalid(const int* lo, const int* hi, int n, int m, int* row);

// ---------------------------------------------------------------- per-row score of the DTW path (path_score.hip)
// Behind launch_dtw(d) on the same stream: for text row i of problem p, cells = the number of path cells in that row and mean = the f32
// rounding of the f64 mean of matrix[i][j] (NOT negated) over them. Within a row the path only moves along the frame axis, so the cells are
// the frames jump[i] .. last[i]: last = M - 1 for the end row, else jump[i+1] where the trace enters row i + 1 vertically (that column is in
// both rows) and jump[i+1] - 1 where it enters diagonally. Rows the path does not reach (past an open end row, a problem the DTW refused,
// i >= N[p]) get (0, 0.0). Reads d.matrix, d.N / d.M, d.trace, d.jump_frame (required), d.path_len and d.end_row (null: N - 1).
struct PathScoreArgs {
  DtwArgs d;
  float* mean;             // [P][out_ld]; rows [0, d.N_max) of every problem are written
  int* cells;              // [P][out_ld]
  int out_ld;              // >= d.N_max
};
hipError_t launch_path_score(const PathScoreArgs& a, hipStream_t s);

}  // namespace wca
