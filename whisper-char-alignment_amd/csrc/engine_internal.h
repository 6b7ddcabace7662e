// What the translation units of the engine share (internal to libwca.so): the engine's state, the error plumbing and the
// functions one engine file calls in another (DESIGN.md has the file map).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/wca.h"
#include "kernels.h"

namespace wca {

int fail(int code, const char* fmt, ...);   // records the message of wca_last_error (thread-local, engine.hip) and returns code

#define HIPCHK(expr)                                                                              \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) return fail(WCA_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)

constexpr int N_FRAMES = 3000, N_CTX = 1500, MAX_TOK = 448, N_BIN = 201, N_FFT = 400;
constexpr int META_SLOTS = 16;

#define WCA_TRY(expr)          \
  do {                         \
    const int _rc = (expr);    \
    if (_rc != WCA_OK) return _rc; \
  } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct GrowBuf {
  void* p = nullptr;
  size_t bytes = 0;
  hipError_t ensure(size_t need) {
    if (need <= bytes) return hipSuccess;
    if (p) {
      hipError_t e = hipFree(p);
      if (e != hipSuccess) return e;
      p = nullptr;
      bytes = 0;
    }
    need = align_up(need, 1 << 20);
    hipError_t e = hipMalloc(&p, need);
    if (e != hipSuccess) return e;
    bytes = need;
    // debugging aid: WCA_POISON_ALLOC=1 fills every grow-only buffer with 0xFF bytes (NaN as f32 / f16, -1 as an index) when it is
    // allocated, so that a read of a never-written element shows as a wrong result on every run instead of depending on what the
    // recycled memory held
    static const bool poison = std::getenv("WCA_POISON_ALLOC") != nullptr;
    if (poison) {
      e = hipMemset(p, 0xFF, need);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
};

struct LayerW {
  float *ln1_g, *ln1_b;
  half_t* qkv_w;
  float* qkv_b;
  half_t* out_w;
  float* out_b;
  float *ln2_g, *ln2_b;  // mlp_ln
  half_t* fc1_w;
  float* fc1_b;
  half_t* fc2_w;
  float* fc2_b;
  // decoder only
  float *lnc_g, *lnc_b;
  half_t* cq_w;
  float* cq_b;
  half_t* co_w;
  float* co_b;
};

}  // namespace wca

struct wca_engine {
  wca_model_dims dims;
  int device = 0;
  int max_batch = 1;
  hipStream_t stream = nullptr;      // phase 1 (log-mel, encoder, cross-K/V) and every non-batched entry point
  hipStream_t own_stream = nullptr;
  hipStream_t stream2 = nullptr;     // phase 2 of wca_align_batch (decoder, post-processing, DTW, D2H): overlaps the next batch's phase 1
  hipEvent_t ev_kv[2] = {};          // cross-K/V of batch slot ready (recorded on `stream`)
  bool finalized = false;
  bool have_filters = false;
  bool profiling = false;
  std::set<std::string> loaded;
  std::map<std::string, size_t> inexact;  // tensors stored as f16 whose fp32 source values were NOT f16-representable: name -> count of rounded elements
  bool allow_rounded = false;             // wca_set_allow_rounded_weights: run split mode on the ROUNDED weights (faster; not the fp32 model's arithmetic)
  char* wslab_lo = nullptr;               // W_lo slab, same layout as wslab (allocated when the first inexact tensor arrives): lo = f16(w - f16(w)) of every
                                          // weight matrix element, zero where the f16 value is exact. A pair GEMM multiplies the extra term A_hi W_lo^T
  std::set<const void*> wlo_bases;        // weight matrices (base pointer the GEMM call sites use) that hold at least one non-zero lo element
  wca::GrowBuf wlo_tmp[2];                     // f32 [M][N] scratch of the extra term for the non-accumulating output modes: [0] launches on `stream` (phase 1),
                                          // [1] on any other stream (phase 2 runs beside the next batch's phase 1)

  // ---- weights
  char* wslab = nullptr;
  size_t wslab_bytes = 0, wslab_used = 0;
  int k1pad = 0;  // padded K of the conv1 GEMM
  wca::half_t *conv1_w = nullptr, *conv2_w = nullptr;
  float *conv1_b = nullptr, *conv2_b = nullptr, *enc_pos = nullptr, *lnpost_g = nullptr, *lnpost_b = nullptr;
  std::vector<wca::LayerW> enc, dec;
  wca::half_t* tok_emb = nullptr;
  float *dec_pos = nullptr, *lnf_g = nullptr, *lnf_b = nullptr;
  wca::half_t* kv_w = nullptr;
  float* kv_b = nullptr;
  float *mel_filters = nullptr, *window = nullptr, *twiddle = nullptr;
  int *filt_lo = nullptr, *filt_hi = nullptr;

  // ---- fixed activation arena (sized for max_batch)
  char* aslab = nullptr;
  float* mel_scratch = nullptr;
  unsigned* gmax = nullptr;
  float* mel_f32 = nullptr;
  wca::half_t* mel_tm = nullptr;
  wca::half_t* h1pad = nullptr;
  float* x = nullptr;      // [B*1500][d]
  wca::half_t* xn = nullptr;    // [B*1500][d]
  wca::half_t* qkv = nullptr;   // [B*1500][3d]
  wca::half_t* att = nullptr;   // [B*1500][d]
  wca::half_t* hid = nullptr;   // [B*1500][4d]
  wca::half_t* kv = nullptr;    // [B*1500][L*2*d]
  wca::half_t* kv_alt = nullptr; // second cross-K/V buffer (batches alternate, see wca_align_batch_enqueue)
  float* xd = nullptr;     // [B*448][d]
  wca::half_t* xdn = nullptr;
  wca::half_t* qkv_d = nullptr;
  wca::half_t* att_d = nullptr;
  wca::half_t* q_d = nullptr;
  wca::half_t* hid_d = nullptr;
  int* meta_dev = nullptr;   // META_SLOTS x 4 x max_batch ints: n_samples, n_tok, n_frames, dtwN
  int* meta_host = nullptr;  // pinned mirror
  int meta_slot = 0;
  unsigned long long* ln_stats = nullptr;  // out_mode 3 GEMMs: per-tile row statistics [n_state/256][B*1500 padded to 256]
  unsigned* ln_cnt = nullptr;              // ... and per-panel arrival counters (zeroed by launch_gemm)
  float* sk_part = nullptr;    // split-K workspace of the few-row GEMM (the decoder's stream) and its
  unsigned* sk_cnt = nullptr;  // arrival counters (zero at creation, self-cleaning)
  size_t sk_floats = 0, sk_tiles = 0;
  float* sk_big[2] = {nullptr, nullptr};   // split-K partials of the 128 x 128 tile GEMM (small batches: fc2): [0] the encoder's stream,
                                            // [1] the decoder's (phase 2 / the decode loop run beside the next batch's encoder)
  size_t sk_big_bytes = 0;
  int n_cu = 0;
  int* err_dev = nullptr;    // device flags raised by kernels. Word 0: phase 2 / synchronous entry points (bit 0 token id outside the
                             // vocabulary, bit 1 LayerNorm hand-off timeout, bit 2 teacher token outside [0, vocab_end) of the token log-probs;
                             // word 3: the same bit of wca_token_logprobs); words 1, 2: phase 1 of the batch in cross-K/V slot 0, 1 (bit 1
                             // only), cleared on `stream` before that batch's encoder and read with the batch's results, so that neither the
                             // phase-2 clear of this batch nor the next batch's encoder (concurrent on `stream`) can wipe or alias it
  int* ln_err = nullptr;     // where the encoder's out_mode-3 GEMMs raise their time-out bit (err_dev, or err_dev + 1 + slot in run_phase1)
  int* err_host = nullptr;   // pinned: read back by the synchronous entry points

  // ---- run-time sized buffers
  wca::GrowBuf cap, wws, colnorm, scores, sel, selsc, matrix, trace, path, pathlen, jump, tmp0, tmp1;
  wca::GrowBuf dtw_out, dtw_meta;   // open-end DTW: end rows [P] then scores [P] of the last launch; wca_dtw_batch_dev_open's flags / row / column counts
  // windowed DTW of the fused alignment: the row windows [2][batch][n_tok_max] (lo, then hi) of the two batches that may be in flight, by
  // enqueue parity like res_host -- pinned host mirror and device copy (a slot is free again once its batch has been fetched). A batch on
  // the alignment-heads route takes no windows: its slot carries the head list [n_heads] instead
  wca::GrowBuf win_dev[2];
  int* win_host[2] = {nullptr, nullptr};
  size_t win_host_ints[2] = {0, 0};
  wca::GrowBuf pscore;              // run_path_score: the per-row path means [P][ld] f32, then the cell counts [P][ld], of the last DTW launch that asked for them
  wca::GrowBuf quiet_out;           // wca_quiet_cuts: the interior cuts [n_pieces - 1] then their levels [n_pieces - 1], copied to the host before the call returns
  wca::GrowBuf vad_buf;             // wca_speech_segments: the call's whole device scratch (VadScratch), result included
  wca::GrowBuf probe_jump;         // the last wca_probe_heads' jump frames [LH][N], kept on the device for wca_probe_strict_tp
  int probe_LH = 0, probe_N = 0;
  // greedy ASR pre-pass (wca_decode): self-attention K/V cache [L][2][B][T_max][d], token rows, masks, logits
  wca::GrowBuf dec_cache, dec_tokens, dec_masks, dec_logits, dec_state;
  wca::GrowBuf dec_rows;              // the per-row wca_decode: the per-row int tables (n_initial - 1, sot_index, n_initial, sample cap; per step: fed position, key count, cur_len)
  wca::GrowBuf dec_gather;            // prefill: the f32 residual rows whose logits are needed ([2B][d]: last initial position, <|sot|>)
  wca::GrowBuf dec_beam;              // wca_decode_group: the beam step's candidates, sources, finished lists and trace
  size_t dec_cache_off = 0;           // halfs from dec_cache.p to the cache the decoder reads and appends to: 0, or the second half while a
                                      // group decode ping-pongs between the two (kv_reorder); wca_test_decode_state reads from there
  int grp_steps = 0, grp_rows = 0;    // the last wca_decode_group in beam mode: choices made and decoder rows (wca_test_beam_trace)
  size_t grp_trace_off = 0;           // bytes from dec_beam.p to its trace [steps][rows][2]
  int* dec_done_host = nullptr;  // pinned: completion counter read back while the loop runs
  // wca_resample_16k: the polyphase tables of the input rates seen so far (f32 on the device, in the layout the plan's table home reads);
  // at most 8, the oldest leaves
  struct ResampleTable { int sr_in; wca::ResamplePlan plan; float* dev; };
  std::vector<ResampleTable> rs_tables;
  int dec_prefill_positions = 0, dec_step_positions = 0;  // the last decode: positions per row fed by the prefill / one at a time
  int dec_batch = 0, dec_T_max = 0, dec_logits_rows = 0;  // the last decode's cache shape and the rows its forwards left in dec_logits (wca_test_decode_state)
  // Encoded micro-batches (log-mel + encoder + cross-K/V done, recorded on `stream`) that no alignment has consumed
  // yet: wca_encode_batch / wca_decode push, wca_align_batch_enqueue(pcm_dev = NULL) pops the oldest. A K/V
  // slot stays busy from its encode until the alignment that consumed it has been fetched.
  // detected: wca_detect_language has read this (still undecoded) state; it waits for the decode that follows with mel_dev = pcm_dev = NULL
  // and is dropped, like a decoded one, when a decode or a detection brings an input of its own
  struct EncState { int slot; int batch; bool decoded; bool detected = false; };
  std::deque<EncState> enc_q;
  bool slot_busy[2] = {false, false};
  int res_kvslot[2] = {-1, -1};
  // results ring: up to 2 wca_align_batch_enqueue calls may be in flight before their _fetch
  int* res_host[2] = {nullptr, nullptr};  // pinned results staging
  size_t res_host_ints[2] = {0, 0};
  hipEvent_t res_ev[2] = {};
  int res_topk[2] = {0, 0}, res_ntok[2] = {0, 0}, res_batch[2] = {0, 0};
  bool res_open[2] = {false, false}; // the batch in that slot was enqueued open-ended (its staging slot holds end rows and scores)
  bool res_ps[2] = {false, false};   // the batch in that slot was enqueued with path_scores (its staging slot holds the means and cell counts)
  bool res_lp[2] = {false, false};   // the batch in that slot was enqueued with token log-probs (its staging slot holds them)
  // teacher-token log-probs of wca_align_batch_enqueue with vocab_end (phase 2's stream): compact f32 rows, their final-LayerNorm output (pairs when DEC
  // is split), the row map, the chunked [rows][ldc] f32 logits scratch and the [B][n_tok_max] results
  wca::GrowBuf lp_x, lp_xn, lp_map, lp_logits, lp_out;
  unsigned long enq_count = 0, fetch_count = 0;
  int last_batch = 0;

  hipEvent_t ev[9] = {};
  // start/stop pairs around each kernel of every encoder layer (profiling only): site = WCA_SITE_* of include/wca.h
  hipEvent_t kev[WCA_N_SITES][33][2] = {};   // slot 32: ln_post of a 32-layer encoder (site LN1, slot n_layer)
  bool kev_set[WCA_N_SITES][33] = {};   // which (site, layer) pairs the last encoder run recorded
  // ---- reference-precision ("split") mode, wca_set_precision: every f16 GEMM / attention operand x travels as the pair
  // hi = f16(x), lo = f16(x - hi) in ONE row [hi(K) | lo(K)], and every weight matrix as [W | W] ([N][2K], built once on the
  // device from the f16 weights, which are exact): A.W^T = [A_hi | A_lo].[W | W]^T is then a K-doubled call of the SAME GEMM
  // kernels with f16 x f16 products exact in the fp32 accumulator. Activation operand buffers are twice as wide.
  bool split = false;        // split mode: every stage runs on (hi, lo) operand pairs, the arena is wide and the K-doubled weight copies exist
  char* wslab2 = nullptr;    // the K-doubled weight copies (allocated while split is on)
  bool sw_dirty = true;      // a weight was (re)loaded since the copies were built
  struct SplitW {
    wca::half_t *conv1_w = nullptr, *conv2_w = nullptr, *kv_w = nullptr, *tok_emb = nullptr;
    wca::half_t *conv1_wlo = nullptr, *conv2_wlo = nullptr;   // [W_lo | 0] per tap group: the conv stem's extra term against [hi(C) | lo(C)] frames (inexact conv weights)
    int k1pad = 0;           // padded K of the split conv1 GEMM: windows of 3 frames x [hi(C) | lo(C)]
    std::vector<wca::LayerW> enc, dec;  // only the half_t* members are used
  } sw;
  // ---- collation over RCCL (wca_comm_init / wca_allgather_results): this engine's rank in a communicator of one rank per GPU
  ncclComm_t comm = nullptr;
  int comm_rank = 0, comm_world = 0;
  wca::GrowBuf coll_send, coll_recv;
  bool fuse_ln = false;      // LayerNorm in the epilogue of the residual GEMMs where the shape allows (wca_set_fuse_ln; never in split
                             // mode). OFF by default: the workgroups of a row panel wait for each other inside the launch, which needs
                             // the GPU to itself -- with a second process (or engine) on the device two such launches can hold each
                             // other's CUs and run into the bounded spin's time-out (measured: two bench ranks on one GPU)
  bool overlap = true;       // phase 2 on its own stream (false: everything on `stream`, for clean per-kernel profiles)
  bool dec_fused = true;     // few-row GEMM with LayerNorm prologue / KV append / split-K for M <= DEC_ROWS_MAX = 128 rows (wca_set_decode_mode)
  bool ev_valid = false;
  float stage_ms[8] = {};
};

namespace wca {

template <typename T>
T* carve(char*& cur, size_t count, size_t align = 256) {
  uintptr_t p = reinterpret_cast<uintptr_t>(cur);
  p = (p + align - 1) / align * align;
  T* r = reinterpret_cast<T*>(p);
  cur = reinterpret_cast<char*>(p + count * sizeof(T));
  return r;
}

// ---- weights that are not exact in f16 (fp32 checkpoints): the W_lo slab mirrors wslab byte for byte
inline bool use_wlo(const wca_engine* e) { return e->wslab_lo != nullptr && !e->wlo_bases.empty() && !e->allow_rounded; }
inline const half_t* wlo_of(const wca_engine* e, const half_t* w) {
  return reinterpret_cast<const half_t*>(e->wslab_lo + (reinterpret_cast<const char*>(w) - e->wslab));
}

// ---- engine.hip
int check_ready(wca_engine* e);   // finalized weights, the device current, the split mode's weight copies built
// stage per-utterance metadata into the next device slot: rows = {n_samples, n_tok, n_frames, dtwN}
int stage_meta(wca_engine* e, int B, const int32_t* a0, const int32_t* a1, const int32_t* a2, const int32_t* a3, int** dev_rows, hipStream_t s = nullptr);
int join_phase2(wca_engine* e);
int enter(wca_engine* e);         // what an entry point on `stream` starts with once its arguments are checked: null engine, the device current, join_phase2
void record(wca_engine* e, int i, hipStream_t s = nullptr);
int take_kv_slot(wca_engine* e);

// ---- engine_weights.hip
size_t layout_weights(wca_engine* e, char* base);
size_t layout_split_weights(wca_engine* e, char* base);
int ensure_split_weights(wca_engine* e);

// ---- engine_forward.hip
// One GEMM call: the kernel's descriptor, filled by name, plus what gemm() needs of a PAIR product: the plain matrix whose W_lo term it gets
// and the [W | W] copy it falls back to.
struct Gemm : GemmArgs {
  const half_t* w_plain = nullptr;   // pair products: the plain [N][k_plain] matrix (the key of wlo_bases)
  int k_plain = 0;
  const half_t* w_pair = nullptr;    // a_lo > 0: the [W | W] copy, [N][2 k_plain]
  const half_t* w_lo = nullptr;      // the W_lo operand where it is not the W_lo slab's image of w_plain (the conv stem's [W_lo | 0] copies, rows of k_plain)
};
// C [M][N] (rows ldc apart) = A [M][K] (lda) W [N][K]^T (ldw): what every call starts from; bias, gelu, out_mode, site, c_lo ... are set by name
inline Gemm flat(const half_t* A, int lda, const half_t* W, int ldw, void* C, int ldc, int M, int N, int K) {
  Gemm g{};
  g.A = A;
  g.lda = lda;
  g.W = W;
  g.ldw = ldw;
  g.C = C;
  g.ldc = ldc;
  g.M = M;
  g.N = N;
  g.K = K;
  return g;
}
// The product of a Linear in either precision mode. pair (split mode): the A buffer holds [hi(K) | lo(K)] rows (row stride 2 K) and the call is
// the candidate with a_lo = K on the plain W1 (each W K-tile staged once), which gemm() keeps exactly where plan_gemm takes it; elsewhere
// it becomes the K-doubled [A_hi | A_lo] [W | W]^T on W2 = the [W | W] copy. Otherwise the plain f16 product A W1^T.
inline Gemm flat(const half_t* A, bool pair, const half_t* W1, const half_t* W2, int K, void* C, int ldc, int M, int N) {
  Gemm g = flat(A, (pair ? 2 : 1) * K, W1, K, C, ldc, M, N, K);
  if (pair) {
    g.a_lo = K;
    g.w_plain = W1;
    g.k_plain = K;
    g.w_pair = W2;
  }
  return g;
}
hipError_t gemm(wca_engine* e, hipStream_t s, Gemm g);
int run_encoder(wca_engine* e, int B);
int run_cross_kv(wca_engine* e, int B, half_t* kvbuf = nullptr, bool skip_last_v = false);
int run_decoder(wca_engine* e, const int64_t* tokens_dev, int B, int n, float* cap, int Fpad, int Fcap, float* logits_out, hipStream_t s = nullptr,
                const half_t* kvbuf = nullptr, bool finish_last = false);
// kv_group > 1: row b attends to the cross-K/V of audio b / kv_group (wca_decode_group)
int run_decode_step(wca_engine* e, hipStream_t s, const half_t* kvbuf, const int* tokens, int B, StepPos pos, int T_max, bool want_logits,
                    int kv_group = 1);
int run_decode_prefill(wca_engine* e, hipStream_t s, const half_t* kvbuf, const int* tokens, int B, int n, int T_max, StepPos last, StepPos sot);
int mel_to_tm(wca_engine* e, const float* mel_dev, int batch);
int run_phase1(wca_engine* e, const float* mel_dev, const float* pcm_dev, int64_t pcm_stride, const int* n_samples_dev, int batch, int slot,
               bool skip_last_v = false);

// ---- engine_align.hip: the argument checks and the two halves of phase 2's post-processing that wca_align_batch_enqueue, the step-by-step
// entry points and the test hook wca_test_align_postproc (engine_test.hip) share
int check_medfilt(int width);
int check_aggregation(const wca_align_opts* o);
int validate_lengths(int B, int n_tok_max, const int32_t* n_tok, const int32_t* max_frames, int* Fmax_out);
int run_head_stats(wca_engine* e, hipStream_t s, HeadStatsArgs* h, const float* qk, int ld, bool input_is_weights, float* weights_out,
                   bool want_rowstats, const int* n_tok_dev, const int* n_frames_dev, int n_max, int Fmax, int LH, int B, int medfilt_width,
                   float qk_scale, float w_col, float w_row, float w_cov);
int run_select_aggregate_dtw(wca_engine* e, hipStream_t s, const HeadStatsArgs& h, const int* dtwN_dev, const wca_align_opts* o, int L_layers,
                             const int* open_dev = nullptr, bool path_scores = false, const int* win_lo_dev = nullptr,
                             const int* win_hi_dev = nullptr);   // win_*: row windows [B][n_tok_max] in DTW rows, checked by the caller
// the alignment-heads route (align_heads.hip) in place of the two calls above: the head list's host check, and the three passes with the
// ragged closed DTW behind them
int check_heads(const int32_t* heads_host, int n_heads, int LH);
int run_align_heads(wca_engine* e, hipStream_t s, const float* qk, int ld, const int* heads_dev, int S, const int* n_tok_dev,
                    const int* n_frames_dev, const int* dtwN_dev, int n_max, int Fmax, int LH, int B, const wca_align_opts* o);

// ---- engine_audio.hip
int check_pcm_lengths(const int32_t* n_samples_host, int batch, int64_t pcm_stride);
int run_logmel(wca_engine* e, const float* pcm_dev, int64_t pcm_stride, const int* n_samples_dev, int B, float* mel_out, bool want_tm);

}  // namespace wca
