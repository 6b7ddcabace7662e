// Which kernel a GEMM gets, and with what grid: plan_gemm, the host arithmetic of launch_gemm (gemm.hip) without a HIP call, so that the
// callers that depend on the outcome ask instead of predicting it, and a CPU test can pin it (wca_test_gemm_plan). plan_dec_gemm is the same for
// the decoder's choice between the few-row kernel and the separate launches (dec_gemm; wca_test_dec_gemm_plan).
#include <algorithm>

#include "kernels.h"

namespace wca {

namespace {

constexpr int BK = 64;
constexpr size_t BUF_RANGE = 0x7fffffffull;   // what a buffer descriptor addresses

GemmPlan refuse(const char* why) {
  GemmPlan p{};
  p.refused = why;
  return p;
}

}  // namespace

GemmPlan plan_gemm(const GemmArgs& a, int n_cu) {
  GemmPlan p{};
  p.kernel = GemmKernel::None;
  p.grid_y = 1;
  p.splitk = 1;
  p.supertile = a.supertile;
  p.a_bytes = a.a_bytes;
  p.w_bytes = a.w_bytes;
  if (a.M <= 0 || a.N <= 0) return p;
  if (a.K <= 0 || (a.K % BK) != 0) return refuse("K is not a positive multiple of 64");
  if ((a.lda % 8) != 0 || (a.ldw % 8) != 0) return refuse("lda / ldw is not a multiple of 8");   // 16-byte LDS-DMA source chunks
  if (a.out_mode == 4 && (a.c_lo <= 0 || (a.c_lo & 7))) return refuse("out_mode 4 without a c_lo that is a multiple of 8");
  // (accumulating modes take the extra term as a second accumulating launch; with an addend the pair product is the K-doubled call)
  if (a.addend != nullptr && (a.out_mode == 2 || a.out_mode == 3 || a.a_lo > 0)) return refuse("addend with an accumulating out_mode or with pair operands");
  const bool gelu_ok = a.out_mode == 0 || a.out_mode == 1 || a.out_mode == 4;   // the out-modes that exist with GELU; 2 and 3 without
  // M <= 64 (greedy-decode steps): weight-streaming skinny kernel; GEMM_TILE_SKINNY forces it, 128 etc. bypass it
  if ((a.force_tile == GEMM_TILE_SKINNY || a.force_tile == GEMM_TILE_AUTO) && a.M <= 64 && (a.K % 512) == 0 && a.a_rows_per_batch == 0 && a.pos == nullptr &&
      a.addend == nullptr && a.out_mode != 4 && a.a_lo <= 0) {
    if (!(gelu_ok || (a.out_mode == 2 && !a.gelu))) return refuse("the skinny kernel has out_mode 0 / 1, and 2 without GELU");
    p.kernel = GemmKernel::Skinny;
    p.grid_x = (unsigned)((a.N + 15) / 16);
    p.block = 256;
    return p;
  }
  if (a.force_tile == GEMM_TILE_SKINNY) return refuse("not a shape of the skinny kernel");
  const long tiles256 = (long)((a.M + 255) / 256) * ((a.N + 255) / 256);
  const bool big = a.force_tile == GEMM_TILE_256 || a.force_tile == GEMM_TILE_PERSIST || a.force_tile == GEMM_TILE_PERSIST_ONE ||
                   (a.force_tile == GEMM_TILE_AUTO && tiles256 >= GEMM_MIN_TILES_256);
  const bool splitw = a.a_lo > 0;
  if (splitw) {
    // pair operands against the plain W: the persistent kernel only, on a flat A, whole pairs of K tiles (the W ring's slot parity carries
    // over a tile boundary), operands of K-doubled rows inside a buffer descriptor's range
    if (a.force_tile == GEMM_TILE_128 || a.force_tile == GEMM_TILE_256 || a.a_rows_per_batch != 0 || a.K < 128 || (a.K % 128) != 0 || (a.a_lo & 7) != 0)
      return refuse("pair operands with a forced tile kernel or a batch-strided A, or K is not a multiple of 128 (a_lo of 8)");
    if (!gelu_ok && a.out_mode != 2) return refuse("pair operands: out_mode 0 / 1 / 2 / 4");
    if (tiles256 < GEMM_MIN_TILES_256) return refuse("pair operands: too few tiles for the persistent kernel");
    if (((size_t)(a.M - 1) * a.lda + 2 * (size_t)a.K) * sizeof(half_t) >= BUF_RANGE || ((size_t)(a.N - 1) * a.K + a.K) * sizeof(half_t) >= BUF_RANGE)
      return refuse("pair operands: beyond a buffer descriptor's range");
  }
  const size_t a_need = ((size_t)(a.M - 1) * a.lda + (splitw ? (size_t)a.a_lo : 0) + a.K) * sizeof(half_t), w_need = ((size_t)(a.N - 1) * a.ldw + a.K) * sizeof(half_t);
  const bool can_buf = a.a_rows_per_batch == 0 && a_need < BUF_RANGE && w_need < BUF_RANGE;
  if (p.a_bytes == 0) p.a_bytes = (unsigned)a_need;
  if (p.w_bytes == 0) p.w_bytes = (unsigned)w_need;
  if (a.cu_limit > 0 && a.cu_limit < n_cu) n_cu = a.cu_limit;   // the tests' cap on the persistent grid: that many workgroups walk the tiles
  // (the pre-activation addend lives in the generic epilogue only: an addend launch takes the two-barrier 256 x 256 kernel)
  const bool persistent = big && can_buf && a.force_tile != GEMM_TILE_256 && a.addend == nullptr;
  const int site = p.site_used = a.site >= 1 && a.site <= 4 ? a.site : 0;
  if (big) {
    p.grid_x = (unsigned)tiles256;
    p.block = 512;
    p.lds = GEMM_LDS_256;
    p.kernel = GemmKernel::Tile256;
    if (persistent) {
      p.lds = GEMM_LDS_256P;
      // one workgroup per CU walks tiles blockIdx.x, + gridDim.x, ... (the ring-slot parity carries over a tile boundary only for an
      // even number of K tiles)
      const int nk = (splitw ? 2 : 1) * (a.K / BK);
      if (a.force_tile != GEMM_TILE_PERSIST_ONE && nk >= 2 && (nk & 1) == 0 && tiles256 > n_cu) p.grid_x = (unsigned)n_cu;
      // (K <= 2048 since round 3: the K-doubled QKV / fc1 of the split mode measure -5 % / -3 % with the supertile order, same-box A/B)
      if (p.supertile <= 0) p.supertile = ((splitw ? 2 : 1) * a.K <= 2048 && (a.N + 255) / 256 <= 32) ? 8 : 1;
      p.kernel = GemmKernel::Persist256;
      if (splitw) {
        // three A slots + one W slot (round 5), sites 1-4; the switch gemm_ring = 1 keeps round 4's two-slot rings (A/B, tests), sites 1 and 4
        const bool ring2 = debug_switch(DBG_GEMM_RING) == 1;
        p.kernel = ring2 ? GemmKernel::Persist256Pair2 : GemmKernel::Persist256Pair3;
        p.site_used = ring2 ? (site == 4 ? 4 : 1) : (site == 0 ? 1 : site);
      }
    }
  } else {
    const int tiles128 = ((a.N + 127) / 128) * ((a.M + 127) / 128);
    p.grid_x = (unsigned)tiles128;
    p.block = 256;
    p.lds = GEMM_LDS_128;
    p.kernel = GemmKernel::Tile128;
    // few tiles and a long K (fc2 of a one- or two-utterance batch: 96 tiles x 64 K tiles): split K over up to 4 workgroups
    // per tile; partial tiles go to the caller's workspace and a second kernel adds them in order (deterministic)
    if (a.out_mode == 2 && !a.gelu && a.sk_part != nullptr && a.pos == nullptr && a.c_rows_per_batch == 0 && (a.N % 4) == 0 && (a.ldc % 4) == 0 &&
        tiles128 <= n_cu / 2 && a.K >= 2048) {
      for (int sk = 4; sk >= 2 && p.splitk == 1; --sk)
        if (a.K % (sk * BK) == 0 && (size_t)sk * a.M * a.N * sizeof(float) <= a.sk_bytes) p.splitk = sk;
    }
    p.grid_y = (unsigned)p.splitk;
  }
  if (a.out_mode == 3) {
    // residual + LayerNorm epilogue: persistent 256 x 256 kernel only, N whole tiles across the row, an even number of K tiles. Every workgroup of
    // a 256-row panel must be resident: grid = CUs rounded down to a multiple of 8, one workgroup per CU, and a round of the n_cu / 8 workgroups of
    // an XCD label holds at least one whole panel (N / 256 tiles). The caller takes out_mode 2 + launch_layernorm_f16 where this is refused
    if (a.N % 256 != 0 || a.N > 2048 || a.K % 128 != 0 || tiles256 < GEMM_MIN_TILES_256 || (n_cu >> 3) < a.N / 256)
      return refuse("out_mode 3: N is no multiple of 256 up to 2048, K no multiple of 128, too few tiles or too few CUs");
    if (a.gelu || !persistent || a.force_tile == GEMM_TILE_PERSIST_ONE || a.pos != nullptr || a.c_rows_per_batch != 0 || !a.ln_gamma || !a.ln_beta ||
        !a.ln_out || !a.ln_stats || !a.ln_cnt || (a.ldc & 3) || (a.ln_ld & 7))
      return refuse("out_mode 3: not the persistent kernel, GELU / pos / batch-strided C, or a LayerNorm argument is missing");
    p.kernel = GemmKernel::Persist256LN;
    p.lds = GEMM_LDS_256P_LN;
    p.grid_x = (unsigned)(n_cu & ~7);   // round-based panel walk: 8 XCD labels x n_cu / 8 workgroups (idle ones exit)
    p.site_used = a.site == 4 ? 4 : 1;
  } else if (!gelu_ok && !(a.out_mode == 2 && !a.gelu)) {
    return refuse("out_mode is not 0 - 4, or out_mode 2 with GELU");
  }
  return p;
}

// few-row GEMM, split-K (K > 1024: fc2; every K of the 1280-wide model): up to DEC_ROWS_MAX rows, N = n_text_state columns
DecSkCapacity dec_sk_capacity(int n_text_state) {
  const int s_max = std::max(std::max(gemm_rows_pick_splitk(n_text_state), gemm_rows_pick_splitk(4 * n_text_state)), 1);
  DecSkCapacity c{};
  c.tiles = (size_t)(DEC_ROWS_MAX / 64) * (((size_t)n_text_state + 15) / 16);
  c.floats = c.tiles * s_max * 64 * 16;
  return c;
}

DecGemmPlan plan_dec_gemm(int M, int N, int K, bool layernorm_a, bool kv_append, const DecSkCapacity& cap) {
  DecGemmPlan p{};
  const int sk = gemm_rows_pick_splitk(K);
  const bool fits = sk <= 1 || (!kv_append && (size_t)((M + 63) / 64) * ((N + 15) / 16) <= cap.tiles &&
                                gemm_rows_workspace_bytes(M, N, sk) <= cap.floats * sizeof(float));
  if (!(M <= DEC_ROWS_MAX && gemm_rows_supported(M, N, K, layernorm_a) && fits)) return p;
  p.few_row = true;
  p.splitk = sk;
  // the grid and the LDS that launch_gemm_rows (gemm_rows.hip) gives this split with groups = 0: 64-row blocks, 16-column groups, an f16 image
  // of 64 rows of K / splitk + 8 halfs, the four quarter accumulators of four m-tiles, one flag word
  const int NG = (N + 15) / 16;
  p.groups = sk > 1 ? 1 : (NG + 255) / 256;
  p.grid_x = (unsigned)(((NG + p.groups - 1) / p.groups) * sk);
  p.grid_y = (unsigned)((M + 63) / 64);
  p.lds = (size_t)64 * (K / sk + 8) * sizeof(half_t) + 4 * 4 * 4 * 64 * sizeof(float) + 16;
  p.ws_bytes = gemm_rows_workspace_bytes(M, N, sk);
  return p;
}

}  // namespace wca
