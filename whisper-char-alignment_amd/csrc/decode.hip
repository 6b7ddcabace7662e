// Greedy ASR pre-pass (reference call sites infer_ali.py:40,60-61 / probe_oracle.py:59-60: `whisper.decode(model,
// mels, DecodingOptions(language="en"))`, upstream openai-whisper decoding.py -- absent third-party dependency,
// restated from its published algorithm): the per-step device kernels of the autoregressive loop.
//   * embed_step:     x[b] = token_embedding[tokens[b][t]] + positional_embedding[t]
//   * kv_append:      self-attention K/V of the new position into the per-layer cache [B][T_max][d]
//   * prefill (embed_prefix, kv_scatter, gather_rows): the batched first forward over all n initial tokens of a prompted
//                     decode (upstream DecodingTask._main_loop, i == 0): embeddings of positions [0, n), their K/V into the
//                     cache, and the compact rows whose logits are needed (the last initial position, <|sot|>)
//   * decode_select:  the logit filters (SuppressBlank, SuppressTokens, ApplyTimestampRules), GreedyDecoder.update
//                     (argmax at temperature 0, log-softmax of the FILTERED logits for sum_logprobs, EOT latching)
//                     for one batch row per workgroup; integer / index work, bit-exact against the oracle on the same
//                     fp32 logits (tests/test_decode_gpu.py). Its sampling form (GreedyDecoder.update at temperature > 0:
//                     Gumbel-max over Philox4x32-10 noise, per-row temperature and seed) is tested token for token against a
//                     float64 restatement (tests/test_decode_sample_gpu.py).
#include "decode_filter.h"

namespace wca {

namespace {

// a row's own position (the rows of the per-row wca_decode sit at different ones), clamped to its n slots
__device__ __forceinline__ int clamp_pos(int t, int n) { return min(max(t, 0), n - 1); }

// x[b] = token_embedding[tokens[b][t]] + positional_embedding[t]
__device__ __forceinline__ void embed_step_row(const int* tokens, int T_max, int t, const half_t* tok_emb, const float* pos_emb, float* x, int d,
                                               int n_vocab) {
  const int b = blockIdx.x;
  long tok = tokens[(long)b * T_max + t];
  tok = (tok < 0 || tok >= n_vocab) ? 0 : tok;  // ids come from decode_select / the validated prompt; never read out of bounds
  const half_t* e = tok_emb + tok * d;
  const float* p = pos_emb + (long)t * d;
  float* o = x + (long)b * d;
  for (int c = threadIdx.x; c < d; c += blockDim.x) o[c] = (float)e[c] + p[c];
}

// qkv [B][3d] (q | k | v) -> kc / vc [B][T_max][d] at position t (8 halfs per thread)
__device__ __forceinline__ void kv_append_row(const half_t* qkv, half_t* kc, half_t* vc, int T_max, int t, int d) {
  const int b = blockIdx.x;
  const half8* k = reinterpret_cast<const half8*>(qkv + (long)b * 3 * d + d);
  const half8* v = reinterpret_cast<const half8*>(qkv + (long)b * 3 * d + 2 * d);
  half8* ko = reinterpret_cast<half8*>(kc + ((long)b * T_max + t) * d);
  half8* vo = reinterpret_cast<half8*>(vc + ((long)b * T_max + t) * d);
  for (int c = threadIdx.x; c < d / 8; c += blockDim.x) {
    ko[c] = k[c];
    vo[c] = v[c];
  }
}

// Each body above has two kernels that differ only in where the position comes from: every row at t, or row b at its own t_rows[b]. They stay
// two __global__ symbols with plain scalar / pointer arguments (a position struct as the argument, or one template over the two, changes the
// generated code), and they read the block index as the int the bodies use: the index types decide the address arithmetic.
__global__ __launch_bounds__(256) void embed_step_kernel(const int* __restrict__ tokens, int T_max, int t, const half_t* __restrict__ tok_emb,
                                                         const float* __restrict__ pos_emb, float* __restrict__ x, int d, int n_vocab) {
  embed_step_row(tokens, T_max, t, tok_emb, pos_emb, x, d, n_vocab);
}

__global__ __launch_bounds__(256) void kv_append_kernel(const half_t* __restrict__ qkv, half_t* __restrict__ kc, half_t* __restrict__ vc,
                                                        int T_max, int t, int d) {
  kv_append_row(qkv, kc, vc, T_max, t, d);
}

__global__ __launch_bounds__(256) void embed_step_rows_kernel(const int* __restrict__ tokens, int T_max, const int* __restrict__ t_rows,
                                                              const half_t* __restrict__ tok_emb, const float* __restrict__ pos_emb,
                                                              float* __restrict__ x, int d, int n_vocab) {
  const int b = blockIdx.x;
  embed_step_row(tokens, T_max, clamp_pos(t_rows[b], T_max), tok_emb, pos_emb, x, d, n_vocab);
}

__global__ __launch_bounds__(256) void kv_append_rows_kernel(const half_t* __restrict__ qkv, half_t* __restrict__ kc, half_t* __restrict__ vc,
                                                             int T_max, const int* __restrict__ t_rows, int d) {
  const int b = blockIdx.x;
  kv_append_row(qkv, kc, vc, T_max, clamp_pos(t_rows[b], T_max), d);
}

// x[b * n + i] = token_embedding[tokens[b][i]] + positional_embedding[i] for i < n (the prefill's rows; n <= n_text_ctx)
__global__ __launch_bounds__(256) void embed_prefix_kernel(const int* __restrict__ tokens, int T_max, int n, const half_t* __restrict__ tok_emb,
                                                           const float* __restrict__ pos_emb, float* __restrict__ x, int d, int n_vocab) {
  const int r = blockIdx.x;  // b * n + i
  const int b = r / n, i = r - b * n;
  long tok = tokens[(long)b * T_max + i];
  tok = (tok < 0 || tok >= n_vocab) ? 0 : tok;  // the initial tokens were validated on the host; never read out of bounds
  const half_t* e = tok_emb + tok * d;
  const float* p = pos_emb + (long)i * d;
  float* o = x + (long)r * d;
  for (int c = threadIdx.x; c < d; c += blockDim.x) o[c] = (float)e[c] + p[c];
}

// qkv [B * n][3d] (q | k | v) -> kc / vc [B][T_max][d] at positions [0, n) (8 halfs per thread)
__global__ __launch_bounds__(256) void kv_scatter_kernel(const half_t* __restrict__ qkv, half_t* __restrict__ kc, half_t* __restrict__ vc,
                                                         int n, int T_max, int d) {
  const int r = blockIdx.x;
  const int b = r / n, i = r - b * n;
  const half8* k = reinterpret_cast<const half8*>(qkv + (long)r * 3 * d + d);
  const half8* v = reinterpret_cast<const half8*>(qkv + (long)r * 3 * d + 2 * d);
  half8* ko = reinterpret_cast<half8*>(kc + ((long)b * T_max + i) * d);
  half8* vo = reinterpret_cast<half8*>(vc + ((long)b * T_max + i) * d);
  for (int c = threadIdx.x; c < d / 8; c += blockDim.x) {
    ko[c] = k[c];
    vo[c] = v[c];
  }
}

// out[j * B + b] = x[r] (f32 residual rows; b, j, B as the kernels below read them)
__device__ __forceinline__ void gather_row(const float* x, float* out, long r, int b, int j, int B, int d) {
  const float* src = x + r * d;
  float* o = out + ((long)j * B + b) * d;
  for (int c = threadIdx.x; c < d; c += blockDim.x) o[c] = src[c];
}

// r = b * n + p with p = p0 for j == 0, p1 for j == 1
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ x, float* __restrict__ out, int n, int p0, int p1, int d) {
  const int b = blockIdx.x, j = blockIdx.y, B = gridDim.x;
  gather_row(x, out, (long)b * n + (j == 0 ? p0 : p1), b, j, B, d);
}

// the same with the positions per batch row: p0_rows[b] (the row's last initial position), p1_rows[b] (its <|sot|>; nullable)
__global__ __launch_bounds__(256) void gather_rows_per_row_kernel(const float* __restrict__ x, float* __restrict__ out, int n,
                                                                  const int* __restrict__ p0_rows, const int* __restrict__ p1_rows, int d) {
  const int b = blockIdx.x, j = blockIdx.y, B = gridDim.x;
  const int p = clamp_pos(j == 0 ? p0_rows[b] : p1_rows[b], n);
  gather_row(x, out, (long)b * n + p, b, j, B, d);
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3"; the Random123 known answers are pinned in
// tests/test_decode_sample_ref.py through the float64 restatement this kernel is tested against): counter c[4], key (k0, k1) -> c[4].
__device__ __forceinline__ void philox4x32_10(unsigned c[4], unsigned k0, unsigned k1) {
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    c[0] = hi1 ^ c[1] ^ k0;
    c[1] = lo1;
    c[2] = hi0 ^ c[3] ^ k1;
    c[3] = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// Standard Gumbel noise of a 32-bit word: u = ((x >> 9) + 0.5) 2^-23 is exact in fp32 and strictly inside (0, 1) (23 bits, not 24: k + 0.5
// with a 24-bit k rounds up to u = 1 and G = +inf), so G = -log(-log(u)) is finite, in about [-2.82, 16.64]. Full-precision logf.
__device__ __forceinline__ float gumbel_of(unsigned x) {
  const float u = ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f;
  return -logf(-logf(u));
}

// One workgroup per batch row. cur_len = number of tokens the row holds (the new token is written at index cur_len).
// ROWS: cur_len, n_initial and the sample cap are per row (cur_len_rows / n_initial_rows / cap_rows); a row that has sampled its
// cap (or whose lengths are not a valid state) is a finished row: EOT where the row still has room, nothing added to sum_logprob,
// counted in n_done, which is indexed by the step (n_done_idx) because the rows' cur_len differ.
// SAMPLE (with ROWS): a row whose temperature_rows[b] is T > 0 draws its token from softmax(filtered logits / T) by Gumbel-max in pass 3:
// argmax_v (lg[v] * (1 / T) + G(v)) with G from Philox keyed by the row's seed and counted by (v >> 2, cur_len - n_initial), one Philox call
// per four consecutive tokens. The draw depends on (seed, sampled count, v, the row's logits) only: not on the batch row, nor on a summation
// order. The filters, text_dead and sum_logprob (the UNTEMPERED log-softmax at the drawn token) are the greedy form's; a row at T == 0 runs
// the greedy pass 3 itself. The instances without SAMPLE hold none of this.
template <bool ROWS, bool SAMPLE = false>
__global__ __launch_bounds__(1024) void decode_select_kernel(DecodeSelectArgs a) {
  __shared__ float red[16];
  __shared__ int red_i[16];
  __shared__ int hist[4];  // last_was_ts, penult_was_ts, have_ts, ts_bound
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const float* lg = a.logits + (long)b * a.ld;
  int* tok = a.tokens + (long)b * a.T_max;
  const int V = a.n_vocab;
  const int cur_len = ROWS ? a.cur_len_rows[b] : a.cur_len;
  const int n_initial = ROWS ? a.n_initial_rows[b] : a.n_initial;
  if (ROWS) {
    const bool valid = n_initial >= 1 && cur_len >= n_initial && cur_len < a.T_max;
    if (!valid || cur_len - n_initial >= a.cap_rows[b]) {  // (uniform over the workgroup)
      if (tid == 0) {
        if (cur_len >= 0 && cur_len < a.T_max) tok[cur_len] = a.eot;
        atomicAdd(a.n_done + a.n_done_idx, 1);
      }
      return;
    }
  }
  const bool first = (cur_len == n_initial);

  if (tid == 0) timestamp_history(tok + n_initial, cur_len - n_initial, a.timestamp_begin, hist);
  __syncthreads();
  const RowFilter filt(a, first, hist);
  auto dead = [&](int v) -> bool { return filt.dead(v); };
  float m_all, s_final;
  bool text_dead;
  filtered_softmax_stats(lg, V, filt, red, &m_all, &s_final, &text_dead);
  // pass 3: argmax (lowest index among equals) of the final filtered logits
  float best = -INFINITY;
  int best_i = 0x7fffffff;
  const float temperature = SAMPLE ? a.temperature_rows[b] : 0.f;  // (uniform over the workgroup)
  if (SAMPLE && temperature > 0.f) {
    // ... of the perturbed scores: a thread takes groups of four consecutive tokens, one Philox call each (the rows are not 16-byte
    // aligned: scalar loads)
    const float inv_T = 1.0f / temperature;
    const unsigned long long seed = a.seed_rows[b];
    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    for (int g = tid; g * 4 < V; g += blockDim.x) {
      unsigned c[4] = {(unsigned)g, (unsigned)(cur_len - n_initial), 0u, 0u};
      philox4x32_10(c, k0, k1);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int v = g * 4 + j;
        if (v >= V || dead(v) || (text_dead && v < a.timestamp_begin)) continue;
        const float x = lg[v] * inv_T + gumbel_of(c[j]);
        if (x > best) {
          best = x;
          best_i = v;
        }
      }
    }
  } else {
    for (int v = tid; v < V; v += blockDim.x) {
      if (dead(v) || (text_dead && v < a.timestamp_begin)) continue;
      const float x = lg[v];
      if (x > best) {
        best = x;
        best_i = v;
      }
    }
  }
  {
    // wave then block arg-reduction
    for (int off = 32; off >= 1; off >>= 1) {
      const float ob = __shfl_xor(best, off);
      const int oi = __shfl_xor(best_i, off);
      if (ob > best || (ob == best && oi < best_i)) {
        best = ob;
        best_i = oi;
      }
    }
    const int w = tid >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((tid & 63) == 0) {
      red[w] = best;
      red_i[w] = best_i;
    }
    __syncthreads();
    best = red[0];
    best_i = red_i[0];
    for (int i = 1; i < nw; ++i)
      if (red[i] > best || (red[i] == best && red_i[i] < best_i)) {
        best = red[i];
        best_i = red_i[i];
      }
  }
  if (tid == 0) {
    const int prev = tok[cur_len - 1];
    // a draw reduced on the perturbed score: the token's own logit (nothing survived the filters: -inf, as the greedy `best`)
    if (SAMPLE && temperature > 0.f) best = best_i == 0x7fffffff ? -INFINITY : lg[best_i];
    const float logprob = (best - m_all) - logf(s_final);  // log_softmax of the filtered logits at the chosen token
    int next = best_i;
    if (best_i == 0x7fffffff) next = a.eot;  // every token filtered out (cannot happen with the stock filters)
    if (prev == a.eot) next = a.eot;         // finished rows keep emitting EOT and stop accumulating
    else a.sum_logprob[b] += logprob;
    tok[cur_len] = next;
    if (next == a.eot) atomicAdd(a.n_done + (ROWS ? a.n_done_idx : cur_len), 1);
  }
}


// probs_at_sot[no_speech] of DecodingTask._main_loop (i == 0): softmax over the vocabulary of the logits at the <|sot|>
// position, probability of the <|nospeech|> token; one workgroup per row.
__global__ __launch_bounds__(1024) void token_prob_kernel(const float* __restrict__ logits, int ld, int n_vocab, int token,
                                                          float* __restrict__ out) {
  __shared__ float red[16];
  const float* lg = logits + (long)blockIdx.x * ld;
  float m = -INFINITY;
  for (int v = threadIdx.x; v < n_vocab; v += blockDim.x) m = fmaxf(m, lg[v]);
  m = block_max(m, red);
  float s = 0.f;
  for (int v = threadIdx.x; v < n_vocab; v += blockDim.x) s += __expf(lg[v] - m);
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = __expf(lg[token] - m) / s;
}

}  // namespace

hipError_t launch_token_prob(const float* logits, int ld, int n_vocab, int token, float* out, int B, hipStream_t s) {
  if (token < 0 || token >= n_vocab) return hipErrorInvalidValue;
  hipLaunchKernelGGL(token_prob_kernel, dim3(B), dim3(1024), 0, s, logits, ld, n_vocab, token, out);
  return hipGetLastError();
}

hipError_t launch_embed_step(const int* tokens, int T_max, StepPos pos, const half_t* tok_emb, const float* pos_emb, float* x, int B, int d,
                             int n_vocab, hipStream_t s) {
  if (pos.rows && T_max < 1) return hipErrorInvalidValue;
  if (pos.rows) hipLaunchKernelGGL(embed_step_rows_kernel, dim3(B), dim3(256), 0, s, tokens, T_max, pos.rows, tok_emb, pos_emb, x, d, n_vocab);
  else hipLaunchKernelGGL(embed_step_kernel, dim3(B), dim3(256), 0, s, tokens, T_max, pos.t, tok_emb, pos_emb, x, d, n_vocab);
  return hipGetLastError();
}

hipError_t launch_kv_append(const half_t* qkv, half_t* kc, half_t* vc, int B, int T_max, StepPos pos, int d, hipStream_t s) {
  if ((d & 7) != 0 || (pos.rows && T_max < 1)) return hipErrorInvalidValue;
  if (pos.rows) hipLaunchKernelGGL(kv_append_rows_kernel, dim3(B), dim3(256), 0, s, qkv, kc, vc, T_max, pos.rows, d);
  else hipLaunchKernelGGL(kv_append_kernel, dim3(B), dim3(256), 0, s, qkv, kc, vc, T_max, pos.t, d);
  return hipGetLastError();
}

hipError_t launch_embed_prefix(const int* tokens, int T_max, int n, const half_t* tok_emb, const float* pos_emb, float* x, int B, int d,
                               int n_vocab, hipStream_t s) {
  if (n < 1 || n > T_max) return hipErrorInvalidValue;
  hipLaunchKernelGGL(embed_prefix_kernel, dim3(B * n), dim3(256), 0, s, tokens, T_max, n, tok_emb, pos_emb, x, d, n_vocab);
  return hipGetLastError();
}

hipError_t launch_kv_scatter(const half_t* qkv, half_t* kc, half_t* vc, int B, int n, int T_max, int d, hipStream_t s) {
  if ((d & 7) != 0 || n < 1 || n > T_max) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kv_scatter_kernel, dim3(B * n), dim3(256), 0, s, qkv, kc, vc, n, T_max, d);
  return hipGetLastError();
}

hipError_t launch_gather_rows(const float* x, float* out, int B, int n, StepPos p0, StepPos p1, int d, hipStream_t s) {
  if (p0.rows) {
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gather_rows_per_row_kernel, dim3(B, p1.rows ? 2 : 1), dim3(256), 0, s, x, out, n, p0.rows, p1.rows, d);
  } else {
    if (p0.t < 0 || p0.t >= n || p1.t >= n) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(B, p1.t >= 0 ? 2 : 1), dim3(256), 0, s, x, out, n, p0.t, p1.t, d);
  }
  return hipGetLastError();
}

hipError_t launch_decode_select(const DecodeSelectArgs& a, int B, hipStream_t s) {
  if (a.cur_len_rows) {
    if (!a.n_initial_rows || !a.cap_rows || a.n_done_idx < 0 || a.T_max < 2) return hipErrorInvalidValue;
    if (a.temperature_rows) {
      if (!a.seed_rows) return hipErrorInvalidValue;
      hipLaunchKernelGGL((decode_select_kernel<true, true>), dim3(B), dim3(1024), 0, s, a);
    } else {
      hipLaunchKernelGGL(decode_select_kernel<true>, dim3(B), dim3(1024), 0, s, a);
    }
  } else {
    if (a.temperature_rows || a.cur_len < 1 || a.cur_len >= a.T_max || a.n_initial < 1 || a.cur_len < a.n_initial) return hipErrorInvalidValue;
    hipLaunchKernelGGL(decode_select_kernel<false>, dim3(B), dim3(1024), 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace wca
