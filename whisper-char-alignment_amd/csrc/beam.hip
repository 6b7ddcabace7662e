// Beam search on the device (wca_decode_group; upstream openai-whisper decoding.py BeamSearchDecoder.update -- absent third-party
// dependency, restated from its published algorithm): decoder row r = b * G + g is beam g of audio b.
//   * beam_topk:   per row, the filters of decode_select (decode_filter.h), the fp32 log-softmax of the filtered logits and its top G + 1
//                  entries -- what upstream's logprobs[idx].topk(beam_size + 1) offers of a beam
//   * beam_merge:  per audio, the G (G + 1) candidates ordered by accumulated score; the ones that end in eot join the audio's finished
//                  list, the best G others become the next beams, whose token rows are gathered from their source rows
//   * kv_reorder:  the self-attention cache rows follow the beams that continue them (upstream's rearrange_kv_cache), between the two
//                  halves of the cache buffer; the same kernel broadcasts an audio's prefill to its G rows
// Index and comparison work on given fp32 logits: tokens, sources and finished lists are tested for identity against a float64
// restatement (tests/beam_ref.py), the scores to the fp32 log-sum-exp order.
#include "decode_filter.h"

namespace wca {

namespace {

constexpr int CAND_MAX = BEAM_GROUP_MAX * (BEAM_GROUP_MAX + 1);

__global__ __launch_bounds__(1024) void beam_topk_kernel(BeamTopkArgs a) {
  __shared__ float red[16];
  __shared__ int red_i[16];
  __shared__ int hist[4];
  const DecodeSelectArgs& s = a.sel;
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const float* lg = s.logits + (long)b * s.ld;
  const int* tok = s.tokens + (long)b * s.T_max;
  const int V = s.n_vocab, K = a.K;
  int* out_tok = a.cand_tok + (long)b * K;
  float* out_lp = a.cand_lp + (long)b * K;
  const int cur_len = s.cur_len_rows[b], n_initial = s.n_initial_rows[b];
  const bool valid = n_initial >= 1 && cur_len >= n_initial && cur_len < s.T_max;
  if (!valid || cur_len - n_initial >= s.cap_rows[b]) {  // (uniform over the workgroup) a row past its budget offers nothing
    if (tid < K) {
      out_tok[tid] = -1;
      out_lp[tid] = -INFINITY;
    }
    return;
  }
  if (tid == 0) timestamp_history(tok + n_initial, cur_len - n_initial, s.timestamp_begin, hist);
  __syncthreads();
  const RowFilter filt(s, cur_len == n_initial, hist);
  float m_all, s_final;
  bool text_dead;
  filtered_softmax_stats(lg, V, filt, red, &m_all, &s_final, &text_dead);
  const float log_s = logf(s_final);
  // K rounds of argmax over what the rounds before left: a token is still in play when it comes after the last pick in the order
  // (logit descending, token ascending)
  float prev = INFINITY;
  int prev_i = -1;
  for (int k = 0; k < K; ++k) {
    float best = -INFINITY;
    int best_i = 0x7fffffff;
    for (int v = tid; v < V; v += blockDim.x) {
      if (filt.dead(v) || (text_dead && v < s.timestamp_begin)) continue;
      const float x = lg[v];
      if (!(x < prev || (x == prev && v > prev_i))) continue;
      if (x > best) {
        best = x;
        best_i = v;
      }
    }
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
    const bool none = best_i == 0x7fffffff;  // fewer than K tokens survive the filters (uniform)
    if (tid == 0) {
      out_tok[k] = none ? -1 : best_i;
      out_lp[k] = none ? -INFINITY : (best - m_all) - log_s;
    }
    if (none) {
      if (tid > k && tid < K) {
        out_tok[tid] = -1;
        out_lp[tid] = -INFINITY;
      }
      break;
    }
    prev = best;
    prev_i = best_i;
  }
}

// candidate x comes before candidate y: score descending, source beam ascending, token ascending (then the slot, so that the order is total)
__device__ __forceinline__ bool cand_before(float sx, int jx, int tx, int ix, float sy, int jy, int ty, int iy) {
  if (sx != sy) return sx > sy;
  if (jx != jy) return jx < jy;
  if (tx != ty) return tx < ty;
  return ix < iy;
}

__global__ __launch_bounds__(64) void beam_merge_kernel(BeamMergeArgs a) {
  __shared__ float sc[CAND_MAX];
  __shared__ int tk[CAND_MAX];
  __shared__ short order[CAND_MAX];
  __shared__ int new_src[BEAM_GROUP_MAX], new_tok[BEAM_GROUP_MAX];
  __shared__ float new_sum[BEAM_GROUP_MAX];
  __shared__ int fin_cand[BEAM_GROUP_MAX], fin_slot[BEAM_GROUP_MAX];
  __shared__ int n_fin;
  const int b = blockIdx.x, lane = threadIdx.x;
  const int G = a.G, K = a.K, N = G * K, T = a.T_max, r0 = b * G;
  const int cur_len = a.cur_len_rows[r0], n_initial = a.n_initial_rows[r0];
  const bool valid = n_initial >= 1 && cur_len >= n_initial && cur_len < T;
  if (!valid || cur_len - n_initial >= a.cap_rows[r0]) {  // past its budget: the rows move to the other buffer as they are
    for (int g = 0; g < G; ++g) {
      for (int t = lane; t < T; t += 64) a.tok_out[(long)(r0 + g) * T + t] = a.tok_in[(long)(r0 + g) * T + t];
      if (lane == 0) {
        a.src[r0 + g] = r0 + g;
        a.trace[2 * (r0 + g)] = r0 + g;
        a.trace[2 * (r0 + g) + 1] = -1;
      }
    }
    if (lane == 0) atomicAdd(a.n_done, 1);
    return;
  }
  for (int i = lane; i < N; i += 64) {
    const int j = i / K;
    int t = a.cand_tok[(long)r0 * K + i];
    if (a.first && j != 0) t = -1;
    sc[i] = t >= 0 ? a.sum_logprob[r0 + j] + a.cand_lp[(long)r0 * K + i] : -INFINITY;
    tk[i] = t;
  }
  __syncthreads();
  for (int i = lane; i < N; i += 64) {
    int rank = 0;
    for (int o = 0; o < N; ++o)
      if (o != i && cand_before(sc[o], o / K, tk[o], o, sc[i], i / K, tk[i], i)) ++rank;
    order[rank] = (short)i;
  }
  __syncthreads();
  if (lane == 0) {
    int saved = 0, nf = 0;
    for (int p = 0; p < N && saved < G; ++p) {
      const int i = order[p];
      if (tk[i] < 0) continue;
      if (tk[i] == a.eot) {
        fin_cand[nf++] = i;  // (a beam offers eot at most once: nf <= G)
      } else {
        new_src[saved] = i / K;
        new_tok[saved] = tk[i];
        new_sum[saved] = sc[i];
        ++saved;
      }
    }
    for (; saved < G; ++saved) {  // fewer than G candidates survived every beam's filters: dead beams that can never be chosen again
      new_src[saved] = saved ? new_src[0] : 0;
      new_tok[saved] = a.eot;
      new_sum[saved] = -INFINITY;
    }
    int n = a.fin_n[b];
    for (int q = 0; q < nf; ++q) {
      fin_slot[q] = -1;
      if (n >= a.max_candidates) continue;
      fin_slot[q] = n;
      a.fin_len[(long)b * a.max_candidates + n] = cur_len;
      a.fin_sum[(long)b * a.max_candidates + n] = sc[fin_cand[q]];
      ++n;
    }
    a.fin_n[b] = n;
    n_fin = nf;
    if (n >= a.max_candidates) atomicAdd(a.n_done, 1);
  }
  __syncthreads();
  for (int g = 0; g < G; ++g) {
    const int* in = a.tok_in + (long)(r0 + new_src[g]) * T;
    int* out = a.tok_out + (long)(r0 + g) * T;
    for (int t = lane; t < cur_len; t += 64) out[t] = in[t];
    if (lane == 0) {
      out[cur_len] = new_tok[g];
      a.sum_logprob[r0 + g] = new_sum[g];
      a.src[r0 + g] = r0 + new_src[g];
      a.trace[2 * (r0 + g)] = r0 + new_src[g];
      a.trace[2 * (r0 + g) + 1] = new_tok[g];
    }
  }
  for (int q = 0; q < n_fin; ++q) {
    if (fin_slot[q] < 0) continue;
    const int* in = a.tok_in + (long)(r0 + fin_cand[q] / K) * T;
    int* out = a.fin_tok + ((long)b * a.max_candidates + fin_slot[q]) * T;
    for (int t = lane; t < T; t += 64) out[t] = t < cur_len ? in[t] : a.eot;
  }
}

__global__ __launch_bounds__(256) void kv_reorder_kernel(const half_t* __restrict__ src, half_t* __restrict__ dst, int rows_src, int rows_dst,
                                                         int T_max, int d, const int* __restrict__ src_idx, int div,
                                                         const int* __restrict__ n_keep) {
  const int r = blockIdx.x, p = blockIdx.y;
  int s = src_idx ? src_idx[r] : r / div;
  s = min(max(s, 0), rows_src - 1);
  const int n = min(max(n_keep[r], 0), T_max);
  const half8* in = reinterpret_cast<const half8*>(src + ((long)p * rows_src + s) * T_max * d);
  half8* out = reinterpret_cast<half8*>(dst + ((long)p * rows_dst + r) * T_max * d);
  const long cnt = (long)n * (d / 8);
  for (long i = (long)blockIdx.z * blockDim.x + threadIdx.x; i < cnt; i += (long)gridDim.z * blockDim.x) out[i] = in[i];
}

}  // namespace

hipError_t launch_beam_topk(const BeamTopkArgs& a, int R, hipStream_t s) {
  const DecodeSelectArgs& q = a.sel;
  if (R < 1 || a.K < 2 || a.K > BEAM_GROUP_MAX + 1 || !q.cur_len_rows || !q.n_initial_rows || !q.cap_rows || q.T_max < 2 || q.n_vocab < 1 ||
      !a.cand_tok || !a.cand_lp)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(beam_topk_kernel, dim3(R), dim3(1024), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_beam_merge(const BeamMergeArgs& a, int B, hipStream_t s) {
  if (B < 1 || a.G < 1 || a.G > BEAM_GROUP_MAX || a.K != a.G + 1 || a.T_max < 2 || a.max_candidates < 1 || a.tok_in == a.tok_out)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(beam_merge_kernel, dim3(B), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_kv_reorder(const half_t* src, half_t* dst, int n_planes, int rows_src, int rows_dst, int T_max, int d, const int* src_idx,
                             int div, const int* n_keep, hipStream_t s) {
  if (n_planes < 1 || rows_src < 1 || rows_dst < 1 || T_max < 1 || d < 8 || (d & 7) != 0 || (!src_idx && div < 1) || !n_keep || src == dst)
    return hipErrorInvalidValue;
  const long per_row = (long)T_max * (d / 8);
  const int z = (int)std::min<long>(8, (per_row + 255) / 256);
  hipLaunchKernelGGL(kv_reorder_kernel, dim3(rows_dst, n_planes, z), dim3(256), 0, s, src, dst, rows_src, rows_dst, T_max, d, src_idx, div, n_keep);
  return hipGetLastError();
}

}  // namespace wca
