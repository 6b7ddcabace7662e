// The logit filters of a decode step, written once for the kernels that choose tokens (decode.hip: decode_select, the greedy / sampling step;
// beam.hip: beam_topk, the per-row candidates of the beam step): upstream decoding.py's SuppressBlank, SuppressTokens and
// ApplyTimestampRules, restated, and the softmax statistics of the filtered logits that both turn into log-probabilities.
#pragma once
#include "kernels.h"
#include "wca_common.h"

namespace wca {

__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  float r = red[0];
  for (int i = 1; i < nw; ++i) r = fmaxf(r, red[i]);
  return r;
}
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  float r = red[0];
  for (int i = 1; i < nw; ++i) r += red[i];
  return r;
}

// ApplyTimestampRules bookkeeping over a row's sampled tokens seq[0 : ns] (decoding.py, restated), by one thread:
// hist = {last_was_ts, penult_was_ts, have_ts, ts_bound}
__device__ __forceinline__ void timestamp_history(const int* seq, int ns, int timestamp_begin, int* hist) {
  const bool last = ns >= 1 && seq[ns - 1] >= timestamp_begin;
  const bool pen = ns < 2 || seq[ns - 2] >= timestamp_begin;
  int last_ts = -1;
  for (int i = 0; i < ns; ++i)
    if (seq[i] >= timestamp_begin) last_ts = seq[i];
  hist[0] = last;
  hist[1] = pen;
  hist[2] = last_ts >= 0;
  // timestamps must not decrease; they may repeat only when closing a segment
  hist[3] = (last_ts >= 0) ? ((last && !pen) ? last_ts : last_ts + 1) : 0;
}

// Which tokens a row's filters remove at this step. `first`: the row's first sampled position.
struct RowFilter {
  const unsigned char* suppress_mask;
  const unsigned char* blank_mask;
  int eot, timestamp_begin, apply_timestamp_rules, max_initial_timestamp_index;
  bool first, last_ts, pen_ts, have_ts;
  int ts_bound;
  __device__ __forceinline__ RowFilter(const DecodeSelectArgs& a, bool first_, const int* hist)
      : suppress_mask(a.suppress_mask), blank_mask(a.blank_mask), eot(a.eot), timestamp_begin(a.timestamp_begin),
        apply_timestamp_rules(a.apply_timestamp_rules), max_initial_timestamp_index(a.max_initial_timestamp_index), first(first_),
        last_ts(hist[0]), pen_ts(hist[1]), have_ts(hist[2]), ts_bound(hist[3]) {}
  __device__ __forceinline__ bool dead(int v) const {
    if (suppress_mask[v]) return true;  // SuppressTokens (+ <|notimestamps|> under the timestamp rules)
    if (first && blank_mask != nullptr && blank_mask[v]) return true;  // SuppressBlank
    if (apply_timestamp_rules) {
      if (last_ts) {
        if (pen_ts) {
          if (v >= timestamp_begin) return true;  // has to be non-timestamp
        } else {
          if (v < eot) return true;  // cannot be normal text tokens
        }
      }
      if (have_ts && v >= timestamp_begin && v < ts_bound) return true;
      if (first) {
        if (v < timestamp_begin) return true;  // must start with a timestamp
        if (max_initial_timestamp_index >= 0 && v > timestamp_begin + max_initial_timestamp_index) return true;
      }
    }
    return false;
  }
};

// The softmax statistics of a row's filtered logits, by the whole workgroup (red: 16 floats of LDS): the maximum m_all, the sum s_final of
// exp(lg - m_all) over the tokens that stay, and text_dead -- "if sum of probability over timestamps is above any other token, sample
// timestamp": every text token is then removed too. log_softmax(filtered)[v] = (lg[v] - m_all) - logf(s_final).
__device__ __forceinline__ void filtered_softmax_stats(const float* lg, int V, const RowFilter& f, float* red, float* m_all_out, float* s_final_out,
                                                       bool* text_dead_out) {
  const int tid = threadIdx.x;
  // pass 1: maxima over the filtered logits (all / text part)
  float m_all = -INFINITY, m_text = -INFINITY;
  for (int v = tid; v < V; v += blockDim.x) {
    if (f.dead(v)) continue;
    const float x = lg[v];
    m_all = fmaxf(m_all, x);
    if (v < f.timestamp_begin) m_text = fmaxf(m_text, x);
  }
  m_all = block_max(m_all, red);
  m_text = block_max(m_text, red);
  // pass 2: partition sums relative to m_all
  float s_text = 0.f, s_ts = 0.f;
  for (int v = tid; v < V; v += blockDim.x) {
    if (f.dead(v)) continue;
    const float e = __expf(lg[v] - m_all);
    if (v < f.timestamp_begin) s_text += e; else s_ts += e;
  }
  s_text = block_sum(s_text, red);
  s_ts = block_sum(s_ts, red);
  // logsumexp(logprobs[ts:]) > max(logprobs[:ts])  <=>  log(s_ts) > m_text - m_all
  bool text_dead = false;
  if (f.apply_timestamp_rules && s_ts > 0.f && logf(s_ts) > m_text - m_all) text_dead = true;
  *m_all_out = m_all;
  *s_final_out = text_dead ? s_ts : s_text + s_ts;
  *text_dead_out = text_dead;
}

}  // namespace wca
