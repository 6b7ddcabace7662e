// libwca.so engine, weights: the slab layout, upload (f16 at rest, the W_lo remainders of inexact fp32 tensors) and the K-doubled
// [W | W] copies of the split mode.
#include "engine_internal.h"

using namespace wca;

namespace wca {

// ---- weight slab layout (two passes: size, then carve)
size_t layout_weights(wca_engine* e, char* base) {
  const wca_model_dims& D = e->dims;
  const int d = D.n_audio_state, dt = D.n_text_state;
  char* cur = base;
  e->k1pad = (int)align_up((size_t)3 * D.n_mels, 64);
  e->conv1_w = carve<half_t>(cur, (size_t)d * e->k1pad);
  e->conv1_b = carve<float>(cur, d);
  e->conv2_w = carve<half_t>(cur, (size_t)d * 3 * d);
  e->conv2_b = carve<float>(cur, d);
  e->enc_pos = carve<float>(cur, (size_t)N_CTX * d);
  e->lnpost_g = carve<float>(cur, d);
  e->lnpost_b = carve<float>(cur, d);
  e->enc.resize(D.n_audio_layer);
  for (auto& l : e->enc) {
    l.ln1_g = carve<float>(cur, d);
    l.ln1_b = carve<float>(cur, d);
    l.qkv_w = carve<half_t>(cur, (size_t)3 * d * d);
    l.qkv_b = carve<float>(cur, 3 * d);
    l.out_w = carve<half_t>(cur, (size_t)d * d);
    l.out_b = carve<float>(cur, d);
    l.ln2_g = carve<float>(cur, d);
    l.ln2_b = carve<float>(cur, d);
    l.fc1_w = carve<half_t>(cur, (size_t)4 * d * d);
    l.fc1_b = carve<float>(cur, 4 * d);
    l.fc2_w = carve<half_t>(cur, (size_t)4 * d * d);
    l.fc2_b = carve<float>(cur, d);
    l.lnc_g = l.lnc_b = nullptr;
    l.cq_w = l.co_w = nullptr;
    l.cq_b = l.co_b = nullptr;
  }
  e->tok_emb = carve<half_t>(cur, (size_t)D.n_vocab * dt);
  e->dec_pos = carve<float>(cur, (size_t)D.n_text_ctx * dt);
  e->lnf_g = carve<float>(cur, dt);
  e->lnf_b = carve<float>(cur, dt);
  e->kv_w = carve<half_t>(cur, (size_t)D.n_text_layer * 2 * dt * d);
  e->kv_b = carve<float>(cur, (size_t)D.n_text_layer * 2 * dt);
  e->dec.resize(D.n_text_layer);
  for (auto& l : e->dec) {
    l.ln1_g = carve<float>(cur, dt);
    l.ln1_b = carve<float>(cur, dt);
    l.qkv_w = carve<half_t>(cur, (size_t)3 * dt * dt);
    l.qkv_b = carve<float>(cur, 3 * dt);
    l.out_w = carve<half_t>(cur, (size_t)dt * dt);
    l.out_b = carve<float>(cur, dt);
    l.lnc_g = carve<float>(cur, dt);
    l.lnc_b = carve<float>(cur, dt);
    l.cq_w = carve<half_t>(cur, (size_t)dt * dt);
    l.cq_b = carve<float>(cur, dt);
    l.co_w = carve<half_t>(cur, (size_t)dt * dt);
    l.co_b = carve<float>(cur, dt);
    l.ln2_g = carve<float>(cur, dt);
    l.ln2_b = carve<float>(cur, dt);
    l.fc1_w = carve<half_t>(cur, (size_t)4 * dt * dt);
    l.fc1_b = carve<float>(cur, 4 * dt);
    l.fc2_w = carve<half_t>(cur, (size_t)4 * dt * dt);
    l.fc2_b = carve<float>(cur, dt);
  }
  e->mel_filters = carve<float>(cur, (size_t)D.n_mels * N_BIN);
  e->window = carve<float>(cur, N_FFT);
  e->twiddle = carve<float>(cur, 2 * N_FFT);
  e->filt_lo = carve<int>(cur, D.n_mels);
  e->filt_hi = carve<int>(cur, D.n_mels);
  return (size_t)(cur - base) + 4096;
}

// ---- split mode: the K-doubled weight copies (two passes like layout_weights: size, then carve)
size_t layout_split_weights(wca_engine* e, char* base) {
  const wca_model_dims& D = e->dims;
  const size_t d = D.n_audio_state, dt = D.n_text_state;
  char* cur = base;
  e->sw.k1pad = (int)align_up((size_t)6 * D.n_mels, 64);
  e->sw.conv1_w = carve<half_t>(cur, d * e->sw.k1pad);
  e->sw.conv2_w = carve<half_t>(cur, d * 6 * d);
  e->sw.conv1_wlo = carve<half_t>(cur, d * e->sw.k1pad);
  e->sw.conv2_wlo = carve<half_t>(cur, d * 6 * d);
  e->sw.enc.assign(D.n_audio_layer, LayerW{});
  for (auto& l : e->sw.enc) {
    l.qkv_w = carve<half_t>(cur, 3 * d * 2 * d);
    l.out_w = carve<half_t>(cur, d * 2 * d);
    l.fc1_w = carve<half_t>(cur, 4 * d * 2 * d);
    l.fc2_w = carve<half_t>(cur, d * 8 * d);
  }
  e->sw.tok_emb = carve<half_t>(cur, (size_t)D.n_vocab * 2 * dt);
  e->sw.kv_w = carve<half_t>(cur, (size_t)D.n_text_layer * 2 * dt * 2 * d);
  e->sw.dec.assign(D.n_text_layer, LayerW{});
  for (auto& l : e->sw.dec) {
    l.qkv_w = carve<half_t>(cur, 3 * dt * 2 * dt);
    l.out_w = carve<half_t>(cur, dt * 2 * dt);
    l.cq_w = carve<half_t>(cur, dt * 2 * dt);
    l.co_w = carve<half_t>(cur, dt * 2 * dt);
    l.fc1_w = carve<half_t>(cur, 4 * dt * 2 * dt);
    l.fc2_w = carve<half_t>(cur, dt * 8 * dt);
  }
  return (size_t)(cur - base) + 4096;
}

}  // namespace wca

namespace {

// dst[n][(j / grp) * 2 * grp + (j % grp) + {0, grp}] = src[n][j] for j < K: every group of `grp` source columns is written twice,
// side by side. grp = K: [W | W] (a Linear weight against [hi(K) | lo(K)] activation rows); grp = channels of a conv input: the
// taps of the time-major conv GEMM against frames stored as [hi(C) | lo(C)]. Columns of dst past 2 K stay zero.
// second_zero: the second copy is zero -- [W_lo | 0]: a remainder matrix against pair rows multiplies the hi halves only
__global__ void dup_cols_kernel(const half_t* __restrict__ src, int ld_src, half_t* __restrict__ dst, int ld_dst, long N, int K, int grp, int second_zero) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * K) return;
  const long n = i / K;
  const int j = (int)(i - n * K);
  const half_t v = src[n * ld_src + j];
  const int g = j / grp, c = j - g * grp;
  half_t* o = dst + n * ld_dst + (long)g * 2 * grp + c;
  o[0] = v;
  o[grp] = second_zero ? (half_t)0.f : v;
}

int dup_cols(hipStream_t s, const half_t* src, int ld_src, half_t* dst, int ld_dst, long N, int K, int grp, int second_zero = 0) {
  const long tot = N * K;
  hipLaunchKernelGGL(dup_cols_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, src, ld_src, dst, ld_dst, N, K, grp, second_zero);
  HIPCHK(hipGetLastError());
  return WCA_OK;
}

}  // namespace

namespace wca {

// (re)build the K-doubled copies from the resident f16 weights when a weight changed since the last build
int ensure_split_weights(wca_engine* e) {
  if (!e->split || !e->sw_dirty) return WCA_OK;
  const wca_model_dims& D = e->dims;
  const int d = D.n_audio_state, dt = D.n_text_state, C = D.n_mels;
  hipStream_t s = e->stream;
  WCA_TRY(dup_cols(s, e->conv1_w, e->k1pad, e->sw.conv1_w, e->sw.k1pad, d, 3 * C, C));
  WCA_TRY(dup_cols(s, e->conv2_w, 3 * d, e->sw.conv2_w, 6 * d, d, 3 * d, d));
  if (e->wslab_lo) {   // the conv stem's remainder matrices in the layout of its pair GEMM
    WCA_TRY(dup_cols(s, wlo_of(e, e->conv1_w), e->k1pad, e->sw.conv1_wlo, e->sw.k1pad, d, 3 * C, C, 1));
    WCA_TRY(dup_cols(s, wlo_of(e, e->conv2_w), 3 * d, e->sw.conv2_wlo, 6 * d, d, 3 * d, d, 1));
  }
  for (int li = 0; li < D.n_audio_layer; ++li) {
    const LayerW& l = e->enc[li];
    const LayerW& w = e->sw.enc[li];
    WCA_TRY(dup_cols(s, l.qkv_w, d, w.qkv_w, 2 * d, 3 * d, d, d));
    WCA_TRY(dup_cols(s, l.out_w, d, w.out_w, 2 * d, d, d, d));
    WCA_TRY(dup_cols(s, l.fc1_w, d, w.fc1_w, 2 * d, 4 * d, d, d));
    WCA_TRY(dup_cols(s, l.fc2_w, 4 * d, w.fc2_w, 8 * d, d, 4 * d, 4 * d));
  }
  WCA_TRY(dup_cols(s, e->tok_emb, dt, e->sw.tok_emb, 2 * dt, D.n_vocab, dt, dt));
  WCA_TRY(dup_cols(s, e->kv_w, d, e->sw.kv_w, 2 * d, (long)D.n_text_layer * 2 * dt, d, d));
  for (int li = 0; li < D.n_text_layer; ++li) {
    const LayerW& l = e->dec[li];
    const LayerW& w = e->sw.dec[li];
    WCA_TRY(dup_cols(s, l.qkv_w, dt, w.qkv_w, 2 * dt, 3 * dt, dt, dt));
    WCA_TRY(dup_cols(s, l.out_w, dt, w.out_w, 2 * dt, dt, dt, dt));
    WCA_TRY(dup_cols(s, l.cq_w, dt, w.cq_w, 2 * dt, dt, dt, dt));
    WCA_TRY(dup_cols(s, l.co_w, dt, w.co_w, 2 * dt, dt, dt, dt));
    WCA_TRY(dup_cols(s, l.fc1_w, dt, w.fc1_w, 2 * dt, 4 * dt, dt, dt));
    WCA_TRY(dup_cols(s, l.fc2_w, 4 * dt, w.fc2_w, 8 * dt, dt, 4 * dt, 4 * dt));
  }
  // the copies are read by kernels on stream2 too: make them visible before anything else is enqueued
  HIPCHK(hipStreamSynchronize(s));
  e->sw_dirty = false;
  return WCA_OK;
}

}  // namespace wca

namespace {

// upload helpers: convert host tensor (f32 or f16) into device f16 / f32
// Every weight matrix is f16 AT REST here, like every openai checkpoint ("weights stored fp16, loaded into fp32 params",
// /root/reference/infer_ali.py:36-37), which is what makes A W^T exact-operand arithmetic in the pair mode. An fp32 source whose values are not
// f16-representable (a fine-tuned fp32 state dict) keeps its REMAINDER lo = f16(w - f16(w)) in the W_lo slab (same offset as the f16 value in wslab;
// allocated when the first such tensor arrives), and the pair GEMMs multiply the extra term A_hi W_lo^T (gemm()): w = hi + lo to 2^-22 |w|, the same
// representation the activations travel in. *n_inexact counts the elements with a non-zero remainder (NaN == NaN for this purpose); `base` is the matrix
// the GEMM call sites address (a fused matrix holds several tensors).
int ensure_wlo_slab(wca_engine* e) {
  if (e->wslab_lo) return WCA_OK;
  HIPCHK(hipMalloc((void**)&e->wslab_lo, e->wslab_bytes));
  HIPCHK(hipMemset(e->wslab_lo, 0, e->wslab_bytes));
  return WCA_OK;
}
int put_f16(wca_engine* e, const half_t* base, half_t* dst, const void* src, int dtype, size_t n, size_t* n_inexact) {
  std::vector<half_t> tmp(n);
  size_t bad = 0;
  if (dtype == WCA_DTYPE_F32) {
    const float* s = static_cast<const float*>(src);
    for (size_t i = 0; i < n; ++i) {
      tmp[i] = (half_t)s[i];
      bad += ((float)tmp[i] != s[i]) && (s[i] == s[i]);
    }
    *n_inexact += bad;
  } else {
    memcpy(tmp.data(), src, n * sizeof(half_t));
  }
  HIPCHK(hipMemcpy(dst, tmp.data(), n * sizeof(half_t), hipMemcpyHostToDevice));
  if (bad > 0 || e->wslab_lo) {   // the remainders (zeros when this tensor is exact and replaces an inexact one)
    if (bad > 0) {
      WCA_TRY(ensure_wlo_slab(e));
      const float* s = static_cast<const float*>(src);
      for (size_t i = 0; i < n; ++i) {
        const float r = s[i] - (float)tmp[i];
        tmp[i] = (r == r && std::fabs(r) < 65504.f) ? (half_t)r : (half_t)0.f;
      }
      e->wlo_bases.insert(base);
    } else {
      std::fill(tmp.begin(), tmp.end(), (half_t)0.f);
    }
    HIPCHK(hipMemcpy(e->wslab_lo + (reinterpret_cast<char*>(dst) - e->wslab), tmp.data(), n * sizeof(half_t), hipMemcpyHostToDevice));
  }
  return WCA_OK;
}
int put_f32(float* dst, const void* src, int dtype, size_t n) {
  if (dtype == WCA_DTYPE_F32) {
    HIPCHK(hipMemcpy(dst, src, n * sizeof(float), hipMemcpyHostToDevice));
  } else {
    std::vector<float> tmp(n);
    const half_t* s = static_cast<const half_t*>(src);
    for (size_t i = 0; i < n; ++i) tmp[i] = (float)s[i];
    HIPCHK(hipMemcpy(dst, tmp.data(), n * sizeof(float), hipMemcpyHostToDevice));
  }
  return WCA_OK;
}
inline float host_val(const void* src, int dtype, size_t i) {
  return dtype == WCA_DTYPE_F32 ? static_cast<const float*>(src)[i] : (float)static_cast<const half_t*>(src)[i];
}

// conv weight [out][in][3] -> f16 [out][kpad] with column tap*in + c (remainders of inexact fp32 values into the W_lo slab, like put_f16)
int put_conv(wca_engine* e, half_t* dst, const void* src, int dtype, int out, int in, int kpad, size_t* n_inexact) {
  std::vector<half_t> tmp((size_t)out * kpad, (half_t)0.f), lo((size_t)out * kpad, (half_t)0.f);
  size_t bad = 0;
  for (int n = 0; n < out; ++n)
    for (int c = 0; c < in; ++c)
      for (int t = 0; t < 3; ++t) {
        const float v = host_val(src, dtype, ((size_t)n * in + c) * 3 + t);
        const half_t h = (half_t)v;
        tmp[(size_t)n * kpad + t * in + c] = h;
        if ((float)h != v && v == v) {
          ++bad;
          const float r = v - (float)h;
          lo[(size_t)n * kpad + t * in + c] = std::fabs(r) < 65504.f ? (half_t)r : (half_t)0.f;
        }
      }
  *n_inexact += bad;
  HIPCHK(hipMemcpy(dst, tmp.data(), tmp.size() * sizeof(half_t), hipMemcpyHostToDevice));
  if (bad > 0 || e->wslab_lo) {
    if (bad > 0) {
      WCA_TRY(ensure_wlo_slab(e));
      e->wlo_bases.insert(dst);
    }
    HIPCHK(hipMemcpy(e->wslab_lo + (reinterpret_cast<char*>(dst) - e->wslab), lo.data(), lo.size() * sizeof(half_t), hipMemcpyHostToDevice));
  }
  return WCA_OK;
}

size_t numel(const int64_t* shape, int ndim) {
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
  return n;
}

int load_block_tensor(wca_engine* e, LayerW& l, bool is_dec, int li, const std::string& rest, const void* p, int dtype,
                      size_t n, int d, size_t* n_inexact) {
  const size_t dd = (size_t)d * d;
  auto expect = [&](size_t want) -> bool { return n == want; };
#define WANT(cnt) \
  if (!expect(cnt)) return fail(WCA_ERR_INVALID, "weight %s: expected %zu elements, got %zu", rest.c_str(), (size_t)(cnt), n)
  if (rest == "attn.query.weight") { WANT(dd); return put_f16(e, l.qkv_w, l.qkv_w, p, dtype, n, n_inexact); }
  if (rest == "attn.query.bias") { WANT(d); return put_f32(l.qkv_b, p, dtype, n); }
  if (rest == "attn.key.weight") { WANT(dd); return put_f16(e, l.qkv_w, l.qkv_w + dd, p, dtype, n, n_inexact); }
  if (rest == "attn.value.weight") { WANT(dd); return put_f16(e, l.qkv_w, l.qkv_w + 2 * dd, p, dtype, n, n_inexact); }
  if (rest == "attn.value.bias") { WANT(d); return put_f32(l.qkv_b + 2 * d, p, dtype, n); }
  if (rest == "attn.out.weight") { WANT(dd); return put_f16(e, l.out_w, l.out_w, p, dtype, n, n_inexact); }
  if (rest == "attn.out.bias") { WANT(d); return put_f32(l.out_b, p, dtype, n); }
  if (rest == "attn_ln.weight") { WANT(d); return put_f32(l.ln1_g, p, dtype, n); }
  if (rest == "attn_ln.bias") { WANT(d); return put_f32(l.ln1_b, p, dtype, n); }
  if (rest == "mlp.0.weight") { WANT(4 * dd); return put_f16(e, l.fc1_w, l.fc1_w, p, dtype, n, n_inexact); }
  if (rest == "mlp.0.bias") { WANT(4 * (size_t)d); return put_f32(l.fc1_b, p, dtype, n); }
  if (rest == "mlp.2.weight") { WANT(4 * dd); return put_f16(e, l.fc2_w, l.fc2_w, p, dtype, n, n_inexact); }
  if (rest == "mlp.2.bias") { WANT(d); return put_f32(l.fc2_b, p, dtype, n); }
  if (rest == "mlp_ln.weight") { WANT(d); return put_f32(l.ln2_g, p, dtype, n); }
  if (rest == "mlp_ln.bias") { WANT(d); return put_f32(l.ln2_b, p, dtype, n); }
  if (is_dec) {
    if (rest == "cross_attn.query.weight") { WANT(dd); return put_f16(e, l.cq_w, l.cq_w, p, dtype, n, n_inexact); }
    if (rest == "cross_attn.query.bias") { WANT(d); return put_f32(l.cq_b, p, dtype, n); }
    if (rest == "cross_attn.key.weight") { WANT(dd); return put_f16(e, e->kv_w, e->kv_w + (size_t)(2 * li) * dd, p, dtype, n, n_inexact); }
    if (rest == "cross_attn.value.weight") { WANT(dd); return put_f16(e, e->kv_w, e->kv_w + (size_t)(2 * li + 1) * dd, p, dtype, n, n_inexact); }
    if (rest == "cross_attn.value.bias") { WANT(d); return put_f32(e->kv_b + (size_t)(2 * li + 1) * d, p, dtype, n); }
    if (rest == "cross_attn.out.weight") { WANT(dd); return put_f16(e, l.co_w, l.co_w, p, dtype, n, n_inexact); }
    if (rest == "cross_attn.out.bias") { WANT(d); return put_f32(l.co_b, p, dtype, n); }
    if (rest == "cross_attn_ln.weight") { WANT(d); return put_f32(l.lnc_g, p, dtype, n); }
    if (rest == "cross_attn_ln.bias") { WANT(d); return put_f32(l.lnc_b, p, dtype, n); }
  }
#undef WANT
  return 1;  // unknown (ignored)
}

}  // namespace

extern "C" {

int wca_load_weight(wca_engine* e, const char* name_c, const void* p, int dtype, const int64_t* shape, int ndim) {
  if (!e || !name_c || !p || !shape) return fail(WCA_ERR_INVALID, "null argument");
  if (dtype != WCA_DTYPE_F32 && dtype != WCA_DTYPE_F16) return fail(WCA_ERR_INVALID, "dtype %d", dtype);
  HIPCHK(hipSetDevice(e->device));
  const std::string name(name_c);
  const size_t n = numel(shape, ndim);
  const wca_model_dims& D = e->dims;
  const int d = D.n_audio_state, dt = D.n_text_state;
  int rc = 1;
  size_t n_inexact = 0;   // elements of this tensor that its f16 storage rounded (put_f16 / put_conv)
#define WANTN(cnt) \
  if (n != (size_t)(cnt)) return fail(WCA_ERR_INVALID, "weight %s: expected %zu elements, got %zu", name_c, (size_t)(cnt), n)
  if (name == "mel_filters") {
    WANTN((size_t)D.n_mels * N_BIN);
    std::vector<float> f(n);
    for (size_t i = 0; i < n; ++i) f[i] = host_val(p, dtype, i);
    std::vector<int> lo(D.n_mels), hi(D.n_mels);
    for (int m = 0; m < D.n_mels; ++m) {
      int l = N_BIN, h = 0;
      for (int k = 0; k < N_BIN; ++k)
        if (f[(size_t)m * N_BIN + k] != 0.f) {
          l = k < l ? k : l;
          h = k + 1;
        }
      if (h == 0) l = 0;
      lo[m] = l;
      hi[m] = h;
    }
    HIPCHK(hipMemcpy(e->mel_filters, f.data(), n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->filt_lo, lo.data(), sizeof(int) * D.n_mels, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->filt_hi, hi.data(), sizeof(int) * D.n_mels, hipMemcpyHostToDevice));
    e->have_filters = true;
    rc = WCA_OK;
  } else if (name == "encoder.conv1.weight") {
    WANTN((size_t)d * D.n_mels * 3);
    rc = put_conv(e, e->conv1_w, p, dtype, d, D.n_mels, e->k1pad, &n_inexact);
  } else if (name == "encoder.conv1.bias") {
    WANTN(d);
    rc = put_f32(e->conv1_b, p, dtype, n);
  } else if (name == "encoder.conv2.weight") {
    WANTN((size_t)d * d * 3);
    rc = put_conv(e, e->conv2_w, p, dtype, d, d, 3 * d, &n_inexact);
  } else if (name == "encoder.conv2.bias") {
    WANTN(d);
    rc = put_f32(e->conv2_b, p, dtype, n);
  } else if (name == "encoder.positional_embedding") {
    WANTN((size_t)N_CTX * d);
    rc = put_f32(e->enc_pos, p, dtype, n);
  } else if (name == "encoder.ln_post.weight") {
    WANTN(d);
    rc = put_f32(e->lnpost_g, p, dtype, n);
  } else if (name == "encoder.ln_post.bias") {
    WANTN(d);
    rc = put_f32(e->lnpost_b, p, dtype, n);
  } else if (name == "decoder.token_embedding.weight") {
    WANTN((size_t)D.n_vocab * dt);
    rc = put_f16(e, e->tok_emb, e->tok_emb, p, dtype, n, &n_inexact);
  } else if (name == "decoder.positional_embedding") {
    WANTN((size_t)D.n_text_ctx * dt);
    rc = put_f32(e->dec_pos, p, dtype, n);
  } else if (name == "decoder.ln.weight") {
    WANTN(dt);
    rc = put_f32(e->lnf_g, p, dtype, n);
  } else if (name == "decoder.ln.bias") {
    WANTN(dt);
    rc = put_f32(e->lnf_b, p, dtype, n);
  } else if (name.rfind("encoder.blocks.", 0) == 0 || name.rfind("decoder.blocks.", 0) == 0) {
    const bool is_dec = name[0] == 'd';
    const size_t p0 = 15;
    const size_t dot = name.find('.', p0);
    if (dot == std::string::npos) return fail(WCA_ERR_INVALID, "bad weight name %s", name_c);
    const int li = atoi(name.substr(p0, dot - p0).c_str());
    const int nl = is_dec ? D.n_text_layer : D.n_audio_layer;
    if (li < 0 || li >= nl) return fail(WCA_ERR_INVALID, "layer index out of range in %s", name_c);
    rc = load_block_tensor(e, is_dec ? e->dec[li] : e->enc[li], is_dec, li, name.substr(dot + 1), p, dtype, n, is_dec ? dt : d, &n_inexact);
  }
#undef WANTN
  if (rc == WCA_OK) {
    e->loaded.insert(name);
    e->sw_dirty = true;
    if (n_inexact) e->inexact[name] = n_inexact;
    else e->inexact.erase(name);
    if (e->inexact.empty()) e->wlo_bases.clear();   // (every remainder in the W_lo slab is zero again)
  }
  return rc < 0 ? rc : WCA_OK;  // unknown names (e.g. alignment_heads) are ignored
}

int wca_finalize_weights(wca_engine* e) {
  if (!e) return fail(WCA_ERR_INVALID, "null engine");
  const wca_model_dims& D = e->dims;
  std::vector<std::string> need = {"encoder.conv1.weight", "encoder.conv1.bias", "encoder.conv2.weight", "encoder.conv2.bias",
                                   "encoder.positional_embedding", "encoder.ln_post.weight", "encoder.ln_post.bias",
                                   "decoder.token_embedding.weight", "decoder.positional_embedding", "decoder.ln.weight",
                                   "decoder.ln.bias"};
  const char* blk[] = {"attn.query.weight", "attn.query.bias", "attn.key.weight", "attn.value.weight", "attn.value.bias",
                       "attn.out.weight", "attn.out.bias", "attn_ln.weight", "attn_ln.bias", "mlp.0.weight", "mlp.0.bias",
                       "mlp.2.weight", "mlp.2.bias", "mlp_ln.weight", "mlp_ln.bias"};
  const char* cblk[] = {"cross_attn.query.weight", "cross_attn.query.bias", "cross_attn.key.weight", "cross_attn.value.weight",
                        "cross_attn.value.bias", "cross_attn.out.weight", "cross_attn.out.bias", "cross_attn_ln.weight",
                        "cross_attn_ln.bias"};
  for (int i = 0; i < D.n_audio_layer; ++i)
    for (const char* b : blk) need.push_back("encoder.blocks." + std::to_string(i) + "." + b);
  for (int i = 0; i < D.n_text_layer; ++i) {
    for (const char* b : blk) need.push_back("decoder.blocks." + std::to_string(i) + "." + b);
    for (const char* b : cblk) need.push_back("decoder.blocks." + std::to_string(i) + "." + b);
  }
  for (const auto& nm : need)
    if (!e->loaded.count(nm)) return fail(WCA_ERR_STATE, "missing weight %s", nm.c_str());
  e->finalized = true;
  return WCA_OK;
}

int wca_weights_inexact(wca_engine* e, long long* n_tensors_out, long long* n_values_out, char* first_name_out, int first_name_cap) {
  if (!e) return fail(WCA_ERR_INVALID, "null engine");
  long long tot = 0;
  for (const auto& kv : e->inexact) tot += (long long)kv.second;
  if (n_tensors_out) *n_tensors_out = (long long)e->inexact.size();
  if (n_values_out) *n_values_out = tot;
  if (first_name_out && first_name_cap > 0) {
    const std::string f = e->inexact.empty() ? std::string() : e->inexact.begin()->first;
    snprintf(first_name_out, (size_t)first_name_cap, "%s", f.c_str());
  }
  return WCA_OK;
}

int wca_set_allow_rounded_weights(wca_engine* e, int on) {
  if (!e) return fail(WCA_ERR_INVALID, "null engine");
  e->allow_rounded = on != 0;
  return WCA_OK;
}

}  // extern "C"
