"""Float64 restatement of the Whisper forward that oracle/whisper_ref.py states in fp32, the forward-level wiring MUTATIONS of it, and
the census of the GEMM plans the engine's forward (csrc/engine_forward.hip) asks for at a given width, batch and precision mode.

ForwardRef(sd, dims).forward(mel, tokens) -> {"enc": ln_post output [B,1500,d], "qk": per decoder layer the cross-attention logits
[B,H,n,1500], "logits": [B,n,V]}, everything float64 and independent of oracle/whisper_ref.py (the convolutions are products over stacked
windows, LayerNorm and GELU are written out, the softmax is torch's in float64). tests/test_forward_ref.py checks it against WhisperRef to
fp32 noise.

f16_operands=True is the reference's own statement of what single f16 operands cost: every Linear / conv input and weight, the softmax
probabilities before P.V, and every Linear output the engine's f16 mode stores as f16 (q / k / v, the attention output, the MLP hidden, the
conv stem's first activation -- the last three are the next product's input -- and the encoder's ln_post output, which the f16 mode keeps
in an f16 buffer) are rounded to f16 and widened again; sums, LayerNorm, softmax, GELU and the residual stream stay float64. 4 x its distance from the float64 forward is the f16 mode's bound.

Bounds (section "bounds" of tests/test_forward_widths_gpu.py uses these; none comes from the engine):
  contract mode   |engine - f64| <= max(8 x |WhisperRef fp32 - f64|, floor), floors = the project's bounds at 256 wide: encoder 1e-5, maps 2e-6,
                  logits 1e-5 of the largest |logit|
  f16 mode        |engine - f64| <= 4 x |f64 with f16_operands - f64|, for the maximum and for the mean
"""
import ctypes
import importlib

import numpy as np
import torch

N_FRAMES, N_CTX = 3000, 1500
FLOOR = {"enc": 1e-5, "maps": 2e-6, "logits": 1e-5}
CONTRACT_FACTOR, F16_FACTOR = 8.0, 4.0

MUTATIONS = ("ln_post_gets_attn_ln", "attn_ln_gets_ln_post", "mlp_ln_before_out", "lo_dropped_at_one_site", "cross_kv_rows_swapped",
             "cross_kv_of_previous_layer", "positions_shifted", "last_conv_frame_dropped", "self_attention_one_key_more", "w_lo_left_out",
             "dec_mlp_ln_before_cross_out", "cross_query_ln_is_attn_ln")
# the two that are a loss of precision and not of wiring: visible at the contract mode's bounds only
PRECISION_MUTATIONS = ("lo_dropped_at_one_site", "w_lo_left_out")
# the one product whose input and weight the lo-dropped mutation rounds to f16: fc1 of the first decoder layer
LO_DROPPED_SITE = "decoder.blocks.0.mlp.0"


def r16(x):
    return x.to(torch.float16).to(torch.float64)


def model_dims(wca, d, layers=2):
    return wca.ModelDimensions(80, 1500, d, d // 64, layers, 51865, 448, d, d // 64, layers)


def model_state_dict(dims, seed, cross_qk_std=0.08, inexact=False):
    """synthetic.random_state_dict with LayerNorm parameters that differ from site to site (gamma 1 + N(0, 0.1), beta N(0, 0.1), f16 values):
    with gamma 1 / beta 0 everywhere a LayerNorm that reads another site's parameters computes the right thing. inexact: every matrix, conv
    kernel and bias becomes an fp32 value that f16 does not hold (relative perturbation up to 2^-12), the checkpoint the W_lo slab is for."""
    syn = importlib.import_module("whisper-char-alignment_amd.synthetic")
    sd = syn.random_state_dict(dims, seed=seed, cross_qk_std=cross_qk_std)
    g = torch.Generator().manual_seed(1000 + seed)
    for k in sorted(sd):
        if k.endswith("_ln.weight") or k in ("encoder.ln_post.weight", "decoder.ln.weight"):
            sd[k] = (1.0 + 0.1 * torch.randn(sd[k].shape, generator=g)).to(torch.float16)
        elif k.endswith("_ln.bias") or k in ("encoder.ln_post.bias", "decoder.ln.bias"):
            sd[k] = (0.1 * torch.randn(sd[k].shape, generator=g)).to(torch.float16)
    if inexact:
        for k in sorted(sd):
            if sd[k].dtype == torch.float16 and "ln" not in k.split(".")[-2]:
                w = sd[k].float()
                sd[k] = w * (1.0 + (torch.rand(w.shape, generator=g) - 0.5) * 2.0 ** -11)
    return sd


class ForwardRef:
    def __init__(self, state_dict, dims, f16_operands=False, mutation=None, device="cpu"):
        """device: where the float64 arithmetic runs (torch's own float64 kernels either way; a GPU only makes the five widths affordable)"""
        assert mutation is None or mutation in MUTATIONS
        self.dims, self.f16, self.mut, self.device = dims, f16_operands, mutation, torch.device(device)
        self.sd = {k: torch.as_tensor(v).to(self.device, torch.float64) for k, v in state_dict.items()}

    # ---- the operations
    def _op(self, x, site=None):
        """an operand of a product: rounded to f16 in the f16-operand statement, or at the one site of the lo-dropped mutation"""
        return r16(x) if self.f16 or (self.mut == "lo_dropped_at_one_site" and site == LO_DROPPED_SITE) else x

    def _w(self, name):
        w = self.sd[name]
        if self.mut == "w_lo_left_out" and w.dim() >= 2:
            return r16(w)
        return self._op(w, name[:-len(".weight")])

    def _st(self, x):
        """a Linear output the f16 mode stores as f16"""
        return r16(x) if self.f16 else x

    def _lin(self, x, prefix, bias=True):
        y = self._op(x, prefix) @ self._w(prefix + ".weight").T
        return y + self.sd[prefix + ".bias"] if bias else y

    def _ln(self, x, prefix):
        mu = x.mean(-1, keepdim=True)
        var = ((x - mu) ** 2).mean(-1, keepdim=True)
        return (x - mu) / torch.sqrt(var + 1e-5) * self.sd[prefix + ".weight"] + self.sd[prefix + ".bias"]

    @staticmethod
    def _gelu(x):
        return 0.5 * x * (1.0 + torch.erf(x / np.sqrt(2.0)))

    def _mha(self, x, src, prefix, n_head, mask=None, kv_prefix=None):
        kv_prefix = kv_prefix or prefix
        q = self._st(self._lin(x, prefix + ".query"))
        k = self._st(self._lin(src, kv_prefix + ".key", bias=False))
        v = self._st(self._lin(src, kv_prefix + ".value"))
        B, n, d = q.shape
        hd = d // n_head
        q = q.view(B, n, n_head, hd).permute(0, 2, 1, 3)
        k = k.view(B, k.shape[1], n_head, hd).permute(0, 2, 1, 3)
        v = v.view(B, v.shape[1], n_head, hd).permute(0, 2, 1, 3)
        qk = (q * hd ** -0.5) @ k.transpose(-1, -2)
        if mask is not None:
            qk = qk + mask
        p = torch.softmax(qk, dim=-1)
        if self.f16:
            p = r16(p)
        out = self._st((p @ v).permute(0, 2, 1, 3).reshape(B, n, d))
        return self._lin(out, prefix + ".out"), qk

    def _conv(self, x, name, stride):
        """Conv1d(kernel 3, padding 1) on x [B, T, C_in] -> [B, T / stride, C_out]: the product of the stacked windows with the kernel"""
        w = self._w(name + ".weight")                                   # [C_out, C_in, 3]
        x = torch.nn.functional.pad(self._op(x, name), (0, 0, 1, 1))
        T = x.shape[1] - 2
        win = torch.cat([x[:, k:k + T:stride] for k in range(3)], dim=-1)   # [B, T / stride, 3 C_in], tap-major
        return win @ w.permute(2, 1, 0).reshape(-1, w.shape[0]) + self.sd[name + ".bias"]

    # ---- the model
    @torch.no_grad()
    def encoder(self, mel):
        """mel [B, n_mels, 3000] -> ln_post output [B, 1500, d]; one utterance at a time (the attention logits of a batch do not fit)"""
        return torch.cat([self._encoder_one(mel[b:b + 1].to(self.device, torch.float64)) for b in range(mel.shape[0])])

    def _encoder_one(self, mel):
        D, mut = self.dims, self.mut
        x = self._gelu(self._conv(mel.permute(0, 2, 1), "encoder.conv1", 1))
        if mut == "last_conv_frame_dropped":
            x = torch.cat([x[:, :-1], torch.zeros_like(x[:, -1:])], dim=1)
        x = self._gelu(self._conv(x, "encoder.conv2", 2))
        pos = self.sd["encoder.positional_embedding"]
        x = x + (torch.roll(pos, 1, 0) if mut == "positions_shifted" else pos)
        L = D.n_audio_layer
        for i in range(L):
            p = f"encoder.blocks.{i}"
            ln1 = "encoder.ln_post" if (mut == "attn_ln_gets_ln_post" and i == L - 1) else p + ".attn_ln"
            h = self._ln(x, ln1)
            x0 = x
            x = x + self._mha(h, h, p + ".attn", D.n_audio_head)[0]
            h = self._ln(x0 if (mut == "mlp_ln_before_out" and i == L - 1) else x, p + ".mlp_ln")
            h = self._st(self._gelu(self._lin(h, p + ".mlp.0")))
            x = x + self._lin(h, p + ".mlp.2")
        # the f16 mode leaves ln_post's output in an f16 buffer (the decoder's cross-K/V product reads it): stored as f16 like q / k / v
        return self._st(self._ln(x, f"encoder.blocks.{L - 1}.attn_ln" if mut == "ln_post_gets_attn_ln" else "encoder.ln_post"))

    @torch.no_grad()
    def decoder(self, tokens, xa):
        """tokens [B, n] int64, xa [B, 1500, d] -> (logits [B, n, V], [qk_l [B, H, n, 1500]] per layer)"""
        D, sd, mut = self.dims, self.sd, self.mut
        tokens, xa = tokens.to(self.device), xa.to(self.device)
        n = tokens.shape[-1]
        if mut == "cross_kv_rows_swapped":
            xa = torch.cat([xa[1:2], xa[0:1], xa[2:]])
        x = sd["decoder.token_embedding.weight"][tokens] + sd["decoder.positional_embedding"][:n]
        mask = torch.full((n, n), float("-inf"), dtype=torch.float64, device=self.device).triu_(1)
        if mut == "self_attention_one_key_more" and n > 3:
            mask[2, 3] = 0.0
        qks = []
        for i in range(D.n_text_layer):
            p = f"decoder.blocks.{i}"
            h = self._ln(x, p + ".attn_ln")
            x = x + self._mha(h, h, p + ".attn", D.n_text_head, mask)[0]
            kvp = f"decoder.blocks.{i - 1}.cross_attn" if (mut == "cross_kv_of_previous_layer" and i > 0) else None
            x0 = x
            y, qk = self._mha(self._ln(x, p + (".attn_ln" if mut == "cross_query_ln_is_attn_ln" else ".cross_attn_ln")), xa, p + ".cross_attn",
                              D.n_text_head, kv_prefix=kvp)
            qks.append(qk)
            x = x + y
            h = self._ln(x0 if (mut == "dec_mlp_ln_before_cross_out" and i == 0) else x, p + ".mlp_ln")
            h = self._st(self._gelu(self._lin(h, p + ".mlp.0")))
            x = x + self._lin(h, p + ".mlp.2")
        x = self._ln(x, "decoder.ln")
        return self._op(x) @ self._w("decoder.token_embedding.weight").T, qks

    @torch.no_grad()
    def forward(self, mel, tokens):
        enc = self.encoder(mel)
        logits, qks = self.decoder(tokens, enc)
        return {"enc": enc, "qk": qks, "logits": logits}


def maps_of(qks, max_frames=N_CTX):
    """what get_attentions(medfilt_width=1) returns: softmax over the first max_frames keys, [B, L, H, n, F]"""
    return torch.softmax(torch.stack(list(qks), dim=1)[..., :max_frames], dim=-1)


def observables(out, max_frames=N_CTX):
    return {"enc": out["enc"], "maps": maps_of(out["qk"], max_frames), "logits": out["logits"]}


def distance(got, ref):
    """per observable (max, mean) of |got - ref|; the logits relative to the reference's largest |logit|"""
    res = {}
    for k in ("enc", "maps", "logits"):
        diff = (torch.as_tensor(got[k]).to(ref[k].device, torch.float64) - ref[k]).abs()
        s = ref[k].abs().max().item() if k == "logits" else 1.0
        res[k] = (diff.max().item() / s, diff.mean().item() / s)
    return res


def contract_bounds(fp32_dist):
    """max(8 x the fp32 oracle's own distance from float64, the project's floor) per observable"""
    return {k: max(CONTRACT_FACTOR * fp32_dist[k][0], FLOOR[k]) for k in FLOOR}


def f16_bounds(f16_dist):
    """4 x the f16-operand statement's distance from float64: (bound of the maximum, bound of the mean) per observable"""
    return {k: (F16_FACTOR * f16_dist[k][0], F16_FACTOR * f16_dist[k][1]) for k in FLOOR}


# ------------------------------------------------------------------------------------------------------------------ the plan census
NONE, SKINNY, TILE128, TILE256, PERSIST, PAIR2, PAIR3, LN = range(8)     # GemmKernel, as wca_test_gemm_plan numbers it
KERNEL_NAMES = ("none", "skinny", "t128", "t256", "persist", "pair2", "pair3", "ln")
ADDEND, BATCH_A, POS, BATCH_C = 1, 2, 4, 8
N_CU = 256
SK_BYTES = 4 * 128 * 128 * 128 * 4       # the engine's split-K workspace (csrc/engine.hip)
DEC_ROWS_MAX = 128
WIDTHS = (384, 512, 768, 1024, 1280)
N_MELS, N_VOCAB, N_LAYERS = 80, 51865, 2
ENCODER_SITES = ("conv1", "conv2", "qkv", "out", "fc1", "fc2", "cross_kv")
DECODER_SITES = ("dec_qkv", "dec_out", "dec_cq", "dec_co", "dec_fc1", "dec_fc2", "logits")


def _plan(lib, M, N, K, lda, out_mode, gelu=0, a_lo=0, site=0, flags=0, sk_bytes=0):
    out = (ctypes.c_int32 * 10)(*([-1] * 10))
    if lib.wca_test_gemm_plan(M, N, K, lda, out_mode, gelu, a_lo, 0, site, N_CU, 0, flags, sk_bytes, out) != 0:
        return None
    return dict(zip(("kernel", "grid_x", "grid_y", "block", "lds", "splitk", "supertile", "site", "a_bytes", "w_bytes"), out))


def _sig(form, p, M, N):
    """what a census entry says of one launch: operand form, kernel, split, and whether persistent workgroups walk tiles or take one each"""
    tiles256 = ((M + 255) // 256) * ((N + 255) // 256)
    walk = p["kernel"] in (PERSIST, PAIR2, PAIR3, LN) and p["grid_x"] < tiles256
    return (form, KERNEL_NAMES[p["kernel"]], p["splitk"], "walk" if walk else "one")


def _gemm(lib, M, N, K, pair, out_mode, gelu=0, site=0, sk=False, inexact=False, lda=None, flags=0, candidate=True):
    """gemm() of engine_forward.hip on a product with plain width K: single operands, or pair operands ([hi | lo] rows: the candidate on the
    plain W where the plan gives it a pair kernel, else the K-doubled call), with the W_lo launch and the addend of an inexact checkpoint.
    Returns the signature of the main launch (+ the W_lo launch's)."""
    sk_bytes = SK_BYTES if sk else 0
    if not pair:
        return _sig("single", _plan(lib, M, N, K, lda or K, out_mode, gelu, 0, site, flags, sk_bytes), M, N)
    om = 4 if out_mode == 0 else out_mode
    lda = lda or 2 * K
    extra = ()
    if inexact:
        x = _plan(lib, M, N, K if candidate else 2 * K, lda, 2 if om == 2 else 1, 0, 0, site, flags & BATCH_A, 0)
        extra = ("w_lo:" + KERNEL_NAMES[x["kernel"]],)
        if om != 2:
            flags |= ADDEND
    p = _plan(lib, M, N, K, lda, om, gelu, K, site, flags, sk_bytes) if candidate else None
    if p is not None and p["kernel"] in (PAIR2, PAIR3):
        return _sig("pair", p, M, N) + extra
    return _sig("doubled", _plan(lib, M, N, 2 * K, lda, om, gelu, 0, site, flags, sk_bytes), M, N) + extra


def site_plans(lib, d, B, n, pair, inexact=False):
    """site -> signature for one forward of the d-wide model (80 mels, 2 + 2 layers, heads d / 64) on B utterances and n tokens per row, with
    the arguments engine_forward.hip gives each site. pair: the contract mode; otherwise the f16 mode, whose out / fc2 entries end with
    whether the fused residual + LayerNorm form (out_mode 3) is available."""
    Me, Mc, Md = B * N_CTX, B * N_FRAMES, B * n
    k1 = (3 * N_MELS + 63) // 64 * 64
    r = {}
    # the conv stem: batch-strided windows; split mode runs it K-doubled (windows of [hi | lo] frames), never as a pair candidate
    assert (6 * N_MELS + 63) // 64 * 64 == 2 * k1      # the split stem's padded K is the doubled one at 80 mels
    r["conv1"] = _gemm(lib, Mc, d, k1, pair, 0, 1, 3, inexact=inexact, lda=(2 if pair else 1) * N_MELS, flags=BATCH_A | BATCH_C, candidate=False)
    r["conv2"] = _gemm(lib, Me, d, 3 * d, pair, 1, 1, 3, inexact=inexact, lda=(4 if pair else 2) * d, flags=BATCH_A | POS, candidate=False)
    r["qkv"] = _gemm(lib, Me, 3 * d, d, pair, 0, 0, 1, inexact=inexact)
    r["fc1"] = _gemm(lib, Me, 4 * d, d, pair, 0, 1, 1, inexact=inexact)
    for name, K, site in (("out", d, 1), ("fc2", 4 * d, 4)):
        r[name] = _gemm(lib, Me, d, K, pair, 2, 0, site, sk=True, inexact=inexact)
        if not pair:
            f = _plan(lib, Me, d, K, K, 3, 0, 0, site)
            r[name] += ("fusable" if f is not None and f["kernel"] == LN else "separate",)
    r["cross_kv"] = _gemm(lib, Me, N_LAYERS * 2 * d, d, pair, 0, 0, 3, inexact=inexact)
    dec = (("dec_qkv", 3 * d, d, 0, 0, 1), ("dec_out", d, d, 2, 0, 0), ("dec_cq", d, d, 0, 0, 1), ("dec_co", d, d, 2, 0, 0),
           ("dec_fc1", 4 * d, d, 0, 1, 1), ("dec_fc2", d, 4 * d, 2, 0, 0), ("logits", N_VOCAB, d, 1, 0, 1))
    for name, N, K, om, gelu, ln in dec:
        site = 3 if name == "logits" else 2
        if pair:
            r[name] = _gemm(lib, Md, N, K, True, om, gelu, site, sk=True, inexact=inexact)
            continue
        out = (ctypes.c_int64 * 8)(*([-1] * 8))
        assert lib.wca_test_dec_gemm_plan(d, Md, N, K, ln, 0, out) == 0
        if out[0]:
            r[name] = ("single", "rows", int(out[1]), "one")
        else:
            r[name] = _gemm(lib, Md, N, K, False, om, gelu, site, sk=True)
    return r


def format_plans(plans):
    """one line: site form/kernel[xsplit]/grid form[/fusable] ..."""
    def one(v):
        return "/".join([v[0], v[1] + ("x%d" % v[2] if v[2] > 1 else ""), v[3]] + [str(x) for x in v[4:]])
    return "  ".join("%s %s" % (s, one(v)) for s, v in plans.items())


# Token counts of the teacher-forced decoder: with 6 tokens every batch run stays within the few-row kernel's 128 rows, with 40 tokens the
# batches from 4 on are beyond it. The float64 reference is one forward per width at the width's largest batch: the census' last switch batch
# (B = 1 .. CENSUS_B) under the ceilings that keep the narrow widths' and the widest width's reference affordable.
TOKEN_COUNTS = (6, 40)
CENSUS_B = 20
B_CEILING = {384: 17, 512: 17, 1280: 7}
_CENSUS = {}


def width_census(lib, d):
    if d not in _CENSUS:
        _CENSUS[d] = census(lib, d, TOKEN_COUNTS, CENSUS_B)
    return _CENSUS[d]


def b_max(lib, d):
    """the largest batch of a width's GPU cases: the census' last switch batch within the width's ceiling"""
    return max(S for S in width_census(lib, d) if S <= B_CEILING.get(d, CENSUS_B))


def case_batches(lib, d):
    """the batches of the GPU cases: S - 1 and S for every switch batch S of the census within the width's ceiling"""
    return sorted({b for S in width_census(lib, d) if S <= B_CEILING.get(d, CENSUS_B) for b in (S - 1, S)})


def census(lib, d, n_of, b_max=20):
    """{B: {(mode, site): (signature at B - 1, signature at B)}} for every B in 2 .. b_max at which a site's signature changes; n_of(B) = the
    token counts run at batch B (the decoder's sites are asked at M = B n for each)."""
    def plans(B, pair):
        r = {}
        for n in n_of:
            for s, v in site_plans(lib, d, B, n, pair).items():
                if s in ENCODER_SITES:
                    r[s] = v
                else:
                    r["%s@n%d" % (s, n)] = v
        return r
    changes = {}
    for pair in (False, True):
        prev = plans(1, pair)
        for B in range(2, b_max + 1):
            cur = plans(B, pair)
            for s in cur:
                if cur[s] != prev[s]:
                    changes.setdefault(B, {})[("contract" if pair else "f16", s)] = (prev[s], cur[s])
            prev = cur
    return changes


# ------------------------------------------------------------------------------------------------------------------ inputs of the GPU cases
SOT, NO_TIMESTAMPS, EOT = (50258, 50259, 50359), 50363, 50257
N_LONG = max(TOKEN_COUNTS)
# seeds for which the reference alone leaves at most 2 % of the batched route's jump frames undecided (tests/test_forward_ref.py checks it;
# 20 + d / 128 at 1024 wide left 5 of 108: five consecutive rows of one utterance hang on one near-tie)
MODEL_SEED = {384: 23, 512: 24, 768: 26, 1024: 128, 1280: 30}
BATCHED_B = 3            # the batched route's batch: rows 0 .. 2 of a width's inputs, 2 s, 13.4 s and 24.75 s (100, 668 and 1237 frames)
MEDFILT_WIDTH, TOPK = 3, 2


def inputs(d, B):
    """B distinct utterances (2 s .. 28 s of gated noise, lengths far apart between neighbours: a duplicated or similar utterance would hide
    a row mix-up) as the oracle's log-mel, and B distinct token rows [sot sequence, no_timestamps, 35 text tokens, eot]. Row b is the same
    for every B."""
    from oracle import whisper_ref
    syn = importlib.import_module("whisper-char-alignment_amd.synthetic")
    audio = importlib.import_module("whisper-char-alignment_amd.audio")
    filt = audio.mel_filters(N_MELS)
    lengths = [32000 + (416000 * ((7 * b) % 17)) // 16 for b in range(B)]
    assert len(set(lengths)) == B
    mel = torch.stack([whisper_ref.log_mel_spectrogram(whisper_ref.pad_or_trim(torch.from_numpy(syn.synth_audio(9000 + d + b, n))), filt)
                       for b, n in enumerate(lengths)])
    text = torch.randint(0, EOT, (CENSUS_B, N_LONG - 5), generator=torch.Generator().manual_seed(d))[:B]
    tokens = torch.cat([torch.tensor([[*SOT, NO_TIMESTAMPS]] * B), text, torch.full((B, 1), EOT)], dim=1)
    assert len({tuple(r) for r in tokens.tolist()}) == B
    return mel, tokens, lengths


# ------------------------------------------------------------------------------------------------------------------ the batched route's DTW
def _dp(c):
    """D[i, j]: the cheapest monotone path (steps right, down, diagonal) from (0, 0) to (i, j), both ends counted. Within a row
    D[i, j] = c[i, j] + min(a[j], D[i, j - 1]) with a[j] = min(D[i - 1, j - 1], D[i - 1, j]), i.e. cs[j] + min over k <= j of a[k] - cs[k - 1]."""
    N, F = c.shape
    D = np.empty_like(c)
    cs = np.cumsum(c, axis=1)
    D[0] = cs[0]
    for i in range(1, N):
        a = D[i - 1].copy()
        a[1:] = np.minimum(a[1:], D[i - 1, :-1])
        D[i] = cs[i] + np.minimum.accumulate(a - (cs[i] - c[i]))
    return D


def _entering(c):
    """E[i, j], i >= 1: the cheapest path from (0, 0) to (N - 1, F - 1) that enters row i at column j (from (i - 1, j - 1) or (i - 1, j))"""
    D, R = _dp(c), _dp(c[::-1, ::-1])[::-1, ::-1]
    a = D[:-1].copy()
    a[:, 1:] = np.minimum(a[:, 1:], D[:-1, :-1])
    return np.concatenate([np.full((1, c.shape[1]), np.inf), a + R[1:]]), D


def jump_decisions(M, rtol, atol):
    """M [N, F] float64: the aggregated matrix whose DTW (cost -M) gives row i's jump frame, the column at which the path enters row i.
    Returns (jump [N], decided [N]). Row i is DECIDED when every DTW that is exact on a matrix within eps of M gives it the same jump frame,
    eps[i, j] = rtol |M[i, j]| + atol + 2^-24 S. Both DTWs of the comparison are of that kind: the oracle's and the kernel's keep their
    cost tables in fp32, and fl(x + c) = (x + r) + c, |r| <= 2^-24 |x + c| <= 2^-24 S with S the largest |table entry|, is the exact
    recurrence on a matrix moved by r; the kernel's matrix is in addition within the project's bound (rtol, atol) of M.
    The rule: with P* the float64 path, c~ = -M + eps on P*'s cells and -M - eps elsewhere. For any path P and any perturbation within eps,
    cost'(P) - cost'(P*) >= c~(P) - c~(P*), because the shared cells cancel. So if the cheapest c~ path that enters row i elsewhere than P*
    does costs more than c~(P*), no such matrix moves row i's jump; an exact tie (where the DTWs' tie-breaking would decide) is not decided."""
    c = -np.asarray(M, dtype=np.float64)
    N, F = c.shape
    E, D = _entering(c)
    i, j, cells = N - 1, F - 1, []
    while True:
        cells.append((i, j))
        if i == 0 and j == 0:
            break
        steps = [(D[i - 1, j - 1], i - 1, j - 1)] if i and j else []
        steps += [(D[i - 1, j], i - 1, j)] if i else []
        steps += [(D[i, j - 1], i, j - 1)] if j else []
        _, i, j = min(steps)
    jump = np.full(N, F, dtype=np.int64)
    for i, j in cells:
        jump[i] = min(jump[i], j)
    S = 1.01 * float(np.abs(D).max())
    eps = rtol * np.abs(c) + atol + 2.0 ** -24 * S
    on = np.zeros(c.shape, dtype=bool)
    on[tuple(np.array(cells).T)] = True
    ct = np.where(on, c + eps, c - eps)
    Et, _ = _entering(ct)
    total = float(ct[on].sum())
    decided = np.ones(N, dtype=bool)
    for i in range(1, N):
        other = Et[i].copy()
        other[jump[i]] = np.inf
        decided[i] = other.min() > total + 1e-9
    return jump, decided


def alignment_reference(qk, n_frames, score_bound, matrix_rtol, matrix_atol, gap_factor):
    """The post-processing behind the batched route in float64 (make_opts(aggregation="topk", topk=TOPK, medfilt_width=MEDFILT_WIDTH), default
    score weights 1, 1, 0), on qk [B, LH, n, 1500] float64 and ragged frame counts. Per utterance: scores [LH]; heads (the TOPK best) and
    whether the selection is decided (the postproc tests' rule: TOPK-th and next score gap_factor score bounds apart); jump, the oracle
    DTW's jump frames on the float64 matrix [n - sot_len - 1]; decided [n - sot_len - 1], the rows whose jump frame hangs on more than the
    bounds (jump_decisions; none where the selection is undecided: the matrix itself hangs on it)."""
    from oracle import timing_ref
    pr = importlib.import_module("postproc_ref")
    out = []
    for b, F in enumerate(n_frames):
        x = pr.median_reflect(np.asarray(qk[b][..., :F], dtype=np.float64), MEDFILT_WIDTH)
        e = np.exp(x - x.max(axis=-1, keepdims=True))
        A = e / e.sum(axis=-1, keepdims=True)
        colnorm = np.sqrt((A * A).sum(axis=-2))
        scores = colnorm.sum(axis=-1) + np.sqrt((A * A).sum(axis=-1)).sum(axis=-1)
        order = [i for _, i in sorted((float(s), i) for i, s in enumerate(scores))]
        heads = order[-TOPK:]
        gap = scores[order[-TOPK]] - scores[order[-TOPK - 1]]
        sel_decided = bool(gap >= gap_factor * score_bound * max(1.0, abs(scores[order[-TOPK]])))
        M = pr.aggregate(A, colnorm, heads, len(heads), len(SOT), qk.shape[2] - 1)
        ti, tj = timing_ref.dtw(-torch.from_numpy(M))
        jump = tj[np.pad(np.diff(ti), (1, 0), constant_values=1).astype(bool)]
        mine, decided = jump_decisions(M, matrix_rtol, matrix_atol)
        assert np.array_equal(jump[decided], mine[decided]), (b, "the oracle DTW and the float64 recurrence differ on a decided row")
        out.append({"scores": scores, "heads": sorted(heads), "selection_decided": sel_decided, "jump": jump,
                    "decided": decided & sel_decided})
    return out
