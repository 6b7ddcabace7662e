"""Test helper: a position-coded checkpoint for the KV-cached greedy decode loop (csrc/engine_decode.hip, run_decode_step / run_decode_prefill of
csrc/engine_forward.hip), a float64 reference of what the loop leaves behind -- the self-attention cache [L][2][B][T_max][d] and the logits of the last
forward --, the cache lengths and the index faults that tests/test_decode_cache_ref.py pins on the CPU and tests/test_decode_cache_gpu.py checks on the GPU.

With random weights the decoder's self-attention is diffuse: a wrong cache slot, stride or key count moves the last-position logits by about 1 / n,
under any f16 tolerance past the first tile of keys. The planted checkpoint makes position p attend to ONE slot tgt(p):

  * decoder channels [0, 64) and [64, 128) are reserved: the token embedding is zero there, positional_embedding[p, 0:64] = C[p] and
    [p, 64:128] = C[tgt(p)] with C random +-1 codes;
  * every decoder layer's self-attention key weight reads channels [0, 64) and its query weight channels [64, 128): per head a permuted identity block
    times GAIN, zero elsewhere, query bias 0. The target's logit is about 2 * 64 * GAIN^2 / 8 above the others (LayerNorm scales the codes to about
    sqrt(2) while the free channels stay small), the others are N(0, (2 GAIN^2)^2);
  * tgt(p) by p % 3: p itself (the newest key), slot 0, and an interior slot: p // 2 below p = 65, above it the first key of the tile of 64 that
    holds p - 1 (p % 6 == 2) or the last key of the tile before (p % 6 == 5).

The values a slot holds are dominated by its position code, so the rows of a batch must be told apart by something else. The uniform decode feeds every
row the same tokens, which leaves the recordings: they differ in length and in level (AUDIO), the encoder's conv stem is scaled by CONV_SCALE so that the
recording and not the sinusoid positions decides the encoder output, the decoder's cross-attention is moderately peaky and loud (CROSS_QK_STD,
CROSS_OUT_SCALE), and the self-attention value weights read the free channels VALUE_FREE_SCALE times louder, so that a slot's V carries its row. The free
channels of the token embedding are scaled by TOK_SCALE. The settings were chosen on the MI355X for the largest ratio of the smallest fault to the f16 error
(a peakier cross-attention or a louder conv stem raises the f16 error of the deeper planes faster than it separates the rows). Every weight is stored in f16
and the reference computes on exactly those values.

The reference is float64 torch, written from the definition of the model (the arithmetic of oracle/whisper_ref.py): `forward` is teacher-forced on a token
matrix and returns every fed position's K_l = LN(x) W_k and V_l = LN(x) W_v + b_v and the final residual stream; `step_logits` is one KV-cached step
of the last position that reads its keys through the index arguments the mutations edit.

Everything is a function of the model width (WIDTHS: 256, the first scene, left bit for bit what it was, and the five Whisper widths with heads =
width / 64): dims, planted_state_dict, scene, the reference (with an f16-operand statement of itself, the yardstick of bounds(width)) and routes(width, M),
the launches a decode step or a prefill of that width is made of. tests/test_decode_widths_gpu.py runs the new widths."""
import functools
import importlib

import numpy as np
import torch
import torch.nn.functional as F

DIMS = (80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)
WIDTHS = (256, 384, 512, 768, 1024, 1280)    # every Whisper width and the 256 of the first scene; heads = width / 64, 2 + 2 layers
NEW_WIDTHS = WIDTHS[1:]
SEED = 31
CODE = 64                    # channels [0, CODE): the slot's own code (keys); [CODE, 2 CODE): the target's code (queries)
GAIN = 2.0
# Per width, from the float64 reference alone (a CPU search over multiples of 1 / 4 on the width's scene): the smallest gain at which every fed
# position of every layer, row and head puts at least 1 - 1e-6 of its attention on its target, 100 times inside the 1 - 1e-4 that
# tests/test_decode_cache_ref.py asserts (the 256-wide scene: 1 - 5e-8). Misses 1 - min p_target of the search, gain: miss --
#   384: 1.75: 1.6e-6, 2.0: 2.6e-8     512: 1.75: 4.5e-6, 2.0: 9.8e-8     768: 1.75: 7.0e-6, 2.0: 1.4e-7
#   1024: 2.0: 1.2e-6, 2.25: 3.1e-8    1280: 1.75: 2.3e-5, 2.0: 6.7e-7
# LayerNorm scales the code channels up with the width, but the free channels, nine times as many at 1280, take their share of the variance:
# the margin hardly grows. The other scene constants carry over once the decoder's Linears are scaled per fan-in (planted_state_dict).
GAIN_OF = {256: GAIN, 384: 2.0, 512: 2.0, 768: 2.0, 1024: 2.25, 1280: 2.0}
# added to the seed of token_row: a width whose reference margins decide fewer than 90 % of the sampled choices gets another token row
TOKEN_SEED = {256: 0, 384: 2000, 512: 0, 768: 0, 1024: 0, 1280: 0}
# the few-row kernel's split of fc2 (K = 4 width) per width, as routes() reports it: the split-K fault leaves the last of these K ranges out
FC2_SPLITK = {384: 2, 512: 2, 768: 3, 1024: 4, 1280: 5}
TOK_SCALE = 4.0              # token embedding, free channels: N(0, 0.02) * TOK_SCALE
CROSS_QK_STD = 0.12          # decoder cross-attention query / key weights: peaky maps, so that the frames of a recording matter
CROSS_OUT_SCALE = 8.0        # decoder cross-attention out-projection, rows of the free channels
VALUE_FREE_SCALE = 16.0      # decoder self-attention value weights, columns of the free channels: a slot's V tells rows and tokens apart
CONV_SCALE = 4.0             # encoder conv stem weights: the recording, not the sinusoid positions, decides the encoder output
LN_SPREAD = 0.3              # new widths: gamma 1 + N(0, LN_SPREAD), beta N(0, LN_SPREAD) at the decoder's cross_attn_ln, mlp_ln and final ln
B = 3                        # the uniform decodes; the per-row decode takes ROWS_N_INITIAL rows
AUDIO = ((0, 48000, 1.0), (1, 112000, 0.1), (2, 176000, 0.01), (3, 80000, 0.3))    # (synth_audio seed, samples, gain) per batch row
# one position to each side of every boundary of a tile of 64 keys (and of the first keys and the context end): n cached keys, last position n - 1
LENGTHS = (1, 2, 3, 4, 63, 64, 65, 66, 127, 128, 129, 130, 255, 256, 257, 258, 446, 447, 448)
LENGTHS_REFERENCE = tuple(n for n in LENGTHS if n >= 63)      # the reference-precision engine: the tile boundaries
PREFILL_LENGTHS = (42, 43, 130)   # B * n = 126 / 129: the few-row and the large-GEMM prefill (128 rows divide them); 130: past two key tiles
PREFILL_STEPS = 6
ROWS_N_INITIAL = (3, 64, 65, 226)
ROWS_STEPS = 4
N_TEXT = 50257               # text tokens [0, N_TEXT): everything from <|endoftext|> on is suppressed in the sampled runs

# max |GPU - float64| measured on an MI355X over every run of tests/test_decode_cache_gpu.py, and the asserted bounds: 4 times the
# measured maximum, which leaves room for other summation orders across kernel choices
# (small_*: the random `small` checkpoint of tests/test_decode_prompt_gpu.py::test_length_edge_and_bounds, one row walked to slot 447)
MEASURED = {"plane0": 1.25e-3, "plane_deep": 1.12e-2, "logits": 2.82e-3, "small_plane0": 6.04e-4, "small_plane_deep": 6.44e-4, "small_logits": 4.76e-4}
TOL = {k: 4.0 * v for k, v in MEASURED.items()}


def _pkg(name=""):
    return importlib.import_module("whisper-char-alignment_amd" + ("." + name if name else ""))


def _fr():
    return importlib.import_module("forward_ref")


def dims(width=256):
    assert width in WIDTHS
    return _pkg().ModelDimensions(*(DIMS if width == 256 else (80, 1500, width, width // 64, 2, DIMS[5], DIMS[6], width, width // 64, 2)))


def kind(p):
    return p % 3


def tgt(p):
    """The slot position p attends to."""
    if p % 3 == 0:
        return p
    if p % 3 == 1:
        return 0
    if p < 65:
        return p // 2
    return 64 * ((p - 1) // 64) - (1 if p % 6 == 5 else 0)


def planted_state_dict(width=256):
    """random_state_dict of the width's dimensions with the position code planted into the decoder (module docstring). f16, like every checkpoint.
    At the new widths the decoder's cross_attn_ln, mlp_ln and final ln get parameters that differ from site to site (gamma 1 + N(0, 0.1), beta
    N(0, 0.1)): with gamma 1 / beta 0 everywhere a LayerNorm that reads another site's parameters computes the right thing. attn_ln, which scales
    the position code, stays the identity scale; the 256-wide checkpoint is what it was."""
    D = dims(width)
    gain = GAIN_OF[width]
    sd = _pkg("synthetic").random_state_dict(D, seed=SEED, cross_qk_std=CROSS_QK_STD)
    for name in ("encoder.conv1.weight", "encoder.conv2.weight"):
        sd[name] = (sd[name].float() * CONV_SCALE).half()
    if width != 256:
        # random_state_dict draws every Linear from N(0, 0.02) whatever its fan-in, so a product's output grows as sqrt(width): two or three
        # products deep the free channels would drown the position code in the LayerNorms, and the cross-attention would turn one-hot.
        # The decoder's Linears are scaled to the 256-wide scene's gain per product.
        for name in sd:
            if name.startswith("decoder.blocks.") and name.endswith(".weight") and sd[name].dim() == 2:
                sd[name] = (sd[name].float() * (256.0 / width) ** 0.5).half()
    g = torch.Generator().manual_seed(SEED + 1)
    dt, H, T = D.n_text_state, D.n_text_head, D.n_text_ctx
    hd = dt // H
    assert hd == CODE and dt >= 2 * CODE
    code = (torch.randint(0, 2, (T, CODE), generator=g) * 2 - 1).float()
    emb = sd["decoder.token_embedding.weight"].float() * TOK_SCALE
    emb[:, :2 * CODE] = 0.0
    sd["decoder.token_embedding.weight"] = emb.half()
    pos = sd["decoder.positional_embedding"].float()
    pos[:, :CODE] = code
    pos[:, CODE:2 * CODE] = code[[tgt(p) for p in range(T)]]
    sd["decoder.positional_embedding"] = pos.half()
    for li in range(D.n_text_layer):
        pre = "decoder.blocks.%d." % li
        wk, wq = torch.zeros(dt, dt), torch.zeros(dt, dt)
        for h in range(H):
            perm = torch.randperm(CODE, generator=g)
            for r in range(CODE):
                wk[h * hd + r, perm[r]] = gain
                wq[h * hd + r, CODE + perm[r]] = gain
        sd[pre + "attn.key.weight"] = wk.half()
        sd[pre + "attn.query.weight"] = wq.half()
        sd[pre + "attn.query.bias"] = torch.zeros(dt).half()
        wv = sd[pre + "attn.value.weight"].float()
        wv[:, 2 * CODE:] *= VALUE_FREE_SCALE
        sd[pre + "attn.value.weight"] = wv.half()
        wo = sd[pre + "cross_attn.out.weight"].float()
        wo[2 * CODE:] *= CROSS_OUT_SCALE
        sd[pre + "cross_attn.out.weight"] = wo.half()
    if width != 256:
        g = torch.Generator().manual_seed(SEED + 2)
        for name in ["decoder.blocks.%d.%s" % (li, ln) for li in range(D.n_text_layer) for ln in ("cross_attn_ln", "mlp_ln")] + ["decoder.ln"]:
            sd[name + ".weight"] = (1.0 + LN_SPREAD * torch.randn(dt, generator=g)).half()
            sd[name + ".bias"] = (LN_SPREAD * torch.randn(dt, generator=g)).half()
    return sd


def mels(rows=len(AUDIO)):
    """The log-mel of each batch row's recording [rows][80][3000] f32, computed on the CPU: the GPU runs and the reference take the same values."""
    syn, audio = _pkg("synthetic"), _pkg("audio")
    wref = importlib.import_module("oracle.whisper_ref")
    filt = audio.mel_filters(80)
    return torch.stack([wref.log_mel_spectrogram(wref.pad_or_trim(torch.from_numpy(syn.synth_audio(s, n_samples=n)) * a), filt) for s, n, a in AUDIO[:rows]])


def token_row(n, row=0, width=256):
    """n text tokens, different for every row and position (and, where TOKEN_SEED says so, for the width)."""
    g = torch.Generator().manual_seed(SEED + 100 + row + TOKEN_SEED[width])
    return torch.randint(0, N_TEXT, (n,), generator=g)


class DecodeRef:
    """float64 Whisper forward over an openai-named state dict (the exact stored values, upcast), with the decoder's self-attention K / V per layer."""

    def __init__(self, sd, D, f16_operands=False, fault=None):
        """f16_operands: the reference's own statement of what the f16 decode costs (the rule of tests/forward_ref.py, whose r16 it uses): every
        product operand, the softmax probabilities before P.V and every activation the engine stores as f16 -- q / k / v (the cached planes and the
        cross-K/V among them), the attention output, the MLP hidden, the conv stem's first activation, the encoder's ln_post output -- are rounded
        to f16 and widened again; sums, LayerNorm, softmax, GELU and the residual stream stay float64. 4 x its distance from the float64
        reference is the bound of the new widths (bounds()).
        fault: None, or one of the two wiring faults that exist only where a decode step leaves the 256-wide routes, on decoder layer 0:
          ("fc2_partial", s)  one split-K partial of fc2 missing: the K range [K / s * (s - 1), K) is left out of the product
          ("fc1_ln", site)    fc1's separately launched LayerNorm reads the parameters of `site` (e.g. "cross_attn_ln") instead of mlp_ln's"""
        self.D, self.f16, self.fault = D, f16_operands, fault
        self.sd = {k: torch.as_tensor(v).to(torch.float64) for k, v in sd.items()}

    def _st(self, x):
        """an activation the f16 engine stores as f16"""
        return _fr().r16(x) if self.f16 else x

    def _lin(self, x, prefix, bias=True, k_end=None):
        w = self.sd[prefix + ".weight"]
        if self.f16:
            x, w = _fr().r16(x), _fr().r16(w)
        if k_end is not None:
            x, w = x[..., :k_end], w[:, :k_end]
        return F.linear(x, w, self.sd[prefix + ".bias"] if bias else None)

    def _ln(self, x, prefix):
        return F.layer_norm(x, (x.shape[-1],), self.sd[prefix + ".weight"], self.sd[prefix + ".bias"], 1e-5)

    def _heads(self, x):
        return x.view(x.shape[0], x.shape[1], -1, 64).permute(0, 2, 1, 3)

    def _attend(self, q, k, v, mask=None):
        """q [B, nq, d], k / v [B, nk, d] -> ([B, nq, d], weights [B, H, nq, nk])"""
        qk = self._heads(self._st(q)) @ self._heads(k).transpose(-1, -2) * 64 ** -0.5
        if mask is not None:
            qk = qk + mask
        w = qk.softmax(-1)
        return self._st((self._st(w) @ self._heads(v)).permute(0, 2, 1, 3).flatten(start_dim=2)), w

    @torch.no_grad()
    def encoder(self, mel):
        sd, D = self.sd, self.D
        x = self._st(F.gelu(F.conv1d(self._st(mel.to(torch.float64)), sd["encoder.conv1.weight"], sd["encoder.conv1.bias"], padding=1)))
        x = F.gelu(F.conv1d(x, sd["encoder.conv2.weight"], sd["encoder.conv2.bias"], stride=2, padding=1))
        x = x.permute(0, 2, 1) + sd["encoder.positional_embedding"]
        for i in range(D.n_audio_layer):
            pre = "encoder.blocks.%d" % i
            h = self._ln(x, pre + ".attn_ln")
            a, _ = self._attend(self._lin(h, pre + ".attn.query"), self._st(self._lin(h, pre + ".attn.key", False)),
                                self._st(self._lin(h, pre + ".attn.value")))
            x = x + self._lin(a, pre + ".attn.out")
            x = x + self._lin(self._st(F.gelu(self._lin(self._ln(x, pre + ".mlp_ln"), pre + ".mlp.0"))), pre + ".mlp.2")
        return self._st(self._ln(x, "encoder.ln_post"))

    @torch.no_grad()
    def cross_kv(self, xa):
        """Per decoder layer the cross-attention (K, V) of the encoder output xa [B, 1500, d]."""
        return [(self._st(self._lin(xa, "decoder.blocks.%d.cross_attn.key" % i, False)), self._st(self._lin(xa, "decoder.blocks.%d.cross_attn.value" % i)))
                for i in range(self.D.n_text_layer)]

    def _after_self(self, x, a, pre, ckv):
        x = x + self._lin(a, pre + ".attn.out")
        c, _ = self._attend(self._lin(self._ln(x, pre + ".cross_attn_ln"), pre + ".cross_attn.query"), *ckv)
        x = x + self._lin(c, pre + ".cross_attn.out")
        fault = self.fault if self.fault and pre == "decoder.blocks.0" else (None, None)
        h = self._ln(x, pre + "." + (fault[1] if fault[0] == "fc1_ln" else "mlp_ln"))
        h = self._st(F.gelu(self._lin(h, pre + ".mlp.0")))
        k_end = h.shape[-1] // fault[1] * (fault[1] - 1) if fault[0] == "fc2_partial" else None
        return x + self._lin(h, pre + ".mlp.2", k_end=k_end)

    def embed(self, tokens, positions):
        return self.sd["decoder.token_embedding.weight"][tokens] + self.sd["decoder.positional_embedding"][positions]

    def logits(self, x):
        h = self._ln(x, "decoder.ln")
        return (_fr().r16(h) if self.f16 else h) @ self.sd["decoder.token_embedding.weight"].T

    @torch.no_grad()
    def forward(self, tokens, ckv, pos_shift=0):
        """Teacher-forced on tokens [B, n] (a [1, n] matrix serves every row of ckv). Returns K, V [L, B, n, d] of every fed position, the final
        residual stream x [B, n, d] (logits(x[:, p]) are position p's) and p_target [L, B, H, n], the self-attention weight on slot tgt(p).
        pos_shift: position p takes positional row p + pos_shift (clamped to the table) -- the positional fault."""
        D = self.D
        Bc, n = ckv[0][0].shape[0], tokens.shape[1]
        positions = (torch.arange(n) + pos_shift).clamp(0, D.n_text_ctx - 1)
        x = self.embed(tokens, positions).expand(Bc, n, -1)
        mask = torch.full((n, n), float("-inf"), dtype=torch.float64).triu_(1)
        Ks, Vs, pt = [], [], []
        t_idx = torch.tensor([tgt(p) for p in range(n)])
        for i in range(D.n_text_layer):
            pre = "decoder.blocks.%d" % i
            h = self._ln(x, pre + ".attn_ln")
            k, v = self._st(self._lin(h, pre + ".attn.key", False)), self._st(self._lin(h, pre + ".attn.value"))
            a, w = self._attend(self._lin(h, pre + ".attn.query"), k, v, mask)
            Ks.append(k)
            Vs.append(v)
            pt.append(w[:, :, torch.arange(n), t_idx])
            x = self._after_self(x, a, pre, ckv[i])
        return torch.stack(Ks), torch.stack(Vs), x, torch.stack(pt)

    @torch.no_grad()
    def step_logits(self, tokens_last, p, planes, ckv, key_idx=None, row_map=None, pos_row=None):
        """One KV-cached step of position p: tokens_last [B] (or [1]), planes [L][2][B][T][d] as the loop's cache (slot p filled), -> logits [B, V].
        The step reads layer l's keys planes[l, 0, row_map[b], key_idx] and values planes[l, 1, ...]: the defaults, key_idx = 0 .. p and
        row_map[b] = b, are the loop's contract; pos_row is the positional row (p)."""
        D = self.D
        Bc = ckv[0][0].shape[0]
        key_idx = torch.arange(p + 1) if key_idx is None else torch.as_tensor(key_idx)
        row_map = torch.arange(Bc) if row_map is None else torch.as_tensor(row_map)
        x = self.embed(tokens_last.view(-1, 1), torch.tensor([p if pos_row is None else pos_row])).expand(Bc, 1, -1)
        for i in range(D.n_text_layer):
            pre = "decoder.blocks.%d" % i
            q = self._lin(self._ln(x, pre + ".attn_ln"), pre + ".attn.query")
            a, _ = self._attend(q, planes[i, 0][row_map][:, key_idx], planes[i, 1][row_map][:, key_idx])
            x = self._after_self(x, a, pre, ckv[i])
        return self.logits(x[:, 0])


def planes_of(K, V, T_max):
    """The cache the loop leaves after feeding K.shape[2] positions: [L][2][B][T_max][d], slots never fed 0."""
    L, Bc, n, d = K.shape
    out = torch.zeros(L, 2, Bc, T_max, d, dtype=K.dtype)
    out[:, 0, :, :n] = K
    out[:, 1, :, :n] = V
    return out


_SCENES = {}


def scene(width=256):
    """What every test of a width shares, computed once per process and left unchanged: the planted checkpoint, its float64 model, the log-mels, the
    encoder output and cross-K/V of the len(AUDIO) rows (`ckv4`; `ckv`: the first B rows), and the uniform decode of B rows teacher-forced on one row of
    448 tokens: K, V [L, B, 448, d], the final residual stream x, p_target. The 256-wide scene stays for the process; of the other widths the one asked
    last (the cases run width by width, and a 1280-wide scene holds a quarter of a gigabyte of cross-K/V)."""
    if width not in _SCENES:
        for w in [w for w in _SCENES if w != 256]:
            del _SCENES[w]
        D = dims(width)
        sd = planted_state_dict(width)
        ref = DecodeRef(sd, D)
        mel = mels()
        ckv4 = ref.cross_kv(ref.encoder(mel))
        ckv = [(k[:B], v[:B]) for k, v in ckv4]
        tokens = token_row(D.n_text_ctx, width=width)
        K, V, x, pt = ref.forward(tokens[None], ckv)
        _SCENES[width] = dict(D=D, sd=sd, ref=ref, mel=mel, ckv4=ckv4, ckv=ckv, tokens=tokens, K=K, V=V, x=x, p_target=pt, width=width)
    return _SCENES[width]


def f16_spacing(v):
    """the distance between neighbouring f16 values at magnitude v"""
    return 2.0 ** (int(np.floor(np.log2(max(float(v), 2.0 ** -14)))) - 10)


@functools.lru_cache(maxsize=None)
def bounds(width):
    """The bounds of a new width's GPU cases (tests/test_decode_widths_gpu.py), from the references alone: per quantity
    max(4 x the distance of the f16_operands statement from float64, one f16 spacing of the largest float64 entry), on the width's scene -- the
    cache planes of the 448 uniform positions, layer 0 and the deeper layers, and the logits of the last position of every length of LENGTHS.
    4 x is the room tests/forward_ref.py gives other summation orders; the spacing is the floor of a quantity stored in f16.
    Returns {"yard": {...}, "floor": {...}, "tol": {...}} over plane0, plane_deep, logits."""
    sc = scene(width)
    r16 = DecodeRef(sc["sd"], sc["D"], f16_operands=True)
    ckv = [(k[:B], v[:B]) for k, v in r16.cross_kv(r16.encoder(sc["mel"][:B]))]
    K, V, x, _ = r16.forward(sc["tokens"][None], ckv)
    last = [n - 1 for n in LENGTHS]
    want = sc["ref"].logits(sc["x"][:, last])
    yard = {"plane0": max(float((K[0] - sc["K"][0]).abs().max()), float((V[0] - sc["V"][0]).abs().max())),
            "plane_deep": max(float((K[1:] - sc["K"][1:]).abs().max()), float((V[1:] - sc["V"][1:]).abs().max())),
            "logits": float((r16.logits(x[:, last]) - want).abs().max())}
    floor = {"plane0": f16_spacing(max(sc["K"][0].abs().max(), sc["V"][0].abs().max())),
             "plane_deep": f16_spacing(max(sc["K"][1:].abs().max(), sc["V"][1:].abs().max())), "logits": f16_spacing(want.abs().max())}
    return {"yard": yard, "floor": floor, "tol": {q: max(_fr().F16_FACTOR * yard[q], floor[q]) for q in yard}}


def tol(width):
    """The asserted bounds of a width: the measured-on-the-MI355X TOL of the 256-wide scene, bounds(width)["tol"] of the others."""
    return TOL if width == 256 else bounds(width)["tol"]


# ---- which launches a decode step (or a prefill) of a width is made of
# site -> (N / d, K / d, out_mode, gelu, LayerNorm-fed): the arguments run_decoder_layers and dec_logits of csrc/engine_forward.hip give dec_gemm
ROUTE_SITES = {"qkv": (3, 1, 0, 0, 1), "out": (1, 1, 2, 0, 0), "cross_q": (1, 1, 0, 0, 1), "cross_out": (1, 1, 2, 0, 0), "fc1": (4, 1, 0, 1, 1),
               "fc2": (1, 4, 2, 0, 0), "logits": (None, 1, 1, 0, 1)}


def routes(width, M, step=True, lib=None):
    """site -> (kernel, splitk, LayerNorm, KV append) for the GEMMs of one f16 decode forward of the width on M rows, as dec_gemm decides them:
    wca_test_dec_gemm_plan says whether the few-row kernel takes the site ("rows": its LayerNorm prologue is "fused", its KV append "in-kernel")
    and wca_test_gemm_plan which kernel the separate route's gemm() lands on (LayerNorm "separate" = launch_layernorm_f16 first, KV append
    "launch" = launch_kv_append behind it). step: a KV-cached step, whose qkv product appends to the cache; a prefill (step=False) scatters
    instead and its qkv is an ordinary product. "-": the site has no LayerNorm / no append."""
    import ctypes
    fr = _fr()
    lib = lib or _pkg("_lib").load()
    r = {}
    for name, (Nd, Kd, om, gelu, ln) in ROUTE_SITES.items():
        N, K = (DIMS[5] if Nd is None else Nd * width), Kd * width
        kv = int(step and name == "qkv")
        out = (ctypes.c_int64 * 8)(*([-1] * 8))
        assert lib.wca_test_dec_gemm_plan(width, M, N, K, ln, kv, out) == 0
        if out[0]:
            r[name] = ("rows", int(out[1]), "fused" if ln else "-", "in-kernel" if kv else "-")
        else:
            p = fr._plan(lib, M, N, K, K, om, gelu, 0, 3 if name == "logits" else 2, 0, fr.SK_BYTES)
            r[name] = (fr.KERNEL_NAMES[p["kernel"]], p["splitk"], "separate" if ln else "-", "launch" if kv else "-")
    return r


def format_route(v):
    """'rows x2', 't128 ln:separate kv:launch', ...: one census entry as the literal table of tests/test_decode_cache_ref.py writes it"""
    return v[0] + (" x%d" % v[1] if v[1] > 1 else "") + (" ln:" + v[2] if v[2] != "-" else "") + (" kv:" + v[3] if v[3] != "-" else "")


# ---- the reference's own greedy decode: which of the GPU cases' sampled choices the float64 margin decides
@torch.no_grad()
def greedy_reference(ref, ckv, initial, steps):
    """initial [1 or B][n] tokens, `steps` choices: each the arg max of the float64 logits over the text tokens, fed back. Returns the margins
    [B][steps] between the best and the second text logit, and the tokens [B][n + steps]."""
    Bc = ckv[0][0].shape[0]
    toks = torch.as_tensor(initial).expand(Bc, -1).clone()
    margins = []
    for _ in range(steps):
        x = ref.forward(toks, ckv)[2]
        top2 = ref.logits(x[:, -1])[:, :N_TEXT].topk(2, dim=-1)
        margins.append(top2.values[:, 0] - top2.values[:, 1])
        toks = torch.cat([toks, top2.indices[:, :1]], dim=1)
    return torch.stack(margins, dim=1), toks


STEPWISE_WIDTHS = (1, 64, 65, 129, 448)      # the stepwise lengths of the new widths: the first key, each side of a tile boundary, the context end
STEPWISE_WIDTHS_REFERENCE = (65, 448)


def sampled_margins(width):
    """The float64 top-2 margins of every choice the GPU cases of a width sample (the reference's own greedy tokens stand in for the GPU's, which
    are the same wherever the margin decides): the stepwise cases' one choice per row, the prefill cases' PREFILL_STEPS, the per-row form's
    ROWS_STEPS."""
    sc = scene(width)
    ref = sc["ref"]
    out = [greedy_reference(ref, sc["ckv"], sc["tokens"][None, :n], 1)[0].reshape(-1) for n in STEPWISE_WIDTHS]
    out += [greedy_reference(ref, sc["ckv"], sc["tokens"][None, :n], PREFILL_STEPS)[0].reshape(-1) for n in PREFILL_LENGTHS]
    for b, n in enumerate(ROWS_N_INITIAL):
        ckv_b = [(k[b:b + 1], v[b:b + 1]) for k, v in sc["ckv4"]]
        out.append(greedy_reference(ref, ckv_b, token_row(n, row=b + 1, width=width)[None], ROWS_STEPS)[0].reshape(-1))
    return torch.cat(out)


# ---- the faults, as index edits of the clean cache `planes` [L][2][B][T][d] (a copy is edited) or of what the last step reads from it
SHIFT_SLOTS = (1, 63, 64, 65, 128, 256, 447)


def mut_slot_holds_previous(planes):
    """a. slot t holds position t - 1"""
    out = planes.clone()
    for t in SHIFT_SLOTS:
        if t < planes.shape[3]:
            out[:, :, :, t] = planes[:, :, :, t - 1]
    return out


def mut_row_stride(planes):
    """b. the rows of a plane are addressed T_max - 1 slots apart"""
    L, two, Bc, T, d = planes.shape
    flat = planes.reshape(L, two, Bc * T, d)
    idx = (torch.arange(Bc)[:, None] * (T - 1) + torch.arange(T)[None, :]).reshape(-1)
    return flat[:, :, idx].reshape(planes.shape).clone()


def mut_swap_kv(planes):
    """c. K and V planes swapped"""
    return planes[:, [1, 0]].clone()


def mut_swap_layers(planes):
    """c. the planes of two layers swapped"""
    return planes[[1, 0]].clone()


def drop_newest(n):
    """e. the newest key invisible: the key indices the last step of n cached keys reads"""
    return list(range(n - 1))


def drop_key(n, j):
    """f. key j dropped"""
    return [i for i in range(n) if i != j]


def previous_row(Bc):
    """g. row b reads row b - 1's cache"""
    return [(b - 1) % Bc for b in range(Bc)]


def text_filters():
    """oracle.decoding_ref filters of the sampled runs: EOT and every special token suppressed, no timestamp rules, no blank suppression."""
    dref = importlib.import_module("oracle.decoding_ref")
    return dref.make_filters(0, N_TEXT, DIMS[5], None, list(range(N_TEXT, DIMS[5])), None, apply_timestamp_rules=False)


def text_suppress_mask():
    sup = np.zeros(DIMS[5], np.uint8)
    sup[N_TEXT:] = 1
    return sup


# ---- what the GPU tests of every width assert (tests/test_decode_cache_gpu.py at 256, tests/test_decode_widths_gpu.py at the others)
def check_state(tag, cache, logits, want_planes, fed, want_logits, tol=None):
    """cache [L][2][B][T][d] f16 and logits [R][V] f32 of the GPU against the float64 planes (row b: slots [0, fed[b])) and logits rows: prints the three
    maxima and their share of the bounds `tol` (TOL, the 256-wide scene's, unless given), then asserts them. Returns the three distances."""
    tol = TOL if tol is None else tol
    cache = torch.from_numpy(cache.astype(np.float64))
    d0 = dd = 0.0
    for b, n in enumerate(fed):
        diff = (cache[:, :, b, :n] - want_planes[:, :, b, :n]).abs()
        d0 = max(d0, float(diff[0].max()))
        dd = max(dd, float(diff[1:].max()))
    dl = float((torch.from_numpy(logits.astype(np.float64)) - want_logits).abs().max())
    print("decode-cache measure %s: plane0 %.3e plane_deep %.3e logits %.3e (|logits| max %.2f)  of the bound: %.2f %.2f %.2f"
          % (tag, d0, dd, dl, float(want_logits.abs().max()), d0 / tol["plane0"], dd / tol["plane_deep"], dl / tol["logits"]))
    assert np.isfinite(logits).all()
    assert d0 <= tol["plane0"], (tag, "layer-0 planes", d0, tol["plane0"])
    assert dd <= tol["plane_deep"], (tag, "deeper planes", dd, tol["plane_deep"])
    assert dl <= tol["logits"], (tag, "logits", dl, tol["logits"])
    return {"plane0": d0, "plane_deep": dd, "logits": dl}


def check_choices(tag, step_logits, chosen, sum_logprob, tol_logits):
    """The sampled tokens and sum_logprob against oracle.decoding_ref.select_step on the float64 logits step_logits [B][S][V] (teacher-forced on the
    GPU's tokens `chosen` [B][S]): the oracle's choice wherever its margin exceeds the logits bound, and the log-probability of the GPU's tokens
    (log-softmax moves by at most twice the largest logit change, per step)."""
    dref = importlib.import_module("oracle.decoding_ref")
    Bc, S = chosen.shape
    filters = text_filters()
    want_lp = torch.zeros(Bc, dtype=torch.float64)
    n_decided = 0
    for i in range(S):
        last = torch.zeros(Bc, 1, dtype=torch.long)   # no row has ended: <|endoftext|> is suppressed
        new, _, filt = dref.select_step(step_logits[:, i], last, torch.zeros(Bc), filters, N_TEXT)
        top2 = filt.topk(2, dim=-1).values
        for b in range(Bc):
            assert chosen[b, i] < N_TEXT, (tag, b, i, int(chosen[b, i]))
            if float(top2[b, 0] - top2[b, 1]) > tol_logits:
                n_decided += 1
                assert int(chosen[b, i]) == int(new[b, -1]), (tag, b, i, int(chosen[b, i]), int(new[b, -1]), float(top2[b, 0] - top2[b, 1]))
        masked = step_logits[:, i].clone()
        masked[:, N_TEXT:] = float("-inf")
        want_lp += masked.log_softmax(-1)[torch.arange(Bc), torch.from_numpy(chosen[:, i].astype(np.int64))]
    err = float((torch.from_numpy(sum_logprob.astype(np.float64)) - want_lp).abs().max())
    print("decode-cache choices %s: %d of %d decided by the reference margin, max |d sum_logprob| %.3e" % (tag, n_decided, Bc * S, err))
    assert n_decided >= 1
    assert err <= S * 2 * tol_logits + 1e-4, (tag, err)
