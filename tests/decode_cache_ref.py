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
of the last position that reads its keys through the index arguments the mutations edit."""
import functools
import importlib

import numpy as np
import torch
import torch.nn.functional as F

DIMS = (80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)
SEED = 31
CODE = 64                    # channels [0, CODE): the slot's own code (keys); [CODE, 2 CODE): the target's code (queries)
GAIN = 2.0
TOK_SCALE = 4.0              # token embedding, free channels: N(0, 0.02) * TOK_SCALE
CROSS_QK_STD = 0.12          # decoder cross-attention query / key weights: peaky maps, so that the frames of a recording matter
CROSS_OUT_SCALE = 8.0        # decoder cross-attention out-projection, rows of the free channels
VALUE_FREE_SCALE = 16.0      # decoder self-attention value weights, columns of the free channels: a slot's V tells rows and tokens apart
CONV_SCALE = 4.0             # encoder conv stem weights: the recording, not the sinusoid positions, decides the encoder output
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


def dims():
    return _pkg().ModelDimensions(*DIMS)


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


def planted_state_dict():
    """random_state_dict(DIMS) with the position code planted into the decoder (module docstring). f16, like every checkpoint."""
    D = dims()
    sd = _pkg("synthetic").random_state_dict(D, seed=SEED, cross_qk_std=CROSS_QK_STD)
    for name in ("encoder.conv1.weight", "encoder.conv2.weight"):
        sd[name] = (sd[name].float() * CONV_SCALE).half()
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
                wk[h * hd + r, perm[r]] = GAIN
                wq[h * hd + r, CODE + perm[r]] = GAIN
        sd[pre + "attn.key.weight"] = wk.half()
        sd[pre + "attn.query.weight"] = wq.half()
        sd[pre + "attn.query.bias"] = torch.zeros(dt).half()
        wv = sd[pre + "attn.value.weight"].float()
        wv[:, 2 * CODE:] *= VALUE_FREE_SCALE
        sd[pre + "attn.value.weight"] = wv.half()
        wo = sd[pre + "cross_attn.out.weight"].float()
        wo[2 * CODE:] *= CROSS_OUT_SCALE
        sd[pre + "cross_attn.out.weight"] = wo.half()
    return sd


def mels(rows=len(AUDIO)):
    """The log-mel of each batch row's recording [rows][80][3000] f32, computed on the CPU: the GPU runs and the reference take the same values."""
    syn, audio = _pkg("synthetic"), _pkg("audio")
    wref = importlib.import_module("oracle.whisper_ref")
    filt = audio.mel_filters(80)
    return torch.stack([wref.log_mel_spectrogram(wref.pad_or_trim(torch.from_numpy(syn.synth_audio(s, n_samples=n)) * a), filt) for s, n, a in AUDIO[:rows]])


def token_row(n, row=0):
    """n text tokens, different for every row and position."""
    g = torch.Generator().manual_seed(SEED + 100 + row)
    return torch.randint(0, N_TEXT, (n,), generator=g)


class DecodeRef:
    """float64 Whisper forward over an openai-named state dict (the exact stored values, upcast), with the decoder's self-attention K / V per layer."""

    def __init__(self, sd, D):
        self.D = D
        self.sd = {k: torch.as_tensor(v).to(torch.float64) for k, v in sd.items()}

    def _lin(self, x, prefix, bias=True):
        return F.linear(x, self.sd[prefix + ".weight"], self.sd[prefix + ".bias"] if bias else None)

    def _ln(self, x, prefix):
        return F.layer_norm(x, (x.shape[-1],), self.sd[prefix + ".weight"], self.sd[prefix + ".bias"], 1e-5)

    def _heads(self, x):
        return x.view(x.shape[0], x.shape[1], -1, 64).permute(0, 2, 1, 3)

    def _attend(self, q, k, v, mask=None):
        """q [B, nq, d], k / v [B, nk, d] -> ([B, nq, d], weights [B, H, nq, nk])"""
        qk = self._heads(q) @ self._heads(k).transpose(-1, -2) * 64 ** -0.5
        if mask is not None:
            qk = qk + mask
        w = qk.softmax(-1)
        return (w @ self._heads(v)).permute(0, 2, 1, 3).flatten(start_dim=2), w

    @torch.no_grad()
    def encoder(self, mel):
        sd, D = self.sd, self.D
        x = F.gelu(F.conv1d(mel.to(torch.float64), sd["encoder.conv1.weight"], sd["encoder.conv1.bias"], padding=1))
        x = F.gelu(F.conv1d(x, sd["encoder.conv2.weight"], sd["encoder.conv2.bias"], stride=2, padding=1))
        x = x.permute(0, 2, 1) + sd["encoder.positional_embedding"]
        for i in range(D.n_audio_layer):
            pre = "encoder.blocks.%d" % i
            h = self._ln(x, pre + ".attn_ln")
            a, _ = self._attend(self._lin(h, pre + ".attn.query"), self._lin(h, pre + ".attn.key", False), self._lin(h, pre + ".attn.value"))
            x = x + self._lin(a, pre + ".attn.out")
            x = x + self._lin(F.gelu(self._lin(self._ln(x, pre + ".mlp_ln"), pre + ".mlp.0")), pre + ".mlp.2")
        return self._ln(x, "encoder.ln_post")

    @torch.no_grad()
    def cross_kv(self, xa):
        """Per decoder layer the cross-attention (K, V) of the encoder output xa [B, 1500, d]."""
        return [(self._lin(xa, "decoder.blocks.%d.cross_attn.key" % i, False), self._lin(xa, "decoder.blocks.%d.cross_attn.value" % i))
                for i in range(self.D.n_text_layer)]

    def _after_self(self, x, a, pre, ckv):
        x = x + self._lin(a, pre + ".attn.out")
        c, _ = self._attend(self._lin(self._ln(x, pre + ".cross_attn_ln"), pre + ".cross_attn.query"), *ckv)
        x = x + self._lin(c, pre + ".cross_attn.out")
        return x + self._lin(F.gelu(self._lin(self._ln(x, pre + ".mlp_ln"), pre + ".mlp.0")), pre + ".mlp.2")

    def embed(self, tokens, positions):
        return self.sd["decoder.token_embedding.weight"][tokens] + self.sd["decoder.positional_embedding"][positions]

    def logits(self, x):
        return self._ln(x, "decoder.ln") @ self.sd["decoder.token_embedding.weight"].T

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
            k, v = self._lin(h, pre + ".attn.key", False), self._lin(h, pre + ".attn.value")
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


@functools.lru_cache(maxsize=None)
def scene():
    """What every test shares, computed once per process and left unchanged: the planted checkpoint, its float64 model, the log-mels, the encoder output
    and cross-K/V of the len(AUDIO) rows (`ckv4`; `ckv`: the first B rows), and the uniform decode of B rows teacher-forced on one row of 448 tokens:
    K, V [L, B, 448, d], the final residual stream x, p_target."""
    D = dims()
    sd = planted_state_dict()
    ref = DecodeRef(sd, D)
    mel = mels()
    ckv4 = ref.cross_kv(ref.encoder(mel))
    ckv = [(k[:B], v[:B]) for k, v in ckv4]
    tokens = token_row(D.n_text_ctx)
    K, V, x, pt = ref.forward(tokens[None], ckv)
    return dict(D=D, sd=sd, ref=ref, mel=mel, ckv4=ckv4, ckv=ckv, tokens=tokens, K=K, V=V, x=x, p_target=pt)


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
