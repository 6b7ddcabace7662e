"""Test helper: two families of attention inputs made for the INDEX arithmetic of csrc/attention.hip and csrc/attention_split.hip (head_dim 64,
scale 1/8), their float64 references written from the definition, and the shapes that tests/test_attention_probe_ref.py pins on the CPU and
tests/test_attention_probes_gpu.py runs on the GPU. With randn operands the softmax is diffuse: one key dropped, counted twice or admitted past
a mask moves an output by about 1 / nk, below the f16 tolerance of 4e-3 for nk > 250. These inputs make every intermediate of the kernels exact,
so that the bound is one rounding. Every value is exactly representable in f16.

Uniform probe (counts keys): Q = 0, K = 0, so every live logit is 0 and p = exp2(0) = 1 in every kernel; V is +-2, drawn per (b, key, h, c). A row's
result is the mean of V over its live keys: an integer sum over an integer count. It moves when a row sees one key too few, one too many, one
twice, or a key of another head or batch row.

Peaked probe (identifies keys): K is +-1, Q[i] = 4 K[t(i)] for a target map t, so the target's logit is 4 * 64 / 8 = 32 and every other logit is
an integer of N(0, 4^2); V[b, j, h, c] = ((((j + 1) (c + 3)) % 1021) - 510) / 256, negated where b + h is odd. The result of row i is V[t(i)]
up to a leaked mass below 1e-5. It moves by 0.25 or more on a permuted or shifted key row, query row, head or channel. Target maps:
`first` t = 0; `last` t = live(i) - 1; `spread` t = (5 i + 3) % live(i) -- with 3 i where live(i) = 5: 5 i + 3 is the same key for every
row there, and no map would tell two query rows of a 5-key launch apart.

Planes are 8 rows longer than the largest key count, and a launch addresses a prefix of them: the rows past its nk are live data of the same
family (a leaked key is counted), and the last 8 rows hold K = 0, V = 64.

Layouts are the kernels': q [B][nq][H * 64], k / v [B][rows][H * 64], head h of a row at column h * 64. `live` is an int64 [B][nq] table of
key counts per batch row and query row (live_counts): nk, or the row's own count, cut to i + 1 under the causal mask."""
import functools

import torch

HEAD, SCALE = 64, 0.125
B, H = 2, 2
NK_MAX, NQ_MAX, GUARD = 1500, 448, 8
GUARD_V = 64.0
SEED = 0
LO = 2.0 ** -13          # pair runs: every lo half is +-2^-13, so hi + lo is exact in f32 and the pair is its own split
MAPS = ("first", "last", "spread")
MUTATIONS = ("drop_last_key", "admit_one_more", "shift_v_by_one", "swap_adjacent_queries", "next_head")
ROWS_B = 300             # the per-row-count decode launch: batch row b has b + 1 keys

_KEYS_200 = list(range(1, 201)) + [255, 256, 257, 448, 1499, 1500]
# (nq, nk, causal) of every launch, the smallest shapes at which each index expression of the kernels changes value
SWEEPS = {
    "key": [(97, nk, False) for nk in _KEYS_200],
    "query": [(nq, 70, False) for nq in range(2, 261)],
    "causal": [(n, n, True) for n in list(range(1, 261)) + [448]],
    "capture": [(nq, nk, False) for nq in (5, 69) for nk in list(range(1, 81)) + [145, 1500]],
    "causal_capture": [(n, n, True) for n in (1, 5, 63, 64, 65, 130)],
    "decode": [(1, nk, False) for nk in range(1, 301)],
}


def cap_cols(nk):
    return min(nk, 145)


def cap_ld(nk):
    return ((cap_cols(nk) + 3) & ~3) + 4


def rows_counts(shuffled):
    """Key counts of the ROWS_B batch rows of the per-row decode launch: 1 .. ROWS_B, in order or in a seeded shuffle."""
    c = torch.arange(1, ROWS_B + 1)
    return c[torch.randperm(ROWS_B, generator=torch.Generator().manual_seed(SEED + 7))] if shuffled else c


# ------------------------------------------------------------------------------- inputs (float64 tensors of f16-exact values)
def _signs(shape, seed):
    return torch.randint(0, 2, shape, generator=torch.Generator().manual_seed(seed)).double() * 2 - 1


@functools.lru_cache(maxsize=None)
def uniform_v(nb=B, nk_max=NK_MAX, nh=H):
    v = 2 * _signs((nb, nk_max + GUARD, nh * HEAD), SEED + 1)
    v[:, nk_max:] = GUARD_V
    return v


@functools.lru_cache(maxsize=None)
def peaked_k(nb=B, nk_max=NK_MAX, nh=H):
    k = _signs((nb, nk_max + GUARD, nh * HEAD), SEED + 2)
    k[:, nk_max:] = 0
    return k


@functools.lru_cache(maxsize=None)
def peaked_v(nb=B, nk_max=NK_MAX, nh=H):
    j = torch.arange(nk_max + GUARD).view(-1, 1)
    c = torch.arange(HEAD).view(1, -1)
    plane = ((((j + 1) * (c + 3)) % 1021) - 510).double() / 256          # [rows][64]
    sign = 1.0 - 2.0 * ((torch.arange(nb).view(-1, 1) + torch.arange(nh).view(1, -1)) % 2).double()   # [nb][nh]
    v = (sign.view(nb, 1, nh, 1) * plane.view(1, -1, 1, HEAD)).reshape(nb, nk_max + GUARD, nh * HEAD).contiguous()
    v[:, nk_max:] = GUARD_V
    return v


def lo_halves(shape, which):
    """The lo halves of a pair run: +-2^-13; `which` names the operand."""
    return LO * _signs(tuple(shape), SEED + 11 + {"q": 0, "k": 1, "v": 2}[which])


def live_counts(nq, nk, causal, counts=None, nb=B):
    """int64 [nb][nq]: keys that query row i of batch row b attends to"""
    base = torch.full((nb, 1), nk, dtype=torch.int64) if counts is None else torch.as_tensor(counts, dtype=torch.int64).view(nb, 1).clamp(1, nk)
    live = base.expand(nb, nq)
    if causal:
        live = torch.minimum(live, torch.arange(1, nq + 1).view(1, nq))
    return live.contiguous()


def targets(name, live):
    """The target key of every query row ([B][nq], as `live`). Works on any device (the GPU test builds Q from it there)."""
    i = torch.arange(live.shape[1], device=live.device).view(1, -1).expand_as(live)
    if name == "first":
        return torch.zeros_like(live)
    if name == "last":
        return live - 1
    assert name == "spread", name
    step = torch.where(live == 5, 3, 5)
    return (step * i + 3) % live


def peaked_q(k, t):
    """q [B][nq][H * 64] = 4 k[b, t[b, i]] (every head of a row aims at the same key index)"""
    return 4 * torch.gather(k, 1, t.unsqueeze(-1).expand(-1, -1, k.shape[-1]))


# ------------------------------------------------------------------------------- references
def _mutate_out(out, nh, mutate):
    if mutate == "swap_adjacent_queries":       # rows 2 m and 2 m + 1 change places (an odd last row stays)
        nq = out.shape[1]
        idx = torch.arange(nq) ^ 1
        idx[idx >= nq] = nq - 1
        return out[:, idx]
    if mutate == "next_head":                   # head h holds the result of head h + 1
        nb, nq, _ = out.shape
        return out.view(nb, nq, nh, HEAD).roll(-1, 2).reshape(nb, nq, nh * HEAD)
    return out


def _mutate_in(v, live, mutate):
    assert mutate is None or mutate in MUTATIONS, mutate
    if mutate == "drop_last_key":               # (a row with one key keeps it)
        live = torch.where(live > 1, live - 1, live)
    elif mutate == "admit_one_more":            # the first key past the row's mask: key nk, or key i + 1 under the causal mask
        live = live + 1
    elif mutate == "shift_v_by_one":            # key j is given the value row of key j + 1
        v = v.roll(-1, 1)
    return v, live


def affected(mutate, live):
    """bool [B][nq]: the rows that a mutation changes by construction"""
    nq = live.shape[1]
    if mutate == "drop_last_key":
        return live > 1
    if mutate == "swap_adjacent_queries":
        partner = (torch.arange(nq) ^ 1) < nq
        return partner.view(1, nq).expand_as(live) & (live.max() > 1)       # with one key every row is that key's value row
    return torch.ones_like(live, dtype=torch.bool)


def uniform_ref(v, nh, live, mutate=None):
    """Mean of v [B][rows][nh * 64] over the first live[b, i] keys: prefix sums (exact integers) over the count -> [B][nq][nh * 64]."""
    v, live = _mutate_in(v.double(), live, mutate)
    prefix = torch.cumsum(v, 1)
    out = torch.gather(prefix, 1, (live - 1).unsqueeze(-1).expand(-1, -1, v.shape[-1])) / live.unsqueeze(-1).double()
    return _mutate_out(out, nh, mutate)


def peaked_ref(q, k, v, nh, live, mutate=None):
    """float64 masked softmax attention, scale 1/8. Returns out [B][nq][nh * 64], the pre-softmax logits q.k / 8 [B][nh][nq][kmax] of EVERY key
    row below kmax = max(live) (masked or not: what a logit capture sees) and the probabilities (same shape)."""
    true_kmax = int(live.max())
    v, live = _mutate_in(v.double(), live, mutate)
    kmax = int(live.max())
    nb, nq, _ = q.shape
    qh = q.double().view(nb, nq, nh, HEAD).permute(0, 2, 1, 3)
    kh = k.double()[:, :kmax].reshape(nb, kmax, nh, HEAD).permute(0, 2, 3, 1)
    vh = v[:, :kmax].reshape(nb, kmax, nh, HEAD).permute(0, 2, 1, 3)
    logits = (qh @ kh) * SCALE
    dead = torch.arange(kmax).view(1, 1, 1, kmax) >= live.view(nb, 1, nq, 1)
    p = torch.softmax(logits.masked_fill(dead, float("-inf")), -1)
    out = (p @ vh).permute(0, 2, 1, 3).reshape(nb, nq, nh * HEAD)
    return _mutate_out(out, nh, mutate), logits[..., :true_kmax], p[..., :true_kmax]


def spacing_f16(x):
    """The distance between neighbouring f16 values at |x| (2^-24 below the smallest normal)."""
    x = x.double().abs()
    e = torch.frexp(x)[1]                           # |x| = m 2^e, m in [0.5, 1)
    return torch.where(x == 0, 2.0 ** -24, torch.pow(2.0, (e - 11).clamp(min=-24).double()))
