"""Float64 restatement of the decode step's sampler (csrc/decode.hip, decode_select_kernel<ROWS, SAMPLE>; test infrastructure only).

Upstream's GreedyDecoder.update at temperature T > 0 draws Categorical(logits = filtered / T) and accumulates the UNTEMPERED
log_softmax(filtered)[token]. The engine draws by Gumbel-max, next = argmax_v (lg[v] / T + G(v)) with the lowest index among equals, over
noise that is a pure function of (seed, sampled count c, token v):
    x(v) = word v & 3 of Philox4x32-10(counter = (v >> 2, c, 0, 0), key = (seed & 0xffffffff, seed >> 32))
    u(v) = ((x >> 9) + 0.5) * 2^-23          exact in float32, strictly inside (0, 1)
    G(v) = -log(-log(u))
Everything here is numpy integers and float64; the filters are oracle/decoding_ref.py's."""
import numpy as np
import torch

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two -> the four output words as uint64 arrays holding 32-bit values."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]   # 32 x 32 -> 64 bits: exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def uniform(x):
    """u of a 32-bit word, float64 (every value is a float32)."""
    return ((np.asarray(x, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel(x):
    return -np.log(-np.log(uniform(x)))


def words(seed, c, n_vocab):
    """x(v) for v < n_vocab: the Philox word of every token at sampled count c."""
    seed = int(seed) % (1 << 64)
    groups = np.arange((n_vocab + 3) // 4, dtype=np.uint64)
    out = philox4x32_10((groups, int(c), 0, 0), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(out, axis=1).reshape(-1)[:n_vocab]


def draw(filtered, temperature, seed, c):
    """Gumbel-max over one row of filtered logits (float64, -inf where a filter removed the token) ->
    (token, untempered log-probability, gap between the two best perturbed scores, margin). token is None when nothing survived.
    margin = 2^-20 (1 + max|lg| / T): what fp32 may move a perturbed score by, generously (two roundings in lg * (1 / T), two logf of at
    most 2 ulp, one add: a few 2^-24 of the largest term). A float32 implementation must pick `token` unless gap < margin."""
    lg = np.asarray(filtered, dtype=np.float64)
    live = np.isfinite(lg)
    if not live.any():
        return None, -np.inf, np.inf, 0.0
    t = float(np.float32(temperature))
    score = np.where(live, lg / t + gumbel(words(seed, c, lg.shape[0])), -np.inf)
    token = int(np.argmax(score))   # the first among equals
    rest = score.copy()
    rest[token] = -np.inf
    gap = float(score[token] - rest.max())
    m = lg[live].max()
    logprob = float(lg[token] - m - np.log(np.exp(lg[live] - m).sum()))
    return token, logprob, gap, 2.0 ** -20 * (1.0 + float(np.abs(lg[live]).max()) / t)


def filtered_row(logits_row, tokens_row, filters):
    """oracle/decoding_ref.py's filters on one row (logits [V], the tokens the row holds) -> float64 [V]."""
    lg = torch.as_tensor(np.asarray(logits_row, dtype=np.float64))[None].clone()
    toks = torch.as_tensor(np.asarray(tokens_row, dtype=np.int64))[None]
    for f in filters:
        f.apply(lg, toks)
    return lg[0].numpy()


def sample_step(logits_row, tokens_row, filters, n_initial, temperature, seed):
    """One step of one row: the filters, then the draw with c = the tokens the row has sampled so far. draw()'s four values."""
    return draw(filtered_row(logits_row, tokens_row, filters), temperature, seed, len(tokens_row) - n_initial)
