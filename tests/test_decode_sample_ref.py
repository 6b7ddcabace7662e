"""The float64 restatement of the sampler (tests/decode_sample_ref.py) on its own, without a GPU: Philox against the Random123 known
answers, the uniforms' exactness, and the law of the Gumbel-max draw against softmax(lg / T)."""
import numpy as np

import decode_sample_ref as R


def _hex(ws):
    return " ".join("%08x" % int(w) for w in ws)


def test_philox_known_answers():
    """Philox4x32-10, the Random123 vectors (kat_vectors: zeros, all ones, the digits of pi)."""
    f = 0xFFFFFFFF
    assert _hex(R.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(R.philox4x32_10((f, f, f, f), (f, f))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(R.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_philox_is_vectorised_over_the_counter():
    got = R.philox4x32_10((np.array([0, 0x243F6A88], np.uint64), np.array([0, 0x85A308D3], np.uint64), np.array([0, 0x13198A2E], np.uint64),
                           np.array([0, 0x03707344], np.uint64)), (0, 0))
    assert _hex(w[0] for w in got) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    # words(): token v reads word v & 3 of the call with counter (v >> 2, c, 0, 0) and the seed's two halves as the key
    seed, c = 0x299F31D0A4093822, 0x85A308D3
    w = R.words(seed, c, 11)
    for v in (0, 3, 4, 10):
        assert int(w[v]) == int(R.philox4x32_10((v >> 2, c, 0, 0), (0xA4093822, 0x299F31D0))[v & 3])
    assert w.shape == (11,)


def test_uniforms_are_exact_in_float32_and_inside_the_unit_interval():
    for x in (0, 0x1FF, 0x200, 0xFFFFFFFF):
        u = float(R.uniform(x))
        assert 0.0 < u < 1.0 and float(np.float32(u)) == u, (x, u)
        # the float32 arithmetic of the kernel gives the same number
        assert float((np.float32(x >> 9) + np.float32(0.5)) * np.float32(2.0 ** -23)) == u
        assert np.isfinite(R.gumbel(x))
    assert float(R.uniform(0)) == 2.0 ** -24 and float(R.uniform(0x1FF)) == 2.0 ** -24 and float(R.uniform(0x200)) == 1.5 * 2.0 ** -23
    assert float(R.uniform(0xFFFFFFFF)) == 1.0 - 2.0 ** -24
    # the 24-bit form the kernel does not use: (k + 0.5) 2^-24 with the largest k rounds to 1 in float32
    assert float(np.float32(0xFFFFFF) + np.float32(0.5)) * 2.0 ** -24 == 1.0


def test_the_draw_follows_softmax_of_the_tempered_logits():
    """8 live tokens among 40 (the others filtered out), 200 000 draws per temperature at consecutive counters of one seed: every
    token's count within 5 binomial standard deviations of softmax(lg / T). Deterministic: the seed is fixed."""
    V, n = 40, 200000
    live = np.array([1, 2, 5, 11, 17, 18, 30, 39])
    lg = np.full(V, -np.inf)
    lg[live] = np.array([2.0, 1.5, 0.0, -1.0, 1.0, 0.5, -2.0, 1.9])
    # all counters at once: noise [n, V] from words() of each counter
    groups = np.arange((V + 3) // 4, dtype=np.uint64)[None, :]
    counters = np.arange(n, dtype=np.uint64)[:, None]
    seed = 12345678901234567
    x = np.stack(R.philox4x32_10((groups, counters, 0, 0), (seed & 0xFFFFFFFF, seed >> 32)), axis=2).reshape(n, -1)[:, :V]
    assert np.array_equal(x[7], R.words(seed, 7, V))
    g = R.gumbel(x)
    for T in (0.5, 1.0):
        picks = np.argmax(np.where(np.isfinite(lg), lg / T + g, -np.inf), axis=1)
        assert set(picks.tolist()) <= set(live.tolist())
        p = np.exp(lg[live] / T - (lg[live] / T).max())
        p /= p.sum()
        counts = np.array([(picks == v).sum() for v in live])
        sd = np.sqrt(n * p * (1 - p))
        print("T = %.1f: counts %s, expected %s, deviations in sd %s" % (T, counts.tolist(), np.round(n * p).tolist(), np.round((counts - n * p) / sd, 2).tolist()))
        assert (np.abs(counts - n * p) <= 5 * sd).all()
        for c in (0, 1, 99):   # draw() is that argmax, one counter at a time
            assert R.draw(lg, T, seed, c)[0] == picks[c]
    # a very low temperature reproduces the argmax
    assert all(R.draw(lg, 0.01, seed, c)[0] == 1 for c in range(200))


def test_draw_reports_the_untempered_logprob_the_gap_and_the_margin():
    lg = np.full(12, -np.inf)
    lg[[2, 3, 7]] = [1.0, 3.0, -8.0]
    token, logprob, gap, margin = R.draw(lg, 0.7, 5, 3)
    lse = np.log(np.exp(1.0) + np.exp(3.0) + np.exp(-8.0))
    assert token in (2, 3, 7) and abs(logprob - (lg[token] - lse)) < 1e-12
    score = lg[[2, 3, 7]] / float(np.float32(0.7)) + R.gumbel(R.words(5, 3, 12))[[2, 3, 7]]
    top = np.sort(score)[::-1]
    assert abs(gap - (top[0] - top[1])) < 1e-12 and token == [2, 3, 7][int(np.argmax(score))]
    assert margin == 2.0 ** -20 * (1 + 8.0 / float(np.float32(0.7)))
    assert R.draw(np.full(5, -np.inf), 1.0, 0, 0)[0] is None
    # equal scores go to the lowest index: two tokens that share logit and noise cannot exist, so force it with one live token twice over
    one = np.full(4, -np.inf)
    one[2] = 0.5
    assert R.draw(one, 1.0, 9, 0)[:2] == (2, 0.0)
