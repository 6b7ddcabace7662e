"""Beam search and best_of end to end on the MI355X (C ABI wca_decode_group: grouped decoder rows that share an audio's cross-K/V, the beam
step, the cache reorder) on the `small` synthetic model of tests/test_decode_gpu.py.

  1. one beam is the greedy decode: token for token and with equal sum_logprob up to each row's first EOT (a grouped row's forward is a
     plain row's, bit for bit, so nothing is allowed here);
  2. the result of an audio does not depend on where in the batch it sits (beam and best_of);
  3. replay: the engine's choices, read from its trace, are scored step by step by the fp32 CPU oracle teacher-forced along the engine's
     own live beams -- an f16 forward cannot be token-exact against fp32 where two scores are closer than its noise, so every kept
     candidate must score within the stated tolerance of the oracle's G-th best, and the bulk must be the oracle's own choice;
  4. best_of: independent samples, the ranker's choice, and best_of = 1 is the plain sampled decode.
"""
import importlib

import numpy as np
import pytest
import torch

import beam_ref

pytestmark = pytest.mark.gpu

dref = importlib.import_module("oracle.decoding_ref")
wref = importlib.import_module("oracle.whisper_ref")


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("whisper-char-alignment_amd")


@pytest.fixture(scope="module")
def small(pkg):
    syn = importlib.import_module("whisper-char-alignment_amd.synthetic")
    dims = pkg.ModelDimensions(80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)
    sd = syn.random_state_dict(dims, seed=5)
    m = pkg.WhisperAMD(dims, device="cuda:0", max_batch=8, precision="f16")
    m.load_state_dict(sd)
    return m, sd, dims


@pytest.fixture(scope="module")
def setup(pkg, small):
    decoding = importlib.import_module("whisper-char-alignment_amd.decoding")
    tokmod = importlib.import_module("whisper-char-alignment_amd.tokenizer")
    tok = tokmod.get_tokenizer(True, language="en", task="transcribe")
    sup, blank = decoding.filter_masks(tok, decoding.DecodingOptions(language="en"), small[2].n_vocab)
    kw = dict(eot=tok.eot, timestamp_begin=tok.timestamp_begin, apply_timestamp_rules=True, max_initial_timestamp_index=50, no_speech=tok.no_speech)
    return decoding, tok, sup, blank, kw


def _mel(m, seeds, n_samples=48000):
    syn = importlib.import_module("whisper-char-alignment_amd.synthetic")
    audio = importlib.import_module("whisper-char-alignment_amd.audio")
    pcm = [syn.synth_audio(s, n_samples=n_samples) for s in seeds]
    return torch.stack([audio.log_mel_spectrogram(audio.pad_or_trim(torch.from_numpy(p)), 80, model=m) for p in pcm]).cuda()


def test_one_beam_is_the_greedy_decode(small, setup):
    m, _, dims = small
    decoding, tok, sup, blank, kw = setup
    B, sample_len = 3, 12
    mel = _mel(m, range(B))
    initial = [list(tok.sot_sequence)] * B
    gt, gn, glp = m.greedy_decode_rows(mel, None, None, initial, [0] * B, [sample_len] * B, sup, blank, **kw)
    nsp = m.last_no_speech_prob.copy()
    bt, bn, blp, n_out = m.decode_group(mel, None, None, initial, [0] * B, [sample_len] * B, sup, blank, n_group=1, mode=0, **kw)
    assert bt.shape == (B, 1, gt.shape[1]) and list(n_out) == [1] * B
    assert np.array_equal(m.last_no_speech_prob, nsp)
    for b in range(B):
        n = int(gn[b])   # the row's first sampled EOT (or its budget)
        assert int(bn[b, 0]) == n and np.array_equal(bt[b, 0, :n], gt[b, :n]), (b, n, bt[b, 0], gt[b])
        assert (bt[b, 0, n:] == tok.eot).all()
        assert blp[b, 0] == glp[b], (b, blp[b, 0], glp[b])


@pytest.mark.parametrize("mode", ["beam", "best_of"])
def test_swapping_the_audios_swaps_the_results(small, setup, mode):
    m, _, dims = small
    decoding, tok, sup, blank, kw = setup
    mel = _mel(m, [3, 4])
    initial = [list(tok.sot_sequence), [tok.sot_prev, 300, 301] + list(tok.sot_sequence)]   # the rows differ in their prompts too
    sot, sl, extra = [0, 3], [10, 8], {}
    if mode == "best_of":
        extra = dict(temperature=[0.7, 0.9], seed=[11, 22])
    order = [1, 0]
    a = m.decode_group(mel, None, None, initial, sot, sl, sup, blank, n_group=3, mode=0 if mode == "beam" else 1, **extra, **kw)
    nsp_a = m.last_no_speech_prob.copy()
    swapped = {k: [v[i] for i in order] for k, v in extra.items()}
    b = m.decode_group(mel[order].contiguous(), None, None, [initial[i] for i in order], [sot[i] for i in order], [sl[i] for i in order], sup,
                       blank, n_group=3, mode=0 if mode == "beam" else 1, **swapped, **kw)
    for x, y in zip(a, b):
        assert np.array_equal(x, y[order]), mode
    assert np.array_equal(nsp_a, m.last_no_speech_prob[order])
    assert (a[3] >= 1).all() and (a[1][:, 0] > np.array([len(r) for r in initial])).all()   # something was decoded


def _oracle_step(ref, xa, beams, sums, filters_for, G, first):
    """The oracle's view of one choice along the given live beams: candidate scores [G, V] (float64, -inf where filtered)."""
    tokens = torch.tensor(beams, dtype=torch.long)
    logits = ref.decoder(tokens, xa.expand(len(beams), -1, -1))[0][:, -1].float()
    filtered = logits.clone()
    for f in filters_for:
        f.apply(filtered, tokens)
    scores = np.stack([beam_ref.log_softmax(row) for row in filtered.double().numpy()]) + np.asarray(sums, dtype=np.float64)[:, None]
    if first:
        scores[1:] = -np.inf
    return logits.numpy(), scores


def test_replay_against_the_fp32_oracle(small, setup):
    m, sd, dims = small
    decoding, tok, sup, blank, kw = setup
    G, sample_len, tol = 3, 12, 0.05   # tol: the existing decode test's (logits are O(1); f16 operands perturb them by ~1e-2)
    ref = wref.WhisperRef({k: v.float() for k, v in sd.items()}, dims)
    initial = list(tok.sot_sequence)
    filters = dref.make_filters(len(initial), tok.eot, tok.timestamp_begin, tok.no_timestamps,
                                [i for i in np.nonzero(sup)[0] if i != tok.no_timestamps], tok.encode(" "), True, 50)
    for audio_seed in (0, 1, 2, 5):   # the first audio whose search reorders its beams often enough to test the cache reorder
        mel = _mel(m, [audio_seed])
        toks, n_tok, lp, n_out = m.decode_group(mel, None, None, [initial], [0], [sample_len], sup, blank, n_group=G, mode=0, **kw)
        trace = m.beam_trace()
        steps = trace.shape[0]
        moved = sum(1 for c in range(1, steps) if any(trace[c, r, 0] != r for r in range(G)))
        if moved >= 3:
            break
    assert moved >= 3 and trace.shape == (steps, G, 2) and steps >= 4, (moved, trace.shape)
    xa = ref.encoder(mel.cpu())
    beams, sums = [list(initial) for _ in range(G)], [0.0] * G
    n_kept = n_same = 0
    fed = None
    for c in range(steps):
        fed = [list(b) for b in beams]   # the rows of forward c
        logits, scores = _oracle_step(ref, xa, beams, sums, filters, G, c == 0)
        live = scores.copy()
        live[:, tok.eot] = -np.inf   # the next beams are the best G candidates that do not end the sequence
        flat = np.sort(live[np.isfinite(live)])[::-1]
        gth = flat[G - 1]
        own = {(int(i // scores.shape[1]), int(i % scores.shape[1])) for i in np.argsort(-live, axis=None, kind="stable")[:G]}
        nxt, nsum = [], []
        for r in range(G):
            src, t = int(trace[c, r, 0]), int(trace[c, r, 1])
            assert 0 <= src < G and t != tok.eot and np.isfinite(scores[src, t]), "the engine kept a candidate the oracle's filters removed (%d, %d, %d)" % (c, src, t)
            print("step %d beam %d: source %d token %d oracle score %.4f, oracle's G-th best %.4f" % (c, r, src, t, scores[src, t], gth))
            assert scores[src, t] >= gth - tol * (c + 1), (c, r, src, t, scores[src, t], gth)
            n_kept += 1
            n_same += (src, t) in own
            nxt.append(beams[src] + [t])
            nsum.append(scores[src, t])
        beams, sums = nxt, nsum
    assert n_same >= 0.8 * n_kept, (n_same, n_kept)
    # the last forward: its rows were the beams before the last choice, in the cache the reorder had arranged for them
    eng_logits, cache = m.decode_state(G, len(initial) + sample_len)
    want = ref.decoder(torch.tensor(fed, dtype=torch.long), xa.expand(G, -1, -1))[0][:, -1].float().numpy()
    diff = float(np.abs(eng_logits - want).max())
    print("last forward: max |engine logits - oracle logits| = %.4f over %d x %d" % (diff, G, want.shape[1]))
    assert diff <= tol, diff
    # and the results are those beams: nothing finished means the live beams, best first
    for i in range(int(n_out[0])):
        n = int(n_tok[0, i])
        assert n == len(initial) + sample_len or toks[0, i, n] == tok.eot
    if int(n_out[0]) == G and (n_tok[0, :G] == len(initial) + sample_len).all():
        for g in range(G):   # no sequence ended before the budget: the results are the live beams as the trace rebuilt them, best first
            assert [int(t) for t in toks[0, g, :n_tok[0, g]]] == beams[g] and lp[0, g] == pytest.approx(sums[g], abs=tol * steps)


def test_best_of_samples_and_the_ranker(small, setup):
    m, _, dims = small
    decoding, tok, sup, blank, kw = setup
    B, sample_len = 2, 10
    mel = _mel(m, [6, 7])
    initial = [list(tok.sot_sequence)] * B
    temps, seeds = [0.8, 0.8], [101, 202]
    t3, n3, lp3, out3 = m.decode_group(mel, None, None, initial, [0] * B, [sample_len] * B, sup, blank, n_group=3, mode=1, temperature=temps,
                                       seed=seeds, **kw)
    assert list(out3) == [3, 3]
    for b in range(B):
        rows = {tuple(t3[b, g, :n3[b, g]]) for g in range(3)}
        assert len(rows) == 3, "the samples of audio %d are not three different sequences" % b
    # sample g of audio b is the plain sampled decode of that audio with the seed group_seed(seed[b], g): six plain rows on the six
    # (audio, sample) pairs -- the same row count, so the same GEMM path, and a grouped row's forward is a plain row's bit for bit
    six = mel.repeat_interleave(3, dim=0).contiguous()
    pt, pn, plp = m.decode_rows_sampled(six, None, None, initial * 3, [0] * 6, [sample_len] * 6, sup, blank, temperature=[0.8] * 6,
                                        seed=[decoding.group_seed(s, g) for s in seeds for g in range(3)], **kw)
    assert np.array_equal(pt, t3.reshape(6, -1)) and np.array_equal(pn, n3.reshape(6)) and np.array_equal(plp, lp3.reshape(6))
    # best_of = 1 is the plain sampled decode
    t1, n1, lp1, _ = m.decode_group(mel, None, None, initial, [0] * B, [sample_len] * B, sup, blank, n_group=1, mode=1, temperature=temps, seed=seeds, **kw)
    qt, qn, qlp = m.decode_rows_sampled(mel, None, None, initial, [0] * B, [sample_len] * B, sup, blank, temperature=temps, seed=seeds, **kw)
    assert np.array_equal(t1[:, 0], qt) and np.array_equal(n1[:, 0], qn) and np.array_equal(lp1[:, 0], qlp)
    # decode(): the ranker's choice among the three, as DecodingResult
    opts = [decoding.DecodingOptions(language="en", sample_len=sample_len, temperature=0.8, seed=s, best_of=3) for s in seeds]
    res = decoding.decode(m, mel, opts, want_text=False)
    for b, r in enumerate(res):
        best = beam_ref.rank(lp3[b], n3[b] - len(initial[b]))
        assert r.tokens == [int(t) for t in t3[b, best, len(initial[b]):n3[b, best]]], b
        assert r.avg_logprob == pytest.approx(float(lp3[b, best]) / (len(r.tokens) + 1)) and r.temperature == 0.8
    one = decoding.decode(m, mel, [decoding.DecodingOptions(language="en", sample_len=sample_len, temperature=0.8, seed=s, best_of=1) for s in seeds],
                          want_text=False)
    plain = decoding.decode(m, mel, [decoding.DecodingOptions(language="en", sample_len=sample_len, temperature=0.8, seed=s) for s in seeds],
                            want_text=False)
    assert [(r.tokens, r.avg_logprob, r.temperature) for r in one] == [(r.tokens, r.avg_logprob, r.temperature) for r in plain]


def test_beam_decode_through_decoding_options(small, setup):
    """decode(DecodingOptions(beam_size=..., patience=..., length_penalty=...)): the ranked result of wca_decode_group, and what it refuses."""
    m, _, dims = small
    decoding, tok, sup, blank, kw = setup
    mel = _mel(m, [8, 9])
    o = decoding.DecodingOptions(language="en", sample_len=10, beam_size=3, patience=2.0, length_penalty=1.0)
    res = decoding.decode(m, mel, o, want_text=False)
    initial = [list(tok.sot_sequence)] * 2
    toks, n_tok, lp, n_out = m.decode_group(mel, None, None, initial, [0, 0], [10, 10], sup, blank, n_group=3, mode=0, max_candidates=6, **kw)
    assert toks.shape[1] == 6 and (n_out >= 3).all()
    for b, r in enumerate(res):
        best = beam_ref.rank(lp[b, :n_out[b]], n_tok[b, :n_out[b]] - 3, 1.0)
        assert r.tokens == [int(t) for t in toks[b, best, 3:n_tok[b, best]]] and r.temperature == 0.0
        assert r.avg_logprob == pytest.approx(float(lp[b, best]) / (len(r.tokens) + 1))
        assert np.isfinite(r.no_speech_prob)
    with pytest.raises(NotImplementedError, match="max_batch"):   # ten decoder rows on an engine of eight: a group is not split over calls
        decoding.decode(m, mel, decoding.DecodingOptions(language="en", beam_size=5))
    _lib = importlib.import_module("whisper-char-alignment_amd._lib")
    with pytest.raises(_lib.WcaError, match="max_batch"):
        m.decode_group(mel, None, None, initial, [0, 0], [10, 10], sup, blank, n_group=5, mode=0, **kw)
    with pytest.raises(_lib.WcaError, match="temperature"):
        m.decode_group(mel, None, None, initial, [0, 0], [10, 10], sup, blank, n_group=2, mode=1, **kw)
    with pytest.raises(_lib.WcaError, match="temperature"):
        m.decode_group(mel, None, None, initial, [0, 0], [10, 10], sup, blank, n_group=2, mode=0, temperature=[0.5, 0.5], seed=[1, 2], **kw)


def test_transcribe_with_beam_search_and_best_of_on_the_rungs(small, setup, fake_vocab, monkeypatch):
    """transcribe(beam_size=...) on a two-window recording: upstream's schema, the first window is decode()'s beam result; with a seed and a
    forced fallback the rung above 0 decodes the state again with best_of rows."""
    m, _, dims = small
    decoding, tok, sup, blank, kw = setup
    tr = importlib.import_module("whisper-char-alignment_amd.transcribe")
    syn = importlib.import_module("whisper-char-alignment_amd.synthetic")
    n = 16000 * 40
    pcm = torch.from_numpy(syn.synth_audio(5, n))
    res = tr.transcribe(m, pcm, language="en", vocab_path=fake_vocab, beam_size=3, patience=1.0, sample_len=16, no_speech_threshold=None)
    assert {"text", "segments", "language", "windows"} <= set(res) and res["language"] == "en" and len(res["windows"]) >= 2
    assert res["windows"][-1]["seek"] + res["windows"][-1]["advance"] == n // 160
    for seg in res["segments"]:
        assert {"id", "seek", "start", "end", "text", "tokens", "temperature", "avg_logprob", "compression_ratio", "no_speech_prob"} <= set(seg)
        assert seg["temperature"] == 0.0 and seg["start"] <= seg["end"]
    window = m.mel_window(m.log_mel_long(pcm.cuda()), 0, 3000)
    want = decoding.decode(m, window, decoding.DecodingOptions(language="en", vocab_path=fake_vocab, sample_len=16, beam_size=3, patience=1.0))
    first = [s for s in res["segments"] if s["seek"] == 0]
    assert first and first[0]["avg_logprob"] == want.avg_logprob and first[0]["no_speech_prob"] == want.no_speech_prob
    assert [t for s in first for t in s["tokens"]] == [t for t in want.tokens if t != tok.eot][:sum(len(s["tokens"]) for s in first)]
    # ---- the ladder: every window fails at temperature 0 (no average log-probability reaches 0) and is decoded again at 0.6
    calls, real = [], m.decode_group

    def spy(*a, **k):
        calls.append((k["n_group"], k["mode"], bool(k.get("redecode"))))
        return real(*a, **k)

    monkeypatch.setattr(m, "decode_group", spy)
    res = tr.transcribe(m, pcm, language="en", vocab_path=fake_vocab, beam_size=3, best_of=2, seed=7, temperature=(0.0, 0.6), logprob_threshold=0.0,
                        compression_ratio_threshold=None, no_speech_threshold=None, sample_len=16)
    assert (3, 0, False) in calls and (2, 1, True) in calls and len(calls) == 2 * len(res["windows"])
    assert res["segments"] and all(seg["temperature"] == 0.6 for seg in res["segments"])
