"""Temperature sampling on the MI355X: the sampling form of the decode step (csrc/decode.hip, wca_test_decode_sample_rows) token for token
against the float64 restatement tests/decode_sample_ref.py; wca_decode with temperature_host / seed_host at temperature 0 against wca_decode with per_row 1, bit
for bit; draws that follow their seed and not their batch row; the sampled loop against the reference sampler fed the teacher-forced
logits; the re-decode of a resident encoder state; and transcribe's fallback ladder end to end on random weights. Small dims (the
`small` fixture of tests/test_decode_rows_gpu.py)."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import decode_sample_ref as R

pytestmark = pytest.mark.gpu

dref = importlib.import_module("oracle.decoding_ref")


def _m(n):
    return importlib.import_module("whisper-char-alignment_amd." + n)


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


@pytest.fixture(scope="module")
def tok():
    return _m("tokenizer").get_tokenizer(True, language="en", task="transcribe")


@pytest.fixture(scope="module")
def small():
    pkg = importlib.import_module("whisper-char-alignment_amd")
    dims = pkg.ModelDimensions(80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)
    m = pkg.WhisperAMD(dims, device="cuda:0", max_batch=4, precision="f16")
    m.load_state_dict(_m("synthetic").random_state_dict(dims, seed=5))
    return m, dims


@pytest.fixture(scope="module")
def mel4(small):
    syn, audio = _m("synthetic"), _m("audio")
    return torch.stack([audio.log_mel_spectrogram(audio.pad_or_trim(torch.from_numpy(syn.synth_audio(s, n_samples=48000))), 80, model=small[0])
                        for s in (3, 4, 8, 9)]).cuda()


def _masks(tok, dims):
    decoding = _m("decoding")
    return decoding.filter_masks(tok, decoding.DecodingOptions(language="en"), dims.n_vocab)


def _filters(tok, sup, n_initial):
    return dref.make_filters(n_initial, tok.eot, tok.timestamp_begin, tok.no_timestamps, [i for i in np.nonzero(sup)[0] if i != tok.no_timestamps],
                             tok.encode(" "), True, 50)


def _initial(tok, n):
    sot = list(tok.sot_sequence)
    if n == len(sot):
        return sot, 0
    prompt = [(37 * i) % 5000 + 200 for i in range(n - len(sot) - 1)]
    return [tok.sot_prev] + prompt + sot, 1 + len(prompt)


def _sample_rows(m, logits, tokens, cur_len, n_init, caps, sup, blank, o, lp0, temps, seeds, n_done_idx=5, n_done_len=8):
    """One launch of the sampling form -> (new token per row, sum_logprob [B] f32, n_done [n_done_len], the whole token matrix)."""
    _lib = _m("_lib")
    B, V = logits.shape
    td, lpd = tokens.clone().cuda(), lp0.clone().float().cuda()
    nd = torch.zeros(n_done_len, dtype=torch.int32, device="cuda")
    dev = [torch.tensor(v, dtype=torch.int32).cuda() for v in (cur_len, n_init, caps)]
    tdev = torch.tensor(temps, dtype=torch.float32).cuda()
    sdev = torch.from_numpy(np.array([s % 2 ** 64 for s in seeds], dtype=np.uint64).view(np.int64)).cuda()
    ld = logits.contiguous().cuda()
    m._bind_stream()
    _lib.check(m._lib.wca_test_decode_sample_rows(m._h, _vp(ld), B, V, _vp(td), tokens.shape[1], _vp(dev[0]), _vp(dev[1]), _vp(dev[2]), n_done_idx,
                                                  n_done_len, _vp(sup), _vp(blank), C.byref(o), _vp(lpd), _vp(nd), _vp(tdev), _vp(sdev)))
    torch.cuda.synchronize()
    got = td.cpu()
    return [int(got[b, cur_len[b]]) for b in range(B)], lpd.cpu().numpy(), nd.cpu().tolist(), got


def _history_rows(tok):
    """The six cases of test_select_rows_kernel_matches_single_row_calls, and two longer text rows for larger sampled counts."""
    tsb, eot = tok.timestamp_begin, tok.eot
    sot = list(tok.sot_sequence)
    prm = [tok.sot_prev, 400, 401]
    rows = [(sot, []),                                             # first sampled position
            (prm + sot, [tsb + 3, 400, 500]),                      # text
            (sot, [tsb + 3, 400, 500, tsb + 10]),                  # after a single timestamp
            (prm[:2] + sot, [tsb + 3, 400, tsb + 10, tsb + 10]),   # after a timestamp pair
            (sot, [tsb + 3, 400, eot]),                            # finished row
            (prm + sot, [tsb + 3, 400, 500]),                      # at its sample cap
            (sot, [tsb + 3] + [300 + i for i in range(8)]),        # text, 9 sampled so far
            (prm + sot, [tsb + 3] + [300 + i for i in range(29)])]  # text, 30 sampled so far
    return rows, [100, 100, 100, 100, 100, 3, 100, 100]


def test_sample_kernel_matches_the_float64_reference(small, tok):
    """Token for token. A case is excused only where the reference's two best perturbed scores are closer than the fp32 margin
    (decode_sample_ref.draw); at most 1 % of the cases may be, and the reference alone says how many before the GPU is looked at."""
    m, dims = small
    _lib = _m("_lib")
    sup, blank = _masks(tok, dims)
    supd, blankd = torch.from_numpy(sup).cuda(), torch.from_numpy(blank).cuda()
    V, T_max, eot, tsb = dims.n_vocab, 48, tok.eot, tok.timestamp_begin
    rows, caps = _history_rows(tok)
    B = len(rows)
    n_init = [len(i) for i, _ in rows]
    cur_len = [len(i) + len(h) for i, h in rows]
    assert sorted(set(c - n for c, n in zip(cur_len, n_init))) == [0, 3, 4, 9, 30]
    tokens = torch.full((B, T_max), eot, dtype=torch.int32)
    for b, (i, h) in enumerate(rows):
        tokens[b, :cur_len[b]] = torch.tensor(i + h, dtype=torch.int32)
    lp0 = torch.tensor([-1.5 * b for b in range(B)])
    o = _lib.DecodeOpts(224, eot, tsb, 1, 50)
    # ---- the reference first: every case's token, log-probability, gap and margin
    cases = []
    for k, (T, scale) in enumerate([(T, s) for T in (0.2, 0.6, 1.0) for s in (3.0, 10.0)]):
        logits = torch.randn(B, V, generator=torch.Generator().manual_seed(100 + k)) * scale
        logits[0, 300] = 50.0   # text at a first position: must not be drawn
        seeds = [0x1234567800000000 * k + 977 * b + 1 for b in range(B)]
        want = []
        for b in range(B):
            if b in (4, 5):   # finished / at its cap: <|endoftext|>, nothing added
                want.append((eot, 0.0, np.inf, 0.0))
            else:
                want.append(R.sample_step(logits[b].numpy(), tokens[b, :cur_len[b]].numpy(), _filters(tok, sup, n_init[b]), n_init[b], T, seeds[b]))
        cases.append((T, scale, logits, seeds, want))
    drawn = [(w[2], w[3]) for c in cases for b, w in enumerate(c[4]) if b not in (4, 5)]
    n_close = sum(gap < margin for gap, margin in drawn)
    print("sample kernel: %d drawn cases, %d with a reference gap below the margin; smallest gap / margin %.2f" % (
        len(drawn), n_close, min(gap / margin for gap, margin in drawn)))
    assert n_close <= 0.01 * len(drawn)
    # ---- the kernel
    n_excused = 0
    for T, scale, logits, seeds, want in cases:
        got_tok, got_lp, n_done, got = _sample_rows(m, logits, tokens, cur_len, n_init, caps, supd, blankd, o, lp0, [T] * B, seeds)
        for b in range(B):
            w_tok, w_lp, gap, margin = want[b]
            if got_tok[b] != w_tok:
                print("sample kernel T=%.1f scale %.0f row %d: token %d, reference %d, gap %.3e, margin %.3e" % (T, scale, b, got_tok[b], w_tok, gap, margin))
                assert gap < margin, (T, scale, b, got_tok[b], w_tok, gap, margin)
                n_excused += 1
                continue
            torch.testing.assert_close(torch.tensor(float(got_lp[b])), torch.tensor(float(lp0[b]) + w_lp, dtype=torch.float32), rtol=1e-4, atol=1e-4)
        assert tsb <= got_tok[0] <= tsb + 50 and got_tok[4] == eot and got_tok[5] == eot
        assert got_lp[4] == lp0[4].item() and got_lp[5] == lp0[5].item()
        assert n_done == [0, 0, 0, 0, 0, sum(t == eot for t in got_tok), 0, 0]
        for b in range(B):   # nothing but the new token was written
            assert torch.equal(got[b, :cur_len[b]], tokens[b, :cur_len[b]]) and (got[b, cur_len[b] + 1:] == eot).all()
    assert n_excused <= 0.01 * len(drawn), n_excused


@pytest.mark.parametrize("V", [3, 7, 64, 1027])
def test_sample_kernel_on_small_unaligned_vocabularies(small, V):
    """Unfiltered rows whose length is no multiple of four (a tail group of fewer than four tokens, rows that are not 16-byte aligned)
    and below the workgroup size: every temperature, several sampled counts."""
    m, _ = small
    _lib = _m("_lib")
    B, T_max = 6, 40
    temps = [0.2, 0.6, 1.0, 0.2, 0.6, 1.0]
    counts = [0, 1, 2, 5, 17, 38]
    seeds = [2 ** 63 + 11 * b + V for b in range(B)]
    logits = torch.randn(B, V, generator=torch.Generator().manual_seed(V)) * 3.0
    tokens = torch.zeros((B, T_max), dtype=torch.int32)   # token 0 everywhere: no row has ended (eot = V - 1)
    o = _lib.DecodeOpts(224, V - 1, V, 0, -1)            # no timestamps, no timestamp rules
    sup = torch.zeros(V, dtype=torch.uint8).cuda()
    want = [R.draw(logits[b].numpy().astype(np.float64), temps[b], seeds[b], counts[b]) for b in range(B)]
    assert all(gap >= margin for _, _, gap, margin in want), [(gap, margin) for _, _, gap, margin in want]
    got_tok, got_lp, n_done, _ = _sample_rows(m, logits, tokens, [1 + c for c in counts], [1] * B, [100] * B, sup, None, o, torch.zeros(B), temps, seeds)
    assert got_tok == [w[0] for w in want], (got_tok, want)
    np.testing.assert_allclose(got_lp, [w[1] for w in want], rtol=1e-4, atol=1e-4)
    assert n_done[5] == sum(t == V - 1 for t in got_tok)


def test_a_draw_follows_its_seed_not_its_row(small, tok):
    m, dims = small
    _lib = _m("_lib")
    sup, blank = _masks(tok, dims)
    supd, blankd = torch.from_numpy(sup).cuda(), torch.from_numpy(blank).cuda()
    V, T_max, eot, tsb = dims.n_vocab, 40, tok.eot, tok.timestamp_begin
    row = list(tok.sot_sequence) + [tsb + 3, 400, 500]
    tokens = torch.full((4, T_max), eot, dtype=torch.int32)
    tokens[:, :len(row)] = torch.tensor(row, dtype=torch.int32)
    logits = (torch.randn(1, V, generator=torch.Generator().manual_seed(31)) * 3.0).repeat(4, 1)
    o = _lib.DecodeOpts(224, eot, tsb, 1, 50)
    seeds = [5, 2 ** 40 + 5, 2 ** 64 - 1, 123456789]
    args = (m, logits, tokens, [len(row)] * 4, [3] * 4, [100] * 4, supd, blankd, o, torch.zeros(4), [1.0] * 4)
    tok_a, lp_a, _, _ = _sample_rows(*args, seeds)
    tok_b, lp_b, _, _ = _sample_rows(*args, seeds[::-1])
    tok_c, lp_c, _, _ = _sample_rows(*args, seeds)
    assert len(set(tok_a)) > 1, tok_a                      # the seeds matter
    assert tok_b == tok_a[::-1] and np.array_equal(lp_b.view(np.int32), lp_a[::-1].view(np.int32))
    assert tok_c == tok_a and np.array_equal(lp_c.view(np.int32), lp_a.view(np.int32))


def _sampled(m, tok, dims, mel, lengths, sample_len, temps, seeds, **kw):
    sup, blank = _masks(tok, dims)
    plans = [_initial(tok, n) for n in lengths]
    out = m.decode_rows_sampled(mel, None, None, [p[0] for p in plans], [p[1] for p in plans], [sample_len] * len(lengths), sup, blank, eot=tok.eot,
                                timestamp_begin=tok.timestamp_begin, apply_timestamp_rules=True, max_initial_timestamp_index=50,
                                no_speech=tok.no_speech, temperature=temps, seed=seeds, **kw)
    return out + (m.last_no_speech_prob.copy(),)


def test_temperature_0_is_the_greedy_decode_bit_for_bit(small, tok, mel4):
    m, dims = small
    sup, blank = _masks(tok, dims)
    lengths, S = (3, 5, 9, 17), 8
    plans = [_initial(tok, n) for n in lengths]
    greedy = m.greedy_decode_rows(mel4, None, None, [p[0] for p in plans], [p[1] for p in plans], [S] * 4, sup, blank, eot=tok.eot,
                                  timestamp_begin=tok.timestamp_begin, apply_timestamp_rules=True, max_initial_timestamp_index=50,
                                  no_speech=tok.no_speech) + (m.last_no_speech_prob.copy(),)
    zero = _sampled(m, tok, dims, mel4, lengths, S, [0.0] * 4, [1, 2, 3, 4])
    for a, b in zip(greedy, zero):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32)), (a, b)
    mixed = _sampled(m, tok, dims, mel4, lengths, S, [0.0, 0.8, 0.0, 0.8], [1, 2, 3, 4])
    for a, b in zip(greedy, mixed):
        assert np.array_equal(a[[0, 2]].view(np.int32), b[[0, 2]].view(np.int32)), (a, b)
    assert not np.array_equal(greedy[0][[1, 3]], mixed[0][[1, 3]])   # the sampled rows did sample
    for bad in ([0.0, -0.5, 0.0, 0.0], [0.0, float("nan"), 0.0, 0.0], [float("inf"), 0.0, 0.0, 0.0]):
        with pytest.raises(_m("_lib").WcaError, match="temperature"):
            _sampled(m, tok, dims, mel4, lengths, S, bad, [1, 2, 3, 4])


def test_the_sampled_loop_draws_what_the_reference_draws(small, tok, mel4):
    """4 rows, 12 sampled tokens at T = 0.7. Every row is replayed teacher-forced through get_attentions; at every sampled position the
    reference sampler, fed those logits and (seed, sampled count), must pick the row's token. The loop's logits and the replay's differ
    by fp32 summation order (the project's near-tie rule bounds that at 1e-3 per logit), so a miss is excused only where the
    reference's two best perturbed scores are closer than 2e-3 / T (either candidate's logit may move by 1e-3, scaled by 1 / T), a row
    is compared up to its first excused position, and at most 2 of the 48 positions may be excused. The log-probability: each step's
    log-softmax moves by at most twice the largest logit change, so |sum| <= S * 2 * 1e-3 + 1e-4, the bound of the greedy loop's test
    (tests/test_decode_cache_gpu.py, _check_choices) at that logit tolerance."""
    m, dims = small
    sup, _ = _masks(tok, dims)
    S, T, n_init = 12, 0.7, 3
    seeds = [101, 2 ** 33 + 7, 2 ** 64 - 5, 99991]
    toks, n_tok, lp, _ = _sampled(m, tok, dims, mel4, [n_init] * 4, S, [T] * 4, seeds)
    filters = _filters(tok, sup, n_init)
    n_excused = 0
    for b in range(4):
        _w, logits = m.get_attentions(mel4[b:b + 1], torch.from_numpy(toks[b:b + 1, :n_init + S - 1].astype(np.int64)).cuda(), [100], 3, 1.0)
        rows = logits[0].float().cpu().numpy().astype(np.float64)
        want_lp, whole = 0.0, True
        for i in range(S):
            pos = n_init + i
            if i > 0 and toks[b, pos - 1] == tok.eot:
                assert (toks[b, pos:] == tok.eot).all()
                break
            want, logprob, gap, _ = R.sample_step(rows[pos - 1], toks[b, :pos], filters, n_init, T, seeds[b])
            if int(toks[b, pos]) != want:
                print("sampled loop row %d position %d: token %d, reference %d, perturbed gap %.3e" % (b, i, toks[b, pos], want, gap))
                assert gap < 2e-3 / T, (b, i, int(toks[b, pos]), want, gap)
                n_excused += 1
                whole = False
                break
            want_lp += logprob
        if whole:
            n = int(n_tok[b]) - n_init
            print("sampled loop row %d: %d tokens, avg_logprob %.6f, reference %.6f" % (b, n, lp[b] / (n + 1), want_lp / (n + 1)))
            assert abs(float(lp[b]) - want_lp) <= S * 2 * 1e-3 + 1e-4, (b, float(lp[b]), want_lp)
    assert n_excused <= 2, n_excused
    # another seed, another text
    one = _sampled(m, tok, dims, mel4, [n_init] * 4, S, [1.0] * 4, [1, 2, 3, 4])[0]
    two = _sampled(m, tok, dims, mel4, [n_init] * 4, S, [1.0] * 4, [5, 6, 7, 8])[0]
    assert sum(not np.array_equal(one[b], two[b]) for b in range(4)) >= 1


def _brief(results):
    return [(r.tokens, r.avg_logprob, r.no_speech_prob, r.temperature) for r in results]


def test_redecode_runs_on_the_state_the_decode_left(small, tok, mel4):
    m, dims = small
    decoding, _lib = _m("decoding"), _m("_lib")
    rows = [decoding.DecodingOptions(language="en", sample_len=8, prompt=[300 + b] * (2 * b) or None) for b in range(4)]
    first = decoding.decode(m, mel4, rows, want_text=False)
    again = decoding.decode(m, None, rows, encoded_batch=4, want_text=False, redecode=True)
    assert _brief(again) == _brief(first)
    # the state is still there for the alignment, which gives what it gives after a single decode
    opts = _m("longform").aligner_options(m, tok, topk=4)
    text = [[tok.encode(ch)[0] for ch in s] for s in (" hello", " a b c", " hello world", " tiny")]   # (single bytes: no vocabulary file)
    token_rows = [[*tok.sot_sequence, tok.no_timestamps, *t, tok.eot] for t in text]
    tokens = _m("longform").pad_token_rows(token_rows, tok.eot).cuda()
    after_pair = m.align_batch(None, None, tokens, [len(r) for r in token_rows], [150] * 4, opts)
    decoding.decode(m, mel4, rows, want_text=False)
    after_one = m.align_batch(None, None, tokens, [len(r) for r in token_rows], [150] * 4, opts)
    assert np.array_equal(after_pair[0], after_one[0]) and np.array_equal(after_pair[1], after_one[1])
    # the alignment consumed the state: nothing is left to decode again; and a re-decode takes no input
    positions = m.last_decode_positions()
    with pytest.raises(_lib.WcaError) as err:
        decoding.decode(m, None, rows, encoded_batch=4, want_text=False, redecode=True)
    assert err.value.code == -4   # WCA_ERR_STATE
    with pytest.raises(_lib.WcaError) as err:
        _sampled(m, tok, dims, mel4, [3] * 4, 8, [0.0] * 4, [0] * 4, redecode=True)
    assert err.value.code == -1   # WCA_ERR_INVALID
    assert m.last_decode_positions() == positions   # neither call reached the loop
    with pytest.raises(ValueError):
        decoding.decode(m, mel4, rows, redecode=True)
    # a re-decode may sample: the rows of a ladder's later rung, one of them riding along for a single token
    decoding.decode(m, mel4, rows, want_text=False)
    rung = [decoding.DecodingOptions(language="en", sample_len=8, prompt=r.prompt, temperature=t, seed=s)
            for r, t, s in zip(rows, (0.0, 0.8, 0.8, 0.0), (None, 7, 8, None))]
    got = decoding.decode(m, None, rung, encoded_batch=4, want_text=False, redecode=True, row_sample_len=[1, None, None, None])
    assert [r.temperature for r in got] == [0.0, 0.8, 0.8, 0.0] and len(got[0].tokens) <= 1 and got[0].tokens == first[0].tokens[:1]
    assert _brief(got[3:]) == _brief(first[3:]) and [r.tokens for r in got[1:3]] != [r.tokens for r in first[1:3]]
    assert _brief(decoding.decode(m, None, rung, encoded_batch=4, want_text=False, redecode=True, row_sample_len=[1, None, None, None])) == _brief(got)


class _Log:
    """decoding.decode with every call's results written down."""

    def __init__(self, decoding):
        self.real, self.calls = decoding.decode, []

    def __call__(self, model, mel, options, **kw):
        res = self.real(model, mel, options, **kw)
        self.calls.append((kw.get("redecode", False), list(res) if isinstance(res, (list, tuple)) else [res]))
        return res


def test_the_ladder_end_to_end_on_random_weights(small, tok, monkeypatch):
    """20 s of synthetic audio, sample_len = 16. Random weights give an avg_logprob far below -1, so the default thresholds fall through
    every rung; with the thresholds off the ladder never leaves its first rung and the result is the one without a seed."""
    m, dims = small
    tr, decoding, syn = _m("transcribe"), _m("decoding"), _m("synthetic")
    audios = [syn.synth_audio(30 + i, 16000 * 20 + 40 * i) for i in range(2)]
    kw = dict(language="en", sample_len=16)
    ladder = dict(temperature=(0.0, 0.4, 0.8), seed=3)
    plain = tr.transcribe(m, audios[0], **kw)
    logs = []
    for pcm in audios:
        log = _Log(decoding)
        monkeypatch.setattr(decoding, "decode", log)
        logs.append((tr.transcribe(m, pcm, **kw, **ladder), log.calls))
        monkeypatch.setattr(decoding, "decode", log.real)
    first, calls = logs[0]
    assert first["segments"] and all(s["temperature"] == 0.8 for s in first["segments"])
    assert all(s["avg_logprob"] < -1.0 for s in first["segments"])
    assert [c[0] for c in calls] == [False, True, True]   # one encoder pass, two re-decodes
    assert tr.transcribe(m, audios[0], **kw, **ladder) == first
    assert tr.transcribe(m, audios[0], **kw, **ladder, logprob_threshold=None, compression_ratio_threshold=None) == plain
    assert tr.transcribe(m, audios[0], **kw, temperature=(0.0, 0.4, 0.8), seed=4) != first
    # two recordings in lock-step: the same temperatures, and each recording's draws are its own (window_seed knows no batch row)
    log = _Log(decoding)
    monkeypatch.setattr(decoding, "decode", log)
    batch = tr.transcribe_batch(m, audios, **kw, **ladder)
    monkeypatch.setattr(decoding, "decode", log.real)
    assert [c[0] for c in log.calls] == [False, True, True] and all(len(c[1]) == 2 for c in log.calls)
    for i, (alone, alone_calls) in enumerate(logs):
        assert [s["temperature"] for s in batch[i]["segments"]] == [s["temperature"] for s in alone["segments"]] == [0.8] * len(alone["segments"])
        a, b = alone_calls[-1][1][0].tokens, log.calls[-1][1][i].tokens   # the last rung's row, alone and in the batch
        if a == b:
            assert batch[i]["segments"] == alone["segments"]
            continue
        # the near-tie rule of tests/test_decode_rows_gpu.py: a teacher-forced logit gap below 1e-3 at the first divergent position
        p_ = next(k for k in range(max(len(a), len(b))) if k >= len(a) or k >= len(b) or a[k] != b[k])
        choice_a, choice_b = (a[p_] if p_ < len(a) else tok.eot), (b[p_] if p_ < len(b) else tok.eot)
        window = m.mel_window(m.log_mel_long(torch.from_numpy(audios[i]).cuda()), 0, 2000 + (40 * i) // 160)
        forced = torch.tensor([list(tok.sot_sequence) + a[:p_]], dtype=torch.int64).cuda()
        _w, logits = m.get_attentions(window[None], forced, [100], 3, 1.0)
        row = logits[0, -1].float().cpu().numpy()
        gap = abs(float(row[choice_a]) - float(row[choice_b]))
        print("ladder recording %d: rows diverge at sampled position %d: tokens %d / %d, teacher-forced logit gap %.3e" % (i, p_, choice_a, choice_b, gap))
        assert gap < 1e-3, (i, p_, gap)
