"""Greedy ASR pre-pass (reference infer_ali.py:40,60-61 `whisper.decode(..., DecodingOptions(language="en"))`)
on the MI355X, through the C ABI, against the CPU oracle (oracle/decoding_ref.py, a restatement of upstream decoding.py).

  * the per-step filter + greedy-update kernel is integer / index work on given fp32 logits: BIT-EXACT token choice,
    EOT latching and completion counts; the accumulated log-probability within 1e-4 (fp32 log-sum-exp order);
  * the full loop (encoder + KV-cached decoder in f16 operands / fp32 accumulate vs the fp32 oracle) cannot be
    token-exact by construction when two logits are closer than the f16 noise, so it is scored step by step: the
    oracle is teacher-forced along the GPU's tokens and every GPU choice must (a) never be a token the oracle's
    filters removed and (b) be the oracle's argmax, or lose to it by less than the stated logit tolerance.
"""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

dref = importlib.import_module("oracle.decoding_ref")
wref = importlib.import_module("oracle.whisper_ref")


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("whisper-char-alignment_amd")


@pytest.fixture(scope="module")
def small(pkg):
    syn = importlib.import_module("whisper-char-alignment_amd.synthetic")
    # tiny model, but the real multilingual vocabulary size so that every special-token id is meaningful
    dims = pkg.ModelDimensions(80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)
    sd = syn.random_state_dict(dims, seed=5)
    m = pkg.WhisperAMD(dims, device="cuda:0", max_batch=4, precision="f16")
    m.load_state_dict(sd)
    return m, sd, dims


def _setup(pkg, dims, without_timestamps=False):
    decoding = importlib.import_module("whisper-char-alignment_amd.decoding")
    tokmod = importlib.import_module("whisper-char-alignment_amd.tokenizer")
    tok = tokmod.get_tokenizer(True, language="en", task="transcribe")
    opts = decoding.DecodingOptions(language="en", without_timestamps=without_timestamps)
    sup, blank = decoding.filter_masks(tok, opts, dims.n_vocab)
    return decoding, tok, opts, sup, blank


@pytest.mark.parametrize("case", ["first", "text", "after_single_ts", "after_ts_pair", "ts_mass_wins", "finished_row", "no_ts_rules"])
def test_select_kernel_bit_exact(pkg, small, case):
    m, _, dims = small
    lib = m._lib
    _lib = importlib.import_module("whisper-char-alignment_amd._lib")
    decoding, tok, opts, sup, blank = _setup(pkg, dims, without_timestamps=(case == "no_ts_rules"))
    V, B, T_max = dims.n_vocab, 4, 40
    tsb, eot = tok.timestamp_begin, tok.eot
    initial = list(tok.sot_sequence) + ([tok.no_timestamps] if case == "no_ts_rules" else [])
    n_init = len(initial)
    g = torch.Generator().manual_seed(hash(case) % 1000)
    logits = torch.randn(B, V, generator=g) * 3.0
    hist = {
        "first": [],
        "no_ts_rules": [],
        "text": [tsb + 3, 400, 500],
        "after_single_ts": [tsb + 3, 400, 500, tsb + 10],
        "after_ts_pair": [tsb + 3, 400, tsb + 10, tsb + 10],
        "ts_mass_wins": [tsb + 3, 400, 500],
        "finished_row": [tsb + 3, 400, 500],
    }[case]
    rows = [list(initial) + list(hist) for _ in range(B)]
    if case == "finished_row":
        rows[1][-1] = eot  # row 1 already ended
        rows[2] = list(initial) + [tsb + 3, 400, eot]
    if case == "ts_mass_wins":
        logits[:, tsb:] += 4.0  # many moderately likely timestamps outweigh the best text token
    if case == "first":
        logits[0, tsb + 70] = 50.0  # beyond max_initial_timestamp: must not be chosen
        logits[1, 300] = 50.0       # text at the first position: must not be chosen
    cur_len = len(rows[0])
    tokens = torch.full((B, T_max), eot, dtype=torch.int32)
    for b in range(B):
        tokens[b, :cur_len] = torch.tensor(rows[b], dtype=torch.int32)
    # ---- oracle
    filters = dref.make_filters(n_init, eot, tsb, tok.no_timestamps, [i for i in np.nonzero(sup)[0] if i != tok.no_timestamps],
                                tok.encode(" "), apply_timestamp_rules=(case != "no_ts_rules"),
                                max_initial_timestamp_index=50)
    otok = torch.tensor(rows, dtype=torch.long)
    osum = torch.zeros(B)
    otok2, completed, _ = dref.select_step(logits, otok, osum, filters, eot)
    # ---- GPU kernel
    ld, td = logits.cuda(), tokens.cuda()
    supd = torch.from_numpy(sup).cuda()
    blankd = torch.from_numpy(blank).cuda()
    lpd = torch.zeros(B, device="cuda")
    nd = torch.zeros(T_max, dtype=torch.int32, device="cuda")
    o = _lib.DecodeOpts(224, eot, tsb, 0 if case == "no_ts_rules" else 1, 50)
    m._bind_stream()
    _lib.check(lib.wca_test_decode_select(m._h, _vp(ld), B, V, _vp(td), T_max, cur_len, n_init, _vp(supd), _vp(blankd), C.byref(o),
                                          _vp(lpd), _vp(nd)))
    torch.cuda.synchronize()
    got = td.cpu()[:, cur_len].long()
    assert torch.equal(got, otok2[:, -1]), (case, got, otok2[:, -1])
    assert int(nd.cpu()[cur_len]) == int((otok2[:, -1] == eot).sum())
    torch.testing.assert_close(lpd.cpu(), osum, rtol=1e-4, atol=1e-4)
    if case == "first":
        assert (got >= tsb).all() and (got <= tsb + 50).all()


def test_greedy_decode_vs_oracle(pkg, small):
    m, sd, dims = small
    syn = importlib.import_module("whisper-char-alignment_amd.synthetic")
    audio = importlib.import_module("whisper-char-alignment_amd.audio")
    decoding, tok, opts, sup, blank = _setup(pkg, dims)
    B, sample_len = 3, 12
    pcm = np.stack([syn.synth_audio(b, n_samples=48000) for b in range(B)])
    mel = torch.stack([audio.log_mel_spectrogram(audio.pad_or_trim(torch.from_numpy(p)), 80, model=m) for p in pcm]).cuda()
    initial = list(tok.sot_sequence)
    toks, n_tok, lps = m.greedy_decode(mel, None, None, initial, sup, blank, sample_len=sample_len, eot=tok.eot,
                                       timestamp_begin=tok.timestamp_begin, apply_timestamp_rules=True, max_initial_timestamp_index=50,
                                       no_speech=tok.no_speech)
    nsp = m.last_no_speech_prob.copy()
    assert toks.shape == (B, len(initial) + sample_len)
    assert (toks[:, :len(initial)] == np.array(initial)).all()
    # ---- oracle, teacher-forced along the GPU's choices
    ref = wref.WhisperRef({k: v.float() for k, v in sd.items()}, dims)
    filters = dref.make_filters(len(initial), tok.eot, tok.timestamp_begin, tok.no_timestamps,
                                [i for i in np.nonzero(sup)[0] if i != tok.no_timestamps], tok.encode(" "), True, 50)
    forced = torch.from_numpy(toks.astype(np.int64))
    _, _, per_step = dref.greedy_decode(ref, mel.cpu(), initial, filters, tok.eot, sample_len, forced=forced)
    # no_speech_prob: softmax of the UNFILTERED logits at the <|sot|> position (DecodingTask._main_loop, i == 0)
    sot_logits = ref.decoder(torch.tensor([initial] * B), ref.encoder(mel.cpu()))[0][:, 0]
    want_nsp = sot_logits.float().softmax(-1)[:, tok.no_speech].numpy()
    assert np.all(np.isfinite(nsp)) and np.allclose(nsp, want_nsp, rtol=0.05, atol=1e-9), (nsp, want_nsp)
    n_exact = n_total = 0
    tol = 0.05  # logits are O(1); f16 operands in a 2-layer model perturb them by ~1e-2
    for i, filt in enumerate(per_step):
        pos = len(initial) + i
        if pos >= toks.shape[1]:
            break
        for b in range(B):
            if i > 0 and toks[b, pos - 1] == tok.eot:
                assert toks[b, pos] == tok.eot  # EOT latches
                continue
            choice = int(toks[b, pos])
            assert torch.isfinite(filt[b, choice]), "GPU chose a token the oracle's filters removed (step %d row %d: %d)" % (i, b, choice)
            best = float(filt[b].max())
            assert float(filt[b, choice]) >= best - tol, (i, b, choice, float(filt[b, choice]), best)
            n_total += 1
            n_exact += int(choice == int(filt[b].argmax()))
    assert n_total >= B * 3
    assert n_exact >= 0.8 * n_total  # the bulk of the steps agree exactly
    # first sampled token is a timestamp <= 1.00 s, and timestamps never decrease
    assert ((toks[:, len(initial)] >= tok.timestamp_begin) & (toks[:, len(initial)] <= tok.timestamp_begin + 50)).all()
    for b in range(B):
        ts = [t for t in toks[b, len(initial):n_tok[b]] if t >= tok.timestamp_begin]
        assert all(x <= y for x, y in zip(ts, ts[1:]))


def test_decode_modes_agree(pkg):
    """wca_set_decode_mode: the few-row GEMM with LayerNorm prologue / KV append / split-K (fc2: K = 2048 -> 2 workgroups per
    column group) against the separate-launch path. Same arithmetic except the split-K summation order: the token rows must agree
    (up to argmax near-ties, bounded below)."""
    syn = importlib.import_module("whisper-char-alignment_amd.synthetic")
    dims = pkg.ModelDimensions(80, 1500, 512, 8, 2, 51865, 448, 512, 8, 2)
    m = pkg.WhisperAMD(dims, device="cuda:0", max_batch=20, precision="f16")
    m.load_state_dict(syn.random_state_dict(dims, seed=11))
    decoding, tok, opts, sup, blank = _setup(pkg, dims)
    B, sample_len = 20, 10
    pcm = torch.from_numpy(np.stack([syn.synth_audio(40 + b, n_samples=32000) for b in range(B)])).cuda()
    ns = np.full(B, 32000, np.int32)
    initial = list(tok.sot_sequence)
    out = {}
    for mode in ((False, 1), (True, 1)):
        m.set_decode_mode(*mode)
        out[mode] = m.greedy_decode(None, pcm, ns, initial, sup, blank, sample_len=sample_len, eot=tok.eot,
                                    timestamp_begin=tok.timestamp_begin, apply_timestamp_rules=True, max_initial_timestamp_index=50,
                                    no_speech=tok.no_speech) + (m.last_no_speech_prob.copy(),)
    m.set_decode_mode(True, 1)
    t1, n1, lp1, ns1 = out[(True, 1)]
    t0, n0, lp0, ns0 = out[(False, 1)]
    # separate launches vs the few-row kernel: the split-K summation order differs, so an argmax near-tie of these random-weight
    # logits may fall the other way in a row (and the row then continues differently): nearly all rows must be identical, and the
    # identical rows' log-probabilities agree to the summation noise; the first position (no_speech_prob) is computed before any choice
    same = np.array([np.array_equal(t0[b], t1[b]) and n0[b] == n1[b] for b in range(B)])
    assert same.mean() >= 0.8, same
    # ... and a differing row is excused ONLY by a measured near-tie: teacher-force the common prefix and require the two paths'
    # choices at the first divergent position to be within the summation noise of each other in the logits (a blanket
    # 20 % allowance would also hide a corrupted split-K workspace)
    for b in np.nonzero(~same)[0]:
        p_ = int(np.nonzero(t0[b] != t1[b])[0][0])
        assert p_ >= len(initial), (b, p_)   # the prompt is given
        mel = m.log_mel(pcm[b:b + 1])
        _w, logits = m.get_attentions(mel, torch.from_numpy(t0[b][:p_].astype(np.int64))[None].cuda(), [100], 3, 1.0)
        row = logits[0, p_ - 1].float().cpu().numpy()
        gap = abs(float(row[t0[b][p_]]) - float(row[t1[b][p_]]))
        print("decode modes: row %d diverges at position %d: tokens %d / %d, logit gap %.2e (|logits| max %.1f)" % (b, p_, t0[b][p_], t1[b][p_], gap, np.abs(row[np.isfinite(row)]).max()))
        assert gap < 1e-3, (b, p_, gap)
    np.testing.assert_allclose(lp0[same], lp1[same], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(ns0, ns1, rtol=1e-4, atol=1e-7)


def test_decode_stops_when_every_row_has_ended(pkg, small):
    """The loop's early exit (every row produced EOT; checked every 4 steps): with every token but EOT
    suppressed the first sampled token of every row is EOT, the rows report zero sampled tokens and the remaining positions
    are EOT-filled."""
    m, sd, dims = small
    syn = importlib.import_module("whisper-char-alignment_amd.synthetic")
    decoding, tok, opts, sup, blank = _setup(pkg, dims, without_timestamps=True)
    only_eot = np.ones(dims.n_vocab, np.uint8)
    only_eot[tok.eot] = 0
    B = 4
    pcm = torch.from_numpy(np.stack([syn.synth_audio(70 + b, n_samples=32000) for b in range(B)])).cuda()
    ns = np.full(B, 32000, np.int32)
    initial = list(tok.sot_sequence) + [tok.no_timestamps]
    toks, n_tok, lp = m.greedy_decode(None, pcm, ns, initial, only_eot, None, sample_len=40, eot=tok.eot,
                                      timestamp_begin=tok.timestamp_begin, apply_timestamp_rules=False, max_initial_timestamp_index=-1)
    assert (n_tok == len(initial)).all()
    assert (toks[:, len(initial):] == tok.eot).all()
    assert np.allclose(lp, 0.0, atol=1e-5)      # log-softmax over a single live token


def test_two_stream_decode_is_refused(pkg, small):
    """wca_set_decode_mode(e, 1, 2): the two-stream form of the loop was removed, so streams = 2 is WCA_ERR_INVALID -- and the refused
    call changes nothing: a 4-row batch decodes to the token rows of the decode made just before it."""
    m, sd, dims = small
    syn = importlib.import_module("whisper-char-alignment_amd.synthetic")
    decoding, tok, opts, sup, blank = _setup(pkg, dims)
    B = 4
    pcm = torch.from_numpy(np.stack([syn.synth_audio(70 + b, n_samples=32000) for b in range(B)])).cuda()
    ns = np.full(B, 32000, np.int32)

    def decode():
        return m.greedy_decode(None, pcm, ns, list(tok.sot_sequence), sup, blank, sample_len=8, eot=tok.eot, timestamp_begin=tok.timestamp_begin,
                               apply_timestamp_rules=True, max_initial_timestamp_index=50)

    toks0, n0, lp0 = decode()
    assert m._lib.wca_set_decode_mode(m._h, 1, 2) == -1   # WCA_ERR_INVALID
    assert b"removed" in m._lib.wca_last_error()
    with pytest.raises(pkg._lib.WcaError, match="removed"):
        m.set_decode_mode(True, 2)
    toks1, n1, lp1 = decode()
    assert np.array_equal(toks0, toks1) and np.array_equal(n0, n1) and np.array_equal(lp0, lp1)


def test_decode_api_and_encoder_reuse(pkg, small, fake_vocab):
    """whisper.decode mirror + the alignment that follows re-uses the encoder state (pcm=None) and gives the same
    jump frames as a from-scratch align_batch on the same tokens."""
    m, sd, dims = small
    syn = importlib.import_module("whisper-char-alignment_amd.synthetic")
    decoding, tok, opts, sup, blank = _setup(pkg, dims)
    B = 2
    pcm = np.stack([syn.synth_audio(10 + b, n_samples=64000) for b in range(B)]).astype(np.float32)
    pcm_d = torch.from_numpy(pcm).cuda()
    n_samples = [64000] * B
    res = decoding.decode(m, None, decoding.DecodingOptions(language="en", sample_len=8, vocab_path=fake_vocab), pcm=pcm_d,
                          n_samples=n_samples)
    assert len(res) == B and all(isinstance(r.text, str) for r in res)
    assert all(len(r.tokens) <= 8 for r in res)
    text_tokens = [tok.encode(c)[0] for c in "ab cd"]
    row = [*tok.sot_sequence, tok.no_timestamps, *text_tokens, tok.eot]
    tokens = torch.tensor([row] * B, dtype=torch.int64, device="cuda")
    o = m.make_opts(aggregation="topk", topk=3, sot_len=len(tok.sot_sequence), medfilt_width=3)
    jump_reuse, _ = m.align_batch(None, None, tokens, [len(row)] * B, [200] * B, o)
    jump_fresh, _ = m.align_batch(pcm_d, n_samples, tokens, [len(row)] * B, [200] * B, o)
    assert np.array_equal(jump_reuse, jump_fresh)
    with pytest.raises(Exception):
        m.align_batch(None, None, tokens, [len(row)] * B, [200] * B, o)  # the state was consumed


def test_decode_rejects_unsupported(pkg, small):
    m, _, dims = small
    decoding = importlib.import_module("whisper-char-alignment_amd.decoding")
    mel = torch.zeros(1, 80, 3000, device="cuda")
    with pytest.raises(NotImplementedError):
        decoding.decode(m, mel, decoding.DecodingOptions(language="en", beam_size=5))
    with pytest.raises(NotImplementedError):
        decoding.decode(m, mel, decoding.DecodingOptions(language=None))
    with pytest.raises(NotImplementedError):
        decoding.decode(m, mel, decoding.DecodingOptions(language="en", temperature=0.2))


def test_pipelined_encode_decode_align(pkg, small, fake_vocab):
    """Two-deep pipeline of the ASR flow: batch 1 is ENCODED (wca_encode_batch, first stream) before batch 0 is decoded
    and aligned (second stream). Tokens and jump frames must equal the one-batch-at-a-time results, and a third encode
    while both K/V slots are live is refused."""
    m, sd, dims = small
    syn = importlib.import_module("whisper-char-alignment_amd.synthetic")
    decoding, tok, opts, sup, blank = _setup(pkg, dims)
    B = 2
    batches = []
    for k in range(2):
        pcm = np.stack([syn.synth_audio(20 + 2 * k + b, n_samples=56000) for b in range(B)]).astype(np.float32)
        batches.append((torch.from_numpy(pcm).cuda(), [56000] * B))
    initial = list(tok.sot_sequence)
    kw = dict(sample_len=6, eot=tok.eot, timestamp_begin=tok.timestamp_begin, apply_timestamp_rules=True, max_initial_timestamp_index=50)
    text_tokens = [tok.encode(c)[0] for c in "ab cd"]
    row = [*tok.sot_sequence, tok.no_timestamps, *text_tokens, tok.eot]
    tokens = torch.tensor([row] * B, dtype=torch.int64, device="cuda")
    o = m.make_opts(aggregation="topk", topk=3, sot_len=len(tok.sot_sequence), medfilt_width=3)
    # ---- serial reference
    serial = []
    for pcm_d, ns in batches:
        t, n, lp = m.greedy_decode(None, pcm_d, ns, initial, sup, blank, **kw)
        j, _ = m.align_batch(None, None, tokens, [len(row)] * B, [170] * B, o)
        serial.append((t.copy(), n.copy(), j.copy()))
    # ---- pipelined
    m.encode_batch(pcm=batches[0][0], n_samples=batches[0][1])
    m.encode_batch(pcm=batches[1][0], n_samples=batches[1][1])
    with pytest.raises(Exception):
        m.encode_batch(pcm=batches[0][0], n_samples=batches[0][1])  # both slots hold undecoded / unconsumed states
    piped = []
    for k in range(2):
        t, n, lp = m.greedy_decode(None, None, None, initial, sup, blank, batch=B, **kw)
        j, _ = m.align_batch(None, None, tokens, [len(row)] * B, [170] * B, o)
        piped.append((t, n, j))
    for (t0, n0, j0), (t1, n1, j1) in zip(serial, piped):
        assert np.array_equal(t0, t1) and np.array_equal(n0, n1) and np.array_equal(j0, j1)
    # the ordinary path still works afterwards (slots were released by the fetches)
    j2, _ = m.align_batch(batches[0][0], batches[0][1], tokens, [len(row)] * B, [170] * B, o)
    assert np.array_equal(j2, serial[0][2])


def test_asr_flow_in_reference_precision_mode(pkg, small):
    """wca_set_precision(SPLIT) with the ASR pre-pass: the encoder and the cross-K/V run in split precision (rows [hi | lo]), the
    greedy decode itself computes in f16 on the hi halves (whisper.decode runs fp16 too), and the alignment that re-uses the state
    (pcm = NULL) runs in split precision. The decoded rows agree with the default mode's up to near-ties of the f16 logits, and the
    re-using alignment gives exactly the frames of a split-mode alignment from the PCM."""
    m, sd, dims = small
    syn = importlib.import_module("whisper-char-alignment_amd.synthetic")
    decoding, tok, opts, sup, blank = _setup(pkg, dims)
    B = 3
    pcm = torch.from_numpy(np.stack([syn.synth_audio(70 + b, n_samples=56000) for b in range(B)]).astype(np.float32)).cuda()
    ns = [56000] * B
    initial = list(tok.sot_sequence)
    kw = dict(sample_len=8, eot=tok.eot, timestamp_begin=tok.timestamp_begin, apply_timestamp_rules=True, max_initial_timestamp_index=50)
    text_tokens = [tok.encode(c)[0] for c in "ab cd ef"]
    row = [*tok.sot_sequence, tok.no_timestamps, *text_tokens, tok.eot]
    tokens = torch.tensor([row] * B, dtype=torch.int64, device="cuda")
    o = m.make_opts(aggregation="topk", topk=3, sot_len=len(tok.sot_sequence), medfilt_width=3)
    t16, n16, lp16 = m.greedy_decode(None, pcm, ns, initial, sup, blank, **kw)
    m.align_batch(None, None, tokens, [len(row)] * B, [170] * B, o)   # consume the state
    m.set_precision("split")
    try:
        ts, nsplit, lps = m.greedy_decode(None, pcm, ns, initial, sup, blank, **kw)
        j_reuse, sel_reuse = m.align_batch(None, None, tokens, [len(row)] * B, [170] * B, o)
        j_pcm, sel_pcm = m.align_batch(pcm, ns, tokens, [len(row)] * B, [170] * B, o)
        assert np.array_equal(j_reuse, j_pcm) and np.array_equal(sel_reuse, sel_pcm)
        assert ts.shape == t16.shape and (ts[:, :len(initial)] == np.array(initial)).all()
        agree = float(np.mean(ts == t16))
        assert agree >= 0.85, agree
        np.testing.assert_allclose(lps, lp16, rtol=0.1, atol=0.2)
    finally:
        m.set_precision("f16")
