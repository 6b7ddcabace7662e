"""Prompted greedy decode on the MI355X (DecodingOptions(prompt=..., prefix=...), wca_decode's sot_index and prefill): the result against
the CPU oracle (oracle/decoding_ref.py) with the prompted initial tokens, the batched prefill against the one-position-at-a-time
path, the n_text_ctx + 1 length edge and a raw zero-default descriptor. Small dims, like the `small` fixture of test_decode_gpu.py."""
import ctypes as C
import glob
import importlib
import json

import numpy as np
import pytest
import torch

import decode_cache_ref as cref

pytestmark = pytest.mark.gpu

dref = importlib.import_module("oracle.decoding_ref")
wref = importlib.import_module("oracle.whisper_ref")


def _m(n):
    return importlib.import_module("whisper-char-alignment_amd." + n)


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("whisper-char-alignment_amd")


@pytest.fixture(scope="module")
def small(pkg):
    dims = pkg.ModelDimensions(80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)
    sd = _m("synthetic").random_state_dict(dims, seed=5)
    m = pkg.WhisperAMD(dims, device="cuda:0", max_batch=4, precision="f16")
    m.load_state_dict(sd)
    return m, sd, dims


@pytest.fixture(scope="module")
def tok():
    return _m("tokenizer").get_tokenizer(True, language="en", task="transcribe")


def _mel(m, seeds, n_samples=48000):
    syn, audio = _m("synthetic"), _m("audio")
    return torch.stack([audio.log_mel_spectrogram(audio.pad_or_trim(torch.from_numpy(syn.synth_audio(s, n_samples=n_samples))), 80, model=m)
                        for s in seeds]).cuda()


def _masks(tok, dims, without_timestamps=False):
    decoding = _m("decoding")
    opts = decoding.DecodingOptions(language="en", without_timestamps=without_timestamps)
    return decoding.filter_masks(tok, opts, dims.n_vocab)


def _score_vs_oracle(sd, dims, tok, mel, initial, rows, sup, n_steps, tol=0.05):
    """Teacher-force the oracle along the GPU's rows and require every GPU choice to survive the oracle's filters and be its
    argmax or lose to it by less than the f16 noise (test_greedy_decode_vs_oracle's scoring). Returns the fp32 oracle model."""
    ref = wref.WhisperRef({k: v.float() for k, v in sd.items()}, dims)
    filters = dref.make_filters(len(initial), tok.eot, tok.timestamp_begin, tok.no_timestamps,
                                [i for i in np.nonzero(sup)[0] if i != tok.no_timestamps], tok.encode(" "), True, 50)
    _, _, per_step = dref.greedy_decode(ref, mel.cpu(), initial, filters, tok.eot, n_steps, forced=torch.from_numpy(rows.astype(np.int64)))
    n_exact = n_total = 0
    for i, filt in enumerate(per_step):
        pos = len(initial) + i
        if pos >= rows.shape[1]:
            break
        for b in range(rows.shape[0]):
            if i > 0 and rows[b, pos - 1] == tok.eot:
                assert rows[b, pos] == tok.eot
                continue
            choice = int(rows[b, pos])
            assert torch.isfinite(filt[b, choice]), "GPU chose a token the oracle's filters removed (step %d row %d: %d)" % (i, b, choice)
            assert float(filt[b, choice]) >= float(filt[b].max()) - tol, (i, b, choice, float(filt[b, choice]), float(filt[b].max()))
            n_total += 1
            n_exact += int(choice == int(filt[b].argmax()))
    assert n_total >= rows.shape[0]
    assert n_exact >= 0.8 * n_total
    return ref


def test_prompted_decode_vs_oracle(pkg, small, tok, fake_vocab):
    """decode(prompt=[...]) through the batched prefill: results exclude the prompt, every step agrees with the oracle run on
    the prompted initial tokens, and no_speech_prob is read at sot_index (after the prompt), not at position 0."""
    m, sd, dims = small
    decoding = _m("decoding")
    B, sample_len = 2, 10
    mel = _mel(m, [3, 4])
    prompt = [tok.encode(c)[0] for c in "the quick brown fox jumps over a lazy dog"]
    opts = decoding.DecodingOptions(language="en", prompt=prompt, sample_len=sample_len, vocab_path=fake_vocab)
    res = decoding.decode(m, mel, opts)
    assert m.last_decode_positions()[0] == 1 + len(prompt) + 3   # the prefill ran over every initial token
    initial = [tok.sot_prev] + prompt + list(tok.sot_sequence)
    sot_index = initial.index(tok.sot)
    rows = np.full((B, len(initial) + sample_len), tok.eot, np.int32)
    for b, r in enumerate(res):
        assert len(r.tokens) <= sample_len and tok.sot_prev not in r.tokens and r.tokens[:1] != prompt[:1]
        rows[b, :len(initial)] = initial
        rows[b, len(initial):len(initial) + len(r.tokens)] = r.tokens
        assert r.tokens and tok.timestamp_begin <= r.tokens[0] <= tok.timestamp_begin + 50   # first-timestamp rules at sample_begin
    sup, _ = _masks(tok, dims)
    ref = _score_vs_oracle(sd, dims, tok, mel, initial, rows, sup, sample_len)
    logits = ref.decoder(torch.tensor([initial] * B), ref.encoder(mel.cpu()))[0]
    want = logits[:, sot_index].float().softmax(-1)[:, tok.no_speech].numpy()
    at0 = logits[:, 0].float().softmax(-1)[:, tok.no_speech].numpy()
    got = np.array([r.no_speech_prob for r in res])
    print("no_speech_prob: GPU %s, oracle at sot_index %s, oracle at position 0 %s" % (got, want, at0))
    assert np.allclose(got, want, rtol=0.05, atol=1e-9), (got, want)
    # the position matters: the GPU value is much closer to the oracle's at sot_index than the position-0 value is
    assert np.all(np.abs(got - want) < 0.25 * np.abs(at0 - want)), (got, want, at0)


def test_prefix_first_token_obeys_timestamp_rules(pkg, small, tok, fake_vocab):
    """A forced prefix: SuppressBlank and the first-timestamp rules apply at the first position AFTER it."""
    m, sd, dims = small
    decoding = _m("decoding")
    B, sample_len = 2, 4
    mel = _mel(m, [8, 9])
    prefix = [tok.timestamp_begin] + [tok.encode(c)[0] for c in " hello"]
    res = decoding.decode(m, mel, decoding.DecodingOptions(language="en", prefix=prefix, sample_len=sample_len, vocab_path=fake_vocab))
    initial = list(tok.sot_sequence) + prefix
    rows = np.full((B, len(initial) + sample_len), tok.eot, np.int32)
    for b, r in enumerate(res):
        assert r.tokens[:len(prefix)] != prefix
        assert r.tokens and tok.timestamp_begin <= r.tokens[0] <= tok.timestamp_begin + 50
        rows[b, :len(initial)] = initial
        rows[b, len(initial):len(initial) + len(r.tokens)] = r.tokens
    sup, _ = _masks(tok, dims)
    _score_vs_oracle(sd, dims, tok, mel, initial, rows, sup, sample_len)


def _decode(m, tok, dims, initial, sample_len, sot_index, prefill, mel=None, batch=None, sup=None, blank=None, rules=True):
    if sup is None:
        sup, blank = _masks(tok, dims)
    out = m.greedy_decode(mel, None, None, initial, sup, blank, sample_len=sample_len, eot=tok.eot, timestamp_begin=tok.timestamp_begin,
                          apply_timestamp_rules=rules, max_initial_timestamp_index=50, batch=batch, no_speech=tok.no_speech,
                          sot_index=sot_index, prefill=prefill)
    return out + (m.last_no_speech_prob.copy(), m.last_decode_positions())


def _raw_decode(m, tok, dims, mel, initial, sample_len):
    """One call of wca_decode through ctypes with every optional field of the descriptor left at zero: per_row 0, prefill 0, sot_index 0."""
    _lib = _m("_lib")
    sup, blank = _masks(tok, dims)
    B, T = mel.shape[0], len(initial) + sample_len
    toks, n_tok, lp, nsp = np.zeros((B, T), np.int32), np.zeros(B, np.int32), np.zeros(B, np.float32), np.zeros(B, np.float32)
    o = _lib.DecodeOpts(sample_len, tok.eot, tok.timestamp_begin, 1, 50, tok.no_speech)
    init, n_init, sot, sl = (_lib.i32_array(v) for v in (initial, [len(initial)], [0], [sample_len]))
    d = _lib.DecodeDesc(mel_dev=mel.data_ptr(), initial_tokens_host=C.addressof(init), n_initial_host=C.addressof(n_init),
                        sot_index_host=C.addressof(sot), sample_len_host=C.addressof(sl), suppress_mask_host=sup.ctypes.data,
                        blank_mask_host=blank.ctypes.data, opts=C.pointer(o), tokens_out_host=toks.ctypes.data, n_tokens_host=n_tok.ctypes.data,
                        sum_logprob_host=lp.ctypes.data, no_speech_prob_host=nsp.ctypes.data, batch=B)
    m._bind_stream()
    _lib.check(m._lib.wca_decode(m._h, C.byref(d)))
    return toks, n_tok, lp, nsp


@pytest.mark.parametrize("precision", ["f16", "reference"])
def test_prefill_matches_stepwise(pkg, tok, precision):
    """The same prompted batch with prefill 1 and 0, from an encode_batch state: identical
    rows except where the first divergence is a measured logit near-tie, log-probabilities and no_speech_prob within the
    summation noise, and the position counts show which path ran."""
    dims = pkg.ModelDimensions(80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)
    m = pkg.WhisperAMD(dims, device="cuda:0", max_batch=16, precision=precision)
    m.load_state_dict(_m("synthetic").random_state_dict(dims, seed=21))
    B, sample_len = 16, 8
    mel = _mel(m, range(100, 100 + B), n_samples=32000)
    prompt = [(37 * i) % 5000 + 200 for i in range(40)]
    initial = [tok.sot_prev] + prompt + list(tok.sot_sequence)
    sot_index = initial.index(tok.sot)
    out = {}
    for prefill in (1, 0):
        m.encode_batch(mel)
        out[prefill] = _decode(m, tok, dims, initial, sample_len, sot_index, prefill, batch=B)
    n_init = len(initial)
    tp, npf, lpp, nsp_p, pos_p = out[1]
    ts, nst, lps, nsp_s, pos_s = out[0]
    # the prefill fed every initial position at once (its first choice included), the stepwise path one at a time
    assert pos_p[0] == n_init and 0 <= pos_p[1] <= sample_len - 1, pos_p
    assert pos_s[0] == 0 and pos_s[1] >= n_init, pos_s
    same = np.array([np.array_equal(tp[b], ts[b]) and npf[b] == nst[b] for b in range(B)])
    assert same.mean() >= 0.75, same
    for b in np.nonzero(~same)[0]:
        p_ = int(np.nonzero(tp[b] != ts[b])[0][0])
        assert p_ >= n_init, (b, p_)
        _w, logits = m.get_attentions(mel[b:b + 1], torch.from_numpy(tp[b][:p_].astype(np.int64))[None].cuda(), [100], 3, 1.0)
        row = logits[0, p_ - 1].float().cpu().numpy()
        gap = abs(float(row[tp[b][p_]]) - float(row[ts[b][p_]]))
        print("prefill vs stepwise (%s): row %d diverges at %d: %d / %d, logit gap %.2e" % (precision, b, p_, tp[b][p_], ts[b][p_], gap))
        assert gap < 2e-2, (b, p_, gap)
    print("prefill vs stepwise (%s): %d/%d rows identical, max |d sum_logprob| %.2e, max |d no_speech| %.2e" % (
        precision, same.sum(), B, np.abs(lpp - lps)[same].max(), np.abs(nsp_p - nsp_s).max()))
    np.testing.assert_allclose(lpp[same], lps[same], rtol=1e-3, atol=1e-2)
    np.testing.assert_allclose(nsp_p, nsp_s, rtol=2e-2, atol=1e-7)


def test_length_edge_and_bounds(pkg, small, tok):
    """223 prompt tokens + sot sequence = 227 initial tokens with sample_len 224: at most 448 + 1 - 227 = 222 tokens are
    sampled; with EOT suppressed all of them are, and the decoder embeds positions up to 447 only (227 prefilled + 221 steps)."""
    m, sd, dims = small
    decoding = _m("decoding")
    opts = decoding.DecodingOptions(language="en", prompt=list(range(1000, 1300)))
    initial, sample_len, sot_index = decoding.decode_plan(tok, opts, dims.n_text_ctx)
    assert len(initial) == 227 and sample_len == 222
    mel = _mel(m, [30])
    sup = np.zeros(dims.n_vocab, np.uint8)
    sup[[tok.eot] + list(range(tok.sot, dims.n_vocab))] = 1   # only text tokens: the loop runs to the context limit
    toks, n_tok, lp, nsp, pos = _decode(m, tok, dims, initial, sample_len, sot_index, 1, mel=mel, sup=sup, blank=None, rules=False)
    assert toks.shape == (1, 449) and n_tok[0] == 449 and (toks[0, 227:] < tok.eot).all()
    assert pos == (227, 221) and pos[0] + pos[1] == dims.n_text_ctx
    assert np.isfinite(lp).all() and np.isfinite(nsp).all()
    # the 448 slots the run filled and the logits of its last forward (position 447) against float64, teacher-forced on the sampled tokens
    logits, cache = m.decode_state(1, 449)
    ref = cref.DecodeRef(sd, dims)
    K, V, x, _ = ref.forward(torch.from_numpy(toks[:, :448].astype(np.int64)), ref.cross_kv(ref.encoder(mel.cpu())))
    diff = (torch.from_numpy(cache.astype(np.float64))[:, :, :, :448] - torch.stack([K, V], 1)).abs()
    dl = float((torch.from_numpy(logits.astype(np.float64)) - ref.logits(x[:, 447])).abs().max())
    print("decode-cache measure length edge: plane0 %.3e plane_deep %.3e logits %.3e" % (float(diff[0].max()), float(diff[1:].max()), dl))
    assert float(diff[0].max()) <= cref.TOL["small_plane0"] and float(diff[1:].max()) <= cref.TOL["small_plane_deep"]
    assert dl <= cref.TOL["small_logits"], dl
    # the one length bound of every decode, n_initial + sample_len <= n_text_ctx + 1, through the Python method and the raw call
    with pytest.raises(_m("_lib").TooLongError):
        _decode(m, tok, dims, initial, sample_len + 1, sot_index, 1, mel=mel)
    with pytest.raises(_m("_lib").TooLongError):
        _decode(m, tok, dims, [tok.sot] * 449, 1, 0, 1, mel=mel)
    with pytest.raises(_m("_lib").TooLongError):
        _raw_decode(m, tok, dims, mel, list(tok.sot_sequence), 447)   # 3 + 447 = n_text_ctx + 2
    toks, n_tok, lp, nsp = _raw_decode(m, tok, dims, mel, list(tok.sot_sequence), 446)   # 3 + 446 = n_text_ctx + 1: not refused, and it runs
    assert toks.shape == (1, 449) and 3 <= n_tok[0] <= 449 and (toks[0, n_tok[0]:] == tok.eot).all() and np.isfinite(lp).all()
    with pytest.raises(_m("_lib").WcaError):
        _decode(m, tok, dims, initial, 8, len(initial), 1, mel=mel)   # sot_index outside the initial tokens


def test_raw_descriptor_matches_greedy_decode(pkg, small, tok):
    """A raw wca_decode_desc with every optional field zero and greedy_decode with its default sot_index and prefill give bit-identical
    results in all four outputs."""
    m, sd, dims = small
    mel = _mel(m, [50, 51, 52])
    initial = list(tok.sot_sequence)
    raw = _raw_decode(m, tok, dims, mel, initial, 12)
    pos = m.last_decode_positions()
    sup, blank = _masks(tok, dims)
    py = m.greedy_decode(mel, None, None, initial, sup, blank, sample_len=12, eot=tok.eot, timestamp_begin=tok.timestamp_begin,
                         apply_timestamp_rules=True, max_initial_timestamp_index=50, no_speech=tok.no_speech) + (m.last_no_speech_prob,)
    assert all(np.array_equal(a, b) for a, b in zip(raw, py))
    assert np.isfinite(raw[3]).all() and pos == m.last_decode_positions() and pos[0] == 0 and pos[1] >= len(initial)


def test_infer_ali_initial_prompt(tmp_path, fake_vocab):
    """--initial_prompt conditions the ASR pre-pass and is recorded in the result JSON; it needs --teacher asr."""
    import os
    pcm = np.load(os.path.join(os.path.dirname(__file__), "golden", "sample_pcm_int16.npy"))
    head = ("NIST_1A\n   1024\nsample_count -i %d\nsample_rate -i 16000\nchannel_count -i 1\nsample_n_bytes -i 2\n"
            "sample_byte_format -s2 01\nsample_coding -s3 pcm\nend_head\n" % len(pcm)).encode()
    (tmp_path / "utt0.wav").write_bytes(head + b" " * (1024 - len(head)) + pcm.astype("<i2").tobytes())
    step = len(pcm) // 4
    (tmp_path / "utt0.wrd").write_text("".join("%d %d %s\n" % (i * step, (i + 1) * step, w) for i, w in enumerate(["one", "two", "three"])))
    (tmp_path / "test.scp").write_text("utt0 %s\n" % (tmp_path / "utt0.wav"))
    infer = _m("infer_ali")
    base = ["--model", "tiny", "--random_init", "--dataset", "TIMIT", "--scp", str(tmp_path / "test.scp"), "--aggr", "topk", "--topk", "5",
            "--aligned_unit_type", "char", "--medfilt_width", "3", "--batch_size", "2", "--vocab", fake_vocab]
    prompt = "Cholmondeley, Featherstonehaugh and Marjoribanks."
    infer.infer_dataset(infer.parse_args(base + ["--output_dir", str(tmp_path / "out"), "--teacher", "asr", "--initial_prompt", prompt]))
    res = json.load(open(glob.glob(str(tmp_path / "out" / "*.json"))[0]))
    assert res["initial_prompt"] == prompt and res["teacher"] == "asr"
    with pytest.raises(SystemExit, match="teacher asr"):
        infer.infer_dataset(infer.parse_args(base + ["--output_dir", str(tmp_path / "x"), "--teacher", "text", "--initial_prompt", prompt]))
