"""Long-form transcribe on the MI355X: the whole-recording log-mel (wca_log_mel_long) against the CPU oracle's torch.stft
restatement, the window cut (wca_mel_window) bit for bit against torch slicing, and transcribe() end to end on the tiny
seeded model of tests/test_decode_gpu.py -- with the engine's own greedy decode (structure of the result) and with a
scripted decoder (the encoder-state reuse, max_frames and the offset arithmetic of the per-window alignment)."""
import importlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 2e-4   # tests/test_kernels_gpu.py::test_logmel_vs_oracle: direct-sum DFT against FFT on the (log10 + 4) / 4 scale


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("whisper-char-alignment_amd")


@pytest.fixture(scope="module")
def mods():
    names = ("audio", "synthetic", "decoding", "tokenizer", "transcribe", "timing", "retokenize", "_lib")
    return {n: importlib.import_module("whisper-char-alignment_amd." + n) for n in names}


@pytest.fixture(scope="module")
def small(pkg, mods):
    dims = pkg.ModelDimensions(80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)
    sd = mods["synthetic"].random_state_dict(dims, seed=5)
    m = pkg.WhisperAMD(dims, device="cuda:0", max_batch=4, precision="f16")
    m.load_state_dict(sd)
    return m


def _burst_audio(n):
    """Very quiet first 10 s, quiet noise after it, one loud burst in the last third only."""
    rng = np.random.default_rng(11)
    x = rng.standard_normal(n)
    amp = np.full(n, 5e-4)
    amp[:160000] = 5e-6
    amp[n - n // 6:n - n // 12] = 0.5
    return (x * amp).astype(np.float32)


def _inputs(mods):
    syn = mods["synthetic"]
    sample = np.load(os.path.join(os.path.dirname(__file__), "golden", "sample_pcm_int16.npy")).astype(np.float32) / 32768.0
    assert len(sample) == 46592
    rng = np.random.default_rng(3)
    return {"sample": sample, "30s": (0.05 * rng.standard_normal(480000)).astype(np.float32),
            "30s+1": (0.05 * rng.standard_normal(480001)).astype(np.float32), "burst": _burst_audio(1123457),
            "5min": syn.synth_audio(21, 16000 * 300 + 77)}


@pytest.mark.parametrize("precision", ["f16", "reference"])
def test_long_logmel_vs_oracle(small, mods, precision):
    from oracle import whisper_ref
    filt = mods["audio"].mel_filters(80)
    small.set_precision(precision)
    try:
        for name, pcm in _inputs(mods).items():
            n = len(pcm)
            got = small.log_mel_long(torch.from_numpy(pcm).cuda()).cpu()
            ref = whisper_ref.log_mel_spectrogram(F.pad(torch.from_numpy(pcm), (0, 480000)), filt)
            assert got.shape == ref.shape == (80, (n + 480000) // 160), name
            err = (got - ref).abs().max().item()
            print("long log-mel %s (%s, n=%d): max |d| = %.3g" % (name, precision, n, err))
            assert err < TOL, (name, precision, err)
            if name == "burst":
                # the floor is max - 8 over the WHOLE recording: the 30 s entry point, which floors its own window, must differ
                short = small.log_mel(torch.from_numpy(pcm[:480000]).cuda()).cpu()
                assert (got[:, :3000] - short).abs().max().item() > TOL
                assert (got[:, :990] - got[:, :990].min()).abs().max().item() == 0.0   # the very quiet part sits on the global floor
        same = mods["audio"].log_mel_spectrogram_long(_inputs(mods)["sample"], 80, model=small)
        assert torch.equal(same.cpu(), small.log_mel_long(torch.from_numpy(_inputs(mods)["sample"])).cpu())
    finally:
        small.set_precision("f16")


def test_long_logmel_honours_the_row_stride(small, mods):
    """The C entry point with ld > n_frames writes the rows at m * ld and leaves the columns beyond n_frames alone; ld < n_frames is refused."""
    import ctypes as C
    _lib = mods["_lib"]
    pcm = torch.from_numpy(_inputs(mods)["sample"]).cuda()
    T = (pcm.shape[0] + 480000) // 160
    want = small.log_mel_long(pcm)
    out = torch.full((80, T + 37), -7.0, device="cuda")
    nf = C.c_int64(0)
    small._bind_stream()
    _lib.check(small._lib.wca_log_mel_long(small._h, C.c_void_p(pcm.data_ptr()), pcm.shape[0], C.c_void_p(out.data_ptr()), T + 37, C.byref(nf)))
    torch.cuda.synchronize()
    assert nf.value == T and torch.equal(out[:, :T], want) and bool((out[:, T:] == -7.0).all())
    rc = small._lib.wca_log_mel_long(small._h, C.c_void_p(pcm.data_ptr()), pcm.shape[0], C.c_void_p(out.data_ptr()), T - 1, C.byref(nf))
    assert rc == -1 and nf.value == T
    assert small._lib.wca_log_mel_long(small._h, C.c_void_p(pcm.data_ptr()), -1, C.c_void_p(out.data_ptr()), T, None) == -1


def test_window_cut_is_bit_identical(small, mods):
    _lib = mods["_lib"]
    mel = small.log_mel_long(torch.from_numpy(_burst_audio(1123457)).cuda())
    T = mel.shape[1]
    assert T == 10021
    cases = [(0, 3000), (777, 3000), (100, 1), (6000, T - 3000 - 6000), (T - 3000, 3000), (T - 1, 1), (1234, 2999)]
    for seek, size in cases:
        want = F.pad(mel[:, seek:seek + size], (0, 3000 - size))
        got = small.mel_window(mel, seek, size)
        assert got.shape == (80, 3000) and torch.equal(got, want), (seek, size)
    got = small.mel_window(mel, [c[0] for c in cases], [c[1] for c in cases])   # more windows than max_batch: several calls
    want = torch.stack([F.pad(mel[:, s:s + z], (0, 3000 - z)) for s, z in cases])
    assert torch.equal(got, want)
    # a long mel with a row stride of its own
    wide = torch.zeros(80, T + 11, device="cuda")
    wide[:, :T] = mel
    assert torch.equal(small.mel_window(wide[:, :T], 777, 3000), mel[:, 777:3777])
    for seek, size in [(0, 0), (0, 3001), (T - 2999, 3000), (T, 1), (-1, 10), (T - 3000, 3001)]:
        with pytest.raises(_lib.WcaError) as exc:
            small.mel_window(mel, seek, size)
        assert exc.value.code == -1, (seek, size)


def _check_structure(res, n_samples):
    content_frames = n_samples // 160
    windows = res["windows"]
    seeks = [w["seek"] for w in windows]
    assert seeks[0] == 0 and all(b > a for a, b in zip(seeks, seeks[1:]))
    assert all(w2["seek"] == w["seek"] + w["advance"] for w, w2 in zip(windows, windows[1:]))
    assert windows[-1]["seek"] + windows[-1]["advance"] == content_frames
    by_seek = {w["seek"]: w for w in windows}
    n_words = 0
    for seg in res["segments"]:
        w = by_seek[seg["seek"]]
        t0 = w["seek"] * 0.01
        assert t0 - 1e-9 <= seg["start"] <= seg["end"] <= t0 + 30.0 + 1e-9
        words = seg["words"]
        n_words += len(words)
        for word in words:
            assert t0 - 1e-9 <= word["start"] <= word["end"] <= t0 + w["size"] * 0.01 + 1e-9
            for t in (word["start"], word["end"]):
                k = (t - t0) / 0.02
                assert abs(k - round(k)) < 1e-6
    for w in windows:   # words are ordered in time within a window
        ws = [word for seg in res["segments"] if seg["seek"] == w["seek"] for word in seg["words"]]
        starts = [word["start"] for word in ws]
        assert all(b >= a for a, b in zip(starts, starts[1:]))
        assert (len(ws) > 0) == w["aligned"]
    assert res["windows_without_words"] == sum(1 for w in windows if not w["skipped"] and not w["aligned"])
    return n_words


@pytest.mark.parametrize("precision", ["f16", "reference"])
def test_transcribe_end_to_end(small, mods, fake_vocab, precision):
    tr, decoding, timing, retok = mods["transcribe"], mods["decoding"], mods["timing"], mods["retokenize"]
    tk = mods["tokenizer"].get_tokenizer(True, language="en", task="transcribe", vocab_path=fake_vocab)
    n = 16000 * 70
    pcm = mods["synthetic"].synth_audio(5, n)
    small.set_precision(precision)
    try:
        # ---- the engine's own decode: random weights decode noise, so only the structure is checked
        res = small.transcribe(pcm, language="en", vocab_path=fake_vocab, word_timestamps=True, word_confidence=True, topk=4, sample_len=40)
        n_words = _check_structure(res, n)
        print("own decode (%s): %d windows, %d segments, %d words, %d windows without words" %
              (precision, len(res["windows"]), len(res["segments"]), n_words, res["windows_without_words"]))
        for seg in res["segments"]:
            for word in seg["words"]:
                assert 0.0 <= word["probability"] <= 1.0

        # ---- scripted decoder over the real decode: the tokens are fixed here, the encoder state is the one the real decode left behind
        ts = tk.timestamp_begin
        text_a, text_b, text_c = tk.encode(" hello tiny world again"), tk.encode(" some more words"), tk.encode(" dropped tail")
        closed = [ts, *text_a, ts + 700]                             # single closing timestamp: advance by the window
        inside = [ts + 10, *text_b, ts + 400, ts + 400, *text_c]     # ended inside speech: advance 800 frames, align text_b on 400 frames
        script = [closed, inside, closed, closed]
        calls = []

        def decode_window(mel_window, prompt):
            options = decoding.DecodingOptions(language="en", prompt=list(prompt) or None, vocab_path=fake_vocab, sample_len=8)
            real = decoding.decode(small, mel_window, options)
            calls.append(mel_window.clone())
            return decoding.DecodingResult(language="en", tokens=list(script[len(calls) - 1]), text="", avg_logprob=real.avg_logprob,
                                           no_speech_prob=real.no_speech_prob, temperature=0.0, compression_ratio=1.0)

        res = tr.transcribe(small, torch.from_numpy(pcm), language="en", vocab_path=fake_vocab, word_timestamps=True, no_speech_threshold=None,
                            topk=4, decode_window=decode_window)
        assert [(w["seek"], w["size"], w["max_frames"], w["aligned"]) for w in res["windows"]] == \
            [(0, 3000, 1500, True), (3000, 3000, 400, True), (3800, 3000, 1500, True), (6800, 200, 100, True)]
        assert _check_structure(res, n) > 0 and res["windows_without_words"] == 0
        opts = small.make_opts(aggregation="topk", topk=4, sot_len=len(tk.sot_sequence), medfilt_width=3)
        mel_long = small.log_mel_long(torch.from_numpy(pcm).cuda())
        for k, (w, kept) in enumerate(zip(res["windows"], (text_a, text_b, text_a, text_a))):
            window = small.mel_window(mel_long, w["seek"], w["size"])
            assert torch.equal(window, calls[k])
            text_tokens = retok.encode(retok.remove_punctuation(tk.decode(kept)), tk, "char")
            tokens = [*tk.sot_sequence, tk.no_timestamps, *text_tokens, tk.eot]
            small.encode_batch(mel=window[None])   # the same window encoded on its own
            jump, _sel = small.align_batch(None, None, torch.tensor([tokens], device="cuda"), [len(tokens)], [w["max_frames"]], opts)
            words, starts, ends = timing.words_from_jump_frames(jump[0], text_tokens, tk, "char")
            got = [word for seg in res["segments"] if seg["seek"] == w["seek"] for word in seg["words"]]
            assert [x["word"] for x in got] == list(words[:len(starts)]) and len(got) == len(starts) >= 2
            t0 = w["seek"] * 0.01
            frames = [(round((x["start"] - t0) / 0.02), round((x["end"] - t0) / 0.02)) for x in got]
            assert frames == [(round(a * 50), round(b * 50)) for a, b in zip(starts, ends)], (k, precision)
            assert all(x["start"] == t0 + float(a) and x["end"] == t0 + float(b) for x, a, b in zip(got, starts, ends))
            assert max(b for _, b in frames) <= w["max_frames"]
    finally:
        small.set_precision("f16")


def test_one_window_equals_decode(small, mods, fake_vocab):
    """A recording of at most 30 s: the first (and, when the decode closes the window, only) window's tokens are those of
    decoding.decode on mel_long[:, :3000]. A random-weight decode that runs out of sample_len after a timestamp pair has "ended inside
    speech", and the rules then open a second window at that pair; so several sample_len are run, the comparison with decode holds for
    each, and at least one of them must be a closed window with exactly one window in the result."""
    tr, decoding = mods["transcribe"], mods["decoding"]
    tk = mods["tokenizer"].get_tokenizer(True, language="en", task="transcribe", vocab_path=fake_vocab)
    single = 0
    for n, size in ((480000, 3000), (16000 * 20 + 80, 2000)):
        pcm = torch.from_numpy(mods["synthetic"].synth_audio(9, n))
        mel_long = small.log_mel_long(pcm.cuda())
        assert mel_long.shape[1] - 3000 == size
        window = mel_long[:, :3000].contiguous() if size == 3000 else small.mel_window(mel_long, 0, size)
        if size == 3000:
            assert torch.equal(small.mel_window(mel_long, 0, 3000), mel_long[:, :3000])
        for sample_len in (60, 24, 8, 3, 1):
            res = tr.transcribe(small, pcm, language="en", vocab_path=fake_vocab, no_speech_threshold=None, sample_len=sample_len)
            want = decoding.decode(small, window, decoding.DecodingOptions(language="en", vocab_path=fake_vocab, sample_len=sample_len))
            assert len(want.tokens) > 0
            segments, advance, _mf = tr.split_window(want.tokens, tk.timestamp_begin, tk.eot, 0, size, want, tk.decode)
            first = [s for s in res["segments"] if s["seek"] == 0]
            assert (res["windows"][0]["seek"], res["windows"][0]["size"], res["windows"][0]["advance"]) == (0, size, advance)
            assert [(s["start"], s["end"], s["text"], s["tokens"]) for s in first] == [(s["start"], s["end"], s["text"], s["tokens"]) for s in segments]
            assert first[0]["avg_logprob"] == want.avg_logprob and first[0]["no_speech_prob"] == want.no_speech_prob
            print("n=%d sample_len=%d: %d tokens, advance %d of %d, %d window(s)" % (n, sample_len, len(want.tokens), advance, size, len(res["windows"])))
            if advance == size:
                single += 1
                assert len(res["windows"]) == 1 and len(res["segments"]) == len(segments)
            else:
                assert res["windows"][1]["seek"] == advance
    assert single >= 2
