"""CPU tests of transcribe_batch (whisper-char-alignment_amd/transcribe.py): several recordings in lock-step against scripted
decoders. Every recording's result must be what transcribe() gives for it alone; the decode batch shrinks as recordings end, every
row carries its own previous text as the prompt, and more recordings than max_batch go in groups. The GPU side is
tests/test_transcribe_batch_gpu.py."""
import ctypes
import importlib
import json
import struct

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def tr():
    return importlib.import_module("whisper-char-alignment_amd.transcribe")


@pytest.fixture(scope="module")
def decoding():
    return importlib.import_module("whisper-char-alignment_amd.decoding")


@pytest.fixture(scope="module")
def tok():
    return importlib.import_module("whisper-char-alignment_amd.tokenizer").get_tokenizer(True, language="en", task="transcribe")


def _result(decoding, tokens, avg_logprob=-0.3, no_speech_prob=0.1):
    return decoding.DecodingResult(language="en", tokens=list(tokens), text="", avg_logprob=avg_logprob, no_speech_prob=no_speech_prob,
                                   temperature=0.0, compression_ratio=1.0)


class _Model:
    """What transcribe / transcribe_batch ask of the engine without words: the long mel carries the recording's id in its first
    element and a window carries (id, seek, size), so a scripted decoder knows which recording and window it is looking at."""
    is_multilingual = True

    def __init__(self, max_batch):
        self.max_batch = max_batch

    def log_mel_long(self, pcm):
        mel = torch.zeros(80, (pcm.shape[0] + 480000) // 160)
        mel[0, 0] = float(pcm[0])
        return mel

    def mel_window(self, mel_long, seek, size):
        w = torch.zeros(80, 3000)
        w[0, :3] = torch.tensor([float(mel_long[0, 0]), float(seek), float(size)])
        return w


def _recording(rec_id, seconds):
    pcm = np.zeros(16000 * seconds, np.float32)
    pcm[0] = rec_id
    return pcm


class _Scripts:
    """Per recording a dict seek -> DecodingResult; plays them for single windows (decode_window) and batches (decode_windows) and
    records every call as a list of (recording id, seek, size, prompt)."""

    def __init__(self, scripts):
        self.scripts, self.calls = scripts, []

    def _one(self, window, prompt):
        rec, seek, size = (int(round(float(v))) for v in window[0, :3])
        return (rec, seek, size, list(prompt)), self.scripts[rec][seek]

    def decode_window(self, window, prompt):
        call, res = self._one(window, prompt)
        self.calls.append([call])
        return res

    def decode_windows(self, windows, prompts):
        assert windows.shape[0] == len(prompts)
        both = [self._one(w, p) for w, p in zip(windows, prompts)]
        self.calls.append([c for c, _ in both])
        return [r for _, r in both]


def _three(tok, decoding):
    ts, (a, b, c) = tok.timestamp_begin, [tok.encode(ch)[0] for ch in "abc"]
    w_pair_single = [ts, a, ts + 50, ts + 50, b, ts + 100]    # advances by the window
    w_inside = [ts, a, ts + 200, ts + 200, b, c]              # ends inside speech: advances to the pair (400 frames)
    w_plain = [ts, c, ts + 100]
    scripts = {
        1: {0: _result(decoding, w_pair_single)},                                                            # 20 s: one window
        2: {0: _result(decoding, w_plain), 3000: _result(decoding, w_plain, avg_logprob=-2.0, no_speech_prob=0.9),   # 70 s: the second window is skipped
            6000: _result(decoding, [ts, a, b, ts + 30])},
        3: {0: _result(decoding, w_inside), 400: _result(decoding, w_pair_single), 3400: _result(decoding, w_plain),   # 94 s: four windows
            6400: _result(decoding, [ts, b, ts + 10])},
    }
    return scripts, [_recording(1, 20), _recording(2, 70), _recording(3, 94)]


def test_batch_equals_each_recording_alone(tr, tok, decoding):
    scripts, audios = _three(tok, decoding)
    alone = [tr.transcribe(_Model(1), a, language="en", initial_prompt=[7, 8], decode_window=_Scripts(scripts).decode_window) for a in audios]
    s = _Scripts(scripts)
    got = tr.transcribe_batch(_Model(4), audios, language="en", initial_prompt=[7, 8], decode_windows=s.decode_windows)
    assert got == alone
    assert [w["skipped"] for w in got[1]["windows"]] == [False, True, False]
    assert [(w["seek"], w["advance"]) for w in got[2]["windows"]] == [(0, 400), (400, 3000), (3400, 3000), (6400, 3000)]
    # the batch handed to the decoder shrinks as recordings finish, and a finished recording is never decoded again
    assert [[c[0] for c in call] for call in s.calls] == [[1, 2, 3], [2, 3], [2, 3], [3]]
    assert [[c[1] for c in call] for call in s.calls] == [[0, 0, 0], [3000, 400], [6000, 3400], [6400]]
    # every recording's prompt is its own previous text (the skipped window adds nothing)
    prompts = {(c[0], c[1]): c[3] for call in s.calls for c in call}
    plain, inside, pair = scripts[2][0].tokens, scripts[3][0].tokens, scripts[3][400].tokens
    assert prompts[(1, 0)] == prompts[(2, 0)] == prompts[(3, 0)] == [7, 8]
    assert prompts[(2, 3000)] == prompts[(2, 6000)] == [7, 8] + plain
    assert prompts[(3, 400)] == [7, 8] + inside[:3] and prompts[(3, 3400)] == [7, 8] + inside[:3] + pair
    assert prompts[(3, 6400)] == [7, 8] + inside[:3] + pair + scripts[3][3400].tokens


def test_without_conditioning_every_row_gets_the_bare_start(tr, tok, decoding):
    scripts, audios = _three(tok, decoding)
    s = _Scripts(scripts)
    got = tr.transcribe_batch(_Model(4), audios, language="en", condition_on_previous_text=False, decode_windows=s.decode_windows)
    assert all(c[3] == [] for call in s.calls for c in call)
    alone = [tr.transcribe(_Model(1), a, language="en", condition_on_previous_text=False, decode_window=_Scripts(scripts).decode_window)
             for a in audios]
    assert got == alone


def test_bare_start_reaches_the_decoder_as_the_sot_sequence(tr, tok, decoding, monkeypatch):
    """Through the real decode_windows: with condition_on_previous_text=False every row's DecodingOptions has no prompt, so its plan is
    the bare start-of-transcript sequence."""
    scripts, audios = _three(tok, decoding)
    seen = []

    def fake_decode(model, mel, options, want_text=True, **kw):
        rows = options if isinstance(options, (list, tuple)) else [options]
        seen.append([decoding.decode_plan(tok, o, 448) for o in rows])
        mel = mel if mel.ndim == 3 else mel[None]
        out = [scripts[int(round(float(w[0, 0])))][int(round(float(w[0, 1])))] for w in mel]
        return out if isinstance(options, (list, tuple)) else out[0]

    monkeypatch.setattr(decoding, "decode", fake_decode)
    tr.transcribe_batch(_Model(4), audios, language="en", condition_on_previous_text=False)
    assert [len(r) for r in seen] == [3, 2, 2, 1]
    assert all(plan[0] == list(tok.sot_sequence) and plan[2] == 0 for r in seen for plan in r)
    seen.clear()
    tr.transcribe_batch(_Model(4), audios, language="en")
    assert seen[0][0][0] == list(tok.sot_sequence)
    plain = scripts[2][0].tokens
    assert seen[1][0][0] == [tok.sot_prev] + plain + list(tok.sot_sequence) and seen[1][0][2] == 1 + len(plain)


def test_more_recordings_than_max_batch_go_in_groups(tr, tok, decoding):
    scripts, audios = _three(tok, decoding)
    s = _Scripts(scripts)
    got = tr.transcribe_batch(_Model(2), audios, language="en", decode_windows=s.decode_windows)
    assert max(len(call) for call in s.calls) <= 2
    assert [[c[0] for c in call] for call in s.calls] == [[1, 2], [2], [2], [3], [3], [3], [3]]
    alone = [tr.transcribe(_Model(1), a, language="en", decode_window=_Scripts(scripts).decode_window) for a in audios]
    assert got == alone
    assert tr.transcribe_batch(_Model(2), [], language="en", decode_windows=s.decode_windows) == []


def test_refusals_match_transcribe(tr):
    with pytest.raises(NotImplementedError):
        tr.transcribe_batch(None, [np.zeros(16000, np.float32)], language="en", temperature=(0.0, 0.2))
    with pytest.raises(NotImplementedError):
        tr.transcribe_batch(None, [np.zeros(16000, np.float32)], language=None)
    with pytest.raises(ValueError, match="vocab"):
        tr.transcribe_batch(None, [np.zeros(16000, np.float32)], language="en", word_timestamps=True)


def test_decode_refuses_rows_that_differ_in_more_than_prompt_and_prefix(decoding):
    mel = torch.zeros(2, 80, 3000)
    with pytest.raises(ValueError, match="language"):
        decoding.decode(None, mel, [decoding.DecodingOptions(language="en"), decoding.DecodingOptions(language="de")])
    with pytest.raises(ValueError, match="sample_len"):
        decoding.decode(None, mel, [decoding.DecodingOptions(language="en", prompt=[5]), decoding.DecodingOptions(language="en", sample_len=9)])
    with pytest.raises(NotImplementedError):
        decoding.decode(None, mel, [decoding.DecodingOptions(language="en"), decoding.DecodingOptions(language="en", beam_size=5)])


class _WordModel:
    """The engine calls transcribe_batch makes WITH words, without a GPU: every row decodes to <|0.00|> hello world <|2.00|> and the
    aligner's jump frames are 0, 1, 2, ... The decode and the alignment of a round must see the same number of rows."""

    def __init__(self, dims, text_tokens, max_batch):
        self.dims, self.is_multilingual, self.device, self.max_batch = dims, True, torch.device("cpu"), max_batch
        self.text_tokens = list(text_tokens)
        self.decoded, self.aligned = [], []

    def log_mel_long(self, pcm):
        return torch.zeros(self.dims.n_mels, (pcm.shape[0] + 480000) // 160)

    def mel_window(self, mel_long, seek, size):
        return torch.zeros(self.dims.n_mels, 3000)

    def _out(self, B, initials, T, eot, timestamp_begin):
        out = [timestamp_begin] + self.text_tokens + [timestamp_begin + 100]
        toks = np.full((B, T), eot, np.int32)
        for b, init in enumerate(initials):
            toks[b, :len(init)] = init
            toks[b, len(init):len(init) + len(out)] = out
        self.last_no_speech_prob = np.full(B, 0.05, np.float32)
        return toks, np.array([len(i) + len(out) for i in initials], np.int32), np.full(B, -1.0, np.float32)

    def greedy_decode(self, mel, pcm, n_samples, initial, sup, blank, sample_len, eot, timestamp_begin, apply_timestamp_rules,
                      max_initial_timestamp_index, batch, no_speech, sot_index=0, prefill=0):
        self.decoded.append(batch)
        return self._out(batch, [list(initial)] * batch, len(initial) + sample_len, eot, timestamp_begin)

    def greedy_decode_rows(self, mel, pcm, n_samples, initial_tokens, sot_index, sample_len, sup, blank, eot, timestamp_begin,
                           apply_timestamp_rules, max_initial_timestamp_index, batch, no_speech):
        self.decoded.append(batch)
        return self._out(batch, initial_tokens, max(len(i) + s for i, s in zip(initial_tokens, sample_len)), eot, timestamp_begin)

    def make_opts(self, **kw):
        return kw

    def align_batch(self, pcm, n_samples, tokens, n_tok, max_frames, opts, enqueue_only=False, token_logprobs_vocab_end=None):
        assert pcm is None and n_samples is None and tokens.shape[0] == self.decoded[-1]
        self.aligned.append((list(n_tok), list(max_frames)))
        B, n = tokens.shape
        jump = np.tile(np.arange(n, dtype=np.int32), (B, 1))
        return (jump, None, np.full((B, n), np.log(0.5), np.float32)) if token_logprobs_vocab_end is not None else (jump, None)


def test_words_one_alignment_per_round(tr, wca, fake_vocab):
    tk = importlib.import_module("whisper-char-alignment_amd.tokenizer").get_tokenizer(True, language="en", task="transcribe", vocab_path=fake_vocab)
    dims = wca.ModelDimensions(80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)
    audios = [np.zeros(16000 * s, np.float32) for s in (70, 20, 40)]
    kw = dict(language="en", vocab_path=fake_vocab, word_timestamps=True, word_confidence=True)
    alone = [tr.transcribe(_WordModel(dims, tk.encode(" hello world"), 1), a, **kw) for a in audios]
    m = _WordModel(dims, tk.encode(" hello world"), 4)
    got = tr.transcribe_batch(m, audios, **kw)
    assert got == alone
    assert m.decoded == [3, 2, 1]
    n_framed = 3 + 1 + len("hello world") + 1
    # rows of one round have their own max_frames (size // 2): 30 s, 20 s and 30 s windows, then 30 s and 10 s, then 10 s
    assert m.aligned == [([n_framed] * 3, [1500, 1000, 1500]), ([n_framed] * 2, [1500, 500]), ([n_framed], [500])]
    assert all(len(seg["words"]) == 2 for res in got for seg in res["segments"])


class _ScriptedWordModel(_WordModel):
    """_WordModel with a scripted decoder: a window carries its seek, and script[seek] = (sampled tokens, sum_logprob, no_speech_prob).
    Records every engine call with its argument shapes."""

    def __init__(self, dims, script):
        super().__init__(dims, [], 1)
        self.script, self.calls = script, []

    def mel_window(self, mel_long, seek, size):
        self.calls.append(("mel_window", tuple(mel_long.shape), seek, size))
        w = torch.zeros(self.dims.n_mels, 3000)
        w[0, 0] = float(seek)
        return w

    def greedy_decode(self, mel, pcm, n_samples, initial, sup, blank, sample_len, eot, timestamp_begin, apply_timestamp_rules,
                      max_initial_timestamp_index, batch, no_speech, sot_index=0, prefill=0):
        out, sum_logprob, no_speech_prob = self.script[int(round(float(mel[0, 0, 0])))]
        self.calls.append(("greedy_decode", tuple(mel.shape), list(initial), sample_len, batch, sot_index, prefill))
        self.decoded.append(batch)
        toks = np.full((1, len(initial) + sample_len), eot, np.int32)
        toks[0, :len(initial)] = initial
        toks[0, len(initial):len(initial) + len(out)] = out
        self.last_no_speech_prob = np.full(1, no_speech_prob, np.float32)
        return toks, np.array([len(initial) + len(out)], np.int32), np.full(1, sum_logprob, np.float32)

    def align_batch(self, pcm, n_samples, tokens, n_tok, max_frames, opts, enqueue_only=False, token_logprobs_vocab_end=None):
        self.calls.append(("align_batch", tuple(tokens.shape), tokens.tolist(), list(n_tok), list(max_frames), token_logprobs_vocab_end))
        return super().align_batch(pcm, n_samples, tokens, n_tok, max_frames, opts, enqueue_only, token_logprobs_vocab_end)


@pytest.mark.parametrize("words", [False, True], ids=["segments", "words"])
@pytest.mark.parametrize("condition", [True, False], ids=["conditioned", "unconditioned"])
def test_transcribe_is_transcribe_batch_of_one(tr, wca, fake_vocab, condition, words):
    """94 s = four windows: one that ends inside speech (seek advances to its timestamp pair), one skipped as no speech, two plain
    ones. transcribe(x) and transcribe_batch([x])[0] give the same result dict and make the same engine calls with the same shapes."""
    tk = importlib.import_module("whisper-char-alignment_amd.tokenizer").get_tokenizer(True, language="en", task="transcribe", vocab_path=fake_vocab)
    dims = wca.ModelDimensions(80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)
    ts, hw = tk.timestamp_begin, tk.encode(" hello world")
    script = {0: ([ts, *hw, ts + 200, ts + 200, *hw], -1.0, 0.05),
              400: ([ts, *hw, ts + 100], -100.0, 0.9),
              3400: ([ts, *hw, ts + 100], -1.0, 0.05),
              6400: ([ts, *hw, ts + 50], -1.0, 0.05)}
    audio = np.zeros(16000 * 94, np.float32)
    kw = dict(language="en", vocab_path=fake_vocab, initial_prompt="abcd", condition_on_previous_text=condition, word_timestamps=words,
              word_confidence=words)
    one, many = _ScriptedWordModel(dims, script), _ScriptedWordModel(dims, script)
    res = tr.transcribe(one, audio, **kw)
    got = tr.transcribe_batch(many, [audio], **kw)
    assert len(got) == 1 and got[0] == res
    assert many.calls == one.calls
    assert [(w["seek"], w["advance"], w["skipped"]) for w in res["windows"]] == [(0, 400, False), (400, 3000, True), (3400, 3000, False),
                                                                                 (6400, 3000, False)]
    assert [w["max_frames"] for w in res["windows"]] == [200, None, 1500, 1500]
    assert [c[0] for c in one.calls].count("greedy_decode") == 4 and [c[0] for c in one.calls].count("align_batch") == (3 if words else 0)
    assert all(c[1] == (1, 80, 3000) and c[4] == 1 for c in one.calls if c[0] == "greedy_decode")
    prompts = [c[2][1:c[5]] if c[5] else [] for c in one.calls if c[0] == "greedy_decode"]
    first = [ts, *hw, ts + 200]
    assert prompts[0] == tk.encode(" abcd")
    assert prompts[1] == prompts[2] == (tk.encode(" abcd") + first if condition else [])
    assert all(len(seg["words"]) == (2 if words else 0) for seg in res["segments"]) and len(res["segments"]) == 3


def _write_wav(path, n):
    data = np.zeros(n, dtype="<i2").tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, 16000, 32000, 2, 16))
        f.write(b"data" + struct.pack("<I", len(data)) + data)


def test_cli_batch_flag_writes_one_json_per_recording(tr, wca, fake_vocab, tmp_path):
    tk = importlib.import_module("whisper-char-alignment_amd.tokenizer").get_tokenizer(True, language="en", task="transcribe", vocab_path=fake_vocab)
    for name, seconds in (("rec_a", 40), ("rec_b", 10), ("rec_c", 70)):
        _write_wav(tmp_path / (name + ".wav"), 16000 * seconds)
    scp = tmp_path / "list.scp"
    scp.write_text("".join("%s %s\n" % (i, tmp_path / (n + ".wav")) for i, n in (("first", "rec_a"), ("second", "rec_b"), ("third", "rec_c"))))
    base = ["--scp", str(scp), "--random_init", "--vocab", fake_vocab, "--word_timestamps"]
    assert tr.parse_args(base + ["--output_dir", "x"]).batch == 1
    args = tr.parse_args(base + ["--output_dir", str(tmp_path / "out"), "--batch", "2"])
    assert args.batch == 2
    dims = wca.ModelDimensions(80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)
    m = _WordModel(dims, tk.encode(" hello world"), 2)
    paths = tr.main(args, model=m)
    assert [p.split("/")[-1] for p in paths] == ["first.json", "second.json", "third.json"]
    assert m.decoded == [2, 1, 1, 1, 1]   # groups of two: (first, second), then third alone
    one = tr.main(tr.parse_args(base + ["--output_dir", str(tmp_path / "one")]), model=_WordModel(dims, tk.encode(" hello world"), 1))
    for p2, p1, n_windows in zip(paths, one, (2, 1, 3)):
        res = json.load(open(p2))
        assert res == json.load(open(p1)) and res["audio"].endswith(".wav") and len(res["windows"]) == n_windows
    with pytest.raises(SystemExit):
        tr.main(tr.parse_args(base + ["--output_dir", str(tmp_path / "out"), "--batch", "0"]), model=m)


def test_dropin_whisper_exports_transcribe_batch(tr):
    import os
    import sys
    dropin = os.path.join(os.path.dirname(os.path.abspath(tr.__file__)), "dropin")
    sys.path.insert(0, dropin)
    try:
        whisper = importlib.import_module("whisper")
        from whisper.transcribe import transcribe_batch as t2
        assert callable(whisper.transcribe_batch) and whisper.transcribe.transcribe_batch is t2
        with pytest.raises(NotImplementedError):
            whisper.transcribe_batch(None, [np.zeros(16000, np.float32)], language="en", temperature=0.2)
    finally:
        sys.path.remove(dropin)


def test_abi_mirror_of_the_rows_entry_points(wca):
    lib = wca._lib.load()
    assert lib.wca_version() >= 11
    assert lib.wca_decode(None, ctypes.byref(wca._lib.DecodeDesc())) < 0
    assert lib.wca_test_decode_select_rows(None, None, 1, 1, None, 2, None, None, None, 0, 1, None, None, None, None, None) < 0
    assert b"null" in lib.wca_last_error()
    assert lib.wca_test_attention_rows(None, None, None, None, None, 1, 1, 1, 1, None, 0) < 0 and b"null" in lib.wca_last_error()
