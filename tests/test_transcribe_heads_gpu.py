"""transcribe(word_timestamps=True, word_aligner="heads") on the MI355X, on the planted-ridge checkpoint of tests/test_align_long_gpu.py
(DTW row r peaks at encoder frame 5 r in head 0 of the upper decoder layer) with a scripted decoder over the real decode: the words join
to their segment's text, their times are word_timing's on the jump frames of align_batch(alignment_heads=True) called directly,
transcribe_batch of two recordings gives the single runs, and a call without the new keywords is the call with word_aligner="char"."""
import importlib
import json
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _m(n):
    return importlib.import_module("whisper-char-alignment_amd." + n)


@pytest.fixture(scope="module")
def planted(wca):
    dims = wca.ModelDimensions(80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)
    m = wca.WhisperAMD(dims, device="cuda:0", max_batch=4, precision="f16")
    m.load_state_dict(_m("synthetic").aligned_state_dict(dims, seed=5, frames_per_token=5.0))
    return m


@pytest.fixture(scope="module")
def tk(fake_vocab):
    return _m("tokenizer").get_tokenizer(True, language="en", task="transcribe", vocab_path=fake_vocab)


def _scripts(tk):
    """Two recordings: 38 s (two windows, the first with two segments) and 20 s (one window)."""
    ts = tk.timestamp_begin
    a = [[ts, *tk.encode(' Hello, "tiny" world.'), ts + 300, ts + 300, *tk.encode(" And (more) words again!"), ts + 700],
         [ts, *tk.encode(" Some more words, then."), ts + 300]]
    b = [[ts, *tk.encode(" Another one - short? Yes."), ts + 900]]
    return a, b


def _result(real, tokens):
    return _m("decoding").DecodingResult(language="en", tokens=list(tokens), text="", avg_logprob=real.avg_logprob, no_speech_prob=real.no_speech_prob,
                                         temperature=0.0, compression_ratio=1.0)


def _single(planted, fake_vocab, pcm, script, **kw):
    """transcribe() of one recording: the engine's real decode leaves the encoder state, the script gives the tokens."""
    decoding, calls = _m("decoding"), []

    def decode_window(mel_window, prompt):
        real = decoding.decode(planted, mel_window, decoding.DecodingOptions(language="en", prompt=list(prompt) or None, vocab_path=fake_vocab,
                                                                             sample_len=4))
        calls.append(1)
        return _result(real, script[len(calls) - 1])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)   # (the synthetic model has no official head table)
        return _m("transcribe").transcribe(planted, pcm, language="en", vocab_path=fake_vocab, word_timestamps=True, no_speech_threshold=None,
                                           topk=4, decode_window=decode_window, **kw)


def _words(res, seek=None):
    return [w for seg in res["segments"] if seek is None or seg["seek"] == seek for w in seg["words"]]


@pytest.fixture(scope="module")
def pcms():
    syn = _m("synthetic")
    return [torch.from_numpy(syn.synth_audio(5, 16000 * 38)), torch.from_numpy(syn.synth_audio(6, 16000 * 20))]


@pytest.fixture(scope="module")
def singles(planted, fake_vocab, tk, pcms):
    a, b = _scripts(tk)
    return [_single(planted, fake_vocab, pcms[0], a, word_aligner="heads"), _single(planted, fake_vocab, pcms[1], b, word_aligner="heads")]


def test_words_join_to_the_text_and_follow_the_direct_call(planted, fake_vocab, tk, pcms, singles):
    tr, wt, decoding = _m("transcribe"), _m("word_timing"), _m("decoding")
    res = singles[0]
    script = _scripts(tk)[0]
    assert [(w["seek"], w["aligned"]) for w in res["windows"]] == [(0, True), (3000, True)] and res["windows_without_words"] == 0
    assert [s["text"] for s in res["segments"]] == [' Hello, "tiny" world.', " And (more) words again!", " Some more words, then."]
    for seg in res["segments"]:
        assert "".join(w["word"] for w in seg["words"]) == seg["text"]
        assert all(set(w) == {"word", "start", "end", "probability"} and w["probability"] is None for w in seg["words"])
    assert [w["word"] for w in res["segments"][0]["words"]] == [" Hello,", ' "tiny"', " world."]
    for win in res["windows"]:
        starts = [w["start"] for w in _words(res, win["seek"])]
        assert starts and all(b >= a for a, b in zip(starts, starts[1:])) and starts[0] >= win["seek"] * 0.01 - 1e-9
    # window 0 again, by hand: its mel encoded alone, the decoded tokens framed, the alignment-heads route called directly
    window = planted.mel_window(planted.log_mel_long(pcms[0].cuda()), 0, 3000)
    text_tokens = [t for t in script[0] if t < tk.eot]
    tokens = [*tk.sot_sequence, tk.no_timestamps, *text_tokens, tk.eot]
    opts = planted.make_opts(sot_len=len(tk.sot_sequence), medfilt_width=3, qk_scale=1.0)
    trow = torch.tensor([tokens], device="cuda")
    planted.encode_batch(mel=window[None])
    jump, sel = planted.align_batch(None, None, trow, [len(tokens)], [1500], opts, alignment_heads=True)
    assert sel is None
    planted.encode_batch(mel=window[None])
    listed = planted.align_batch(None, None, trow, [len(tokens)], [1500], opts, alignment_heads=list(planted.alignment_heads))
    assert np.array_equal(jump, listed[0])
    real = decoding.DecodingResult(language="en", tokens=script[0], text="", avg_logprob=0.0, no_speech_prob=0.0, temperature=0.0, compression_ratio=1.0)
    segments, _advance, max_frames = tr.split_window(script[0], tk.timestamp_begin, tk.eot, 0, 3000, real, tk.decode)
    assert max_frames == 1500
    alignment = wt.alignment_from_jump_frames(jump[0], text_tokens, tk)
    wt.add_word_timestamps(segments, alignment, tk, time_offset=0.0, last_speech_timestamp=0.0)
    assert [w for seg in segments for w in seg["words"]] == _words(res, 0)
    assert [(s["start"], s["end"]) for s in segments] == [(s["start"], s["end"]) for s in res["segments"] if s["seek"] == 0]
    # the planted head alone: row r peaks at frame 5 r (the fixture's construction), so the path enters it between the peaks of rows r - 1
    # and r: within one row spacing, 5 frames, of 5 r. The last text row is left out: the frames behind the ridge (225 .. 1500) have no peak to decide them
    planted.encode_batch(mel=window[None])
    one = planted.align_batch(None, None, trow, [len(tokens)], [1500], opts, alignment_heads=[(1, 0)])[0][0][:len(text_tokens) - 1]
    off = 5 * np.arange(len(one)) - one
    print("heads route, planted head alone: 5 r - jump in [%d, %d] over %d rows" % (off.min(), off.max(), len(off)))
    assert np.abs(off).max() <= 5 and bool((np.diff(one) >= 0).all())


def test_word_confidence_fills_the_probabilities(planted, fake_vocab, tk, pcms, singles):
    res = _single(planted, fake_vocab, pcms[1], _scripts(tk)[1], word_aligner="heads", word_confidence=True, append_punctuations=".",
                  prepend_punctuations="")
    words = _words(res)
    assert [w["word"] for w in words] == [" Another", " one", " -", " short", "?", " Yes."]
    assert all(0.0 <= w["probability"] <= 1.0 for w in words)
    plain = _words(singles[1])
    # (the byte-level test vocabulary has no " -" token: the space is its own word, which the backward sweep puts in front of "-")
    assert [w["word"] for w in plain] == [" Another", " one", " -", " short?", " Yes."]


def test_transcribe_batch_equals_the_single_runs(planted, fake_vocab, tk, pcms, singles):
    """Two recordings in lock-step (rounds of two rows, then one): the words are the single runs' -- strings, count and times (the tokens
    are scripted, so no decode near-tie can excuse a difference: the rule of tests/test_transcribe_batch_gpu.py where the tokens agree)."""
    decoding = _m("decoding")
    a, b = _scripts(tk)
    rounds, calls = [[a[0], b[0]], [a[1]]], []

    def decode_windows(mel_windows, prompts):
        rows = [decoding.DecodingOptions(language="en", prompt=list(p) or None, vocab_path=fake_vocab, sample_len=4) for p in prompts]
        real = decoding.decode(planted, mel_windows, rows) if len(rows) > 1 else [decoding.decode(planted, mel_windows[0], rows[0])]
        calls.append(len(rows))
        return [_result(r, t) for r, t in zip(real, rounds[len(calls) - 1])]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        got = _m("transcribe").transcribe_batch(planted, pcms, language="en", vocab_path=fake_vocab, word_timestamps=True, no_speech_threshold=None,
                                                word_aligner="heads", decode_windows=decode_windows)
    assert calls == [2, 1]
    for g, s in zip(got, singles):
        assert [w["word"] for w in _words(g)] == [w["word"] for w in _words(s)]
        assert _words(g) == _words(s)
        assert [(x["start"], x["end"], x["text"]) for x in g["segments"]] == [(x["start"], x["end"], x["text"]) for x in s["segments"]]


def test_without_the_new_keywords_nothing_changes(planted, fake_vocab, tk, pcms):
    """The call without word_aligner is the call with word_aligner="char" given explicitly: the same keys and values, and the character
    aligner's words (no leading spaces, no punctuation), not upstream's."""
    script = _scripts(tk)[0]
    plain = _single(planted, fake_vocab, pcms[0], script)
    explicit = _single(planted, fake_vocab, pcms[0], script, word_aligner="char")
    assert json.dumps(plain) == json.dumps(explicit)   # (key order included; a NaN compares equal as text)
    char_words = [w["word"] for w in _words(plain, 0)]
    assert [w.strip().lower() for w in char_words][:3] == ["hello", "tiny", "world"] and not any(c in ',."()!' for w in char_words for c in w)
    with pytest.raises(ValueError):
        _single(planted, fake_vocab, pcms[0], script, prepend_punctuations="(")
    with pytest.raises(ValueError):
        _single(planted, fake_vocab, pcms[0], script, word_aligner="heads", word_alignment_score=True)
