"""CPU tests of whisper-char-alignment_amd/word_timing.py (the host half of upstream's word aligner, restated) and of its way into
transcribe (word_aligner="heads"): merge_punctuations on hand-made alignments, every duration rule of add_word_timestamps on hand-computed
numbers, the distribution of the words over the segments, last_speech_timestamp from window to window, what is refused, and seek_loop with a
scripted decoder and a scripted align_batch. The GPU side is tests/test_align_heads_gpu.py and tests/test_transcribe_heads_gpu.py."""
import importlib

import numpy as np
import pytest


@pytest.fixture(scope="module")
def wt():
    return importlib.import_module("whisper-char-alignment_amd.word_timing")


@pytest.fixture(scope="module")
def tr():
    return importlib.import_module("whisper-char-alignment_amd.transcribe")


class _Tok:
    """add_word_timestamps reads only the eot of its tokenizer."""
    eot = 1000


TS = 2000   # a timestamp token: >= eot, so not a text token


def _w(wt, word, tokens, start, end, probability=None):
    return wt.WordTiming(word, list(tokens), start, end, probability)


def _brief(alignment):
    return [(t.word, t.tokens) for t in alignment]


# ------------------------------------------------------------------------------------------------ merge_punctuations
def test_merge_prepend_chain_and_append_chain(wt):
    a = [_w(wt, " hello", [1], 0, 1), _w(wt, " (", [2], 1, 2), _w(wt, ' "', [3], 2, 3), _w(wt, "world", [4], 3, 4), _w(wt, ")", [5], 4, 5),
         _w(wt, ".", [6], 5, 6)]
    wt.merge_punctuations(a, wt.PREPEND_PUNCTUATIONS, wt.APPEND_PUNCTUATIONS)
    # backwards: ' "' goes in front of "world", then " (" in front of that; forwards: ")" and "." go behind it. Times are not merged.
    assert _brief(a) == [(" hello", [1]), (' ( "world).', [2, 3, 4, 5, 6])]
    assert (a[1].start, a[1].end) == (3, 4)


def test_merge_respects_spaces_and_the_given_sets(wt):
    # a word that ends in a space takes nothing; a mark that does not start with a space is not prepended; unknown marks stay words
    a = [_w(wt, " so ", [1], 0, 1), _w(wt, ",", [2], 1, 2), _w(wt, "(", [3], 2, 3), _w(wt, " now", [4], 3, 4), _w(wt, " ...", [5], 4, 5)]
    wt.merge_punctuations(a, wt.PREPEND_PUNCTUATIONS, wt.APPEND_PUNCTUATIONS)
    assert _brief(a) == [(" so ", [1]), (",", [2]), ("(", [3]), (" now", [4]), (" ...", [5])]
    a = [_w(wt, " so", [1], 0, 1), _w(wt, ",", [2], 1, 2), _w(wt, " (", [3], 2, 3), _w(wt, " now", [4], 3, 4)]
    wt.merge_punctuations(a, "", "")   # nothing is a punctuation: nothing merges
    assert _brief(a) == [(" so", [1]), (",", [2]), (" (", [3]), (" now", [4])]
    wt.merge_punctuations(a, "(", ",")
    assert _brief(a) == [(" so,", [1, 2]), (" ( now", [3, 4])]


def test_merge_punctuation_only_words_and_empty_inputs(wt):
    a = [_w(wt, " -", [1], 0, 1)]   # nothing to lean on: it stays a word
    wt.merge_punctuations(a, wt.PREPEND_PUNCTUATIONS, wt.APPEND_PUNCTUATIONS)
    assert _brief(a) == [(" -", [1])]
    a = [_w(wt, " hello", [1], 0, 1), _w(wt, " (", [2], 1, 2)]   # a prepended mark without a follower stays too
    wt.merge_punctuations(a, wt.PREPEND_PUNCTUATIONS, wt.APPEND_PUNCTUATIONS)
    assert _brief(a) == [(" hello", [1]), (" (", [2])]
    a = [_w(wt, " -", [1], 0, 1), _w(wt, " .", [2], 1, 2), _w(wt, "!", [3], 2, 3)]   # only punctuation: one word of it
    wt.merge_punctuations(a, wt.PREPEND_PUNCTUATIONS, wt.APPEND_PUNCTUATIONS)
    assert _brief(a) == [(" - .!", [1, 2, 3])]
    a = []
    wt.merge_punctuations(a, wt.PREPEND_PUNCTUATIONS, wt.APPEND_PUNCTUATIONS)
    assert a == []
    assert wt.add_word_timestamps([], [], _Tok, time_offset=0.0, last_speech_timestamp=1.5) == 1.5


# ------------------------------------------------------------------------------------------------ the duration rules
def _segment(tokens, start, end):
    return {"tokens": [TS, *tokens, TS + 1], "start": start, "end": end, "words": []}


def _times(seg):
    """(word, start, end), the times to the microsecond: the rules behind the round(t, 2) of the hand-out compute in binary floats"""
    return [(w["word"], round(w["start"], 6), round(w["end"], 6)) for w in seg["words"]]


def test_truncation_at_sentence_marks(wt):
    # durations 0.2, 0.2, 2.0: median 0.2, max_duration 0.4. The long word IS a mark: cut at its start + 0.4 (kept apart: no append set)
    a = [_w(wt, " a", [1], 0.0, 0.2), _w(wt, " b", [2], 0.2, 0.4), _w(wt, ".", [3], 0.4, 2.4)]
    seg = _segment([1, 2, 3], 10.0, 13.0)
    last = wt.add_word_timestamps([seg], a, _Tok, time_offset=10.0, last_speech_timestamp=10.0, prepend_punctuations="", append_punctuations="")
    assert _times(seg) == [(" a", 10.0, 10.2), (" b", 10.2, 10.4), (".", 10.4, 10.8)]
    assert (seg["start"], seg["end"], last) == (10.0, 10.8, 10.8)   # the segment follows its words
    # the long word FOLLOWS a mark: cut at its end - 0.4; the mark itself merges into " a" and keeps that word's times
    a = [_w(wt, " a", [1], 0.0, 0.2), _w(wt, ".", [2], 0.2, 0.4), _w(wt, " b", [3], 0.4, 2.4), _w(wt, " c", [4], 2.4, 2.6)]
    seg = _segment([1, 2, 3, 4], 0.0, 2.6)
    wt.add_word_timestamps([seg], a, _Tok, time_offset=0.0, last_speech_timestamp=0.0)
    assert _times(seg) == [(" a.", 0.0, 0.2), (" b", 2.0, 2.4), (" c", 2.4, 2.6)]
    # neither: a long word between ordinary words keeps its times (no pause either: the last speech ended 0.1 s ago)
    a = [_w(wt, " a", [1], 0.0, 0.2), _w(wt, " b", [2], 0.2, 2.2), _w(wt, " c", [3], 2.2, 2.4)]
    seg = _segment([1, 2, 3], 0.0, 2.4)
    wt.add_word_timestamps([seg], a, _Tok, time_offset=0.0, last_speech_timestamp=0.1)
    assert _times(seg) == [(" a", 0.0, 0.2), (" b", 0.2, 2.2), (" c", 2.2, 2.4)]
    # the median is capped at 0.7: durations 1.0, 1.0, 4.0 -> max_duration 1.4
    a = [_w(wt, " a", [1], 0.0, 1.0), _w(wt, " b", [2], 1.0, 2.0), _w(wt, "?", [3], 2.0, 6.0)]
    seg = _segment([1, 2, 3], 0.0, 6.0)
    wt.add_word_timestamps([seg], a, _Tok, time_offset=0.0, last_speech_timestamp=0.5, prepend_punctuations="", append_punctuations="")
    assert _times(seg)[-1] == ("?", 2.0, 3.4)


def test_first_words_after_a_pause(wt):
    # median 0.2, max_duration 0.4, pause threshold 0.8. The first word is too long, the second is not: it starts 0.4 before its end
    a = [_w(wt, " a", [1], 0.0, 3.0), _w(wt, " b", [2], 3.0, 3.2), _w(wt, " c", [3], 3.2, 3.4)]
    seg = _segment([1, 2, 3], 2.6, 3.4)
    wt.add_word_timestamps([seg], a, _Tok, time_offset=0.0, last_speech_timestamp=0.0)
    assert _times(seg) == [(" a", 2.6, 3.0), (" b", 3.0, 3.2), (" c", 3.2, 3.4)]
    # the second is too long as well: the boundary between them moves to max(3.0 / 2, 3.0 - 0.4) = 2.6, the first starts at 2.2
    a = [_w(wt, " a", [1], 0.0, 1.0), _w(wt, " b", [2], 1.0, 3.0), _w(wt, " c", [3], 3.0, 3.2), _w(wt, " d", [4], 3.2, 3.4), _w(wt, " e", [5], 3.4, 3.6)]
    seg = _segment([1, 2, 3, 4, 5], 2.2, 3.6)
    wt.add_word_timestamps([seg], a, _Tok, time_offset=0.0, last_speech_timestamp=0.0)
    assert _times(seg)[:2] == [(" a", 2.2, 2.6), (" b", 2.6, 3.0)]
    # the first alone is short, the first TWO together exceed 2 * max_duration = 0.8: the same cut, on the second word's length
    a = [_w(wt, " a", [1], 1.0, 1.3), _w(wt, " b", [2], 1.3, 2.3), _w(wt, " c", [3], 2.3, 2.5), _w(wt, " d", [4], 2.5, 2.7), _w(wt, " e", [5], 2.7, 2.9)]
    seg = _segment([1, 2, 3, 4, 5], 1.5, 2.9)
    wt.add_word_timestamps([seg], a, _Tok, time_offset=0.0, last_speech_timestamp=0.0)
    assert _times(seg)[:2] == [(" a", 1.5, 1.9), (" b", 1.9, 2.3)]   # boundary max(2.3 / 2, 2.3 - 0.4) = 1.9, start 1.9 - 0.4
    # no pause (the last speech ended 0.5 s before the first word's end): nothing moves
    a = [_w(wt, " a", [1], 0.0, 3.0), _w(wt, " b", [2], 3.0, 3.2), _w(wt, " c", [3], 3.2, 3.4)]
    seg = _segment([1, 2, 3], 0.0, 3.4)
    wt.add_word_timestamps([seg], a, _Tok, time_offset=0.0, last_speech_timestamp=2.5)
    assert _times(seg)[0] == (" a", 0.0, 3.0)


def test_segment_bounds_against_first_and_last_word(wt):
    # (no pause rule: last speech at 2.5.) The segment starts 1.0 s into a 3 s first word: the word takes the segment's start
    a = [_w(wt, " a", [1], 0.0, 3.0), _w(wt, " b", [2], 3.0, 3.2), _w(wt, " c", [3], 3.2, 3.4)]
    seg = _segment([1, 2, 3], 1.0, 3.4)
    wt.add_word_timestamps([seg], a, _Tok, time_offset=0.0, last_speech_timestamp=2.5)
    assert _times(seg)[0] == (" a", 1.0, 3.0) and seg["start"] == 1.0
    # ... but not later than the word's end - median_duration
    seg = _segment([1, 2, 3], 2.95, 3.4)
    a = [_w(wt, " a", [1], 0.0, 3.0), _w(wt, " b", [2], 3.0, 3.2), _w(wt, " c", [3], 3.2, 3.4)]
    wt.add_word_timestamps([seg], a, _Tok, time_offset=0.0, last_speech_timestamp=2.5)
    assert _times(seg)[0] == (" a", 2.8, 3.0) and seg["start"] == 2.95
    # within the 0.5 s slack the segment takes the word's start instead
    seg = _segment([1, 2, 3], 0.4, 3.4)
    a = [_w(wt, " a", [1], 0.0, 3.0), _w(wt, " b", [2], 3.0, 3.2), _w(wt, " c", [3], 3.2, 3.4)]
    wt.add_word_timestamps([seg], a, _Tok, time_offset=0.0, last_speech_timestamp=2.5)
    assert _times(seg)[0] == (" a", 0.0, 3.0) and seg["start"] == 0.0
    # the segment ends 2 s before a long last word does: the word ends with the segment (at least median_duration after its start)
    a = [_w(wt, " a", [1], 0.0, 0.2), _w(wt, " b", [2], 0.2, 0.4), _w(wt, " c", [3], 0.4, 3.0)]
    seg = _segment([1, 2, 3], 0.0, 1.0)
    last = wt.add_word_timestamps([seg], a, _Tok, time_offset=0.0, last_speech_timestamp=0.0)
    assert _times(seg)[-1] == (" c", 0.4, 1.0) and seg["end"] == 1.0 and last == 1.0
    a = [_w(wt, " a", [1], 0.0, 0.2), _w(wt, " b", [2], 0.2, 0.4), _w(wt, " c", [3], 0.4, 3.0)]
    seg = _segment([1, 2, 3], 0.0, 0.45)
    wt.add_word_timestamps([seg], a, _Tok, time_offset=0.0, last_speech_timestamp=0.0)
    assert _times(seg)[-1] == (" c", 0.4, 0.6) and seg["end"] == 0.45
    # within the slack the segment takes the word's end
    a = [_w(wt, " a", [1], 0.0, 0.2), _w(wt, " b", [2], 0.2, 0.4), _w(wt, " c", [3], 0.4, 3.0)]
    seg = _segment([1, 2, 3], 0.0, 2.6)
    wt.add_word_timestamps([seg], a, _Tok, time_offset=0.0, last_speech_timestamp=0.0)
    assert _times(seg)[-1] == (" c", 0.4, 3.0) and seg["end"] == 3.0


def test_words_are_handed_out_by_token_count(wt):
    a = [_w(wt, " a", [1], 0.0, 0.2, 0.9), _w(wt, " bc", [2, 3], 0.2, 0.4, 0.8), _w(wt, ",", [4], 0.4, 0.4), _w(wt, " d", [5], 0.4, 0.6, 0.7),
         _w(wt, " e", [6], 0.6, 0.8, 0.6)]
    segs = [_segment([1, 2, 3, 4], 20.0, 20.4), {"tokens": [], "start": 20.4, "end": 20.4, "words": []}, _segment([5, 6], 20.4, 20.8)]
    last = wt.add_word_timestamps(segs, a, _Tok, time_offset=20.0, last_speech_timestamp=20.0)
    assert [[w["word"] for w in s["words"]] for s in segs] == [[" a", " bc,"], [], [" d", " e"]]
    assert [w["probability"] for s in segs for w in s["words"]] == [0.9, 0.8, 0.7, 0.6]
    assert _times(segs[2]) == [(" d", 20.4, 20.6), (" e", 20.6, 20.8)] and last == 20.8
    assert all(set(w) == {"word", "start", "end", "probability"} for s in segs for w in s["words"])


# ------------------------------------------------------------------------------------------------ through transcribe
class _Model:
    """What HeadsWindowAligner touches of the engine: make_opts, dims.n_audio_ctx, device and a scripted align_batch."""
    device = "cpu"
    max_batch = 1
    alignment_heads_source = "set_alignment_heads"

    class dims:
        n_audio_ctx, n_text_layer, n_text_head = 1500, 2, 4

    def __init__(self, jump_rows):
        self.jump_rows, self.calls = list(jump_rows), []

    def make_opts(self, **kw):
        return kw

    def align_batch(self, pcm, n_samples, tokens, n_tok, max_frames, opts, **kw):
        assert pcm is None and n_samples is None
        self.calls.append(([int(t) for t in tokens[0, :n_tok[0]]], list(max_frames), opts, kw))
        jump = np.zeros(tuple(tokens.shape), np.int32)
        row = self.jump_rows[len(self.calls) - 1]
        jump[0, :len(row)] = row
        lp = np.log(np.full(tuple(tokens.shape), 0.5, np.float32))
        return (jump, None) + ((lp,) if kw.get("token_logprobs_vocab_end") is not None else ())


def _jump_row(tk, text_tokens, word_frames, end_frame):
    """Jump frames of text_tokens + [eot]: every token of word k enters at word_frames[k], the eot at end_frame."""
    _, word_tokens = tk.split_to_word_tokens(list(text_tokens) + [tk.eot])
    assert len(word_tokens) == len(word_frames) + 1
    return [f for toks, f in zip(word_tokens, word_frames) for _ in toks] + [end_frame]


def test_seek_loop_words_join_to_the_segment_text_and_carry_the_last_speech(tr, fake_vocab):
    decoding = importlib.import_module("whisper-char-alignment_amd.decoding")
    tk = importlib.import_module("whisper-char-alignment_amd.tokenizer").get_tokenizer(True, language="en", task="transcribe", vocab_path=fake_vocab)
    ts = tk.timestamp_begin
    t0a, t0b, t1 = tk.encode(' Hello, "tiny" world.'), tk.encode(" And (more) words!"), tk.encode(" Then a long one, yes.")
    w0 = [ts, *t0a, ts + 500, ts + 500, *t0b, ts + 1500]   # two segments, closed: the window advances by 3000 frames
    w1 = [ts, *t1, ts + 200]
    # window 0: seven split words (" Hello" "," ' "' "tiny" '"' " world" ".") + (" And" " (" "more" ")" " words" "!"); " words" ends at 29.9 s
    j0 = _jump_row(tk, t0a + t0b, [0, 10, 20, 20, 30, 40, 50, 1440, 1450, 1450, 1460, 1470, 1495], 1500)
    # window 1: " Then" 0.0 - 0.6 s, then words of 0.2 s
    j1 = _jump_row(tk, t1, [0, 30, 40, 50, 60, 60, 70], 80)
    model = _Model([j0, j1])
    aligner = tr.make_aligner(model, tk, word_aligner="heads", word_confidence=True, medfilt_width=7, aggr="topk", topk=10)
    results = [decoding.DecodingResult(language="en", tokens=w, text="", avg_logprob=-0.3, no_speech_prob=0.1, temperature=0.0, compression_ratio=1.0)
               for w in (w0, w1)]
    calls = []

    def decode_window(window, prompt):
        calls.append(window)
        return results[len(calls) - 1]

    out = tr.seek_loop(6000 + 3000, lambda seek, size: (seek, size), decode_window, tk, align_window=aligner.align_window)
    assert [w["aligned"] for w in out["windows"]] == [True, True] and out["windows_without_words"] == 0
    segs = out["segments"]
    assert [s["text"] for s in segs] == [' Hello, "tiny" world.', " And (more) words!", " Then a long one, yes."]
    for s in segs:
        assert "".join(w["word"] for w in s["words"]) == s["text"]
    assert [w["word"] for w in segs[0]["words"]] == [" Hello,", ' "tiny"', " world."]
    assert [w["word"] for w in segs[1]["words"]] == [" And", " (more)", " words!"]
    assert all(w["probability"] == pytest.approx(0.5) for s in segs for w in s["words"])
    # the framed rows are the decoded tokens themselves, one call per window, on the alignment-heads route
    assert [c[0] for c in model.calls] == [[*tk.sot_sequence, tk.no_timestamps, *t0a, *t0b, tk.eot], [*tk.sot_sequence, tk.no_timestamps, *t1, tk.eot]]
    assert all(c[3]["alignment_heads"] is True and c[2]["medfilt_width"] == 7 and c[2]["sot_len"] == len(tk.sot_sequence) for c in model.calls)
    assert [c[1] for c in model.calls] == [[1500], [1500]]
    # window 0's last word (" words!": the merged mark does not move its times) ended at 29.9 s and window 1's first word ends 0.7 s later:
    # no pause (4 x the 0.2 s median), so " Then" keeps its 0.6 s; an aligner that forgot the carry would cut it to 0.4 s
    assert segs[1]["words"][-1]["end"] == 29.9 and aligner.last_speech[None] == segs[2]["words"][-1]["end"]
    first = segs[2]["words"][0]
    assert (first["word"], first["start"], first["end"]) == (" Then", 30.0, 30.6)
    fresh = tr.make_aligner(_Model([j1]), tk, word_aligner="heads")
    seg = {"tokens": list(w1), "start": 30.0, "end": 34.0, "words": []}
    assert fresh.align_window(3000, 3000, 1500, [seg]) is True
    assert _times(seg)[0] == (" Then", 30.2, 30.6) and seg["words"][0]["probability"] is None
    # a window without text tokens gets no call and no words
    empty = tr.make_aligner(_Model([]), tk, word_aligner="heads")
    assert empty.align_window(0, 3000, 1500, [{"tokens": [], "start": 0.0, "end": 1.0, "words": []}]) is False and empty.model.calls == []
    assert isinstance(tr.make_aligner(model, tk, aligned_unit_type="char"), tr.WindowAligner)


def test_refusals_and_the_command_line(tr):
    model = object()
    for kw in (dict(prepend_punctuations="("), dict(append_punctuations="."), dict(word_timestamps=True, vocab_path="v", append_punctuations="."),
               dict(word_aligner="heads"), dict(word_aligner="heads", word_timestamps=True, vocab_path="v", word_alignment_score=True),
               dict(word_aligner="subword", word_timestamps=True, vocab_path="v")):
        with pytest.raises(ValueError):
            tr.transcribe_batch(model, [], language="en", **kw)
        with pytest.raises(ValueError):
            tr.transcribe(model, None, language="en", **kw)
    assert tr.transcribe_batch(model, [], language="en", word_aligner="heads", word_timestamps=True, vocab_path="v", prepend_punctuations="(") == []
    with pytest.warns(UserWarning, match="upper half"):
        class Plain:
            alignment_heads_source = "default (upper half of the decoder layers)"
        tr.transcribe_batch(Plain(), [], language="en", word_aligner="heads", word_timestamps=True, vocab_path="v")
    base = ["--audio", "a.wav", "--output_dir", "o"]
    plain = tr.parse_args(base)
    assert not any(hasattr(plain, k) for k in ("word_aligner", "prepend_punctuations", "append_punctuations"))
    args = tr.parse_args(base + ["--word_timestamps", "--word_aligner", "heads", "--prepend_punctuations", "(", "--append_punctuations", ".,"])
    assert (args.word_aligner, args.prepend_punctuations, args.append_punctuations) == ("heads", "(", ".,")
    with pytest.raises(SystemExit):
        tr.parse_args(base + ["--word_aligner", "words"])
    doc = tr.__doc__
    assert "hallucination_silence_threshold is not built" in doc and "prepend_punctuations / append_punctuations are not built" not in doc
