"""Upstream-style words for transcribe(word_aligner="heads"): the host half of openai-whisper's `whisper/timing.py` -- WordTiming,
merge_punctuations and the window-level body of add_word_timestamps -- on the jump frames of the engine's alignment-heads route
(WhisperAMD.align_batch(alignment_heads=True): csrc/align_heads.hip is find_alignment's arithmetic).

Upstream `timing.py` is an absent third-party dependency (like `decoding.py` and `transcribe.py`, see their docstrings); its published
text is restated here from memory of that text: PARITY UNPINNED against upstream itself. What is pinned: every rule below on hand-computed
numbers (tests/test_word_timing.py), and the kernels against float64 (tests/test_align_heads_gpu.py). Quality on speech is UNVALIDATED:
no checkpoint is at hand.

The guarantee the restatement keeps: "".join(w["word"] for w in segment["words"]) == segment["text"] -- every word carries its leading
space and the punctuation merged into it -- whenever the segment boundaries fall between words (a segment starts with a timestamp token,
and the text after one starts a new word in every vocabulary seen).
"""
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from .audio import TOKENS_PER_SECOND

PREPEND_PUNCTUATIONS = "\"'“¿([{-"
APPEND_PUNCTUATIONS = "\"'.。,，!！?？:：”)]}、"
SENTENCE_END_MARKS = ".。!！?？"


@dataclass
class WordTiming:
    word: str
    tokens: List[int]
    start: float
    end: float
    probability: Optional[float]


def merge_punctuations(alignment, prepended, appended):
    """Upstream's two sweeps, in place. Backwards: a word that starts with a space and whose stripped text is in `prepended` is put in
    front of its follower (the nearest later word that is not itself emptied). Forwards: a follower whose text is in `appended` is put
    behind the nearest earlier word that does not end in a space. In both the tokens are merged and the emptied word is dropped."""
    i, j = len(alignment) - 2, len(alignment) - 1
    while i >= 0:
        previous, following = alignment[i], alignment[j]
        if previous.word.startswith(" ") and previous.word.strip() in prepended:
            following.word = previous.word + following.word
            following.tokens = previous.tokens + following.tokens
            previous.word, previous.tokens = "", []
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < len(alignment):
        previous, following = alignment[i], alignment[j]
        if not previous.word.endswith(" ") and following.word in appended:
            previous.word = previous.word + following.word
            previous.tokens = previous.tokens + following.tokens
            following.word, following.tokens = "", []
        else:
            i = j
        j += 1
    alignment[:] = [t for t in alignment if t.word]


def alignment_from_jump_frames(jump_frames, text_tokens, tokenizer, token_logprobs=None):
    """find_alignment's tail: the WordTimings of text_tokens (without the eot's) from one row of align_batch's jump frames -- entry i is
    the encoder frame at which the DTW path enters the row of text_tokens[i], entry len(text_tokens) the eot's. token_logprobs (that
    row of align_batch's token log-probs, or None): a word's probability is the mean of exp over its tokens, else None. [] when the text
    has no word."""
    from .timing import default_word_spans
    jump_times = np.asarray(jump_frames[:len(text_tokens) + 1], dtype=np.int64) / TOKENS_PER_SECOND
    spans = default_word_spans(jump_times, text_tokens, tokenizer)
    if spans is None:
        return []
    words, word_tokens, boundaries, starts, ends = spans
    probs = [None] * len(starts)
    if token_logprobs is not None:
        p = np.exp(np.asarray(token_logprobs, dtype=np.float64)[:len(text_tokens)])
        probs = [float(np.mean(p[i:j])) for i, j in zip(boundaries[:-1], boundaries[1:])]
    return [WordTiming(w, list(t), float(a), float(b), pr) for w, t, a, b, pr in zip(words, word_tokens, starts, ends, probs)]


def add_word_timestamps(segments, alignment, tokenizer, *, time_offset, last_speech_timestamp, prepend_punctuations=PREPEND_PUNCTUATIONS,
                        append_punctuations=APPEND_PUNCTUATIONS):
    """The body of upstream's add_word_timestamps for ONE window behind its find_alignment: `alignment` (the window's WordTimings, times
    relative to the window) is trimmed, merged and handed out to `segments` (the window's segments, in order; their "tokens", "start" and
    "end" are read, "words", "start" and "end" written). time_offset: the window's first frame in seconds. Returns the
    last_speech_timestamp to carry into the next window: the end of this window's last word, or the one given when it has none.
      * median_duration = min(0.7, median of the non-zero word durations), max_duration = 2 * median_duration;
      * a word longer than max_duration that IS a sentence mark is cut at its start + max_duration, one that FOLLOWS a sentence mark at
        its end - max_duration;
      * merge_punctuations;
      * a segment takes words until their tokens cover its text tokens (t < eot), times round(time_offset + t, 2);
      * after a pause (first word's end more than 4 * median_duration past last_speech_timestamp) a first word longer than
        max_duration, or first two words longer than 2 * max_duration together, are cut back: the boundary between the two moves to
        max(second end / 2, second end - max_duration) where the second is itself too long, and the first starts at most max_duration
        before its end;
      * a segment start more than 0.5 s inside a too-long first word wins over the word's start (else the segment takes the word's), and
        likewise a segment end more than 0.5 s before a too-long last word's end."""
    if not segments:
        return last_speech_timestamp
    eot = tokenizer.eot
    text_tokens_per_segment = [[t for t in seg["tokens"] if t < eot] for seg in segments]
    durations = np.array([t.end - t.start for t in alignment])
    durations = durations[durations.nonzero()] if len(durations) else durations
    median_duration = min(0.7, float(np.median(durations)) if len(durations) > 0 else 0.0)
    max_duration = median_duration * 2
    if len(durations) > 0:
        for i in range(1, len(alignment)):
            if alignment[i].end - alignment[i].start > max_duration:
                if alignment[i].word in SENTENCE_END_MARKS:
                    alignment[i].end = alignment[i].start + max_duration
                elif alignment[i - 1].word in SENTENCE_END_MARKS:
                    alignment[i].start = alignment[i].end - max_duration
    merge_punctuations(alignment, prepend_punctuations, append_punctuations)

    word_index = 0
    for segment, text_tokens in zip(segments, text_tokens_per_segment):
        saved_tokens, words = 0, []
        while word_index < len(alignment) and saved_tokens < len(text_tokens):
            timing = alignment[word_index]
            if timing.word:
                words.append(dict(word=timing.word, start=round(time_offset + timing.start, 2), end=round(time_offset + timing.end, 2),
                                  probability=timing.probability))
            saved_tokens += len(timing.tokens)
            word_index += 1
        if words:
            if words[0]["end"] - last_speech_timestamp > median_duration * 4 and (
                    words[0]["end"] - words[0]["start"] > max_duration or
                    (len(words) > 1 and words[1]["end"] - words[0]["start"] > max_duration * 2)):
                if len(words) > 1 and words[1]["end"] - words[1]["start"] > max_duration:
                    boundary = max(words[1]["end"] / 2, words[1]["end"] - max_duration)
                    words[0]["end"] = words[1]["start"] = boundary
                words[0]["start"] = max(0, words[0]["end"] - max_duration)
            if segment["start"] < words[0]["end"] and segment["start"] - 0.5 > words[0]["start"]:
                words[0]["start"] = max(0, min(words[0]["end"] - median_duration, segment["start"]))
            else:
                segment["start"] = words[0]["start"]
            if segment["end"] > words[-1]["start"] and segment["end"] + 0.5 < words[-1]["end"]:
                words[-1]["end"] = max(words[-1]["start"] + median_duration, segment["end"])
            else:
                segment["end"] = words[-1]["end"]
            last_speech_timestamp = segment["end"]
        segment["words"] = words
    ends = [w["end"] for seg in segments for w in seg["words"]]
    return ends[-1] if ends else last_speech_timestamp
