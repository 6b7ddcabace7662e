#!/usr/bin/env python3
"""Long-form forced alignment: word times of a recording of ANY length against its GIVEN transcript (a book chapter with its text, a
talk with its subtitles, a corpus recording with its reference transcript) on the MI355X engine.

Neither the reference repository (its entry points stop at one 30 s window and 448 framed tokens, infer_ali.py:78-81) nor upstream
openai-whisper (which only times its own ASR hypothesis) has this path: PARITY IS UNPINNED. The window loop below is this project's own
design; its mechanics and the open-end DTW kernel under it are pinned by tests, its quality on real speech is UNVALIDATED until a real
checkpoint is at hand.

What runs where: audio handling is transcribe's (longform.py: `as_pcm`, the GPU resampler, the log-mel of the whole recording once, the window cut
`mel_window`); every window is ONE fused alignment (encode_batch of the window's mel, then align_batch(pcm=None, open_end=[...])): the
teacher-forced forward with capture, median filter, softmax, head scores, aggregation and the DTW are the 30 s path's. The one new piece
below the host is the OPEN-END DTW (csrc/dtw.hip, include/wca.h wca_dtw_open): an interior window holds only a PREFIX of the text it is
offered, so its path must end in the last frame at whichever text row fits best -- the row of the smallest cost per path cell. The loop
itself (`AlignState`) is host Python over a callable, like transcribe.SeekState: it runs without a GPU against a scripted aligner, and
several recordings can be driven in lock-step (`force_align_long_batch`).

The loop's rules
  * units: the whole transcript is normalised and tokenised ONCE, the way `infer_ali.py --teacher text` does it: remove_punctuation, then
    retokenize.encode in `aligned_unit_type`. Word starts come from the existing splitters (char_word_starts, else
    split_tokens_on_spaces). A single word longer than the token limit is a ValueError before any GPU work.
  * request() -> (seek, size, w0, w1, closed): size = min(3000, content_frames - seek) mel frames, max_frames = size // 2 encoder frames;
    [w0, w1) is the longest run of whole words from the text cursor whose framed row [*sot_sequence, no_timestamps, *units, eot] has at
    most 448 tokens (at least one word). `closed` iff the window reaches the end of the recording AND offers all remaining words: such a
    window runs the closed DTW and words_from_jump_frames unchanged, and every offered word is committed.
  * receive(jump_frames, end_row) of an open window: DTW row r is unit r of the offered run, row n_units the final eot. A word is
    COMPLETE if the row of its last unit is <= end_row; its start is the jump frame of its first unit; its end is the jump frame of the
    next word's first unit if that row is <= end_row, else max_frames. Every complete word EXCEPT THE LAST is committed: the window edge
    may have cut that one, so it is offered again. With fewer than two complete words nothing is committed. The one exception: a window
    that offers ALL remaining words and whose path reaches the eot row saw the transcript end before the window edge; its last word is
    committed too, its end being the eot row's jump frame, and the text is used up (without this a transcript that ends before the audio
    would drag its last word through every window of the remaining audio into the final, closed one).
  * advance: if words were committed, seek += 2 * (jump frame of the held-back word's first unit): the next window starts where that
    word starts, and the text cursor moves to it. If nothing was committed, or that advance is 0 (then nothing is committed either),
    seek += size and the cursor stays: the window was silence or could not be aligned (`windows_without_words`).
  * seek strictly increases; the loop ends at content_frames or when the text is used up. A remainder of less than one encoder frame
    (a single mel frame) holds nothing and ends the recording.
  * result: {"words": [{"word", "start", "end"}], "windows": [{seek, size, w0, w1, closed, end_row, score, committed}],
    "unaligned_words": k, "windows_without_words": n}. Times are absolute seconds, seek * 0.01 + frame * 0.02. Words left over when the
    audio ends carry start = end = None and are counted in "unaligned_words". `score` (cost per path cell at the end row) is a
    diagnostic: no decision reads it.
  * word_scores=True (off by default; without it no result gains a key): every window's align_batch also runs the path-score kernel, and
    every word carries "score": the mean of the aggregated attention matrix over the cells of the window's DTW path in the word's unit
    rows (timing.word_alignment_scores on the window that committed it; in [0, 1], uncalibrated; None for an unaligned word). Every window
    entry carries "mean_word_score": the mean of the scores of the words it committed, None where it committed none. No decision reads
    either.

  * trim_silence (off by default; without it no result changes): the DTW gives every frame to some unit, so a word's end is the next
    word's start and a pause counts as part of the word before it. trim_silence=True, or a dict of VAD options, runs the engine's level
    detector once per recording on the log-mel the loop already has (WhisperAMD.speech_segments; under True with min_speech=5,
    min_silence=20, pad=3: pad and the shortest silence must be short here, a dict changes single options of these), passes the
    committed words through timing.trim_words_to_speech at the end -- a word is cut back to the speech its frames meet, a word that meets
    none is left alone -- and adds "speech_segments": [{"start_frame", "stop_frame"}] to the result. The window loop never sees the
    segments. An energy detector: music and noise count as speech, and its defaults are UNVALIDATED on real speech.

Subtitles: force_align_cues
Most transcripts of long recordings are subtitles (SRT, WebVTT, a corpus's segment-level reference), whose cue times already say when
each cue is spoken, to within a second or so. force_align_cues(model, audio, cues) uses them as anchors: every window is planned on the
host from the cue times alone, every unit row of a window gets a permitted frame interval from its cue's times, and the window runs the
WINDOWED closed DTW (csrc/dtw.hip WIN form, include/wca.h wca_dtw_windows) through align_batch(row_windows=...). A window that goes wrong
-- music, text the audio skips -- cannot move any later window, and one recording's windows are the rows of a batch. Its rules:
  * cues: [(start_s, end_s, text)], or a path to an .srt / .vtt file (longform.parse_cues). They must be sorted by start with
    end >= start, else ValueError (ends need not be sorted: cues may overlap). Each cue is normalised and tokenised on its own as
    transcript_units does the transcript; a cue without units carries no words and is skipped (it stays in "cues" with w0 == w1 and
    window None).
  * frames: start s = floor(start_s * 50), end e = ceil(end_s * 50) encoder frames (after rounding start_s * 50 to 1e-6, so that 1.2 s is
    frame 60); g = ceil(cue_slack * 50).
  * planning (CuePlan, before any audio is read): a window starts at mel frame seek = 2 * max(0, s_a - g) of its first cue a and takes the
    longest run of consecutive cues with 2 * (E + g) - seek <= 3000, E the running maximum of their ends, whose framed token row
    [*sot_sequence, no_timestamps, *units of the cues, eot] has at most 448 tokens. A cue that does not fit a window alone is a
    ValueError naming it. Once the recording's length is known the window covers size = min(3000, content_frames - seek,
    2 * (E + g) - seek) mel frames, M = size // 2 encoder frames; a window with M < 1 (its cues lie past the end of the audio) is not run
    and its words stay unaligned (start = end = None).
  * row windows of a window with cues 0..K-1, in window frames (off = seek // 2, clamp to [0, M-1]): every unit row of cue k has
    lo = 0 if k == 0 else clamp(s_k - g - off) and hi = M - 1 if k == K-1 else clamp(max(e_k, s_{k+1}) + g - off), made non-decreasing by
    a running maximum; the eot row has [clamp(e_{K-1} - g - off), M - 1]. These are valid windows (wca_dtw_windows) for any sorted cues.
    Leading silence goes to the first row and the gap after a cue to its last word, as the DTW does everywhere; trim_silence is the remedy.
  * execution: the windows of all recordings of a group (max_batch recordings) are independent and closed; they run in rounds of up to
    max_batch rows, a round being one cut_windows + encode_batch + align_batch(pcm=None, row_windows=...). One recording with W windows
    takes ceil(W / max_batch) rounds, not W.
  * words: DTW row r of a window is unit r of its cues' units, side by side, and the last row the eot. A word starts at the jump frame of its
    first unit and ends at the jump frame of the next word's first unit in the window (the next cue's first word, or the eot row for the
    window's last word): seconds = seek * 0.01 + frame * 0.02, absolute. (force_align_long's closed window goes through
    words_from_jump_frames instead; the cue path forms the times itself, since its word starts come per cue.)
  * result: {"words": [{"word", "start", "end", "cue"}], "cues": [{"start", "end", "text", "w0", "w1", "window"}], "windows": [{"seek",
    "size", "c0", "c1"}], "unaligned_words"}: "cue" indexes "cues" (every given cue, in order), [w0, w1) are a cue's words in "words",
    "window" indexes "windows" (None for a cue without units), and [c0, c1) are a window's cues (a cue without units between them
    belongs to no window). word_scores adds "score" per word and "mean_word_score" per window as in force_align_long; trim_silence trims
    the words and adds "speech_segments" the same way.
  * windows overlap by the slack: consecutive windows are aligned independently, so a word may start before the previous window's last
    word ends. It is reported as it is.
UNVALIDATED: no checkpoint and no subtitle corpus is at hand. The default cue_slack = 1.0 s is a guess, and the quality on real speech is
not established; the mechanics are pinned by tests on planted checkpoints.

Limits: 448 framed tokens and 1500 encoder frames per window (the engine's), so at most 446 - len(sot_sequence) units per window; no
per-word confidence, no music detection (trim_silence is by level only), no fallback to ASR for a window that fails, one GPU.
"""
import argparse
import functools
import json
import os
import sys

import numpy as np

if __package__ in (None, ""):
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _pkg = importlib.import_module("whisper-char-alignment_amd")
    __package__ = _pkg.__name__

from .audio import N_FRAMES, SAMPLE_RATE, TOKENS_PER_SECOND  # noqa: E402
from .longform import (ALIGNER_KEYWORDS, FRAME_SECONDS, INPUT_STRIDE, MAX_LENGTH, add_aligner_options, add_model_options,  # noqa: E402
                       aligner_options, as_pcm, cut_windows, groups_of, load_model, pad_token_rows, read_cues, sample_rates, source)


class AlignState:
    """One recording's side of the window loop as a state machine (module docstring: the loop's rules):
        while not st.done:
            seek, size, w0, w1, closed = st.request()          # the next window and the run of words it is offered
            st.receive(jump_frames, end_row, score)            # the window's DTW result: commits words, advances seek and the cursor
    n_frames: frames of the recording's log-mel (its own plus the 3000 of padding); word_starts: index of every word's first unit in the
    transcript's unit sequence, then the number of units (n_words + 1 entries); words: the n_words strings; sot_len = len(sot_sequence)."""

    def __init__(self, n_frames, word_starts, words, sot_len, max_length=MAX_LENGTH, word_scores=False):
        self.word_scores = bool(word_scores)   # receive() is given the window's path scores: words carry "score", windows "mean_word_score"
        self.content_frames = int(n_frames) - N_FRAMES
        self.word_starts = [int(v) for v in word_starts]
        self.word_text = list(words)
        self.n_words = len(self.word_starts) - 1
        if self.n_words < 0 or len(self.word_text) != self.n_words:
            raise ValueError("word_starts needs one entry per word plus the unit count; got %d entries for %d words"
                             % (len(self.word_starts), len(self.word_text)))
        self.unit_limit = int(max_length) - int(sot_len) - 2   # len(sot_sequence) + 1 + n_units + 1 <= max_length
        for k in range(self.n_words):
            n = self.word_starts[k + 1] - self.word_starts[k]
            if n > self.unit_limit:
                raise ValueError("word %d (%r) has %d units: more than the %d a window's token row can hold" % (k, self.word_text[k], n, self.unit_limit))
        self.seek, self.cursor = 0, 0
        self.words, self.windows = [], []
        self.without_words = 0
        self._skip_sliver()

    def _skip_sliver(self):
        if 0 < self.content_frames - self.seek < INPUT_STRIDE:   # less than one encoder frame is left
            self.seek = self.content_frames

    @property
    def done(self):
        return self.seek >= self.content_frames or self.cursor >= self.n_words

    def request(self):
        size = min(N_FRAMES, self.content_frames - self.seek)
        w0 = w1 = self.cursor
        first = self.word_starts[w0]
        while w1 < self.n_words and self.word_starts[w1 + 1] - first <= self.unit_limit:
            w1 += 1
        closed = self.seek + size >= self.content_frames and w1 == self.n_words
        return self.seek, size, w0, w1, closed

    def unit_span(self, w0, w1):
        """The offered run [w0, w1) as a slice of the transcript's units."""
        return self.word_starts[w0], self.word_starts[w1]

    def _attach_scores(self, window, n_before, rows, path):
        """The words receive() just committed (self.words[n_before:], the first offered words of the window, in order) get their "score":
        the cell-weighted mean of path = (path_mean, path_cells) over the word's rows, as timing.word_alignment_scores forms it."""
        if not self.word_scores:
            return window
        if path is None:
            raise ValueError("an AlignState with word_scores=True needs every window's path scores")
        mean = np.asarray(path[0][:rows[-1] + 1], dtype=np.float64)
        cells = np.asarray(path[1][:rows[-1] + 1], dtype=np.float64)
        got = []
        for k, w in enumerate(self.words[n_before:]):
            c = cells[rows[k]:rows[k + 1]].sum()
            w["score"] = float((mean[rows[k]:rows[k + 1]] * cells[rows[k]:rows[k + 1]]).sum() / c) if c > 0 else float("nan")
            got.append(w["score"])
        live = [s for s in got if s == s]
        window["mean_word_score"] = float(np.mean(live)) if live else None
        return window

    def receive(self, jump_frames, end_row, score=None, times=None, path=None):
        """jump_frames[r]: the encoder frame at which the window's DTW path enters row r (row r = unit r of the offered run, row n_units
        = eot); end_row: the path's last row. times (closed windows only): (starts, ends) in window seconds as words_from_jump_frames
        gives them for the offered run, else they are formed here the same way. path (word_scores only): the window's (path_mean,
        path_cells) rows."""
        n_before = len(self.words)
        seek, size, w0, w1, closed = self.request()
        max_frames = size // INPUT_STRIDE
        base = self.word_starts[w0]
        rows = [self.word_starts[k] - base for k in range(w0, w1 + 1)]   # first row of every offered word, then the eot row
        jump = np.asarray(jump_frames[:rows[-1] + 1], dtype=np.int64)
        end_row = int(end_row)
        window = {"seek": seek, "size": size, "w0": w0, "w1": w1, "closed": closed, "end_row": end_row,
                  "score": None if score is None else float(score), "committed": 0}
        self.windows.append(window)
        offset = seek * FRAME_SECONDS
        if closed:
            if times is None or len(times[0]) != w1 - w0:
                t = jump / TOKENS_PER_SECOND
                times = (t[rows[:-1]], t[rows[1:]])
            for k in range(w0, w1):
                self.words.append({"word": self.word_text[k], "start": offset + float(times[0][k - w0]), "end": offset + float(times[1][k - w0])})
            window["committed"] = w1 - w0
            self.cursor, self.seek = w1, self.content_frames
            return self._attach_scores(window, n_before, rows, path)
        complete = 0
        while complete < w1 - w0 and rows[complete + 1] - 1 <= end_row:
            complete += 1
        if w1 == self.n_words and end_row >= rows[-1]:   # the path reached the eot of the transcript's last words: the text ends in this window
            for k in range(w0, w1):
                self.words.append({"word": self.word_text[k], "start": offset + int(jump[rows[k - w0]]) / TOKENS_PER_SECOND,
                                   "end": offset + int(jump[rows[k - w0 + 1]]) / TOKENS_PER_SECOND})
            window["committed"] = w1 - w0
            self.cursor = w1
            self.seek += INPUT_STRIDE * int(jump[rows[-1]])
            return self._attach_scores(window, n_before, rows, path)
        advance = INPUT_STRIDE * int(jump[rows[complete - 1]]) if complete >= 2 else 0
        if advance <= 0:   # silence, or a window that could not be aligned: nothing is committed and the cursor stays
            self.without_words += 1
            self.seek += size
            self._skip_sliver()
            return self._attach_scores(window, n_before, rows, path)
        for k in range(complete - 1):   # every complete word but the last, which the window edge may have cut
            end = int(jump[rows[k + 1]]) if rows[k + 1] <= end_row else max_frames
            self.words.append({"word": self.word_text[w0 + k], "start": offset + int(jump[rows[k]]) / TOKENS_PER_SECOND,
                               "end": offset + end / TOKENS_PER_SECOND})
        window["committed"] = complete - 1
        self.cursor = w0 + complete - 1
        self.seek += advance
        self._skip_sliver()
        return self._attach_scores(window, n_before, rows, path)

    def result(self):
        words = list(self.words)
        left = self.n_words - self.cursor
        extra = {"score": None} if self.word_scores else {}
        words.extend({"word": self.word_text[k], "start": None, "end": None, **extra} for k in range(self.cursor, self.n_words))
        return {"words": words, "windows": self.windows, "unaligned_words": left, "windows_without_words": self.without_words}


def align_loop(states, align_rows):
    """The window loop over one or several recordings in lock-step: every round asks each unfinished state for its next window and hands
    them to align_rows(live, requests) -> one (jump_frames, end_row[, score[, times]]) per row; `live` holds the rows' indices into
    `states`. The batch shrinks as recordings end. Returns the states' results, in order."""
    states = list(states)
    while True:
        live = [i for i, st in enumerate(states) if not st.done]
        if not live:
            break
        outs = align_rows(live, [states[i].request() for i in live])
        for i, out in zip(live, outs):
            states[i].receive(*out)
    return [st.result() for st in states]


def transcript_units(text, tokenizer, aligned_unit_type="char"):
    """The whole transcript as (units, word_starts, words): remove_punctuation + retokenize.encode as `infer_ali.py --teacher text`, word
    starts from char_word_starts, else split_tokens_on_spaces; word_starts ends with len(units)."""
    from .retokenize import char_word_starts, encode, remove_punctuation, split_tokens_on_spaces
    units = [int(t) for t in encode(remove_punctuation(text), tokenizer, aligned_unit_type)]
    if not units:
        return [], [0], []
    toks = units + [tokenizer.eot]
    starts = char_word_starts(toks, tokenizer) if aligned_unit_type == "char" else None
    if starts is None:
        _words, word_tokens = split_tokens_on_spaces(toks, tokenizer, aligned_unit_type)
        starts = np.pad(np.cumsum([len(t) for t in word_tokens[:-1]]), (1, 0))
    starts = [int(v) for v in starts]   # the last "word" is the eot: its start is len(units)
    words = [tokenizer.decode_with_timestamps(units[a:b]) for a, b in zip(starts[:-1], starts[1:])]
    return units, starts, words


def align_group_rows(model, tokenizer, opts, aligned_unit_type, mels, units, states, live, requests):
    """align_loop's align_rows for one group of recordings, once all but `live` and `requests` are bound: mels, units and states are the
    group's long log-mels, transcript units and AlignStates, by position in the group. A round is ONE encode_batch of the live rows'
    windows and ONE align_batch, whose rows may mix open and closed windows (with path_scores where the states ask for word scores)."""
    from .timing import words_from_jump_frames
    windows = cut_windows(model, mels, [(i, seek, size) for i, (seek, size, _w0, _w1, _c) in zip(live, requests)])
    runs = [units[i][slice(*states[i].unit_span(w0, w1))] for i, (_s, _z, w0, w1, _c) in zip(live, requests)]
    rows = [[*tokenizer.sot_sequence, tokenizer.no_timestamps, *run, tokenizer.eot] for run in runs]
    model.encode_batch(mel=windows)
    want_scores = any(states[i].word_scores for i in live)
    res = model.align_batch(None, None, pad_token_rows(rows, tokenizer.eot).to(model.device), [len(r) for r in rows],
                            [size // INPUT_STRIDE for _s, size, _w0, _w1, _c in requests], opts,
                            open_end=[not closed for _s, _z, _w0, _w1, closed in requests], **({"path_scores": True} if want_scores else {}))
    jump, _sel, end_rows, scores = res[:4]
    outs = []
    for b, (run, req) in enumerate(zip(runs, requests)):
        # a closed window: today's DTW and words_from_jump_frames, unchanged -- its (starts, ends)
        times = words_from_jump_frames(jump[b], run, tokenizer, aligned_unit_type, want_words=False)[1:] if req[4] else None
        outs.append((jump[b], end_rows[b], scores[b], times) + (((res[4][b], res[5][b]),) if want_scores else ()))
    return outs


TRIM_SILENCE_OPTIONS = dict(min_speech=5, min_silence=20, pad=3)   # trim_silence=True: pauses between words are short


def trim_result(result, segments):
    """force_align_long's result with its words trimmed to the speech segments (timing.trim_words_to_speech) and "speech_segments" added."""
    from .timing import trim_words_to_speech
    return {**result, "words": trim_words_to_speech(result["words"], segments),
            "speech_segments": [{"start_frame": int(a), "stop_frame": int(b)} for a, b in segments]}


def force_align_long_batch(model, audios, texts, *, language, vocab_path, aligned_unit_type="char", sample_rate=SAMPLE_RATE, word_scores=False,
                           trim_silence=False, **aligner):
    """force_align_long() of several recordings in lock-step: a list with force_align_long()'s result for every (audio, text) pair, in
    order. Every round cuts the next window of every unfinished recording and aligns them in ONE encode_batch + align_batch, whose rows
    may mix open and closed windows; the batch shrinks as recordings end, and more recordings than model.max_batch go in groups of
    max_batch. sample_rate is one int for every array / tensor input or one per recording (a path carries its own rate); aligner: aggr="topk",
    topk=10, medfilt_width=3, w_colnorm=1.0, w_rownorm=1.0, w_coverage=0.0 (longform.aligner_options). word_scores=True: every word gets
    a "score" and every window a "mean_word_score" (module docstring). trim_silence=True or a dict of VAD options: the words are trimmed
    to the recording's speech segments and the result gains "speech_segments" (module docstring)."""
    from .tokenizer import get_tokenizer
    vad = _check_trim_silence(trim_silence)
    audios, texts = list(audios), list(texts)
    if len(audios) != len(texts):
        raise ValueError("%d recordings for %d transcripts" % (len(audios), len(texts)))
    if vocab_path is None:
        raise ValueError("the transcript is tokenised with the model's vocabulary: pass vocab_path=<local *.tiktoken file>")
    rates = sample_rates(sample_rate, len(audios))
    tokenizer = get_tokenizer(model.is_multilingual, language=language, vocab_path=vocab_path)
    sot_len = len(tokenizer.sot_sequence)
    opts = aligner_options(model, tokenizer, **aligner)
    prepared = [transcript_units(t, tokenizer, aligned_unit_type) for t in texts]
    for _units, starts, words in prepared:   # an over-long word is refused before any GPU work
        AlignState(N_FRAMES, starts, words, sot_len)
    results = []
    for group in groups_of(range(len(audios)), int(getattr(model, "max_batch", 1))):
        mels = [model.log_mel_long(as_pcm(audios[i], model, rates[i])) for i in group]
        states = [AlignState(mel.shape[1], prepared[i][1], prepared[i][2], sot_len, word_scores=word_scores) for i, mel in zip(group, mels)]
        units = [prepared[i][0] for i in group]
        # (one detector call per recording with content, on the mel the loop runs over, before the loop: the words are trimmed at the end)
        segments = [model.speech_segments(mel, **vad)[0] if mel.shape[1] > N_FRAMES else [] for mel in mels] if vad is not None else None
        outs = align_loop(states, functools.partial(align_group_rows, model, tokenizer, opts, aligned_unit_type, mels, units, states))
        results.extend(outs if vad is None else [trim_result(out, seg) for out, seg in zip(outs, segments)])
    return results


def _check_trim_silence(trim_silence):
    if trim_silence is not False and trim_silence is not True and not isinstance(trim_silence, dict):
        raise ValueError("trim_silence is False, True or a dict of VAD options, not %r" % (trim_silence,))
    return None if trim_silence is False else dict(TRIM_SILENCE_OPTIONS, **(trim_silence if isinstance(trim_silence, dict) else {}))


# ------------------------------------------------------------------------------------------------ subtitles: cue-anchored alignment
def cue_frames(start_s, end_s):
    """A cue's times as encoder frames (50 per second): the start floors, the end ceils. t * 50 is first rounded to 1e-6 frames, so that
    a time like 1.2 s, which is not a binary fraction, is frame 60 on both sides."""
    import math
    return int(math.floor(round(float(start_s) * TOKENS_PER_SECOND, 6))), int(math.ceil(round(float(end_s) * TOKENS_PER_SECOND, 6)))


def as_cues(cues):
    """cues as [(start_s, end_s, text)]: a list of such triples, or a path to an .srt / .vtt file."""
    if isinstance(cues, (str, os.PathLike)):
        return read_cues(cues)
    return [(float(a), float(b), str(t)) for a, b, t in cues]


class CuePlan:
    """One recording's side of force_align_cues (module docstring: its rules). The constructor checks the cues and plans the windows from
    the cue times alone; set_audio(n_frames) gives them their sizes once the recording's log-mel (its own frames plus 3000 of padding) is
    known; request(w) -> (seek, size, units, lo, hi) is window w's call and receive(w, jump_frames, path) takes its result; `pending`
    lists the windows that run. cues: [(start_s, end_s, text)]; cue_units: transcript_units(text) of every cue, in order."""

    def __init__(self, cues, cue_units, sot_len, cue_slack=1.0, max_length=MAX_LENGTH, word_scores=False):
        import math
        self.word_scores = bool(word_scores)
        self.g = g = int(math.ceil(round(float(cue_slack) * TOKENS_PER_SECOND, 6)))
        if g < 0:
            raise ValueError("cue_slack %r is negative" % (cue_slack,))
        if len(cues) != len(cue_units):
            raise ValueError("%d cues with %d tokenised texts" % (len(cues), len(cue_units)))
        unit_limit = int(max_length) - int(sot_len) - 2
        self.cues, self.frames, self.units, self.words = [], [], [], []
        self.word_rows = []   # per cue: the first unit of every word, then the cue's unit count
        for k, ((a, b, text), (units, starts, words)) in enumerate(zip(cues, cue_units)):
            if not b >= a:
                raise ValueError("cue %d (%r) ends at %r before it starts at %r" % (k, text, b, a))
            if k and a < cues[k - 1][0]:
                raise ValueError("cue %d (%r) starts at %r, before cue %d at %r: cues must be sorted by start" % (k, text, a, k - 1, cues[k - 1][0]))
            s, e = cue_frames(a, b)
            if units and (len(units) > unit_limit or INPUT_STRIDE * (e + g) - INPUT_STRIDE * max(0, s - g) > N_FRAMES):
                raise ValueError("cue %d (%r, %.3f-%.3f s, %d units) does not fit one window of %d mel frames and %d units with a slack of "
                                 "%d frames" % (k, text, a, b, len(units), N_FRAMES, unit_limit, g))
            w0 = len(self.words)
            self.words.extend({"word": w, "start": None, "end": None, "cue": k, **({"score": None} if self.word_scores else {})} for w in words)
            self.cues.append({"start": float(a), "end": float(b), "text": text, "w0": w0, "w1": len(self.words), "window": None})
            self.frames.append((s, e))
            self.units.append([int(u) for u in units])
            self.word_rows.append([int(v) for v in starts])
        live = [k for k in range(len(self.cues)) if self.units[k]]
        self.windows, self.members = [], []   # members[w]: the cues with units of window w
        i = 0
        while i < len(live):
            a = live[i]
            seek = INPUT_STRIDE * max(0, self.frames[a][0] - g)
            E, n_units, j = self.frames[a][1], len(self.units[a]), i + 1
            while j < len(live):
                k = live[j]
                E2 = max(E, self.frames[k][1])
                if INPUT_STRIDE * (E2 + g) - seek > N_FRAMES or n_units + len(self.units[k]) > unit_limit:
                    break
                E, n_units, j = E2, n_units + len(self.units[k]), j + 1
            for k in live[i:j]:
                self.cues[k]["window"] = len(self.windows)
            self.windows.append({"seek": seek, "size": None, "c0": a, "c1": live[j - 1] + 1, **({"mean_word_score": None} if self.word_scores else {})})
            self.members.append((live[i:j], E))
            i = j
        self.pending = []

    def set_audio(self, n_frames):
        content_frames = int(n_frames) - N_FRAMES
        self.pending = []
        for w, (win, (_members, E)) in enumerate(zip(self.windows, self.members)):
            win["size"] = max(0, min(N_FRAMES, content_frames - win["seek"], INPUT_STRIDE * (E + self.g) - win["seek"]))
            if win["size"] // INPUT_STRIDE >= 1:
                self.pending.append(w)
        return self

    def row_windows(self, w):
        """(lo, hi) of window w's DTW rows: its cues' unit rows, then the eot row; window-relative encoder frames."""
        members, _E = self.members[w]
        M, off, g = self.windows[w]["size"] // INPUT_STRIDE, self.windows[w]["seek"] // INPUT_STRIDE, self.g
        clamp = lambda v: min(max(int(v), 0), M - 1)   # noqa: E731
        lo, hi, top = [], [], 0
        for n, k in enumerate(members):
            s, e = self.frames[k]
            a = 0 if n == 0 else clamp(s - g - off)
            top = M - 1 if n == len(members) - 1 else max(top, clamp(max(e, self.frames[members[n + 1]][0]) + g - off))
            lo.extend([a] * len(self.units[k]))
            hi.extend([top] * len(self.units[k]))
        lo.append(clamp(self.frames[members[-1]][1] - g - off))
        hi.append(M - 1)
        return lo, hi

    def request(self, w):
        win = self.windows[w]
        lo, hi = self.row_windows(w)
        return win["seek"], win["size"], [u for k in self.members[w][0] for u in self.units[k]], lo, hi

    def receive(self, w, jump_frames, path=None):
        """jump_frames[r]: the encoder frame at which window w's DTW path enters row r. path (word_scores only): its (path_mean,
        path_cells) rows."""
        members, _E = self.members[w]
        rows, owners, base = [], [], 0   # the first row of every word of the window, in order, and the words themselves
        for k in members:
            rows.extend(base + r for r in self.word_rows[k][:-1])
            owners.extend(range(self.cues[k]["w0"], self.cues[k]["w1"]))
            base += len(self.units[k])
        rows.append(base)   # the eot row
        jump = np.asarray(jump_frames[:base + 1], dtype=np.int64)
        offset = self.windows[w]["seek"] * FRAME_SECONDS
        if self.word_scores:
            if path is None:
                raise ValueError("a CuePlan with word_scores=True needs every window's path scores")
            mean, cells = np.asarray(path[0][:base + 1], dtype=np.float64), np.asarray(path[1][:base + 1], dtype=np.float64)
        got = []
        for n, k in enumerate(owners):
            word = self.words[k]
            word["start"], word["end"] = offset + int(jump[rows[n]]) / TOKENS_PER_SECOND, offset + int(jump[rows[n + 1]]) / TOKENS_PER_SECOND
            if self.word_scores:
                c = cells[rows[n]:rows[n + 1]].sum()
                word["score"] = float((mean[rows[n]:rows[n + 1]] * cells[rows[n]:rows[n + 1]]).sum() / c) if c > 0 else float("nan")
                got.append(word["score"])
        if self.word_scores:
            live = [v for v in got if v == v]
            self.windows[w]["mean_word_score"] = float(np.mean(live)) if live else None

    def result(self):
        return {"words": self.words, "cues": self.cues, "windows": self.windows,
                "unaligned_words": sum(1 for w in self.words if w["start"] is None)}


def cue_rounds(plans, max_batch, align_rows):
    """Runs every pending window of `plans` (CuePlans after set_audio) in rounds of up to max_batch rows, a recording's windows side by
    side: align_rows(requests) -> one (jump_frames[, (path_mean, path_cells)]) per row, requests = [(plan index, window index)].
    Returns the number of rounds."""
    todo = [(i, w) for i, plan in enumerate(plans) for w in plan.pending]
    rounds = groups_of(todo, max(1, int(max_batch)))
    for requests in rounds:
        for (i, w), out in zip(requests, align_rows(requests)):
            plans[i].receive(w, *out)
    return len(rounds)


def align_cue_rows(model, tokenizer, opts, mels, plans, requests):
    """cue_rounds' align_rows for one group of recordings, once all but `requests` is bound: ONE cut_windows + encode_batch + align_batch
    (pcm=None, row_windows=...) for the round, with path_scores where the plans ask for word scores."""
    reqs = [plans[i].request(w) for i, w in requests]
    windows = cut_windows(model, mels, [(i, seek, size) for (i, _w), (seek, size, _u, _lo, _hi) in zip(requests, reqs)])
    rows = [[*tokenizer.sot_sequence, tokenizer.no_timestamps, *units, tokenizer.eot] for _s, _z, units, _lo, _hi in reqs]
    toks = pad_token_rows(rows, tokenizer.eot)
    lo, hi = np.zeros(tuple(toks.shape), np.int32), np.zeros(tuple(toks.shape), np.int32)
    for b, (_s, _z, _u, rlo, rhi) in enumerate(reqs):   # counted in DTW rows: entries past the eot row are not read
        lo[b, :len(rlo)], hi[b, :len(rhi)] = rlo, rhi
    model.encode_batch(mel=windows)
    want_scores = any(plans[i].word_scores for i, _w in requests)
    res = model.align_batch(None, None, toks.to(model.device), [len(r) for r in rows], [size // INPUT_STRIDE for _s, size, _u, _lo, _hi in reqs], opts,
                            row_windows=(lo, hi), **({"path_scores": True} if want_scores else {}))
    return [(res[0][b],) + (((res[-2][b], res[-1][b]),) if want_scores else ()) for b in range(len(reqs))]


def force_align_cues_batch(model, audios, cues, *, language, vocab_path, cue_slack=1.0, aligned_unit_type="char", sample_rate=SAMPLE_RATE,
                           word_scores=False, trim_silence=False, **aligner):
    """force_align_cues() of several recordings: a list with its result for every (audio, cues) pair, in order. The windows of the
    recordings of a group (max_batch recordings: their long log-mels are held together) share the rounds of up to model.max_batch rows;
    a recording's windows are planned as if it were alone, so its result is force_align_cues()'s up to the row-count-dependent GEMM
    paths of the forward. Every recording's cues are checked before any audio is read. Options as force_align_cues."""
    from .tokenizer import get_tokenizer
    vad = _check_trim_silence(trim_silence)
    audios, cues = list(audios), list(cues)
    if len(audios) != len(cues):
        raise ValueError("%d recordings for %d cue lists" % (len(audios), len(cues)))
    if vocab_path is None:
        raise ValueError("the cues are tokenised with the model's vocabulary: pass vocab_path=<local *.tiktoken file>")
    rates = sample_rates(sample_rate, len(audios))
    tokenizer = get_tokenizer(model.is_multilingual, language=language, vocab_path=vocab_path)
    opts = aligner_options(model, tokenizer, **aligner)
    plans = []
    for one in cues:   # refusals come before any audio is read
        one = as_cues(one)
        plans.append(CuePlan(one, [transcript_units(t, tokenizer, aligned_unit_type) for _a, _b, t in one], len(tokenizer.sot_sequence),
                             cue_slack=cue_slack, word_scores=word_scores))
    max_batch = int(getattr(model, "max_batch", 1))
    results = []
    for group in groups_of(list(range(len(audios))), max_batch):
        mels = [model.log_mel_long(as_pcm(audios[i], model, rates[i])) for i in group]
        mine = [plans[i].set_audio(mel.shape[1]) for i, mel in zip(group, mels)]
        segments = [model.speech_segments(mel, **vad)[0] if mel.shape[1] > N_FRAMES else [] for mel in mels] if vad is not None else None
        cue_rounds(mine, max_batch, functools.partial(align_cue_rows, model, tokenizer, opts, mels, mine))
        outs = [plan.result() for plan in mine]
        results.extend(outs if vad is None else [trim_result(out, seg) for out, seg in zip(outs, segments)])
    return results


def force_align_cues(model, audio, cues, **options):
    """Word times of one recording against its subtitle cues (module docstring: Subtitles -- rules, what is unvalidated). audio: as
    force_align_long takes it. cues: [(start_s, end_s, text)] sorted by start, or a path to an .srt / .vtt file. Keywords: language,
    vocab_path (required), cue_slack=1.0 (seconds a cue's words may lie outside its times; a guess), aligned_unit_type="char",
    sample_rate, word_scores=False, trim_silence=False, and the aligner's options (longform.aligner_options). Returns {"words": [{"word",
    "start", "end", "cue"}], "cues": [...], "windows": [...], "unaligned_words"}; it is force_align_cues_batch of one recording."""
    return force_align_cues_batch(model, [audio], [cues], **options)[0]


def force_align_long(model, audio, text, **options):
    """Word times of one recording of any length against its given transcript `text` (module docstring: rules, limits, what is pinned).
    audio: a path, or mono samples [n] (or [channels, n]) at `sample_rate` Hz, as transcribe() takes them. Returns {"words": [{"word",
    "start", "end"}], "windows": [...], "unaligned_words", "windows_without_words"}; it is force_align_long_batch of one recording."""
    return force_align_long_batch(model, [audio], [text], **options)[0]


# ------------------------------------------------------------------------------------------------ command line
def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Long-form forced alignment of a recording against its transcript (one JSON of word times per recording)")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--audio", type=str, help="one recording (WAV / SPHERE / FLAC at any rate, or a raw .npy array); needs --text or --cues")
    src.add_argument("--scp", type=str, help="list of recordings: `<audio path><TAB><transcript text file>` per line; a second column ending "
                     "in .srt / .vtt is a cue file (force_align_cues)")
    txt = p.add_mutually_exclusive_group()
    txt.add_argument("--text", type=str, default=None, help="the transcript of --audio: a UTF-8 text file")
    txt.add_argument("--cues", type=str, default=argparse.SUPPRESS, help="the subtitles of --audio, an .srt / .vtt file: cue-anchored alignment "
                     "(force_align_cues; unvalidated on real speech) instead of the sequential window loop")
    p.add_argument("--cue_slack", type=float, default=argparse.SUPPRESS, help="seconds a cue's words may lie outside its times (default 1.0, a guess)")
    p.add_argument("--output_dir", type=str, required=True)
    add_model_options(p)
    p.add_argument("--vocab", type=str, required=True, help="local tiktoken vocabulary file")
    p.add_argument("--language", type=str, default="en")
    add_aligner_options(p)
    # (absent from the namespace unless given: the parsed defaults are what they were)
    p.add_argument("--word_scores", action="store_true", default=argparse.SUPPRESS, help="every word also gets a `score`, the mean of the aggregated attention matrix along "
                   "its stretch of the DTW path (in [0, 1]; uncalibrated), and every window its `mean_word_score`")
    p.add_argument("--trim_silence", action="store_true", default=argparse.SUPPRESS, help="trim every word to the speech its frames meet (a level "
                   "detector on the GPU; its defaults are unvalidated on real speech) and add `speech_segments` to the output")
    return p.parse_args(argv)


def _recordings(args):
    if args.audio:
        if getattr(args, "cues", None):
            return [(args.audio, args.cues)]
        if not args.text:
            raise SystemExit("--audio needs --text <transcript file>")
        return [(args.audio, args.text)]
    out = []
    with open(args.scp) as f:
        for line in f:
            parts = line.rstrip("\n").split("\t")
            if len(parts) == 2 and parts[0].strip():
                out.append((parts[0].strip(), parts[1].strip()))
            elif line.strip():
                raise SystemExit("--scp lines are `<audio path><TAB><transcript text file>`; got %r" % line)
    return out

def main(args, model=None):
    """Writes <output_dir>/<audio basename>.json per recording (force_align_long()'s result plus "audio" and "text"; for a recording with a
    cue file force_align_cues()'s plus "audio" and "cue_file"); returns the paths."""
    if args.batch < 1:
        raise SystemExit("--batch must be at least 1")
    recordings = _recordings(args)
    if model is None:
        model = load_model(args)
    os.makedirs(args.output_dir, exist_ok=True)
    kw = dict(language=args.language, vocab_path=args.vocab, sample_rate=args.sample_rate, **{k: getattr(args, k) for k in ALIGNER_KEYWORDS})
    if getattr(args, "word_scores", False):   # (otherwise the call is what it was)
        kw["word_scores"] = True
    if getattr(args, "trim_silence", False):   # (likewise)
        kw["trim_silence"] = True
    ckw = dict(kw, **({"cue_slack": args.cue_slack} if hasattr(args, "cue_slack") else {}))
    # (a cue file: what --cues names, or in --scp mode a second column ending in .srt / .vtt)
    is_cues = lambda a, t: t.lower().endswith((".srt", ".vtt")) if args.scp else t == getattr(args, "cues", None)   # noqa: E731
    done = {}
    with_cues = [r for r in recordings if is_cues(*r)]
    for group in groups_of([r for r in recordings if not is_cues(*r)], args.batch):
        texts = [open(t, encoding="utf-8").read() for _a, t in group]
        for rec, result in zip(group, force_align_long_batch(model, [source(a) for a, _t in group], texts, **kw)):
            done[rec] = {"audio": rec[0], "text": rec[1], **result}
    for group in groups_of(with_cues, args.batch):
        for rec, result in zip(group, force_align_cues_batch(model, [source(a) for a, _c in group], [c for _a, c in group], **ckw)):
            done[rec] = {"audio": rec[0], "cue_file": rec[1], **result}
    paths = []
    for audio, second in recordings:   # (written in the list's order)
        result = done[(audio, second)]
        out = os.path.join(args.output_dir, os.path.splitext(os.path.basename(audio))[0] + ".json")
        with open(out, "w") as f:
            json.dump(result, f)
        paths.append(out)
        print("%s: %d words (%d unaligned), %d windows -> %s" % (audio, len(result["words"]), result["unaligned_words"],
                                                                 len(result["windows"]), out))
    return paths


if __name__ == "__main__":
    main(parse_args())
