#!/usr/bin/env python3
"""Long-form transcription: `whisper.transcribe(model, audio, ...)` at temperature 0 on the MI355X engine, with word times
from this project's character aligner or (word_aligner="heads") from upstream's alignment-heads aligner.

Upstream openai-whisper `transcribe.py` is an absent third-party dependency (like `decoding.py`, see decoding.py's
docstring); its published seek loop is restated here: PARITY UNPINNED against upstream itself. The reference
repository has no long-form path at all (its entry points stop at 30 s, infer_ali.py:78-81).

What runs where: audio that is not at 16 kHz (a 44.1 / 48 kHz file, 8 kHz telephone audio, an array with sample_rate=...) is converted
on the GPU first (wca_resample_16k: torchaudio.functional.resample's default filter on the mean over the channels; upstream's load_audio
leaves this to ffmpeg), then the log-mel of the WHOLE recording once (wca_log_mel_long: one `max - 8` floor over the recording), the
window cut pad_or_trim(mel[:, seek:seek+size], 3000) with zeros in the mel domain (wca_mel_window), greedy decode of each
window with the previous text as the prompt (wca_decode), and -- with word_timestamps=True -- the fused alignment
on the encoder state that decode left in the engine (align_batch(pcm=None): no second encoder pass). The loop itself
(`seek_loop`) is host Python over two callables, so it runs without a GPU against a scripted decoder.

Limits (part of the contract):
  * the temperature fallback ladder is opt-in through seed=<int>. Without a seed (the default) temperature is 0.0 (or a tuple holding
    only 0.0) and anything else raises NotImplementedError, as before the sampler existed: the engine's sampling is reproducible by
    construction and picks no seed for the caller. With a seed, temperature may be upstream's (0.0, 0.2, 0.4, 0.6, 0.8, 1.0) or any
    number or non-empty tuple: a window whose result has compression_ratio > compression_ratio_threshold (2.4) or avg_logprob <
    logprob_threshold (-1), and is not taken for silence, is decoded again at the next temperature, on the encoder state its first
    decode left in the engine (wca_decode with temperature_host / seed_host, redecode: a rung costs decoder positions only, where upstream encodes the window
    again); the last rung is accepted whatever it gives, and a window accepted above 0.5 does not condition the next one. Without a
    vocabulary the compression ratio is NaN and only the log-probability test can fire. What is pinned: the sampler against a float64
    restatement, token for token (tests/test_decode_sample_gpu.py), and the ladder's mechanics (tests/test_transcribe_ladder.py). What is
    not: the law of the draws is upstream's (Categorical(logits / T), untempered log-probabilities), the draws themselves are not
    torch's -- another generator --, and what the ladder does to repetition loops on real speech is UNVALIDATED: no checkpoint is at
    hand, and random weights fall through every rung.
  * beam_size, patience, length_penalty and best_of are upstream's and default to None (a call without them is what it was): the beam at
    temperature 0, best_of on the rungs above it (so best_of needs a seed), each window on max(beam_size, best_of) decoder rows of the
    engine's max_batch (C ABI wca_decode_group; transcribe_batch's docstring). What is pinned: the beam step, the cache reorder and the
    loop (tests/test_beam_step_gpu.py, tests/test_kv_reorder_gpu.py, tests/test_decode_beam_gpu.py); parity with upstream itself is not.
  * the language is given, or language="auto" detects it (decoding.detect_language, C ABI wca_detect_language) on each recording's
    first window mel_window(mel, 0, size) -- the frames the first decode sees; upstream also detects on the first 30 s -- in the
    99-language numbering of the decode tokenizer, so the detected token is the one that lands in the sot sequence. The first windows
    of a group are detected in ONE batch; the result carries the detected "language" and its "language_probability". One decode cannot
    mix languages, so transcribe_batch partitions a group by detected language and runs the lock-step loop once per language. Where
    the whole group comes out in one language (transcribe() always does), the first round decodes the encoder state that detection
    left in the engine (decode(..., encoded_batch=B)): detection then costs one decoder position, not a second encoder pass.
    Otherwise the group is simply re-encoded language by language. An English-only model reports "en" without a detection pass
    (probability None), and so little audio that there is no window to look at leaves "language" None. language=None stays refused
    (NotImplementedError), as in decode: say "auto". PARITY UNPINNED against upstream, like decode.
  * transcribe() takes one recording, window after window (window k+1 starts where window k ended). transcribe_batch() takes
    several and runs them in lock-step: every round decodes the next window of every unfinished recording in ONE batch
    (wca_decode with per_row 1: every row carries its own previous text as the prompt, so the rows sit at different decoder
    positions), the batch shrinks as recordings end, and with word_timestamps one align_batch(pcm=None) per round aligns the
    rows that have words. A recording's result is what transcribe() gives for it alone, up to argmax near-ties of the f16
    logits (the GEMM path, and with it the fp32 summation order, depends on the number of rows in the batch).
  * clip_timestamps is upstream's (SeekState(clips=...) restates its seek_clips loop). pieces=N / "auto" has no upstream counterpart: ONE
    recording is cut at quiet frames (wca_quiet_cuts: near each equal share the even frame with the lowest smoothed log-mel level) and its
    pieces are decoded side by side as the rows of one batch, each conditioned on its own previous text only. What a cut does to the
    text around it on real speech -- a word split where no quiet frame was in reach, a piece that starts without the context the
    sequential loop would have carried over -- is UNVALIDATED: no checkpoint is at hand here, the tests run on random weights and compare
    pieces=N with the same ranges given as clip_timestamps.
  * vad_filter=True (off by default; faster-whisper's and WhisperX's keyword, not upstream's) finds the speech first and decodes only
    that: the recording's log-mel goes through the engine's level detector (WhisperAMD.speech_segments, C ABI wca_speech_segments: a noise
    floor and a peak from two order statistics of the smoothed level, hysteresis, minimum durations, padding; all on the GPU, exact
    against its integer definition) and the segments it returns are the clips of the seek loop, the mechanism clip_timestamps uses, so
    segment and word times stay absolute. It is an ENERGY detector, not a trained one: music and loud noise count as speech, and the
    quality of its defaults on real speech is UNVALIDATED (they were looked at on one 2.9 s recording laid out between stretches of
    silence; no corpus is at hand). Not together with clip_timestamps or pieces.
  * hallucination_silence_threshold is not built (it belongs to upstream's own word aligner's seek loop); vad_filter is this project's
    remedy for text invented over silence.
  * word_aligner="heads" (the default stays "char") takes upstream's own word aligner instead: find_alignment over model.alignment_heads
    on the GPU (align_batch(alignment_heads=True), csrc/align_heads.hip) and a restatement of add_word_timestamps with
    prepend_punctuations / append_punctuations (word_timing.py). Pinned: the kernels against float64, every host rule on hand-computed
    numbers. Not pinned: parity with upstream itself (its source is not at hand), and quality on speech is UNVALIDATED.

Decisions the upstream text leaves open:
  * a window that ended inside speech (its tokens do not end in a single timestamp; seek advances to the last consecutive
    timestamp pair) has its tail decoded again by the next window, so only the text of the segments that were KEPT is
    aligned, against max_frames = last_timestamp_pos encoder frames: no word is reported twice. Every other window aligns
    against max_frames = size // 2.
  * a window whose framed text [*sot_sequence, no_timestamps, *text, eot] is longer than 448 tokens, or has at most one word,
    or cannot be tokenised, or has max_frames < 1, gets segment times only and words = [] (the reference's skip,
    infer_ali.py:79-81, timing.py:106-107); result["windows_without_words"] counts them.
  * a word belongs to the segment whose [start, end) contains its start; if none does, to the last segment of its window
    that starts at or before it (else the window's first segment).
  * a window that ended inside speech with last_timestamp_pos == 0 would not advance at all (upstream's loop can spin there at a
    fixed temperature), and in a short last window a timestamp beyond the window's `size` frames would carry seek past the end of the
    recording: both advance by the window size instead, so seek strictly increases and ends at content_frames.
  * without a vocabulary (vocab_path=None) token ids cannot be turned into text: "text" fields are "" and the "segment without text
    is cleared" rule is not applied; tokens and times are complete. word_timestamps=True needs the vocabulary.
"""
import argparse
import json
import os
import sys

import numpy as np

if __package__ in (None, ""):
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _pkg = importlib.import_module("whisper-char-alignment_amd")
    __package__ = _pkg.__name__

from . import decoding  # noqa: E402  (decoding.decode is looked up when it is called)
from .audio import N_FRAMES, SAMPLE_RATE  # noqa: E402
from .longform import (ALIGNER_KEYWORDS, FRAME_SECONDS, FRAMES_PER_SECOND, INPUT_STRIDE, MAX_LENGTH, TIME_PRECISION,  # noqa: E402,F401
                       add_aligner_options, add_model_options, aligner_options, as_pcm, cut_windows, groups_of, load_model,
                       pad_token_rows, sample_rates, source)
from .tokenizer import get_tokenizer  # noqa: E402

PLACEHOLDER_FRAMES = 100   # max_frames of a row that rides along in a round's alignment without words


SEEK_MIX, RUNG_MIX = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9


def window_seed(seed, seek, rung):
    """The Philox seed a window is sampled with: the call's seed mixed with the window's first frame and the index of the temperature in
    the ladder, so that a recording's draws do not depend on the batch row or the group it rides in."""
    return (int(seed) ^ (int(seek) * SEEK_MIX) ^ (int(rung) * RUNG_MIX)) % (1 << 64)


def check_supported(temperature, language, seed=None):
    """What this transcribe refuses instead of silently differing from upstream. Returns the temperature ladder: 0.0 without a seed (any
    other temperature is refused then, as it always was), with an int seed the tuple of temperatures (a number or a non-empty sequence of
    finite numbers >= 0, as upstream takes them)."""
    temps = tuple(temperature) if isinstance(temperature, (tuple, list)) else (temperature,)
    if seed is not None:
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
            raise ValueError("seed must be an int (or None: temperature 0.0 only), not %r" % (seed,))
        if not temps or not all(isinstance(t, (int, float, np.integer, np.floating)) and 0.0 <= float(t) < float("inf") for t in temps):
            raise ValueError("temperature must be a finite number >= 0 or a non-empty tuple of them, not %r" % (temperature,))
    elif len(temps) != 1 or float(temps[0]) != 0.0:
        raise NotImplementedError("transcribe runs at temperature 0.0 only: the fallback ladder %r needs sampling, which the engine's "
                                  "greedy decode does not do (decoding._check_supported)" % (temperature,))
    if language is None:
        raise NotImplementedError("language=None is not taken: pass language=\"auto\" to detect it on the first window "
                                  "(decoding.detect_language), or the language itself (as DecodingOptions(language=...) in decode)")
    return 0.0 if seed is None else tuple(float(t) for t in temps)


def needs_fallback(result, compression_ratio_threshold, logprob_threshold, no_speech_threshold):
    """Upstream's decode_with_fallback rule for one window: too repetitive (compression ratio above its threshold) or too improbable
    (average log-probability below its threshold) -- unless the window is taken for silence (no_speech_prob above its threshold and the
    average log-probability below its own), which the seek loop skips anyway. A threshold of None switches its test off; a NaN
    compression ratio (no vocabulary: no text to compress) never fires."""
    fallback = False
    if compression_ratio_threshold is not None and result.compression_ratio > compression_ratio_threshold:
        fallback = True
    if logprob_threshold is not None and result.avg_logprob < logprob_threshold:
        fallback = True
    if (no_speech_threshold is not None and result.no_speech_prob > no_speech_threshold and logprob_threshold is not None and
            result.avg_logprob < logprob_threshold):
        fallback = False
    return fallback


def split_window(tokens, timestamp_begin, eot, seek, size, result, decode_text):
    """One window of upstream's loop: decoded tokens -> (segments, frames to advance, max_frames for the aligner).
    Segments split at consecutive timestamp pairs; a window that ends in a single timestamp (or has no pair) advances by `size`, one
    that ended inside speech advances to its last pair. decode_text(tokens) -> str, or None when there is no vocabulary."""
    tokens = [int(t) for t in tokens]
    time_offset = seek * FRAME_SECONDS
    is_ts = [t >= timestamp_begin for t in tokens]

    def new_segment(start, end, toks):
        text = decode_text([t for t in toks if t < eot])
        return {"seek": seek, "start": start, "end": end, "text": text if text is not None else "", "tokens": list(toks),
                "temperature": result.temperature, "avg_logprob": result.avg_logprob, "compression_ratio": result.compression_ratio,
                "no_speech_prob": result.no_speech_prob, "_has_text": None if text is None else bool(text.strip())}

    segments = []
    single_timestamp_ending = is_ts[-2:] == [False, True]
    consecutive = [i + 1 for i in range(len(tokens) - 1) if is_ts[i] and is_ts[i + 1]]
    max_frames = size // INPUT_STRIDE
    if consecutive:
        slices = list(consecutive)
        if single_timestamp_ending:
            slices.append(len(tokens))
        last_slice = 0
        for current_slice in slices:
            sliced = tokens[last_slice:current_slice]
            segments.append(new_segment(time_offset + (sliced[0] - timestamp_begin) * TIME_PRECISION,
                                        time_offset + (sliced[-1] - timestamp_begin) * TIME_PRECISION, sliced))
            last_slice = current_slice
        advance = size
        if not single_timestamp_ending:
            last_timestamp_pos = tokens[last_slice - 1] - timestamp_begin
            if 0 < last_timestamp_pos * INPUT_STRIDE <= size:   # (see the module docstring for the two cases left out)
                advance = last_timestamp_pos * INPUT_STRIDE
                max_frames = last_timestamp_pos
    else:
        duration = size * FRAME_SECONDS
        timestamps = [t for t in tokens if t >= timestamp_begin]
        if timestamps and timestamps[-1] != timestamp_begin:
            duration = (timestamps[-1] - timestamp_begin) * TIME_PRECISION
        segments.append(new_segment(time_offset, time_offset + duration, tokens))
        advance = size
    for seg in segments:   # an instantaneous segment, or one without text, is cleared
        has_text = seg.pop("_has_text")
        if seg["start"] == seg["end"] or has_text is False:
            seg["text"], seg["tokens"] = "", []
        seg["words"] = []
    return segments, advance, max_frames


class SeekState:
    """One recording's side of whisper.transcribe's loop as a state machine, so that several recordings can share a decode batch:
        while not st.done:
            seek, size, prompt = st.request()          # the next window and the prompt tokens it is decoded with
            pending = st.receive(decoding_result)      # None: the window was skipped (no speech) and the state has advanced
            if pending is not None:                    # (seek, size, max_frames, segments): align the segments in place, then
                st.commit(aligned)                     # aligned: bool, or None when no aligner runs
    seek_loop (one recording) and transcribe_batch (several in lock-step) both drive it.
    clips: upstream's seek_clips, a list of (start, stop) frame pairs: the loop runs over [start, stop) of each in turn, a window never
    reaches past its clip's stop (size = min(3000, content_frames - seek, stop - seek)) and the next clip starts when seek >= stop. A stop
    beyond the recording is clamped to content_frames. None is the whole recording, [(0, content_frames)]. transcribe(pieces=...) gives
    every piece of a recording a state of its own with one clip."""

    def __init__(self, n_frames, tokenizer, *, initial_prompt_tokens=(), condition_on_previous_text=True, no_speech_threshold=0.6,
                 logprob_threshold=-1.0, decode_text=None, clips=None):
        if decode_text is None:
            def decode_text(toks):
                return tokenizer.decode(toks) if getattr(tokenizer, "has_vocab", True) else None
        self.tokenizer, self.decode_text = tokenizer, decode_text
        self.condition_on_previous_text = condition_on_previous_text
        self.no_speech_threshold, self.logprob_threshold = no_speech_threshold, logprob_threshold
        self.content_frames = n_frames - N_FRAMES
        self.all_tokens = [int(t) for t in initial_prompt_tokens]
        self.all_segments, self.windows = [], []
        self.prompt_reset_since = 0
        self.without_words = 0
        # upstream's seek_clips: the loop runs over these frame ranges, one after the other; None is the whole recording
        self.clips = [(0, self.content_frames)] if clips is None else [(int(a), min(int(b), self.content_frames)) for a, b in clips]
        if any(a < 0 for a, _ in self.clips):
            raise ValueError("a clip starts before the recording: %r" % (clips,))
        self.clip_idx = 0
        self.seek = self.clips[0][0] if self.clips else 0
        self._pending = None
        self._settle()

    def _settle(self):
        """Upstream's clip bookkeeping at the top of its loop: seek is pulled up to the clip's start, and a clip that seek has reached the end
        of hands over to the next one, which starts at its own start."""
        while self.clip_idx < len(self.clips):
            start, stop = self.clips[self.clip_idx]
            self.seek = max(self.seek, start)
            if self.seek < stop:
                return
            self.clip_idx += 1
            if self.clip_idx < len(self.clips):
                self.seek = self.clips[self.clip_idx][0]

    @property
    def done(self):
        return self.clip_idx >= len(self.clips)

    def request(self):
        size = min(N_FRAMES, self.content_frames - self.seek, self.clips[self.clip_idx][1] - self.seek)
        return self.seek, size, self.all_tokens[self.prompt_reset_since:]

    def receive(self, result):
        seek, size, _ = self.request()
        window = {"seek": seek, "size": size, "advance": size, "skipped": False, "max_frames": None, "aligned": False}
        self.windows.append(window)
        if self.no_speech_threshold is not None:
            should_skip = result.no_speech_prob > self.no_speech_threshold
            if self.logprob_threshold is not None and result.avg_logprob > self.logprob_threshold:
                should_skip = False
            if should_skip:
                window["skipped"] = True
                self.seek += size
                self._settle()
                return None
        segments, advance, max_frames = split_window(result.tokens, self.tokenizer.timestamp_begin, self.tokenizer.eot, seek, size, result,
                                                     self.decode_text)
        window["max_frames"], window["advance"] = max_frames, advance
        self._pending = (window, segments, advance, result.temperature)
        return seek, size, max_frames, segments

    def commit(self, aligned=None):
        window, segments, advance, temperature = self._pending
        self._pending = None
        if aligned is not None:
            window["aligned"] = bool(aligned)
            self.without_words += 0 if window["aligned"] else 1
        self.seek += advance
        self._settle()
        self.all_segments.extend({"id": i, **seg} for i, seg in enumerate(segments, start=len(self.all_segments)))
        self.all_tokens.extend(t for seg in segments for t in seg["tokens"])
        # (as upstream: a window rescued at a high temperature does not condition the next one; a greedy result never gets here)
        if not self.condition_on_previous_text or (temperature is not None and temperature > 0.5):
            self.prompt_reset_since = len(self.all_tokens)

    def result(self):
        return {"segments": self.all_segments, "tokens": self.all_tokens, "windows": self.windows, "windows_without_words": self.without_words}


def seek_loop(n_frames, cut_window, decode_window, tokenizer, *, initial_prompt_tokens=(), condition_on_previous_text=True,
              no_speech_threshold=0.6, logprob_threshold=-1.0, align_window=None, decode_text=None, clips=None):
    """whisper.transcribe's loop over a log-mel of `n_frames` frames (the recording's frames plus 3000 of padding).
    cut_window(seek, size) -> mel window; decode_window(mel_window, prompt_tokens) -> DecodingResult (tokens, avg_logprob,
    no_speech_prob, ...); align_window(seek, size, max_frames, segments) -> bool fills the kept segments' "words" (False: the window
    got none); clips: SeekState's. Returns {"segments", "tokens" (initial prompt included), "windows", "windows_without_words"}."""
    st = SeekState(n_frames, tokenizer, initial_prompt_tokens=initial_prompt_tokens, condition_on_previous_text=condition_on_previous_text,
                   no_speech_threshold=no_speech_threshold, logprob_threshold=logprob_threshold, decode_text=decode_text, clips=clips)
    while not st.done:
        seek, size, prompt = st.request()
        pending = st.receive(decode_window(cut_window(seek, size), prompt))
        if pending is not None:
            st.commit(align_window(*pending) if align_window is not None else None)
    return st.result()


def attach_words(segments, words):
    """words: [{"word", "start", "end", "probability"}] of one window, in time order -> into the segment that contains their start."""
    live = [s for s in segments if s["tokens"]] or list(segments)
    for w in words:
        home = next((s for s in live if s["start"] <= w["start"] < s["end"]), None)
        if home is None:
            before = [s for s in live if s["start"] <= w["start"]]
            home = before[-1] if before else live[0]
        home["words"].append(w)


class WindowAligner:
    """The paper's aligner on the encoder state a round's decode left in the engine (make_aligner's result)."""

    def __init__(self, model, tokenizer, *, aligned_unit_type="char", word_confidence=False, word_alignment_score=False, **options):
        self.model, self.tokenizer, self.unit, self.word_confidence = model, tokenizer, aligned_unit_type, word_confidence
        self.word_alignment_score = word_alignment_score
        self.opts = aligner_options(model, tokenizer, **options)
        self.placeholder = [*tokenizer.sot_sequence, tokenizer.no_timestamps, tokenizer.encode(" a")[-1], tokenizer.eot]   # a row without words

    def prepare(self, max_frames, segments):
        """The framed token row the window is aligned with and its text tokens, or None where the window gets no words."""
        from .retokenize import encode, remove_punctuation
        tokenizer = self.tokenizer
        text = tokenizer.decode([t for seg in segments for t in seg["tokens"] if t < tokenizer.eot])
        try:
            text_tokens = encode(remove_punctuation(text), tokenizer, self.unit)
        except Exception:   # a character the byte-level dry-run tokenizer cannot encode
            return None
        tokens = [*tokenizer.sot_sequence, tokenizer.no_timestamps, *text_tokens, tokenizer.eot]
        if not text_tokens or len(tokens) > MAX_LENGTH or not 1 <= max_frames <= self.model.dims.n_audio_ctx:
            return None
        return tokens, text_tokens

    def attach(self, seek, segments, text_tokens, jump_row, logprob_row, path_rows=None):
        from .timing import word_alignment_scores, word_probabilities, words_from_jump_frames
        words, starts, ends = words_from_jump_frames(jump_row, text_tokens, self.tokenizer, self.unit)
        if not len(starts):
            return False
        probs = word_probabilities(logprob_row[:len(text_tokens)], text_tokens, self.tokenizer, self.unit) if self.word_confidence else None
        offset = seek * FRAME_SECONDS
        out = [{"word": words[i], "start": offset + float(starts[i]), "end": offset + float(ends[i]),
                "probability": probs[i] if probs is not None else None} for i in range(len(starts))]
        if path_rows is not None:   # (only then do the words carry the key)
            for w, s in zip(out, word_alignment_scores(path_rows[0], path_rows[1], text_tokens, self.tokenizer, self.unit)):
                w["alignment_score"] = s
        attach_words(segments, out)
        return True

    def align_round(self, rows, keys=None):
        """rows: one entry per row of the batch the last decode left in the engine, in order: (seek, size, max_frames, segments), or
        None for a row that was skipped. ONE align_batch(pcm=None) for the rows that have words; a row without (skipped, or refused by
        `prepare`) rides along as a minimal placeholder row whose output is dropped. Returns one bool per row (None for a skipped row).
        keys (which recording and piece a row belongs to) are HeadsWindowAligner's; this aligner carries nothing from round to round."""
        preps = [self.prepare(r[2], r[3]) if r is not None else None for r in rows]
        if not any(p is not None for p in preps):
            return [None if r is None else False for r in rows]   # nothing to align: the next decode drops the state
        token_rows = [p[0] if p is not None else self.placeholder for p in preps]
        max_frames = [r[2] if p is not None else PLACEHOLDER_FRAMES for r, p in zip(rows, preps)]
        res = self.model.align_batch(None, None, pad_token_rows(token_rows, self.tokenizer.eot).to(self.model.device), [len(t) for t in token_rows],
                                     max_frames, self.opts, token_logprobs_vocab_end=self.tokenizer.eot if self.word_confidence else None,
                                     **({"path_scores": True} if self.word_alignment_score else {}))
        out = []
        for b, (r, p) in enumerate(zip(rows, preps)):
            if r is None:
                out.append(None)
            elif p is None:
                out.append(False)
            else:
                out.append(self.attach(r[0], r[3], p[1], res[0][b][:len(token_rows[b])], res[2][b] if self.word_confidence else None,
                                       (res[-2][b], res[-1][b]) if self.word_alignment_score else None))
        return out

    def align_window(self, seek, size, max_frames, segments):
        """seek_loop's align_window: a round of one row."""
        return self.align_round([(seek, size, max_frames, segments)])[0]


class HeadsWindowAligner:
    """Upstream's aligner on the encoder state a round's decode left in the engine (word_aligner="heads"): the decoded text tokens of the
    kept segments themselves are framed -- no re-tokenisation, so a window has a few dozen rows, not hundreds of characters --, one
    align_batch(pcm=None, alignment_heads=True) per round runs upstream's find_alignment on the GPU (csrc/align_heads.hip), and
    word_timing.add_word_timestamps hands the words out: each with its leading space and its punctuation, so that a segment's words join
    to its text. last_speech_timestamp is carried from window to window per recording (and piece): `keys`."""

    def __init__(self, model, tokenizer, *, word_confidence=False, medfilt_width=3, prepend_punctuations=None, append_punctuations=None,
                 aligned_unit_type=None, aggr=None, topk=None, w_colnorm=None, w_rownorm=None, w_coverage=None):
        # (the last six are the character aligner's, which transcribe hands to either aligner: taken and not read; anything else is a TypeError)
        from . import word_timing
        self.model, self.tokenizer, self.word_confidence = model, tokenizer, word_confidence
        self.prepend = word_timing.PREPEND_PUNCTUATIONS if prepend_punctuations is None else prepend_punctuations
        self.append = word_timing.APPEND_PUNCTUATIONS if append_punctuations is None else append_punctuations
        self.opts = model.make_opts(sot_len=len(tokenizer.sot_sequence), medfilt_width=medfilt_width, qk_scale=1.0)
        self.placeholder = [*tokenizer.sot_sequence, tokenizer.no_timestamps, tokenizer.encode(" a")[-1], tokenizer.eot]   # a row without words
        self.last_speech = {}   # key -> the end of the last word of that recording's (piece's) windows so far

    def prepare(self, max_frames, segments):
        """The framed token row the window is aligned with and its text tokens, or None where the window gets no words."""
        tokenizer = self.tokenizer
        text_tokens = [t for seg in segments for t in seg["tokens"] if t < tokenizer.eot]
        tokens = [*tokenizer.sot_sequence, tokenizer.no_timestamps, *text_tokens, tokenizer.eot]
        if not text_tokens or len(tokens) > MAX_LENGTH or not 1 <= max_frames <= self.model.dims.n_audio_ctx:
            return None
        return tokens, text_tokens

    def attach(self, seek, segments, text_tokens, jump_row, logprob_row, key=None):
        from . import word_timing
        alignment = word_timing.alignment_from_jump_frames(jump_row, text_tokens, self.tokenizer, logprob_row if self.word_confidence else None)
        if not alignment:
            return False
        self.last_speech[key] = word_timing.add_word_timestamps(
            segments, alignment, self.tokenizer, time_offset=seek * FRAME_SECONDS, last_speech_timestamp=self.last_speech.get(key, 0.0),
            prepend_punctuations=self.prepend, append_punctuations=self.append)
        return any(seg["words"] for seg in segments)

    def align_round(self, rows, keys=None):
        """WindowAligner.align_round on the alignment-heads route; keys[b]: whose last_speech_timestamp row b reads and leaves."""
        preps = [self.prepare(r[2], r[3]) if r is not None else None for r in rows]
        if not any(p is not None for p in preps):
            return [None if r is None else False for r in rows]   # nothing to align: the next decode drops the state
        token_rows = [p[0] if p is not None else self.placeholder for p in preps]
        max_frames = [r[2] if p is not None else PLACEHOLDER_FRAMES for r, p in zip(rows, preps)]
        res = self.model.align_batch(None, None, pad_token_rows(token_rows, self.tokenizer.eot).to(self.model.device), [len(t) for t in token_rows],
                                     max_frames, self.opts, token_logprobs_vocab_end=self.tokenizer.eot if self.word_confidence else None,
                                     alignment_heads=True)
        out = []
        for b, (r, p) in enumerate(zip(rows, preps)):
            if r is None:
                out.append(None)
            elif p is None:
                out.append(False)
            else:
                out.append(self.attach(r[0], r[3], p[1], res[0][b][:len(token_rows[b])], res[2][b] if self.word_confidence else None,
                                       keys[b] if keys is not None else None))
        return out

    def align_window(self, seek, size, max_frames, segments):
        """seek_loop's align_window: a round of one row."""
        return self.align_round([(seek, size, max_frames, segments)])[0]


def make_aligner(model, tokenizer, *, word_aligner="char", **options):
    """The window aligner of a call: `.align_window` is the align_window that seek_loop takes, `.align_round` what the lock-step loop calls."""
    return (HeadsWindowAligner if word_aligner == "heads" else WindowAligner)(model, tokenizer, **options)


def clip_frames(clip_timestamps, content_frames):
    """upstream's clip_timestamps ("a,b,..." or a list of seconds: start, end, start, end, ...) -> [(start, stop)] in frames, round(ts * 100);
    an odd count is closed with content_frames, and none at all is the whole recording."""
    if isinstance(clip_timestamps, str):
        clip_timestamps = [float(ts) for ts in clip_timestamps.split(",")] if clip_timestamps else []
    elif isinstance(clip_timestamps, (int, float)):
        clip_timestamps = [clip_timestamps]
    points = [round(float(ts) * FRAMES_PER_SECOND) for ts in clip_timestamps] or [0]
    if len(points) % 2 == 1:
        points.append(content_frames)
    return list(zip(points[::2], points[1::2]))


PIECE_FRAMES_AUTO = 2 * N_FRAMES   # pieces="auto": at least two windows per piece, so that conditioning on previous text keeps a meaning
PIECE_RADIUS = 500                 # a cut may move 5 s off its equal share to find a quiet frame


def plan_pieces(content_frames, pieces, max_batch):
    """How many pieces a recording of content_frames frames is cut into, and how far a cut may move off its equal share: (n, radius) for
    model.quiet_cuts. pieces: an int, capped so that a piece has at least 4 frames, or "auto": min(max_batch, content_frames // 6000).
    radius = min(500, content_frames // n // 2 - 1), which keeps the search ranges of neighbouring cuts apart. n < 2: the recording is
    not split, (1, 0). An int above max_batch is a ValueError: every piece is one row of the decode batch."""
    if isinstance(pieces, str):
        if pieces.lower() != "auto":
            raise ValueError("pieces is an int or \"auto\", not %r" % (pieces,))
        n = min(int(max_batch), content_frames // PIECE_FRAMES_AUTO)
    else:
        n = int(pieces)
        if n < 1:
            raise ValueError("pieces must be at least 1, not %r" % (pieces,))
        if n > int(max_batch):
            raise ValueError("pieces=%d needs %d decode rows: more than model.max_batch = %d" % (n, n, max_batch))
        n = min(n, content_frames // 4)
    if n < 2:
        return 1, 0
    return n, min(PIECE_RADIUS, content_frames // n // 2 - 1)


def transcribe(model, audio, *, language, decode_window=None, **options):
    """whisper.transcribe(model, audio, ...) -> {"text", "segments": [{"id", "seek", "start", "end", "text", "tokens", "temperature",
    "avg_logprob", "compression_ratio", "no_speech_prob", "words": [{"word", "start", "end", "probability"}]}], "language"} plus
    "windows" (every decoded window: seek, size, advance, skipped, max_frames, aligned) and "windows_without_words".
    language: a code or name, or "auto": the language is detected on the first window ("language" is then the detected code and
    "language_probability", present only then, its probability) and the first decode runs on the encoder state detection left behind.
    audio: a path (audio.load_audio: any rate from 2 to 384 kHz, up to 8 channels), or a numpy array or tensor of mono samples [n] (or
    [channels, n]) at `sample_rate` Hz, any length. Audio that is not at 16 kHz is resampled on the GPU first (WhisperAMD.resample), as
    upstream's load_audio has ffmpeg do. word_timestamps=True: word times
    from the character aligner per window (module docstring); word_confidence=True adds each word's probability (None otherwise);
    word_alignment_score=True adds each word's "alignment_score" (timing.word_alignment_scores: the mean of the aggregated attention
    matrix along the word's stretch of the DTW path, in [0, 1]; uncalibrated), a key the words carry only then.
    clip_timestamps: upstream's "start,end,start,end,..." in seconds (a str or a list; an odd count runs to the end of the recording): only
    those ranges are transcribed, one after the other. pieces: an int or "auto" (plan_pieces): the recording is cut at quiet frames
    (WhisperAMD.quiet_cuts) into that many pieces, which are decoded side by side as the rows of ONE batch per round; every piece starts
    from initial_prompt only and conditions on its own previous text. The result then carries "pieces" and every window its "piece"
    (transcribe_batch has the details). pieces and clip_timestamps together are a ValueError. vad_filter=True (with vad_options, a dict, or
    None for the defaults): only the speech segments the engine's level detector finds are decoded, and the result gains
    "speech_segments" and "vad" (transcribe_batch has the details; not together with clip_timestamps or pieces).
    decode_window(mel_window, prompt_tokens) -> DecodingResult replaces the engine's greedy decode (tests; with pieces it is called row by
    row; with seed= it is also given temperature= and seed=, transcribe_batch's temperatures= / seeds= for its row); decode_options go to DecodingOptions. Limits: module docstring. It is transcribe_batch of one recording, whose single row is
    decoded and aligned alone. The other keywords and their defaults are transcribe_batch's."""
    def row_by_row(mel_windows, prompts, temperatures=None, seeds=None):
        if temperatures is None:
            return [decode_window(w, p) for w, p in zip(mel_windows, prompts)]
        return [decode_window(w, p, temperature=t, seed=s) for w, p, t, s in zip(mel_windows, prompts, temperatures, seeds)]   # (with seed=)

    if decode_window is None:
        row_by_row = None
    return transcribe_batch(model, [audio], language=language, decode_windows=row_by_row, **options)[0]


class _Call:
    """What one transcribe_batch call carries from round to round: the model and options, one tokenizer per language code, the initial prompt's
    tokens, and `state_left`: rows of encoded, undecoded state the engine's own detection left behind for the decode that comes next."""

    def __init__(self, model, language, initial_prompt, vocab_path, decode_options, decode_windows, detect_languages, seek_options, aligner_options,
                 temperatures=(0.0,), seed=None, compression_ratio_threshold=2.4, group_options=None):
        self.model, self.vocab_path, self.decode_options, self.seek_options = model, vocab_path, decode_options, seek_options
        self.group_options = group_options or {}   # beam_size / patience / best_of: which of them a row carries depends on its temperature
        self.temperatures, self.seed, self.compression_ratio_threshold = temperatures, seed, compression_ratio_threshold   # seed None: no ladder
        self.decode_windows, self.detect_languages, self.aligner_options = decode_windows, detect_languages, aligner_options   # (None: no words)
        self.auto = isinstance(language, str) and language.lower() == "auto"
        self.tokenizers, self.state_left, self.prompt_tokens = {}, None, []
        if initial_prompt is not None:
            self.prompt_tokens = decoding._text_tokens(self.tokenizer_for(None if self.auto else language), initial_prompt,
                                                       decoding.DecodingOptions(vocab_path=vocab_path), "initial_prompt")
        self.detect_tokenizer = None   # the engine's own detection, in the numbering the decode tokenizer uses
        if self.auto and detect_languages is None and model.is_multilingual:
            self.detect_tokenizer = get_tokenizer(True, num_languages=99)

    def tokenizer_for(self, code):   # (the special tokens but the language's own are the same in every language)
        if code not in self.tokenizers:
            self.tokenizers[code] = get_tokenizer(self.model.is_multilingual, language=code, task=self.decode_options.get("task", "transcribe"),
                                                  vocab_path=self.vocab_path)
        return self.tokenizers[code]

    def detect(self, mel_windows):
        """(codes, probabilities) of the rows of mel_windows; the engine's own detection leaves their encoded state behind."""
        if self.detect_languages is not None:
            return self.detect_languages(mel_windows)
        tok = self.detect_tokenizer
        tokens, probs = decoding.detect_language(self.model, mel_windows, tok)
        self.state_left = len(probs)
        codes = [tok.all_language_codes[int(t) - tok.all_language_tokens[0]] for t in tokens]
        return codes, [p[c] for c, p in zip(codes, probs)]

    def decode(self, code, mel_windows, prompts, seeks=None):
        """One round's decode: a DecodingResult per row, every row with its own previous text as the prompt. With a seed (seeks: the
        windows' first frames) the round walks upstream's temperature ladder: every row at temperatures[0]; then, while a row needs a
        fallback (needs_fallback) and rungs remain, the SAME encoded state is decoded again (decoding.decode(redecode=True): decoder
        positions only, where upstream encodes the window again) with the failed rows at the next temperature and the accepted rows
        riding along on a sample budget of 1, their output ignored: a decoded position costs about the same for 16 rows as for one. The
        last rung is accepted whatever it gives. Row b of rung r draws with window_seed(seed, seeks[b], r). The state is left decoded,
        for the round's one alignment."""
        if self.seed is None:
            return self.decode_windows(mel_windows, prompts) if self.decode_windows is not None else self.decode_rung(code, mel_windows, prompts)
        n, ladder = len(prompts), self.temperatures
        results, failed = [None] * n, [True] * n
        for rung, t in enumerate(ladder):
            seeds = [window_seed(self.seed, seek, rung) for seek in seeks]
            temps = [t if f else None for f in failed]   # None: the row is accepted; whatever it gives now is ignored
            if self.decode_windows is not None:
                got = self.decode_windows(mel_windows, prompts, temperatures=temps, seeds=seeds)
            else:
                got = self.decode_rung(code, mel_windows, prompts, temps, seeds, redecode=rung > 0)
            for b in range(n):
                if failed[b]:
                    results[b] = got[b]
                    failed[b] = rung + 1 < len(ladder) and needs_fallback(got[b], self.compression_ratio_threshold, self.seek_options["logprob_threshold"],
                                                                          self.seek_options["no_speech_threshold"])
            if not any(failed):
                break
        return results

    def decode_rung(self, code, mel_windows, prompts, temperatures=None, seeds=None, redecode=False):
        """The engine's decode of a round's rows. temperatures None: at temperature 0, the call it always was."""
        greedy = temperatures is None or all(t == 0.0 for t in temperatures)
        temperatures, seeds = temperatures or [0.0] * len(prompts), seeds or [None] * len(prompts)
        # upstream's decode_with_fallback: the beam (beam_size, patience) at temperature 0, best_of above it; a row that only rides along
        # (None) on a rung of sampled rows carries neither
        beam = {k: v for k, v in self.group_options.items() if k in ("beam_size", "patience") and v is not None}
        best = {k: v for k, v in self.group_options.items() if k == "best_of" and v is not None}
        rows = [decoding.DecodingOptions(language=code, temperature=0.0, prompt=list(p) or None, vocab_path=self.vocab_path,
                                         **(beam if greedy else {}), **self.decode_options)
                if greedy or not t else
                decoding.DecodingOptions(language=code, temperature=t, seed=s, prompt=list(p) or None, vocab_path=self.vocab_path, **best,
                                         **self.decode_options)
                for p, t, s in zip(prompts, temperatures, seeds)]
        want_text = self.vocab_path is not None
        if redecode:   # a later rung: the state of this round's first decode again, the accepted rows (None) for one token
            return decoding.decode(self.model, None, rows, encoded_batch=len(rows), want_text=want_text, redecode=True,
                                   row_sample_len=[None if t is not None else 1 for t in temperatures])
        waiting, self.state_left = self.state_left == len(rows), None
        if waiting:   # the first round of a group that detection found in one language: its state is waiting
            return decoding.decode(self.model, None, rows[0] if len(rows) == 1 else rows, encoded_batch=len(rows), want_text=want_text)
        if len(rows) == 1:   # a single row (transcribe(), or the last recording of a group): a uniform decode of one window
            return [decoding.decode(self.model, mel_windows[0], rows[0], want_text=want_text)]
        return decoding.decode(self.model, mel_windows, rows, want_text=want_text)


def plan_recording(mel, clip_timestamps, pieces, max_batch, model, vad=None):
    """What one recording contributes to the lock-step loop: (clips, pieces). clips: one SeekState(clips=...) argument per decode row it
    takes; pieces: the result's "pieces" entry (None unless pieces were asked for). vad (None, or the VAD options of vad_filter=True): the
    clips are the speech segments model.speech_segments finds in the mel, and a third entry holds the keys the result gains,
    {"speech_segments": [{"start_frame", "stop_frame"}], "vad": the stats}."""
    content = mel.shape[1] - N_FRAMES
    if vad is not None:
        if clip_timestamps is not None or pieces is not None:
            raise ValueError("vad_filter chooses the frame ranges itself: it cannot be combined with clip_timestamps or pieces")
        segments, stats = model.speech_segments(mel, **vad) if content >= 1 else ([], None)
        return ([[(int(a), int(b)) for a, b in segments]], None,
                {"speech_segments": [{"start_frame": int(a), "stop_frame": int(b)} for a, b in segments], "vad": stats})
    if clip_timestamps is not None:
        return [clip_frames(clip_timestamps, content)], None
    if pieces is None:
        return [None], None
    n, radius = plan_pieces(content, pieces, max_batch)
    cuts, levels = model.quiet_cuts(mel, n, radius=radius) if n > 1 else ([0, content], [])
    levels = [None, *levels]
    return ([[(cuts[k], cuts[k + 1])] for k in range(n)] if n > 1 else [None],   # (not split: the plain loop, as without pieces)
            [{"start_frame": cuts[k], "stop_frame": cuts[k + 1], "level": levels[k]} for k in range(n)])


def _prepared(model, audio, rate, clip_timestamps, pieces, max_batch, vad=None):
    mel = model.log_mel_long(as_pcm(audio, model, rate))
    return mel, plan_recording(mel, clip_timestamps, pieces, max_batch, model, vad)


def form_groups(model, audios, rates, clip_timestamps, pieces, max_batch, vad=None):
    """The groups of recordings that share the decode batch: yields (indices, mels, plans), mels and plans by index. A group holds as
    many recordings as their decode rows fit into max_batch (without pieces: max_batch recordings). A recording's log-mel is computed as
    it joins its group -- or one recording ahead, where the rows it takes depend on its length (pieces="auto") -- and is dropped when the
    next group is asked for: both dicts are valid until then."""
    group, mels, plans, used = [], {}, {}, 0
    for i, (audio, rate) in enumerate(zip(audios, rates)):
        ahead = _prepared(model, audio, rate, clip_timestamps, pieces, max_batch, vad) if isinstance(pieces, str) else None
        rows = 1 if pieces is None else len(ahead[1][0]) if ahead is not None else int(pieces)   # decode rows it takes in a round
        if group and used + rows > max_batch:
            yield group, mels, plans
            group, used = [], 0
            mels.clear(), plans.clear()
        mels[i], plans[i] = ahead or _prepared(model, audio, rate, clip_timestamps, pieces, max_batch, vad)
        group.append(i)
        used += rows
    if group:
        yield group, mels, plans


def detect_group(call, group, mels, plans):
    """language="auto" for one group, its first windows detected in ONE batch: (codes, extra) by recording, the language code (None
    where there was no window to look at) and {"language_probability": p}. The state detection left in the engine is dropped unless the
    detected rows are the first round's rows: one language, every recording heard, none with clips or pieces. With vad_filter the window
    starts at the first speech segment's start (an intro of silence is what a detection on frame 0 gets wrong), and a recording without
    a segment has no window."""
    codes, extra = {i: None for i in group}, {i: {"language_probability": None} for i in group}
    first = {i: plans[i][0][0][0][0] if plans[i][0][0] else None for i in group if len(plans[i]) > 2}   # vad_filter: where speech starts
    heard = [i for i in group if mels[i].shape[1] > N_FRAMES and first.get(i, 0) is not None]   # recordings that have a first window
    if call.detect_languages is None and call.detect_tokenizer is None:   # an English-only model: "en" without a detection pass, as upstream
        codes.update({i: "en" for i in heard})
    elif heard:
        found, probs = call.detect(cut_windows(call.model, mels, [(i, first.get(i, 0), min(N_FRAMES, mels[i].shape[1] - N_FRAMES - first.get(i, 0)))
                                                                  for i in heard]))
        for i, code, prob in zip(heard, found, probs):
            codes[i], extra[i] = code, {"language_probability": None if prob is None else float(prob)}
    if len(set(codes.values())) != 1 or heard != group or any(plans[i][0] != [None] for i in group):
        call.state_left = None   # the detected rows are not one decode batch: every language's first round encodes its own windows
    return codes, extra


def lock_step(call, code, rows, mels, plans):
    """The lock-step loop over the recordings `rows` of a group, all in language `code`: returns their SeekStates, finished, by
    (recording, piece). A recording takes one decode row per entry of its plan's clips (one, unless it is cut into pieces)."""
    tokenizer = call.tokenizer_for(code)
    aligner = make_aligner(call.model, tokenizer, **call.aligner_options) if call.aligner_options is not None else None
    states = {(i, k): SeekState(mels[i].shape[1], tokenizer, initial_prompt_tokens=call.prompt_tokens, clips=clips, **call.seek_options)
              for i in rows for k, clips in enumerate(plans[i][0])}   # (in recording, then piece order)
    while True:
        live = [u for u in states if not states[u].done]   # a finished recording (or piece) is never decoded again
        if not live:
            return states
        requests = [states[u].request() for u in live]
        windows = cut_windows(call.model, mels, [(u[0], seek, size) for u, (seek, size, _) in zip(live, requests)])
        decoded = call.decode(code, windows, [prompt for _, _, prompt in requests], [seek for seek, _, _ in requests])
        pending = [states[u].receive(r) for u, r in zip(live, decoded)]
        aligned = aligner.align_round(pending, live) if aligner is not None else [None] * len(live)
        for u, pend, al in zip(live, pending, aligned):
            if pend is not None:
                states[u].commit(al)


def merge_pieces(outs, pieces, *, tokenizer, language, extra, n_prompt):
    """A recording's result from the SeekState results of its pieces, in order (one piece: the state's own result): segment ids run on,
    "windows" are concatenated, each with its "piece" where pieces were asked for (pieces: the result's entry, else None), and the text
    is all tokens but the initial prompt's n_prompt, decoded by `tokenizer` (None without a vocabulary: "")."""
    segments, windows = [], []
    for k, out in enumerate(outs):
        for seg in out["segments"]:
            seg["id"] = len(segments)
            segments.append(seg)
        for w in out["windows"]:
            if pieces is not None:
                w["piece"] = k
            windows.append(w)
    tokens = [t for out in outs for t in out["tokens"][n_prompt:]]
    result = {"text": tokenizer.decode(tokens) if tokenizer is not None else "", "segments": segments, "language": language, **extra,
              "windows": windows, "windows_without_words": sum(out["windows_without_words"] for out in outs)}
    if pieces is not None:
        result["pieces"] = pieces
    return result


def transcribe_batch(model, audios, *, language, initial_prompt=None, condition_on_previous_text=True, no_speech_threshold=0.6,
                     logprob_threshold=-1.0, word_timestamps=False, word_confidence=False, aligned_unit_type="char", aggr="topk", topk=10,
                     medfilt_width=3, word_alignment_score=False, vocab_path=None, temperature=0.0, w_colnorm=1.0, w_rownorm=1.0, w_coverage=0.0, decode_windows=None,
                     detect_languages=None, sample_rate=SAMPLE_RATE, clip_timestamps=None, pieces=None, seed=None,
                     compression_ratio_threshold=2.4, beam_size=None, patience=None, length_penalty=None, best_of=None, vad_filter=False,
                     vad_options=None, word_aligner="char", prepend_punctuations=None, append_punctuations=None, **decode_options):
    """transcribe() of several recordings in lock-step: a list with transcribe()'s result for every recording of `audios`, in order.
    Each round cuts the next window of every unfinished recording, decodes them in ONE batch with every row's own previous text as its
    prompt (decoding.decode with one DecodingOptions per row: wca_decode with per_row 1) and, with word_timestamps, aligns the rows that
    have words in one align_batch(pcm=None) on the state that decode left behind. The batch shrinks as recordings end; more recordings
    than model.max_batch are processed in groups of max_batch. The keyword arguments are transcribe()'s; sample_rate is one int for
    every array / tensor input or one per recording (a path carries its own rate);
    decode_windows(mel_windows [B, n_mels, 3000], prompts: B token lists) -> B DecodingResults replaces the engine's decode (tests).
    language="auto": the first windows of a group are detected in one batch (detect_languages(mel_windows [B, n_mels, 3000]) ->
    (B codes, B probabilities) replaces the engine's detection: tests), the group is partitioned by detected language and the
    lock-step loop runs once per language (one decode cannot mix languages); the results still come back in input order, each with
    its own "language" and "language_probability". A group that comes out in ONE language decodes its first round on the encoder state
    detection left in the engine (no second encoder pass); a group with several languages is simply re-encoded, language by language.
    clip_timestamps (upstream's, in seconds; the same for every recording): every recording's loop runs over those ranges only
    (SeekState(clips=...)).
    pieces (an int or "auto"; not together with clip_timestamps): every recording is cut into n pieces (plan_pieces; a short recording
    into fewer, or not at all) at the quietest even frame near each equal share (model.quiet_cuts) and contributes one SeekState per
    piece, with clips=[(cuts[k], cuts[k + 1])], to the lock-step loop: round r decodes the r-th window of every unfinished piece of every
    recording of the group in one batch. Every piece starts from initial_prompt only and conditions on its own previous text. A group
    holds as many recordings as their pieces fit into max_batch rows (max_batch // n for an int; for "auto" a recording's share depends on
    its length, so its log-mel is computed before the group it ends up in is closed). A round's windows are cut with ONE mel_window call
    per recording. The pieces are merged in order: segment ids run on, "windows" are concatenated, each with its "piece", and the result
    carries "pieces": [{"start_frame", "stop_frame", "level"}], level being the smoothed level (wca_quiet_cuts) at the cut the piece starts
    at, None for the first. language="auto" still detects on the recording's first window and all its pieces take that language; the first
    round then has other rows than the detection saw, so the state detection left in the engine is simply dropped and the round encodes
    its own windows. Without pieces and clip_timestamps the result is what it was before either existed.
    vad_filter (False: no key is added and no kernel launched; not together with clip_timestamps or pieces): every recording's speech
    segments (WhisperAMD.speech_segments on its log-mel, with vad_options: a dict of its options, None for the defaults) are the clips its
    loop runs over, so silence is never decoded; times stay absolute. The result gains "speech_segments": [{"start_frame", "stop_frame"}]
    and "vad": the detector's stats. language="auto" then detects on the window that starts at the first segment, and a recording
    without a segment reports "language": None. The detector is exact against its definition; its defaults are UNVALIDATED on real
    speech (module docstring).
    seed (an int; None: temperature 0.0 only, every call as it always was) switches on upstream's temperature fallback: temperature may
    then be a number or a tuple such as upstream's default (0.0, 0.2, 0.4, 0.6, 0.8, 1.0), and a window whose result is too repetitive
    (compression_ratio > compression_ratio_threshold) or too improbable (avg_logprob < logprob_threshold), and not taken for silence, is
    decoded again at the next temperature (_Call.decode; needs_fallback) with the seed window_seed(seed, seek, rung). A threshold of None
    switches its test off; without a vocabulary there is no text, the compression ratio is NaN and that test never fires. A segment's
    "temperature" is the rung its window was accepted at, and a window accepted above 0.5 does not condition the next one. With a seed
    decode_windows is also given temperatures= (one per row; None for a row whose earlier result was kept and whose new one is ignored)
    and seeds= (one per row). The law of the draws is upstream's, the draws are not (decoding.decode); what the ladder does to real
    speech is UNVALIDATED here (module docstring).
    beam_size, patience, length_penalty, best_of (upstream's; all None: every call as it always was): as upstream's decode_with_fallback, a
    window at temperature 0 is decoded by beam search (beam_size beams, a finished list of round(beam_size * patience) sequences) and a
    window on a rung above 0 as the best of best_of independent samples (which therefore needs a seed); the winner is
    MaximumLikelihoodRanker's, with length_penalty. Every window then takes G = max(beam_size, best_of) decoder rows (C ABI
    wca_decode_group), so a round holds at most max_batch // G windows and G above max_batch is a ValueError. What is pinned: the beam
    step and the cache reorder against a float64 restatement of upstream's BeamSearchDecoder, the loop against the fp32 oracle
    (tests/test_beam_step_gpu.py, tests/test_decode_beam_gpu.py). PARITY with upstream itself stays UNPINNED, as for decode.
    word_aligner ("char", the default: every call as it always was, and nothing new runs; or "heads"): with word_timestamps, "heads" takes
    upstream's words instead of the character aligner's (HeadsWindowAligner): the decoded tokens themselves are aligned over
    model.alignment_heads by upstream's find_alignment on the GPU (align_batch(alignment_heads=True)) and handed out by a restatement of
    upstream's add_word_timestamps (word_timing), so every word carries its leading space and its punctuation and a segment's words join
    to its text; segment starts and ends follow their first and last word as upstream's do. prepend_punctuations / append_punctuations
    are upstream's (None: upstream's defaults) and belong to "heads" only, as word_alignment_score belongs to "char" only: the other
    combination is a ValueError before any audio is read. medfilt_width is this keyword's value (3 here; upstream's own default is 7);
    aligned_unit_type, aggr, topk and the w_* weights are the character aligner's and are not read. A model without an official head
    table (model.alignment_heads_source) aligns over every head of the upper decoder half, and a warning says so. "probability" stays
    None unless word_confidence=True. hallucination_silence_threshold and upstream's re-seek to the last word's end are not built.
    PARITY with upstream is UNPINNED and quality on speech UNVALIDATED (word_timing's docstring)."""
    temperatures = check_supported(temperature, language, seed)
    group_options = dict(beam_size=beam_size, patience=patience, best_of=best_of)
    if length_penalty is not None:
        decode_options = dict(decode_options, length_penalty=length_penalty)
    if beam_size is not None or best_of is not None or patience is not None:
        # (the checks of decoding._check_supported, before any audio is read; a probe per kind of row the ladder will build)
        if beam_size is not None and best_of is not None and seed is None:
            raise ValueError("best_of is for the rungs above temperature 0: it needs seed=<int> and a temperature ladder that reaches them")
        if beam_size is not None or patience is not None:
            decoding._check_supported(decoding.DecodingOptions(language="en", beam_size=beam_size, patience=patience, length_penalty=length_penalty), grouped=True)
        if best_of is not None:
            if seed is None:
                raise ValueError("best_of draws samples: it needs seed=<int>, as all sampling here does")
            decoding._check_supported(decoding.DecodingOptions(language="en", temperature=1.0, seed=0, best_of=best_of, length_penalty=length_penalty),
                                       grouped=True)
    if pieces is not None and clip_timestamps is not None:
        raise ValueError("pieces cuts the whole recording: it cannot be combined with clip_timestamps")
    if vad_filter and (clip_timestamps is not None or pieces is not None):
        raise ValueError("vad_filter chooses the frame ranges itself: it cannot be combined with clip_timestamps or pieces (cutting pieces "
                         "inside speech only is not built)")
    if vad_options is not None and not vad_filter:
        raise ValueError("vad_options are the options of vad_filter=True")
    vad = dict(vad_options or {}) if vad_filter else None
    if word_confidence and not word_timestamps:
        raise ValueError("word_confidence is a property of the aligned words: it needs word_timestamps=True")
    if word_alignment_score and not word_timestamps:
        raise ValueError("word_alignment_score is a property of the aligned words: it needs word_timestamps=True")
    if word_timestamps and vocab_path is None:
        raise ValueError("word_timestamps aligns the decoded TEXT: pass vocab_path=<local *.tiktoken file>")
    if word_aligner not in ("char", "heads"):
        raise ValueError("word_aligner is \"char\" or \"heads\", not %r" % (word_aligner,))
    if word_aligner == "char" and (prepend_punctuations is not None or append_punctuations is not None):
        raise ValueError("prepend_punctuations / append_punctuations belong to upstream's word aligner: pass word_aligner=\"heads\"")
    if word_aligner == "heads":
        if not word_timestamps:
            raise ValueError("word_aligner chooses how the words are aligned: it needs word_timestamps=True")
        if word_alignment_score:
            raise ValueError("word_alignment_score is defined on the character aligner's [0, 1] matrix: not with word_aligner=\"heads\"")
        if str(getattr(model, "alignment_heads_source", "")).startswith("default"):
            import warnings
            warnings.warn("word_aligner=\"heads\" on a model without an official alignment-head table: aligning over %s "
                          "(model.alignment_heads_source; see use_official_alignment_heads / set_alignment_heads)" % model.alignment_heads_source)
    max_batch = int(getattr(model, "max_batch", 1))
    if max_batch < 1:
        raise ValueError("transcribe_batch needs model.max_batch >= 1")
    n_group = max(beam_size or 1, best_of or 1)
    if n_group > max_batch:
        raise ValueError("beam_size / best_of = %d needs %d decoder rows per window: more than model.max_batch = %d" % (n_group, n_group, max_batch))
    max_batch //= n_group   # windows per round: each takes n_group decoder rows
    if pieces is not None:
        plan_pieces(4 * max_batch, pieces, max_batch)   # (what does not depend on the recording is refused before any audio is read)
    seek = dict(condition_on_previous_text=condition_on_previous_text, no_speech_threshold=no_speech_threshold, logprob_threshold=logprob_threshold)
    words = dict(aligned_unit_type=aligned_unit_type, aggr=aggr, topk=topk, medfilt_width=medfilt_width, w_colnorm=w_colnorm,
                 w_rownorm=w_rownorm, w_coverage=w_coverage, word_confidence=word_confidence) if word_timestamps else None
    if word_alignment_score:   # (otherwise the aligner is made as it always was)
        words["word_alignment_score"] = True
    if word_aligner == "heads":   # (likewise)
        words.update(word_aligner="heads", prepend_punctuations=prepend_punctuations, append_punctuations=append_punctuations)
    call = _Call(model, language, initial_prompt, vocab_path, decode_options, decode_windows, detect_languages, seek, words,
                 *(() if seed is None else (temperatures, int(seed), compression_ratio_threshold)), group_options=group_options)
    audios = list(audios)
    results = [None] * len(audios)
    for group, mels, plans in form_groups(model, audios, sample_rates(sample_rate, len(audios)), clip_timestamps, pieces, max_batch, vad):
        codes, extra = detect_group(call, group, mels, plans) if call.auto else ({i: language for i in group}, {})
        for code in dict.fromkeys(codes[i] for i in group):   # one decode cannot mix languages: the loop runs once per language
            rows = [i for i in group if codes[i] == code]
            states = lock_step(call, code, rows, mels, plans)
            for i in rows:
                outs = [states[(i, k)].result() for k in range(len(plans[i][0]))]
                results[i] = merge_pieces(outs, plans[i][1], tokenizer=call.tokenizer_for(code) if vocab_path is not None else None,
                                          language=code, extra={**extra.get(i, {}), **(plans[i][2] if len(plans[i]) > 2 else {})},
                                          n_prompt=len(call.prompt_tokens))
    return results


# ------------------------------------------------------------------------------------------------ command line
VAD_OPTION_HELP = {   # the options of WhisperAMD.speech_segments (include/wca.h: wca_vad_opts), durations in frames of 10 ms
    "half_width": "the level is smoothed over 2 half_width + 1 frames (default 7)",
    "floor_permille": "the noise floor is this permille quantile of the level (default 50)",
    "peak_permille": "the peak is this permille quantile of the level (default 950)",
    "on_share": "speech starts above floor + on_share / 1024 of the range (default 410)",
    "off_share": "and ends below floor + off_share / 1024 of the range (default 307)",
    "min_range": "a range below this, in 1/4096 of a log-mel unit per mel row, is no speech / silence contrast: nothing is dropped (default 1024)",
    "min_speech": "shorter runs of speech are dropped (default 25)",
    "min_silence": "shorter gaps between speech are closed (default 200)",
    "pad": "every run is widened by this on both sides (default 40)",
}


def _pieces_arg(value):
    return "auto" if value.lower() == "auto" else int(value)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Long-form transcription with character-aligned word times (one JSON per recording)")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--audio", type=str, help="one recording (WAV / SPHERE / FLAC at any rate from 2 to 384 kHz, or a raw .npy array)")
    src.add_argument("--scp", type=str, help="list of recordings: `<id> <path>` or `<path>` per line")
    p.add_argument("--output_dir", type=str, required=True)
    add_model_options(p)
    p.add_argument("--vocab", type=str, default=None, help="local tiktoken vocabulary file (text output, word times)")
    p.add_argument("--language", type=str, default="en", help="a language code or name, or `auto`: detected on each recording's first window "
                   "(the detected code and its probability go into the output JSON)")
    p.add_argument("--initial_prompt", type=str, default=None)
    p.add_argument("--no_condition_on_previous_text", action="store_true")
    p.add_argument("--word_timestamps", action="store_true")
    p.add_argument("--word_confidence", action="store_true")
    # (absent from the namespace unless given, like the ladder's options below: the parsed defaults are what they were)
    p.add_argument("--word_alignment_score", action="store_true", default=argparse.SUPPRESS, help="with --word_timestamps: every word also gets its `alignment_score`, the "
                   "mean of the aggregated attention matrix along its stretch of the DTW path (in [0, 1]; uncalibrated)")
    add_aligner_options(p)
    # upstream's own word aligner (likewise absent unless given)
    p.add_argument("--word_aligner", choices=["char", "heads"], default=argparse.SUPPRESS, help="with --word_timestamps: `heads` aligns the decoded "
                   "tokens over the model's alignment heads as openai-whisper does (words keep their spaces and punctuation); default char")
    p.add_argument("--prepend_punctuations", type=str, default=argparse.SUPPRESS, help="with --word_aligner heads: merged with the next word "
                   "(default: upstream's)")
    p.add_argument("--append_punctuations", type=str, default=argparse.SUPPRESS, help="with --word_aligner heads: merged with the previous word "
                   "(default: upstream's)")
    p.add_argument("--pieces", type=_pieces_arg, default=None, metavar="N|auto", help="cut every recording at quiet frames into N pieces that are "
                   "decoded side by side (auto: as many as --batch rows allow, at least 60 s each); needs --batch >= N")
    p.add_argument("--clip_timestamps", type=str, default=None, metavar="a,b,...", help="transcribe only these ranges: start,end,start,end,... in "
                   "seconds (an odd count runs to the end of the recording)")
    # the temperature fallback (needs --seed). An option that is not given is absent from the namespace (main reads the defaults named here):
    # without --seed the parsed arguments and the call they make are what they were before the ladder existed
    ladder = dict(default=argparse.SUPPRESS)
    p.add_argument("--seed", type=int, help="switches on the temperature fallback: windows that loop or are improbable are decoded again with "
                   "sampling, reproducibly for this seed (default: none, temperature 0 only)", **ladder)
    p.add_argument("--temperature", type=float, help="the first temperature (default 0; anything else needs --seed)", **ladder)
    p.add_argument("--temperature_increment_on_fallback", type=float, help="the ladder's step up to 1.0 (upstream's default is 0.2; default: "
                   "none, --temperature alone)", **ladder)
    p.add_argument("--compression_ratio_threshold", type=float, help="default 2.4", **ladder)
    # beam search and best_of (upstream's options; likewise absent unless given). Each window takes max(beam_size, best_of) of the --batch rows
    p.add_argument("--beam_size", type=int, help="beams of the search at temperature 0 (upstream's command line runs 5; default: none, greedy)", **ladder)
    p.add_argument("--patience", type=float, help="the search ends after round(beam_size * patience) finished sequences (default 1.0)", **ladder)
    p.add_argument("--length_penalty", type=float, help="alpha of the ranker's length normalisation (default: none, sum / length)", **ladder)
    p.add_argument("--best_of", type=int, help="independent samples per window on the rungs above temperature 0 (needs --seed)", **ladder)
    # speech activity first (likewise absent unless given): --vad_filter, and one option per parameter of the detector
    p.add_argument("--vad_filter", action="store_true", help="find the speech first (a level detector on the GPU) and decode only that; its "
                   "defaults are unvalidated on real speech", **ladder)
    for name, text in VAD_OPTION_HELP.items():
        p.add_argument("--vad_" + name, type=int, help="with --vad_filter: " + text, **ladder)
    return p.parse_args(argv)


def temperature_ladder(temperature, increment):
    """upstream's cli: np.arange(temperature, 1.0 + 1e-6, increment) as a tuple, or the one temperature without an increment."""
    if increment is None:
        return (float(temperature),)
    return tuple(float(t) for t in np.arange(temperature, 1.0 + 1e-6, increment))


def _recordings(args):
    if args.audio:
        return [(os.path.splitext(os.path.basename(args.audio))[0], args.audio)]
    out = []
    with open(args.scp) as f:
        for line in f:
            parts = line.split()
            if parts:
                out.append((parts[0] if len(parts) > 1 else os.path.splitext(os.path.basename(parts[0]))[0], parts[-1]))
    return out


def main(args, model=None):
    """Writes <output_dir>/<id>.json per recording (transcribe()'s result plus "audio"); returns the paths."""
    if args.word_timestamps and args.vocab is None:
        raise SystemExit("--word_timestamps aligns the decoded text: pass --vocab <local multilingual.tiktoken>")
    if args.batch < 1:
        raise SystemExit("--batch must be at least 1")
    if isinstance(args.pieces, int) and not 1 <= args.pieces <= args.batch:
        raise SystemExit("--pieces %d needs --batch >= %d: every piece is one row of the decode batch" % (args.pieces, args.pieces))
    if args.pieces is not None and args.clip_timestamps is not None:
        raise SystemExit("--pieces cuts the whole recording: it cannot be combined with --clip_timestamps")
    vad_options = {name: getattr(args, "vad_" + name) for name in VAD_OPTION_HELP if getattr(args, "vad_" + name, None) is not None}
    if vad_options and not getattr(args, "vad_filter", False):
        raise SystemExit("--vad_%s is an option of --vad_filter" % next(iter(vad_options)))
    if getattr(args, "vad_filter", False) and (args.pieces is not None or args.clip_timestamps is not None):
        raise SystemExit("--vad_filter chooses the frame ranges itself: it cannot be combined with --pieces or --clip_timestamps")
    if model is None:
        model = load_model(args)
    os.makedirs(args.output_dir, exist_ok=True)
    paths = []
    kw = dict(language=args.language, initial_prompt=args.initial_prompt, condition_on_previous_text=not args.no_condition_on_previous_text,
              word_timestamps=args.word_timestamps, word_confidence=args.word_confidence, vocab_path=args.vocab, sample_rate=args.sample_rate,
              **{k: getattr(args, k) for k in ALIGNER_KEYWORDS})
    if args.pieces is not None or args.clip_timestamps is not None:   # (otherwise the call is what it was before either existed)
        kw.update(pieces=args.pieces, clip_timestamps=args.clip_timestamps)
    if getattr(args, "seed", None) is not None:   # (likewise: without --seed the call is what it was)
        kw.update(seed=args.seed, compression_ratio_threshold=getattr(args, "compression_ratio_threshold", 2.4),
                  temperature=temperature_ladder(getattr(args, "temperature", 0.0), getattr(args, "temperature_increment_on_fallback", None)))
    elif getattr(args, "temperature", 0.0) != 0.0 or getattr(args, "temperature_increment_on_fallback", None) is not None:
        raise SystemExit("--temperature / --temperature_increment_on_fallback sample: pass --seed <int>")
    if getattr(args, "word_alignment_score", False):   # (likewise)
        kw["word_alignment_score"] = True
    if getattr(args, "vad_filter", False):   # (likewise)
        kw["vad_filter"] = True
        if vad_options:
            kw["vad_options"] = vad_options
    for name in ("beam_size", "patience", "length_penalty", "best_of", "word_aligner", "prepend_punctuations", "append_punctuations"):   # (likewise: given options only)
        if getattr(args, name, None) is not None:
            kw[name] = getattr(args, name)
    for group in groups_of(_recordings(args), args.batch):   # a group's files are written before the next group starts
        if args.batch > 1:
            results = transcribe_batch(model, [source(path) for _, path in group], **kw)
        else:
            results = [transcribe(model, source(group[0][1]), **kw)]
        for (rec_id, path), result in zip(group, results):
            out = os.path.join(args.output_dir, rec_id + ".json")
            with open(out, "w") as f:
                json.dump({"audio": path, **result}, f)
            paths.append(out)
            print("%s: %d segments, %d windows -> %s" % (rec_id, len(result["segments"]), len(result["windows"]), out))
    return paths


if __name__ == "__main__":
    main(parse_args())
