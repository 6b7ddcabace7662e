"""Test helper: a numpy / int64 restatement of the speech-segment definition (include/wca.h: wca_speech_segments), written from the
definition and not from the kernels (csrc/speech_segments.hip), as tests/quiet_cuts_ref.py restates the quiet cuts.

    q(x), e[t], s[t]   exactly the quiet cuts' (quiet_cuts_ref.smoothed_level)
    lo, hi             the r-th smallest (0-based) of {s[t]}, r = (cf - 1) * floor_permille // 1000 and (cf - 1) * peak_permille // 1000
    flat               (hi - lo) < min_range * n_mels * (2 half_width + 1)
    on_thr, off_thr    lo + (((hi - lo) * on_share) >> 10), lo + (((hi - lo) * off_share) >> 10)
    a0[t]              1 if s[t] >= on_thr; 0 if s[t] < off_thr; else a0[t - 1], a0[-1] = 0
    close              a maximal run of 0 shorter than min_silence with a 1 on both sides becomes 1
    open               then a maximal run of 1 shorter than min_speech becomes 0
    pad                then every run [a, b) becomes [max(0, a - pad), min(cf, b + pad)); runs that overlap or touch merge
    result             the runs in order; if flat: the one pair (0, cf)

Everything after q is Python / int64 integer arithmetic. It works on RUNS (np.sort for the two order statistics, np.maximum.accumulate
over the indices of the decisive frames, then the run lists), which is not how kernels that scan over frames do it; a million frames
take seconds."""
import numpy as np

import quiet_cuts_ref

DEFAULTS = dict(half_width=7, floor_permille=50, peak_permille=950, on_share=410, off_share=307, min_range=1024, min_speech=25, min_silence=200,
                pad=40)
OPTION_NAMES = tuple(DEFAULTS)   # the order of wca_vad_opts
STAT_NAMES = ("lo", "hi", "on_thr", "off_thr", "flat", "n_segments")


def options(**changes):
    unknown = set(changes) - set(DEFAULTS)
    if unknown:
        raise ValueError("unknown option %r" % sorted(unknown))
    return dict(DEFAULTS, **changes)


def valid(content_frames, ld, **changes):
    """The argument ranges outside which wca_speech_segments returns WCA_ERR_INVALID."""
    o = options(**changes)
    return (1 <= content_frames <= ld and content_frames < 2 ** 31 and 0 <= o["half_width"] <= 100
            and 0 <= o["floor_permille"] <= o["peak_permille"] <= 1000 and 1 <= o["on_share"] <= 1023 and 0 <= o["off_share"] <= o["on_share"]
            and 0 <= o["min_range"] <= 32768 and 1 <= o["min_speech"] <= 2 ** 24 and 1 <= o["min_silence"] <= 2 ** 24 and 0 <= o["pad"] <= 2 ** 24)


def thresholds(s, n_mels, o):
    """(lo, hi, on_thr, off_thr, flat) of the smoothed levels s (int64 [cf])."""
    cf = len(s)
    srt = np.sort(s)
    lo, hi = int(srt[(cf - 1) * o["floor_permille"] // 1000]), int(srt[(cf - 1) * o["peak_permille"] // 1000])
    flat = (hi - lo) < o["min_range"] * n_mels * (2 * o["half_width"] + 1)
    return lo, hi, lo + (((hi - lo) * o["on_share"]) >> 10), lo + (((hi - lo) * o["off_share"]) >> 10), int(flat)


def runs_of(active):
    """The maximal runs of True as two int64 arrays (starts, stops)."""
    edge = np.diff(np.concatenate([[0], np.asarray(active, dtype=np.int8), [0]]))
    return np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)


def _merge(starts, stops, joined):
    """joined[i]: run i and run i + 1 become one."""
    keep = ~np.asarray(joined, dtype=bool)
    return starts[np.concatenate([[True], keep])], stops[np.concatenate([keep, [True]])]


def segments_of_levels(s, n_mels, **changes):
    """-> (segments: list of (start, stop), stats: dict) of the smoothed levels s."""
    o = options(**changes)
    s = np.asarray(s, dtype=np.int64)
    cf = len(s)
    lo, hi, on_thr, off_thr, flat = thresholds(s, n_mels, o)
    decisive = (s >= on_thr) | (s < off_thr)
    last = np.maximum.accumulate(np.where(decisive, np.arange(cf), -1))
    a0 = (last >= 0) & (s[np.maximum(last, 0)] >= on_thr)
    starts, stops = runs_of(a0)
    if len(starts):
        starts, stops = _merge(starts, stops, starts[1:] - stops[:-1] < o["min_silence"])          # close
        long_enough = stops - starts >= o["min_speech"]                                              # open
        starts, stops = starts[long_enough], stops[long_enough]
    if len(starts):
        starts, stops = np.maximum(starts - o["pad"], 0), np.minimum(stops + o["pad"], cf)           # pad
        starts, stops = _merge(starts, stops, starts[1:] <= stops[:-1])
    segments = [(0, cf)] if flat else [(int(a), int(b)) for a, b in zip(starts, stops)]
    return segments, dict(zip(STAT_NAMES, (lo, hi, on_thr, off_thr, flat, len(segments))))


def speech_segments(mel, content_frames=None, **changes):
    """-> (segments, stats). mel [n_mels][T] float32; content_frames defaults to T - 3000."""
    mel = np.asarray(mel)
    if content_frames is None:
        content_frames = mel.shape[1] - 3000
    if not valid(content_frames, mel.shape[1], **changes):
        raise ValueError("invalid arguments")
    s = quiet_cuts_ref.smoothed_level(mel, content_frames, options(**changes)["half_width"])
    return segments_of_levels(s, mel.shape[0], **changes)
