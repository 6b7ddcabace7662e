"""CPU tests around the speech segments (include/wca.h: wca_speech_segments): the numpy restatement (tests/speech_segments_ref.py) against
a slow loop over frames written separately, the definition on the one real recording at hand, timing.trim_words_to_speech, the wiring of
vad_filter through transcribe's plan (a stub model whose speech_segments is scripted) and the two command lines. The kernels themselves
are tests/test_speech_segments_gpu.py's, the engine's decode under vad_filter tests/test_transcribe_vad_gpu.py's."""
import importlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import speech_segments_ref as ref
import test_transcribe_pieces as stub   # (its stub model, scripted decoder and recordings)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _m(n):
    return importlib.import_module("whisper-char-alignment_amd." + n)


@pytest.fixture(scope="module")
def tr():
    return _m("transcribe")


@pytest.fixture(scope="module")
def decoding():
    return _m("decoding")


@pytest.fixture(scope="module")
def tok():
    return _m("tokenizer").get_tokenizer(True, language="en", task="transcribe")


# ------------------------------------------------------------------------------------------------ the restatement against a slow loop
def _slow(s, n_mels, **changes):
    """The definition, one frame and one run at a time."""
    o = ref.options(**changes)
    cf = len(s)
    ordered = sorted(int(v) for v in s)
    lo, hi = ordered[(cf - 1) * o["floor_permille"] // 1000], ordered[(cf - 1) * o["peak_permille"] // 1000]
    flat = (hi - lo) < o["min_range"] * n_mels * (2 * o["half_width"] + 1)
    on_thr, off_thr = lo + (((hi - lo) * o["on_share"]) >> 10), lo + (((hi - lo) * o["off_share"]) >> 10)
    active, state = [], 0
    for t in range(cf):
        state = 1 if s[t] >= on_thr else 0 if s[t] < off_thr else state
        active.append(state)

    def runs(value):
        out, t = [], 0
        while t < cf:
            u = t
            while u < cf and active[u] == value:
                u += 1
            if u > t:
                out.append((t, u))
            t = max(u, t + 1)
        return out

    for a, b in runs(0):
        if a > 0 and b < cf and b - a < o["min_silence"]:
            active[a:b] = [1] * (b - a)
    for a, b in runs(1):
        if b - a < o["min_speech"]:
            active[a:b] = [0] * (b - a)
    segments = []
    for a, b in runs(1):
        a, b = max(0, a - o["pad"]), min(cf, b + o["pad"])
        if segments and a <= segments[-1][1]:
            segments[-1] = (segments[-1][0], max(b, segments[-1][1]))
        else:
            segments.append((a, b))
    if flat:
        segments = [(0, cf)]
    return segments, dict(zip(ref.STAT_NAMES, (lo, hi, on_thr, off_thr, int(flat), len(segments))))


def _random_options(rng, scale):
    o = dict(half_width=0, floor_permille=int(rng.integers(0, 500)), on_share=int(rng.integers(1, 1024)), min_range=int(rng.integers(0, 3)) * 20,
             min_speech=int(rng.integers(1, scale)), min_silence=int(rng.integers(1, scale)), pad=int(rng.integers(0, scale)))
    o["peak_permille"] = int(rng.integers(o["floor_permille"], 1001))
    o["off_share"] = int(rng.integers(0, o["on_share"] + 1))
    return o


def test_restatement_equals_the_slow_loop_on_random_levels_and_options():
    rng = np.random.default_rng(0)
    seen_flat, seen_empty, seen_many = 0, 0, 0
    for trial in range(600):
        cf = int(rng.integers(1, 120))
        if trial % 3 == 0:
            s = rng.integers(-50, 50, cf)
        elif trial % 3 == 1:
            s = np.repeat(rng.integers(0, 3, cf), rng.integers(1, 6, cf))[:cf] * 100   # plateaus: the middle level sits inside the band
        else:
            s = np.cumsum(rng.integers(-3, 4, cf)) * 10
        o = _random_options(rng, 9)
        want, got = _slow(s, 1, **o), ref.segments_of_levels(s, 1, **o)
        assert got == want, (trial, list(s), o)
        seen_flat += got[1]["flat"]
        seen_empty += not got[0]
        seen_many += len(got[0]) > 2
    assert seen_flat > 20 and seen_empty > 20 and seen_many > 20   # (the trials reach every kind of result)


def test_restatement_by_hand():
    lvl = np.array([0] * 10 + [1000] * 5 + [0] * 3 + [1000] * 5 + [0] * 10 + [1000] * 2 + [0] * 10)
    o = dict(half_width=0, floor_permille=0, peak_permille=1000, min_range=0, min_speech=3, min_silence=4, pad=2)
    segs, stats = ref.segments_of_levels(lvl, 80, **o)
    assert segs == [(8, 25)] and stats == {"lo": 0, "hi": 1000, "on_thr": 400, "off_thr": 299, "flat": 0, "n_segments": 1}
    assert ref.segments_of_levels(lvl, 80, **dict(o, min_silence=3))[0] == [(8, 25)]   # (8, 17) and (16, 25): the pads of 2 meet over a gap of 3
    assert ref.segments_of_levels(lvl, 80, **dict(o, min_silence=3, pad=1))[0] == [(9, 16), (17, 24)]
    assert ref.segments_of_levels(lvl, 80, **dict(o, min_speech=6, min_silence=3))[0] == []           # zero segments is a legal result
    assert ref.segments_of_levels(lvl, 80, **dict(o, min_range=13))[0] == [(0, 45)]                   # 1000 < 13 x 80: flat
    assert ref.valid(10, 10) and not ref.valid(0, 10) and not ref.valid(11, 10) and not ref.valid(10, 10, on_share=0)
    assert not ref.valid(10, 10, off_share=411) and not ref.valid(10, 10, floor_permille=951) and not ref.valid(10, 10, pad=2 ** 24 + 1)


# ------------------------------------------------------------------------------------------------ the one real recording
@pytest.fixture(scope="module")
def sample_layout():
    """Three copies of the 2.9 s sample at mel frames 300, 991 and 1532: 3 s of digital silence, gaps of 4 s and 2.5 s, 1 s at the end."""
    pcm = np.load(os.path.join(GOLD, "sample_pcm_int16.npy")).astype(np.float32) / 32768.0
    gap = lambda seconds: np.zeros(int(16000 * seconds), np.float32)
    x = np.concatenate([gap(3), pcm, gap(4), pcm, gap(2.5), pcm, gap(1)])
    starts = [48000, 48000 + len(pcm) + 64000, 48000 + 2 * len(pcm) + 104000]
    return x, [(a // 160, -(-(a + len(pcm)) // 160)) for a in starts]


def _oracle_mel(x):
    from oracle import whisper_ref
    filt = _m("audio").mel_filters(80)
    return whisper_ref.log_mel_spectrogram(F.pad(torch.from_numpy(x), (0, 480000)), filt).numpy()


@pytest.mark.parametrize("noise_dbfs", [None, -60])
def test_real_sample_gives_one_segment_per_copy(sample_layout, noise_dbfs):
    x, copies = sample_layout
    if noise_dbfs is not None:
        x = x + (10.0 ** (noise_dbfs / 20.0) * np.random.default_rng(1).standard_normal(len(x))).astype(np.float32)
    segs, stats = ref.speech_segments(_oracle_mel(x))
    print("noise %s dBFS: %s %s" % (noise_dbfs, segs, stats))
    assert [c[0] for c in copies] == [300, 991, 1532] and stats["flat"] == 0 and len(segs) == 3
    slack = ref.DEFAULTS["pad"] + ref.DEFAULTS["half_width"] + 3
    for (a, b), (c0, c1) in zip(segs, copies):
        assert c0 - slack <= a < b <= c1 + slack and b - a >= 200, ((a, b), (c0, c1))


def test_real_sample_in_loud_noise_is_flat(sample_layout):
    x, _ = sample_layout
    x = x + (10.0 ** (-40 / 20.0) * np.random.default_rng(1).standard_normal(len(x))).astype(np.float32)
    segs, stats = ref.speech_segments(_oracle_mel(x))
    assert stats["flat"] == 1 and segs == [(0, len(x) // 160)]


# ------------------------------------------------------------------------------------------------ pause-aware words
def test_trim_words_to_speech():
    trim = _m("timing").trim_words_to_speech
    segments = [(100, 200), (300, 400), (900, 950)]
    words = [{"word": "a", "start": 0.5, "end": 1.5, "score": 0.25},    # frames [50, 150): cut back to where speech starts
             {"word": "b", "start": 1.5, "end": 3.5},                   # [150, 350) spans two segments: it keeps the pause between them
             {"word": "c", "start": 3.5, "end": 6.0},                   # [350, 600): its end moves to the segment's stop
             {"word": "d", "start": 6.0, "end": 7.0},                   # [600, 700) meets no segment: untouched
             {"word": "e", "start": None, "end": None},                 # an unaligned word
             {"word": "f", "start": 9.2, "end": 9.3},                   # inside a segment: untouched in value
             {"word": "g", "start": 9.5, "end": 9.6},                   # [950, 960) starts at a stop: no frame in common
             {"word": "h", "start": 2.0, "end": 3.0}]                   # [200, 300): exactly the pause
    got = trim(words, segments)
    assert [(w["start"], w["end"]) for w in got] == [(1.0, 1.5), (1.5, 3.5), (3.5, 4.0), (6.0, 7.0), (None, None), (9.2, 9.3), (9.5, 9.6), (2.0, 3.0)]
    assert got[0]["score"] == 0.25 and [w["word"] for w in got] == list("abcdefgh")
    assert words[0]["start"] == 0.5 and got[0] is not words[0]   # (new dicts)
    assert trim(words, []) == words and trim([], segments) == []
    al = _m("align_long")
    res = al.trim_result({"words": words[:2], "windows": [], "unaligned_words": 0, "windows_without_words": 0}, segments[:2])
    assert res["speech_segments"] == [{"start_frame": 100, "stop_frame": 200}, {"start_frame": 300, "stop_frame": 400}]
    assert [(w["start"], w["end"]) for w in res["words"]] == [(1.0, 1.5), (1.5, 3.5)] and res["unaligned_words"] == 0
    with pytest.raises(ValueError, match="trim_silence"):
        al.force_align_long_batch(object(), [], [], language="en", vocab_path="v", trim_silence=3)


# ------------------------------------------------------------------------------------------------ transcribe's plan
class _VadModel(stub._Model):
    """The stub engine with a scripted detector: recording id -> its segments."""

    def __init__(self, max_batch, script):
        super().__init__(max_batch)
        self.script = script

    def speech_segments(self, mel_long, content_frames=None, **vad_options):
        self.calls.append(("speech_segments", int(mel_long[0, 0]), dict(vad_options)))
        segs = self.script[int(mel_long[0, 0])]
        return list(segs), {"lo": -5, "hi": 7, "on_thr": 1, "off_thr": 0, "flat": 0, "n_segments": len(segs)}


def test_plan_recording_hands_the_segments_over_as_clips(tr):
    model = _VadModel(4, {7: [(100, 900), (4000, 9000)], 8: []})
    mel = model.log_mel_long(stub._recording(7, 100))
    clips, pieces, extra = tr.plan_recording(mel, None, None, 4, model, {"pad": 5})
    assert clips == [[(100, 900), (4000, 9000)]] and pieces is None
    assert extra == {"speech_segments": [{"start_frame": 100, "stop_frame": 900}, {"start_frame": 4000, "stop_frame": 9000}],
                     "vad": {"lo": -5, "hi": 7, "on_thr": 1, "off_thr": 0, "flat": 0, "n_segments": 2}}
    assert model.calls == [("speech_segments", 7, {"pad": 5})]
    assert tr.plan_recording(model.log_mel_long(stub._recording(8, 40)), None, None, 4, model, {})[0] == [[]]   # no speech: no clip
    assert tr.plan_recording(torch.zeros(80, 3000), None, None, 4, model, {}) == ([[]], None, {"speech_segments": [], "vad": None})   # no frame
    for bad in (dict(clip_timestamps="0,5"), dict(pieces=2)):
        with pytest.raises(ValueError, match="vad_filter"):
            tr.plan_recording(mel, bad.get("clip_timestamps"), bad.get("pieces"), 4, model, {})
    n = len(model.calls)
    assert tr.plan_recording(mel, None, None, 4, model) == ([None], None) and len(model.calls) == n   # without vad: the plan it always was


def test_vad_filter_runs_the_loop_over_the_segments_only(tr, tok, decoding, monkeypatch):
    script = {1: [(500, 2500), (7000, 11000)], 2: [], 3: [(0, 4000)]}
    model, dec = _VadModel(4, script), stub._Decoder(tok, decoding)
    seen = []
    real = tr.SeekState

    class _Spy(real):
        def __init__(self, n_frames, tokenizer, **kw):
            seen.append(kw.get("clips"))
            super().__init__(n_frames, tokenizer, **kw)

    monkeypatch.setattr(tr, "SeekState", _Spy)
    audios = [stub._recording(1, 120), stub._recording(2, 50), stub._recording(3, 40)]
    res = tr.transcribe_batch(model, audios, language="en", decode_windows=dec.decode_windows, vad_filter=True, vad_options={"min_speech": 9})
    assert seen == [[(500, 2500)] + [(7000, 11000)], [], [(0, 4000)]]
    assert [c for c in model.calls if c[0] == "speech_segments"] == [("speech_segments", i, {"min_speech": 9}) for i in (1, 2, 3)]
    assert [(w["seek"], w["size"]) for w in res[0]["windows"]] == [(500, 2000), (7000, 3000), (10000, 1000)]
    assert res[1]["windows"] == [] and res[1]["segments"] == [] and res[1]["speech_segments"] == []
    assert [(w["seek"], w["size"]) for w in res[2]["windows"]] == [(0, 3000), (3000, 1000)]
    assert res[0]["speech_segments"] == [{"start_frame": 500, "stop_frame": 2500}, {"start_frame": 7000, "stop_frame": 11000}]
    assert res[0]["vad"]["n_segments"] == 2 and res[2]["vad"]["n_segments"] == 1
    assert [s["start"] for s in res[0]["segments"]] == [5.0, 70.0, 100.0]   # times stay absolute
    # every decoded window lies inside a segment: no window of silence reaches the decoder
    assert sorted((r, s, z) for rows in dec.calls for r, s, z, _ in rows) == [(1, 500, 2000), (1, 7000, 3000), (1, 10000, 1000), (3, 0, 3000), (3, 3000, 1000)]
    # it equals the same ranges given as clip_timestamps, key by key apart from the two new keys
    clip = tr.transcribe_batch(_VadModel(4, script), audios[:1], language="en", decode_windows=stub._Decoder(tok, decoding).decode_windows,
                               clip_timestamps="5,25,70,110")[0]
    assert {k: v for k, v in res[0].items() if k not in ("speech_segments", "vad")} == clip and "vad" not in clip


def test_without_vad_filter_nothing_is_asked_and_no_key_is_added(tr, tok, decoding):
    model = _VadModel(4, {})
    res = tr.transcribe_batch(model, [stub._recording(1, 40)], language="en", decode_windows=stub._Decoder(tok, decoding).decode_windows)[0]
    assert not [c for c in model.calls if c[0] == "speech_segments"]
    assert "speech_segments" not in res and "vad" not in res and len(res["windows"]) == 2
    plain = tr.transcribe_batch(stub._Model(4), [stub._recording(1, 40)], language="en",
                                decode_windows=stub._Decoder(tok, decoding).decode_windows)[0]
    assert res == plain
    for bad in (dict(clip_timestamps="0,5"), dict(pieces=2)):
        with pytest.raises(ValueError, match="vad_filter"):
            tr.transcribe_batch(model, [stub._recording(1, 40)], language="en", vad_filter=True, **bad)
    with pytest.raises(ValueError, match="vad_options"):
        tr.transcribe_batch(model, [stub._recording(1, 40)], language="en", vad_options={"pad": 3})
    assert not [c for c in model.calls if c[0] == "speech_segments"]   # (refused before any audio is looked at)


def test_language_is_detected_where_speech_starts(tr, tok, decoding):
    model = _VadModel(4, {1: [(3100, 5000)], 2: [], 3: [(200, 900)]})
    looked = []

    def detect(windows):
        looked.extend(tuple(int(round(float(v))) for v in w[0, :3]) for w in windows)
        return ["de"] * len(windows), [0.75] * len(windows)

    audios = [stub._recording(1, 60), stub._recording(2, 60), stub._recording(3, 10)]
    res = tr.transcribe_batch(model, audios, language="auto", detect_languages=detect, decode_windows=stub._Decoder(tok, decoding).decode_windows,
                              vad_filter=True)
    assert looked == [(1, 3100, 2900), (3, 200, 800)]   # (recording, seek, size): from the first segment's start to the recording's end
    assert [(r["language"], r["language_probability"]) for r in res] == [("de", 0.75), (None, None), ("de", 0.75)]
    assert res[1]["windows"] == [] and res[1]["speech_segments"] == []


# ------------------------------------------------------------------------------------------------ command lines
def test_command_lines_parse_the_new_options_and_keep_their_defaults(tr):
    al = _m("align_long")
    base = ["--audio", "x.wav", "--output_dir", "out", "--random_init"]
    plain = vars(tr.parse_args(base))
    assert not [k for k in plain if k.startswith("vad")]   # absent unless given: the parsed defaults are what they were
    args = tr.parse_args(base + ["--vad_filter", "--vad_min_silence", "50", "--vad_pad", "10"])
    assert args.vad_filter is True and args.vad_min_silence == 50 and args.vad_pad == 10 and not hasattr(args, "vad_min_speech")
    assert {k: v for k, v in vars(args).items() if not k.startswith("vad")} == plain
    every = tr.parse_args(base + ["--vad_filter"] + [v for i, name in enumerate(ref.OPTION_NAMES) for v in ("--vad_" + name, str(i + 1))])
    assert [getattr(every, "vad_" + name) for name in ref.OPTION_NAMES] == list(range(1, 10))
    assert tuple(tr.VAD_OPTION_HELP) == ref.OPTION_NAMES == tuple(f[0] for f in _m("_lib").VadOpts._fields_) and _m("_lib").VAD_DEFAULTS == ref.DEFAULTS
    for bad in (["--vad_pad", "3"], ["--vad_filter", "--clip_timestamps", "0,5"], ["--vad_filter", "--pieces", "2", "--batch", "2"]):
        with pytest.raises(SystemExit):   # (refused before the model is looked at)
            tr.main(tr.parse_args(base + bad), model=object())
    ab = ["--audio", "a.wav", "--text", "a.txt", "--vocab", "v", "--output_dir", "x"]
    assert "trim_silence" not in vars(al.parse_args(ab)) and al.parse_args(ab + ["--trim_silence"]).trim_silence is True
    assert {k: v for k, v in vars(al.parse_args(ab + ["--trim_silence"])).items() if k != "trim_silence"} == vars(al.parse_args(ab))
