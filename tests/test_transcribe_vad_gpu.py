"""transcribe(vad_filter=True) and force_align_long(trim_silence=True) on the MI355X, on the tiny seeded model of
tests/test_transcribe_pieces_gpu.py (seed 5, max_batch 4, sample_len 24). The recording is 43 s: synthetic audio at 3 .. 23 s and at
29 .. 41 s, DIGITAL silence before, between and after. The speech segments the engine finds become the clips of the seek loop, so the
run equals transcribe(clip_timestamps=<the same segments in seconds>) exactly: the same code path at the same batch shape, no case
left out. transcribe_batch of two such recordings equals the single calls under the near-tie rule of tests/test_transcribe_batch_gpu.py
(a first differing window is excused only by a teacher-forced logit gap below 1e-3, for at most one recording)."""
import importlib

import numpy as np
import pytest
import torch

import speech_segments_ref as ref
import test_transcribe_batch_gpu as lockstep   # (its decode log and its near-tie rule)

pytestmark = pytest.mark.gpu

LAYOUT = (3, 20, 6, 12, 2)    # seconds: silence, audio, silence, audio, silence
SLACK = ref.DEFAULTS["pad"] + ref.DEFAULTS["half_width"] + 3   # how far a segment may reach into the silence next to it, in frames


def _m(n):
    return importlib.import_module("whisper-char-alignment_amd." + n)


def _recording(seed, shift=0):
    silence = lambda seconds: np.zeros(16000 * seconds + shift, np.float32)
    syn = _m("synthetic").synth_audio
    return np.concatenate([silence(LAYOUT[0]), syn(seed, 16000 * LAYOUT[1]), silence(LAYOUT[2]), syn(seed + 1, 16000 * LAYOUT[3] + 40), silence(LAYOUT[4])])


@pytest.fixture(scope="module")
def small():
    pkg = importlib.import_module("whisper-char-alignment_amd")
    dims = pkg.ModelDimensions(80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)
    m = pkg.WhisperAMD(dims, device="cuda:0", max_batch=4, precision="f16")
    m.load_state_dict(_m("synthetic").random_state_dict(dims, seed=5))
    return m


@pytest.fixture(scope="module")
def audio():
    return _recording(33)


def _silences():
    """The planted silences in frames, each shrunk by SLACK on the sides where audio borders it."""
    a0, a1, b0, b1 = 300, 2300, 2900, 4100
    return [(0, a0 - SLACK), (a1 + SLACK, b0 - SLACK), (b1 + SLACK, 4300)]


@pytest.mark.parametrize("words", [False, True], ids=["tokens-only", "word-timestamps"])
def test_vad_filter_equals_the_same_segments_as_clips_and_skips_the_silence(small, audio, fake_vocab, words):
    tr = _m("transcribe")
    kw = dict(language="en", sample_len=24)
    if words:
        kw.update(vocab_path=fake_vocab, word_timestamps=True, topk=4)
    got = tr.transcribe(small, audio, vad_filter=True, **kw)
    mel = small.log_mel_long(torch.from_numpy(audio).cuda())
    segs, stats = small.speech_segments(mel)
    assert (segs, stats) == ref.speech_segments(mel.cpu().numpy())   # the engine's segments of its own log-mel, bit for bit
    print("speech segments %s, stats %s" % (segs, stats))
    assert got["speech_segments"] == [{"start_frame": a, "stop_frame": b} for a, b in segs] and got["vad"] == stats
    assert len(segs) == 2 and stats["flat"] == 0
    for (a, b), (s0, s1) in zip(segs, [(300, 2300), (2900, 4100)]):
        assert s0 - SLACK <= a <= s0 and s1 <= b <= s1 + SLACK, ((a, b), (s0, s1))
    clip = tr.transcribe(small, audio, clip_timestamps=[t / 100 for ab in segs for t in ab], **kw)
    assert "speech_segments" not in clip and "vad" not in clip
    assert {k: v for k, v in got.items() if k not in ("speech_segments", "vad")} == clip   # key by key, every key
    assert got["windows"][0]["seek"] == segs[0][0] and len(got["windows"]) >= 2
    for w in got["windows"]:   # no window starts in the planted silence, and every window lies inside a segment
        assert not any(s0 <= w["seek"] < s1 for s0, s1 in _silences()), w
        assert any(a <= w["seek"] and w["seek"] + w["size"] <= b for a, b in segs), w
    plain = tr.transcribe(small, audio, **kw)
    assert "speech_segments" not in plain and plain["windows"][0]["seek"] == 0
    if words:
        assert sum(len(s["words"]) for s in got["segments"]) > 0
        assert all(w["start"] >= segs[0][0] / 100 for s in got["segments"] for w in s["words"])   # times stay absolute


def test_batch_of_two_equals_the_single_calls(small, fake_vocab, monkeypatch):
    tr, decoding = _m("transcribe"), _m("decoding")
    tok = _m("tokenizer").get_tokenizer(True, language="en", task="transcribe", vocab_path=None)
    kw = dict(language="en", sample_len=24, vad_filter=True)
    audios = [_recording(33), _recording(40, shift=800)]
    logs_alone, alone = [], []
    for pcm in audios:
        log = lockstep._Log(decoding)
        monkeypatch.setattr(decoding, "decode", log)
        alone.append(tr.transcribe(small, pcm, **kw))
        monkeypatch.setattr(decoding, "decode", log.real)
        logs_alone.append(log.rows)
    log = lockstep._Log(decoding)
    monkeypatch.setattr(decoding, "decode", log)
    batch = small.transcribe_batch(audios, **kw)
    monkeypatch.setattr(decoding, "decode", log.real)
    assert log.batches[0] == 2 and sum(log.batches) == sum(len(r["windows"]) for r in batch)
    n_excused = 0
    for i, (a, b) in enumerate(zip(alone, batch)):
        what = "recording %d" % i
        assert a["speech_segments"] == b["speech_segments"] and a["vad"] == b["vad"] and len(a["speech_segments"]) == 2, what
        k = lockstep._first_difference(a, b)
        print("%s: %d windows alone, %d in the batch, first difference: %s" % (what, len(a["windows"]), len(b["windows"]), k))
        if k is not None:
            n_excused += 1
            lockstep._excused(small, tok, small.log_mel_long(torch.from_numpy(audios[i]).cuda()), a, b, k, logs_alone[i], log.rows, what)
            continue
        assert [w["max_frames"] for w in a["windows"]] == [w["max_frames"] for w in b["windows"]], what
        assert len(a["segments"]) == len(b["segments"]) and a["text"] == b["text"], what
        for sa, sb in zip(a["segments"], b["segments"]):   # (what that file compares: the log-probabilities depend on the batch's GEMM path)
            assert (sa["id"], sa["seek"], sa["start"], sa["end"], sa["tokens"], sa["text"]) == \
                (sb["id"], sb["seek"], sb["start"], sb["end"], sb["tokens"], sb["text"]), what
    assert n_excused <= 1, n_excused


@pytest.fixture(scope="module")
def aligner():
    """An engine of its own for the alignment: align_batch(pcm=None) takes the OLDEST encoded state of the engine, and a transcribe
    without words leaves its last decoded state behind."""
    pkg = importlib.import_module("whisper-char-alignment_amd")
    dims = pkg.ModelDimensions(80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)
    m = pkg.WhisperAMD(dims, device="cuda:0", max_batch=4, precision="f16")
    m.load_state_dict(_m("synthetic").random_state_dict(dims, seed=5))
    return m


def test_trim_silence_is_the_untrimmed_alignment_trimmed(aligner, audio, fake_vocab):
    small = aligner
    al, timing = _m("align_long"), _m("timing")
    text = _m("synthetic").synth_text(7, 300)
    kw = dict(language="en", vocab_path=fake_vocab, aligned_unit_type="char", aggr="topk", topk=4, medfilt_width=3)
    plain = al.force_align_long(small, audio, text, **kw)
    trimmed = al.force_align_long(small, audio, text, trim_silence=True, **kw)
    assert "speech_segments" not in plain
    segs = [(s["start_frame"], s["stop_frame"]) for s in trimmed["speech_segments"]]
    mel = small.log_mel_long(torch.from_numpy(audio).cuda())
    assert segs == small.speech_segments(mel, **al.TRIM_SILENCE_OPTIONS)[0] == ref.speech_segments(mel.cpu().numpy(), **al.TRIM_SILENCE_OPTIONS)[0]
    assert len(segs) >= 2 and al.TRIM_SILENCE_OPTIONS == dict(min_speech=5, min_silence=20, pad=3)
    assert trimmed["words"] == timing.trim_words_to_speech(plain["words"], segs)
    assert {k: v for k, v in trimmed.items() if k not in ("words", "speech_segments")} == {k: v for k, v in plain.items() if k != "words"}
    changed = sum(a != b for a, b in zip(plain["words"], trimmed["words"]))
    print("%d words, %d trimmed, segments %s" % (len(plain["words"]), changed, segs))
    assert len(plain["words"]) > 10 and all(w["start"] is None or w["end"] >= w["start"] for w in trimmed["words"])
    custom = al.force_align_long(small, audio, text, trim_silence={"pad": 0, "min_silence": 100}, **kw)
    assert [(s["start_frame"], s["stop_frame"]) for s in custom["speech_segments"]] == small.speech_segments(mel, min_speech=5, min_silence=100, pad=0)[0]
