"""CPU tests of transcribe's temperature fallback ladder (whisper-char-alignment_amd/transcribe.py: check_supported, needs_fallback,
window_seed, _Call.decode, SeekState's prompt reset) against scripted decoders. The sampler itself is tests/test_decode_sample_ref.py and
tests/test_decode_sample_gpu.py."""
import importlib

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


class _Model:
    """The engine as transcribe_batch sees it without words (tests/test_transcribe_batch.py): a window carries (recording id, seek, size)."""
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


def _recording(rec_id, seconds=20):
    pcm = np.zeros(16000 * seconds, np.float32)
    pcm[0] = rec_id
    return pcm


class _Ladder:
    """A scripted decoder for ladder runs: quality(rec, seek, temperature) -> (avg_logprob, compression_ratio, no_speech_prob); the tokens
    name the temperature (text token 1000 + 10 T). Records every call as [(rec, seek, temperature or None, seed)]."""

    def __init__(self, decoding, tok, quality):
        self.decoding, self.tok, self.quality, self.calls = decoding, tok, quality, []

    def decode_windows(self, windows, prompts, temperatures=None, seeds=None):
        assert temperatures is not None and seeds is not None, "a ladder run passes temperatures= and seeds="
        assert windows.shape[0] == len(prompts) == len(temperatures) == len(seeds)
        ids = [tuple(int(round(float(v))) for v in w[0, :3]) for w in windows]
        self.calls.append([(rec, seek, t, s) for (rec, seek, _), t, s in zip(ids, temperatures, seeds)])
        out, ts = [], self.tok.timestamp_begin
        for (rec, seek, _), t in zip(ids, temperatures):
            if t is None:   # an accepted row: whatever comes back must be ignored
                out.append(self.decoding.DecodingResult(language="en", tokens=[ts, 7, ts + 1], avg_logprob=-9.0, no_speech_prob=0.0, temperature=-1.0,
                                                        compression_ratio=99.0))
                continue
            lp, cr, nsp = self.quality(rec, seek, t)
            out.append(self.decoding.DecodingResult(language="en", tokens=[ts, 1000 + int(round(10 * t)), ts + 100], avg_logprob=lp,
                                                    no_speech_prob=nsp, temperature=t, compression_ratio=cr))
        return out


GOOD, LOOPS, UNLIKELY = (-0.3, 1.0, 0.1), (-0.3, 3.0, 0.1), (-1.5, 1.0, 0.1)


def _run(tr, decoding, tok, quality, audios=None, **kw):
    h = _Ladder(decoding, tok, quality)
    kw.setdefault("temperature", (0.0, 0.4, 0.8))
    got = tr.transcribe_batch(_Model(4), audios or [_recording(1)], language="en", seed=11, decode_windows=h.decode_windows, **kw)
    return got, h


def _temps(result):
    return [s["temperature"] for s in result["segments"]]


def test_window_seed_values(tr):
    assert tr.window_seed(0, 0, 0) == 0 and tr.window_seed(5, 0, 0) == 5
    assert tr.window_seed(0, 1, 0) == 0x9E3779B97F4A7C15 and tr.window_seed(0, 0, 1) == 0xBF58476D1CE4E5B9
    assert tr.window_seed(0, 3000, 2) == ((3000 * 0x9E3779B97F4A7C15) ^ (2 * 0xBF58476D1CE4E5B9)) % 2 ** 64 == 0x64AAFB118917DD6A
    assert tr.window_seed(-1, 0, 0) == 2 ** 64 - 1 and tr.window_seed(2 ** 64 + 3, 2, 1) == tr.window_seed(3, 2, 1)
    assert len({tr.window_seed(7, seek, rung) for seek in (0, 400, 3000, 3400) for rung in range(6)}) == 24


def test_check_supported_with_and_without_a_seed(tr):
    assert tr.check_supported(0.0, "en") == 0.0 and tr.check_supported((0.0,), "en", seed=None) == 0.0
    assert tr.check_supported(0.0, "en", seed=0) == (0.0,) and tr.check_supported(0.2, "en", seed=0) == (0.2,)
    assert tr.check_supported((0.0, 0.2, 0.4, 0.6, 0.8, 1.0), "en", seed=3) == (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)
    for bad in ((), (0.0, -0.2), float("nan"), float("inf"), "0.2", (0.0, None)):
        with pytest.raises(ValueError):
            tr.check_supported(bad, "en", seed=0)
    for bad_seed in (1.5, "3", True):
        with pytest.raises(ValueError):
            tr.check_supported(0.0, "en", seed=bad_seed)
    with pytest.raises(NotImplementedError):
        tr.check_supported((0.0, 0.2), None, seed=0)


def test_each_criterion_alone_and_the_silence_clause(tr, decoding):
    def r(lp, cr, nsp):
        return decoding.DecodingResult(language="en", avg_logprob=lp, compression_ratio=cr, no_speech_prob=nsp)

    assert not tr.needs_fallback(r(*GOOD), 2.4, -1.0, 0.6)
    assert tr.needs_fallback(r(*LOOPS), 2.4, -1.0, 0.6) and not tr.needs_fallback(r(-0.3, 2.4, 0.1), 2.4, -1.0, 0.6)   # strictly above
    assert tr.needs_fallback(r(*UNLIKELY), 2.4, -1.0, 0.6) and not tr.needs_fallback(r(-1.0, 1.0, 0.1), 2.4, -1.0, 0.6)   # strictly below
    # silence: improbable AND no_speech above its threshold is not decoded again (the seek loop skips it), even when it also loops
    assert not tr.needs_fallback(r(-1.5, 1.0, 0.9), 2.4, -1.0, 0.6) and not tr.needs_fallback(r(-1.5, 3.0, 0.9), 2.4, -1.0, 0.6)
    assert tr.needs_fallback(r(-0.3, 3.0, 0.9), 2.4, -1.0, 0.6)   # probable: the clause does not apply
    # None switches a test off -- and the silence clause needs both of its thresholds
    assert not tr.needs_fallback(r(*LOOPS), None, -1.0, 0.6) and not tr.needs_fallback(r(*UNLIKELY), 2.4, None, 0.6)
    assert tr.needs_fallback(r(-1.5, 1.0, 0.9), 2.4, -1.0, None) and tr.needs_fallback(r(-0.3, 3.0, 0.9), 2.4, None, 0.6)
    # no vocabulary: the compression ratio is NaN and never fires
    assert not tr.needs_fallback(r(-0.3, float("nan"), 0.1), 2.4, -1.0, 0.6)


@pytest.mark.parametrize("bad", [LOOPS, UNLIKELY], ids=["compression_ratio", "avg_logprob"])
def test_one_fallback_then_accepted(tr, decoding, tok, bad):
    (got,), h = _run(tr, decoding, tok, lambda rec, seek, t: bad if t == 0.0 else GOOD)
    assert _temps(got) == [0.4] and got["segments"][0]["tokens"][1] == 1004
    assert [[c[2] for c in call] for call in h.calls] == [[0.0], [0.4]]
    assert [[c[3] for c in call] for call in h.calls] == [[tr.window_seed(11, 0, 0)], [tr.window_seed(11, 0, 1)]]


def test_thresholds_of_none_and_the_silence_clause_stop_the_ladder(tr, decoding, tok):
    (got,), h = _run(tr, decoding, tok, lambda rec, seek, t: LOOPS, compression_ratio_threshold=None)
    assert _temps(got) == [0.0] and len(h.calls) == 1
    (got,), h = _run(tr, decoding, tok, lambda rec, seek, t: UNLIKELY, logprob_threshold=None)
    assert _temps(got) == [0.0] and len(h.calls) == 1
    # a silent window: decoded once, then skipped by the seek loop
    (got,), h = _run(tr, decoding, tok, lambda rec, seek, t: (-1.5, 1.0, 0.9))
    assert got["segments"] == [] and [w["skipped"] for w in got["windows"]] == [True] and len(h.calls) == 1
    # a custom threshold
    (got,), h = _run(tr, decoding, tok, lambda rec, seek, t: (-0.3, 2.0, 0.1) if t < 0.8 else GOOD, compression_ratio_threshold=1.5)
    assert _temps(got) == [0.8] and len(h.calls) == 3


def test_the_last_rung_is_accepted_whatever_it_gives(tr, decoding, tok):
    (got,), h = _run(tr, decoding, tok, lambda rec, seek, t: LOOPS)
    assert _temps(got) == [0.8] and got["segments"][0]["compression_ratio"] == 3.0
    assert [[c[2] for c in call] for call in h.calls] == [[0.0], [0.4], [0.8]]
    (got,), h = _run(tr, decoding, tok, lambda rec, seek, t: LOOPS, temperature=0.3)   # a ladder of one rung
    assert _temps(got) == [0.3] and len(h.calls) == 1


def test_accepted_rows_are_kept_while_others_fall_back(tr, decoding, tok):
    """Three recordings that need 0, 1 and 2 fallbacks share the rounds: the batch stays whole, an accepted row is passed with temperature
    None and what it returns then is ignored, and every recording's result is what transcribe() gives for it alone."""
    need = {1: 0, 2: 1, 3: 2}
    ladder = (0.0, 0.4, 0.8)

    def quality(rec, seek, t):
        return GOOD if ladder.index(t) >= need[rec] else UNLIKELY

    audios = [_recording(1), _recording(2), _recording(3)]
    got, h = _run(tr, decoding, tok, quality, audios=audios)
    assert [_temps(r) for r in got] == [[0.0], [0.4], [0.8]]
    assert [r["segments"][0]["tokens"][1] for r in got] == [1000, 1004, 1008]
    assert [r["segments"][0]["avg_logprob"] for r in got] == [-0.3, -0.3, -0.3]
    assert [[c[:3] for c in call] for call in h.calls] == [[(1, 0, 0.0), (2, 0, 0.0), (3, 0, 0.0)], [(1, 0, None), (2, 0, 0.4), (3, 0, 0.4)],
                                                          [(1, 0, None), (2, 0, None), (3, 0, 0.8)]]
    # a row's seed follows (seed, seek, rung), not its place in the batch
    assert all(c[3] == tr.window_seed(11, 0, rung) for rung, call in enumerate(h.calls) for c in call)
    for rec, want in zip((1, 2, 3), got):
        h1 = _Ladder(decoding, tok, quality)
        alone = tr.transcribe(_Model(1), _recording(rec), language="en", seed=11, temperature=ladder,
                              decode_window=lambda w, p, temperature, seed: h1.decode_windows(w[None], [p], [temperature], [seed])[0])
        assert alone == want
        assert [c[0][2:] for c in h1.calls] == [(t, tr.window_seed(11, 0, rung)) for rung, t in enumerate(ladder[:need[rec] + 1])]


class _FakeDecode:
    """Stands in for decoding.decode: records the keywords of every call and answers by temperature."""

    def __init__(self, decoding, tok, accept_at):
        self.decoding, self.tok, self.accept_at, self.calls = decoding, tok, accept_at, []

    def __call__(self, model, mel, options, **kw):
        rows = list(options) if isinstance(options, (list, tuple)) else [options]
        self.calls.append(dict(kw, mel=mel is not None, per_row=isinstance(options, (list, tuple)), temperature=[o.temperature for o in rows],
                               seed=[o.seed for o in rows]))
        ts = self.tok.timestamp_begin
        out = [self.decoding.DecodingResult(language="en", tokens=[ts, 1000 + int(round(10 * o.temperature)), ts + 100], no_speech_prob=0.1,
                                            avg_logprob=-0.3 if o.temperature >= self.accept_at[b] else -1.5, temperature=o.temperature,
                                            compression_ratio=float("nan")) for b, o in enumerate(rows)]
        return out if isinstance(options, (list, tuple)) or mel is None or mel.ndim == 3 else out[0]


def test_redecode_is_asked_for_exactly_on_the_rungs_after_the_first(tr, decoding, tok, monkeypatch):
    fake = _FakeDecode(decoding, tok, accept_at=[0.0, 0.8])
    monkeypatch.setattr(decoding, "decode", fake)
    got = tr.transcribe_batch(_Model(2), [_recording(1), _recording(2)], language="en", seed=4, temperature=(0.0, 0.4, 0.8))
    assert [_temps(r) for r in got] == [[0.0], [0.8]]
    first, second, third = fake.calls
    # rung 0 at temperature 0: the call transcribe always made (a mel, no seed, no redecode)
    assert first["mel"] and first["temperature"] == [0.0, 0.0] and first["seed"] == [None, None]
    assert not first.get("redecode", False) and first.get("row_sample_len") is None and "encoded_batch" not in first
    # later rungs: the same state again, the accepted row riding along greedily for one token
    for rung, call in ((1, second), (2, third)):
        assert call["redecode"] is True and not call["mel"] and call["encoded_batch"] == 2 and call["per_row"]
        assert call["temperature"] == [0.0, (0.0, 0.4, 0.8)[rung]] and call["row_sample_len"] == [1, None]
        assert call["seed"] == [None, tr.window_seed(4, 0, rung)]
    # a first rung above 0 samples at once, with the rung-0 seed
    fake = _FakeDecode(decoding, tok, accept_at=[0.0])
    monkeypatch.setattr(decoding, "decode", fake)
    got = tr.transcribe(_Model(1), _recording(1), language="en", seed=4, temperature=(0.6, 1.0))
    assert _temps(got) == [0.6] and len(fake.calls) == 1
    assert fake.calls[0]["temperature"] == [0.6] and fake.calls[0]["seed"] == [tr.window_seed(4, 0, 0)] and not fake.calls[0].get("redecode", False)


def test_prompt_reset_above_half_and_not_at_0_4(tr, decoding, tok):
    """A window accepted at a temperature above 0.5 does not condition the next one (upstream: prompt_reset_since = len(all_tokens))."""
    prompts = {}

    def run(ladder):
        h = _Ladder(decoding, tok, lambda rec, seek, t: GOOD if (seek > 0 or t == ladder[-1]) else UNLIKELY)
        inner = h.decode_windows

        def spy(windows, p, temperatures=None, seeds=None):
            prompts[(ladder, int(round(float(windows[0][0, 1]))))] = list(p[0])
            return inner(windows, p, temperatures=temperatures, seeds=seeds)

        return tr.transcribe_batch(_Model(1), [_recording(1, 70)], language="en", seed=1, temperature=ladder, initial_prompt=[7, 8],
                                   decode_windows=spy)[0]

    ts = tok.timestamp_begin
    low = run((0.0, 0.4))
    assert _temps(low) == [0.4, 0.0, 0.0]
    assert prompts[((0.0, 0.4), 3000)] == [7, 8, ts, 1004, ts + 100] and len(prompts[((0.0, 0.4), 6000)]) == 8
    high = run((0.0, 0.6))
    assert _temps(high) == [0.6, 0.0, 0.0]
    assert prompts[((0.0, 0.6), 3000)] == [] and prompts[((0.0, 0.6), 6000)] == [ts, 1000, ts + 100]
    assert [s["tokens"] for s in high["segments"]] == [[ts, 1006, ts + 100], [ts, 1000, ts + 100], [ts, 1000, ts + 100]]   # all kept


def test_without_a_seed_a_ladder_is_still_refused_before_any_decode(tr, decoding, tok):
    called = []

    def never(windows, prompts, **kw):
        called.append(1)
        return []

    for temperature in ((0.0, 0.2), 0.2, (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)):
        with pytest.raises(NotImplementedError, match="temperature 0.0 only"):
            tr.transcribe_batch(_Model(1), [_recording(1)], language="en", temperature=temperature, decode_windows=never)
        with pytest.raises(NotImplementedError, match="temperature 0.0 only"):
            tr.transcribe(_Model(1), _recording(1), language="en", temperature=temperature, seed=None, decode_window=never)
    assert not called
    with pytest.raises(NotImplementedError):
        decoding._check_supported(decoding.DecodingOptions(language="en", temperature=0.5))
    decoding._check_supported(decoding.DecodingOptions(language="en", temperature=0.5, seed=0))
    for kw in ({"beam_size": 5}, {"best_of": 2}, {"patience": 1.0}):
        with pytest.raises(NotImplementedError):
            decoding._check_supported(decoding.DecodingOptions(language="en", temperature=0.5, seed=0, **kw))


def test_seed_0_at_temperature_0_gives_the_result_of_no_seed(tr, decoding, tok):
    ts = tok.timestamp_begin
    res = decoding.DecodingResult(language="en", tokens=[ts, 1000, ts + 100], avg_logprob=-1.5, no_speech_prob=0.1, temperature=0.0,
                                  compression_ratio=3.0)   # would fall back if there were a rung to fall to
    calls = []

    def plain(windows, prompts):
        calls.append("plain")
        return [res] * len(prompts)

    def ladder(windows, prompts, temperatures, seeds):
        calls.append((temperatures, seeds))
        return [res] * len(prompts)

    without = tr.transcribe_batch(_Model(1), [_recording(1, 40)], language="en", decode_windows=plain)
    with_seed = tr.transcribe_batch(_Model(1), [_recording(1, 40)], language="en", seed=0, temperature=0.0, decode_windows=ladder)
    assert with_seed == without
    assert calls == ["plain", "plain", ([0.0], [tr.window_seed(0, 0, 0)]), ([0.0], [tr.window_seed(0, 3000, 0)])]


def test_cli_ladder_arguments(tr, tmp_path, monkeypatch):
    base = ["--audio", "a.npy", "--output_dir", "o", "--random_init"]
    args = tr.parse_args(base)
    # an option that is not given is not in the namespace: without --seed the parsed arguments are what they always were
    assert not {"seed", "temperature", "temperature_increment_on_fallback", "compression_ratio_threshold"} & set(vars(args))
    given = tr.parse_args(base + ["--seed", "7", "--temperature", "0.2"])
    assert given.seed == 7 and given.temperature == 0.2 and not hasattr(given, "compression_ratio_threshold")
    assert tr.temperature_ladder(0.0, None) == (0.0,) and tr.temperature_ladder(0.5, None) == (0.5,)
    assert np.allclose(tr.temperature_ladder(0.0, 0.2), (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)) and len(tr.temperature_ladder(0.0, 0.2)) == 6
    assert np.allclose(tr.temperature_ladder(0.5, 0.25), (0.5, 0.75, 1.0))
    rec = tmp_path / "rec.npy"
    np.save(rec, np.zeros(16000, np.float32))
    seen = []

    def fake_transcribe(model, audio, **kw):
        seen.append(kw)
        return {"text": "", "segments": [], "language": "en", "windows": [], "windows_without_words": 0}

    monkeypatch.setattr(tr, "transcribe", fake_transcribe)
    out = ["--audio", str(rec), "--output_dir", str(tmp_path / "out"), "--random_init"]
    tr.main(tr.parse_args(out), model=object())
    assert not {"seed", "temperature", "compression_ratio_threshold"} & set(seen[-1])   # without --seed the call is what it was
    tr.main(tr.parse_args(out + ["--seed", "5", "--temperature_increment_on_fallback", "0.5", "--compression_ratio_threshold", "2.0"]), model=object())
    assert seen[-1]["seed"] == 5 and seen[-1]["temperature"] == (0.0, 0.5, 1.0) and seen[-1]["compression_ratio_threshold"] == 2.0
    with pytest.raises(SystemExit):
        tr.main(tr.parse_args(out + ["--temperature", "0.4"]), model=object())
