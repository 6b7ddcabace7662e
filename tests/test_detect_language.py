"""CPU tests of language identification (whisper-char-alignment_amd: tokenizer.py, decoding.detect_language, transcribe's
language="auto", the C ABI's wca_detect_language): the tokenizer's language members restate upstream's, the entry point refuses a
null engine before any HIP call, and transcribe_batch partitions a group by detected language against scripted hooks. The GPU side is
tests/test_detect_language_gpu.py."""
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
def tokmod():
    return importlib.import_module("whisper-char-alignment_amd.tokenizer")


def test_language_tokens_are_the_contiguous_range_after_sot(tokmod):
    codes = list(tokmod.LANGUAGES)
    assert len(codes) == 100
    for n in (99, 100):
        tok = tokmod.get_tokenizer(True, num_languages=n, language="de", task="transcribe")
        assert tok.all_language_tokens == tuple(range(tok.sot + 1, tok.sot + 1 + n))
        assert tok.all_language_tokens[-1] == tok.sot + n and tok.all_language_tokens[-1] + 1 == tok.translate
        assert tok.all_language_codes == tuple(codes[:n])            # LANGUAGES order
        assert tok.language_token == tok.sot_sequence[1] == tok.sot + 1 + codes.index("de")
        assert tok.to_language_token("en") == tok.sot + 1
    assert "yue" not in tokmod.get_tokenizer(True).all_language_codes and tokmod.get_tokenizer(True, num_languages=100).all_language_codes[-1] == "yue"
    with pytest.raises(KeyError):
        tokmod.get_tokenizer(True).to_language_token("yue")          # the 99-language numbering has no Cantonese
    english_only = tokmod.get_tokenizer(False)
    with pytest.raises(ValueError):
        english_only.language_token


def test_abi_version_and_null_engine(wca, lib):
    assert lib.wca_version() >= 13
    rc = lib.wca_detect_language(None, None, None, 0, None, 1, 50258, 50259, 99, None, None)
    assert rc == -1                                                  # WCA_ERR_INVALID
    assert b"null" in lib.wca_last_error()
    assert lib.wca_test_language_head(None, None, 1, 50259, 99, None, None) == -1


def test_detect_language_refuses_an_english_only_model(decoding):
    class _EnglishOnly:
        is_multilingual, num_languages = False, 99

    with pytest.raises(ValueError, match="language tokens"):
        decoding.detect_language(_EnglishOnly(), torch.zeros(80, 3000))


def test_detect_language_schema_over_a_scripted_engine(decoding, tokmod):
    """decoding.detect_language over an object that answers the thin engine call: upstream's return schema, the default tokenizer's
    numbering from model.num_languages, and the argument the engine is handed."""
    class _Engine:
        is_multilingual = True

        def __init__(self, num_languages):
            self.num_languages, self.calls = num_languages, []

        def detect_language(self, mel, *, pcm, n_samples, sot, lang_begin, n_lang):
            self.calls.append((tuple(mel.shape), sot, lang_begin, n_lang))
            probs = np.full((mel.shape[0], n_lang), 0.5 / (n_lang - 1), np.float32)
            picks = [(7 * b + 2) % n_lang for b in range(mel.shape[0])]
            for b, j in enumerate(picks):
                probs[b, j] = 0.5
            return np.array([lang_begin + j for j in picks], np.int32), probs

    codes = list(tokmod.LANGUAGES)
    for n in (99, 100):
        eng = _Engine(n)
        tokens, probs = decoding.detect_language(eng, torch.zeros(3, 80, 3000))
        assert eng.calls == [((3, 80, 3000), 50258, 50259, n)]
        assert tokens.dtype == torch.int64 and tokens.tolist() == [50259 + 2, 50259 + 9, 50259 + 16]
        assert [list(p) for p in probs] == [codes[:n]] * 3 and [max(p, key=p.get) for p in probs] == [codes[2], codes[9], codes[16]]
        token, prob = decoding.detect_language(eng, torch.zeros(80, 3000))
        assert token.ndim == 0 and int(token) == 50259 + 2 and isinstance(prob, dict) and prob[codes[2]] == 0.5


# ---------------------------------------------------------------------------------------------- transcribe_batch(language="auto")
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


def _recording(rec_id, seconds):
    pcm = np.zeros(16000 * seconds, np.float32)
    pcm[0] = rec_id
    return pcm


class _Hooks:
    def __init__(self, decoding, scripts, languages):
        self.decoding, self.scripts, self.languages = decoding, scripts, languages
        self.detect_calls, self.decode_calls = [], []

    def detect_languages(self, windows):
        ids = [tuple(int(round(float(v))) for v in w[0, :3]) for w in windows]
        self.detect_calls.append(ids)
        return [self.languages[i][0] for i, _, _ in ids], [self.languages[i][1] for i, _, _ in ids]

    def decode_windows(self, windows, prompts):
        assert windows.shape[0] == len(prompts)
        ids = [tuple(int(round(float(v))) for v in w[0, :3]) for w in windows]
        self.decode_calls.append([(rec, seek) for rec, seek, _ in ids])
        return [self.decoding.DecodingResult(language="?", tokens=list(self.scripts[rec][seek]), text="", avg_logprob=-0.3, no_speech_prob=0.1,
                                             temperature=0.0, compression_ratio=1.0) for rec, seek, _ in ids]


def _scripts(tokmod):
    tok = tokmod.get_tokenizer(True, language="en", task="transcribe")
    ts, (a, b, c) = tok.timestamp_begin, [tok.encode(ch)[0] for ch in "abc"]
    return {1: {0: [ts, a, ts + 50, ts + 50, b, ts + 100]},                              # 20 s: one window
            2: {0: [ts, c, ts + 100], 3000: [ts, a, b, ts + 30]},                          # 40 s: two windows
            3: {0: [ts, a, ts + 200, ts + 200, b, c], 400: [ts, c, ts + 100], 3400: [ts, b, ts + 10]}}   # 64 s: ends inside speech once


def test_auto_partitions_by_detected_language_and_keeps_the_input_order(tr, decoding, tokmod):
    scripts = _scripts(tokmod)
    audios = [_recording(1, 20), _recording(2, 40), _recording(3, 64)]
    languages = {1: ("en", 0.75), 2: ("de", 0.5), 3: ("en", 0.625)}
    h = _Hooks(decoding, scripts, languages)
    got = tr.transcribe_batch(_Model(4), audios, language="auto", detect_languages=h.detect_languages, decode_windows=h.decode_windows)
    # one detection batch over the group's first windows: the frames the first decode sees (seek 0, the window's own size)
    assert h.detect_calls == [[(1, 0, 2000), (2, 0, 3000), (3, 0, 3000)]]
    # input order, each result with its own language and probability
    assert [r["language"] for r in got] == ["en", "de", "en"]
    assert [r["language_probability"] for r in got] == [0.75, 0.5, 0.625]
    assert [[w["seek"] for w in r["windows"]] for r in got] == [[0], [0, 3000], [0, 400, 3400]]
    # each language's recordings were decoded together, and never with another language's
    assert h.decode_calls == [[(1, 0), (3, 0)], [(3, 400)], [(3, 3400)], [(2, 0)], [(2, 3000)]]
    # the en results are what language="en" gives for those recordings with the same scripted decoder
    h_en = _Hooks(decoding, scripts, languages)
    want = tr.transcribe_batch(_Model(4), [audios[0], audios[2]], language="en", decode_windows=h_en.decode_windows)
    for r, w in zip((got[0], got[2]), want):
        assert "language_probability" not in w
        assert {k: v for k, v in r.items() if k != "language_probability"} == w
    h_de = _Hooks(decoding, scripts, languages)
    want_de = tr.transcribe_batch(_Model(4), [audios[1]], language="de", decode_windows=h_de.decode_windows)[0]
    assert {k: v for k, v in got[1].items() if k != "language_probability"} == want_de


def test_auto_detects_group_by_group_and_transcribe_is_the_single_row(tr, decoding, tokmod):
    scripts = _scripts(tokmod)
    audios = [_recording(1, 20), _recording(2, 40), _recording(3, 64)]
    languages = {1: ("en", 0.75), 2: ("de", 0.5), 3: ("en", 0.625)}
    h = _Hooks(decoding, scripts, languages)
    got = tr.transcribe_batch(_Model(2), audios, language="auto", detect_languages=h.detect_languages, decode_windows=h.decode_windows)
    assert h.detect_calls == [[(1, 0, 2000), (2, 0, 3000)], [(3, 0, 3000)]]     # groups of max_batch
    assert [r["language"] for r in got] == ["en", "de", "en"]
    h1 = _Hooks(decoding, scripts, languages)
    one = tr.transcribe(_Model(1), audios[1], language="auto", detect_languages=h1.detect_languages,
                        decode_window=lambda w, p: h1.decode_windows(w[None], [p])[0])
    assert one == got[1] and one["language"] == "de" and one["language_probability"] == 0.5


def test_auto_on_an_english_only_model_reports_en_without_detection(tr, decoding, tokmod):
    class _EnglishOnly(_Model):
        is_multilingual = False

    tok = tokmod.get_tokenizer(False)
    ts, a = tok.timestamp_begin, tok.encode("a")[0]
    h = _Hooks(decoding, {1: {0: [ts, a, ts + 100]}}, {})
    got = tr.transcribe_batch(_EnglishOnly(1), [_recording(1, 20)], language="auto", decode_windows=h.decode_windows)
    assert got[0]["language"] == "en" and got[0]["language_probability"] is None and h.detect_calls == []
    assert [s["tokens"] for s in got[0]["segments"]] == [[ts, a, ts + 100]]


def test_language_none_still_raises_and_points_at_auto(tr, decoding):
    with pytest.raises(NotImplementedError, match="auto"):
        tr.transcribe_batch(_Model(1), [_recording(1, 20)], language=None, decode_windows=lambda w, p: [])
    with pytest.raises(NotImplementedError, match="detect_language"):
        decoding.decode(None, torch.zeros(80, 3000), decoding.DecodingOptions(language=None))


def test_dropin_exposes_detect_language(wca, decoding):
    import os
    import sys
    dropin = os.path.join(os.path.dirname(os.path.abspath(decoding.__file__)), "dropin")
    sys.path.insert(0, dropin)
    try:
        whisper = importlib.import_module("whisper")
        from whisper.decoding import detect_language as d2
        assert callable(whisper.detect_language) and d2 is whisper.detect_language
        assert whisper.model.Whisper is wca.WhisperAMD and callable(whisper.model.Whisper.detect_language)   # model.detect_language
        with pytest.raises(ValueError, match="language tokens"):
            whisper.detect_language(type("EnglishOnly", (), {"is_multilingual": False, "num_languages": 99})(), torch.zeros(80, 3000))
    finally:
        sys.path.remove(dropin)


def test_cli_language_auto_reaches_transcribe_and_the_json(tr, tmp_path, monkeypatch):
    import json
    assert tr.parse_args(["--audio", "a.npy", "--output_dir", "o", "--random_init"]).language == "en"      # the default stays en
    rec = tmp_path / "rec.npy"
    np.save(rec, np.zeros(16000, np.float32))
    seen = {}

    def fake_transcribe(model, audio, **kw):
        seen.update(kw)
        return {"text": "", "segments": [], "language": "de", "language_probability": 0.5, "windows": [], "windows_without_words": 0}

    monkeypatch.setattr(tr, "transcribe", fake_transcribe)
    args = tr.parse_args(["--audio", str(rec), "--output_dir", str(tmp_path / "out"), "--random_init", "--language", "auto"])
    (path,) = tr.main(args, model=object())
    assert seen["language"] == "auto"
    out = json.load(open(path))
    assert out["language"] == "de" and out["language_probability"] == 0.5 and out["audio"] == str(rec)
