"""transcribe_batch on the MI355X: three synthetic recordings of 20 s, 47 s and 75 s in lock-step on the tiny seeded model of
tests/test_decode_gpu.py, through the engine's own decode (wca_decode with per_row 1), against transcribe() of each recording alone.
The windows (seek, size, advance, skipped) and the tokens must be equal; where they are not, the first differing window is excused
only by a measured argmax near-tie of that window's decode (the rule of tests/test_decode_rows_gpu.py: a teacher-forced logit gap
below 1e-3 at the first divergent position), for at most one recording of the three. Where the tokens agree, the segment times are
equal and the words are equal in text, count and times."""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

SECONDS = (20, 47, 75)


def _m(n):
    return importlib.import_module("whisper-char-alignment_amd." + n)


@pytest.fixture(scope="module")
def small():
    pkg = importlib.import_module("whisper-char-alignment_amd")
    dims = pkg.ModelDimensions(80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)
    m = pkg.WhisperAMD(dims, device="cuda:0", max_batch=4, precision="f16")
    m.load_state_dict(_m("synthetic").random_state_dict(dims, seed=5))
    return m


@pytest.fixture(scope="module")
def audios():
    return [_m("synthetic").synth_audio(30 + i, 16000 * s + 40 * i) for i, s in enumerate(SECONDS)]


def _key(window):
    return window[:, :64].detach().cpu().numpy().tobytes()


class _Log:
    """decoding.decode with every decoded row written down: window key -> (prompt, sampled tokens, the window)."""

    def __init__(self, decoding):
        self.real, self.rows, self.batches = decoding.decode, {}, []

    def __call__(self, model, mel, options, **kw):
        res = self.real(model, mel, options, **kw)
        many = isinstance(options, (list, tuple))
        mels = mel if mel.ndim == 3 else mel[None]
        self.batches.append(mels.shape[0])
        for w, o, r in zip(mels, options if many else [options], res if many else [res]):
            self.rows[_key(w)] = (list(o.prompt or []), list(r.tokens), w.clone())
        return res


def _brief_windows(res):
    return [(w["seek"], w["size"], w["advance"], w["skipped"]) for w in res["windows"]]


def _tokens_by_seek(res):
    out = {}
    for s in res["segments"]:
        out.setdefault(s["seek"], []).extend(s["tokens"])
    return out


def _first_difference(a, b):
    """Index of the first window at which the two results differ in (seek, size, advance, skipped) or in the kept tokens, or None."""
    ta, tb = _tokens_by_seek(a), _tokens_by_seek(b)
    wa, wb = _brief_windows(a), _brief_windows(b)
    for k in range(max(len(wa), len(wb))):
        if k >= len(wa) or k >= len(wb) or wa[k] != wb[k] or ta.get(wa[k][0], []) != tb.get(wb[k][0], []):
            return k
    return None


def _excused(model, tok, mel_long, alone, batch, k, log_alone, log_batch, what):
    """The k-th window starts from the same state in both runs (everything before it agrees), so both decoded the same window with
    the same prompt: its two token rows may differ only from a position at which the teacher-forced logits of the two choices
    are closer than 1e-3."""
    wa, wb = alone["windows"][k], batch["windows"][k]
    assert (wa["seek"], wa["size"]) == (wb["seek"], wb["size"]), what
    key = _key(model.mel_window(mel_long, wa["seek"], wa["size"]))
    (prompt_a, toks_a, window), (prompt_b, toks_b, _) = log_alone[key], log_batch[key]
    assert prompt_a == prompt_b, what
    assert toks_a != toks_b, (what, "the decodes agree: the difference is in the host loop")
    p_ = next(i for i in range(max(len(toks_a), len(toks_b))) if i >= len(toks_a) or i >= len(toks_b) or toks_a[i] != toks_b[i])
    initial = ([tok.sot_prev] + prompt_a[-(448 // 2 - 1):] if prompt_a else []) + list(tok.sot_sequence)
    choice_a = toks_a[p_] if p_ < len(toks_a) else tok.eot
    choice_b = toks_b[p_] if p_ < len(toks_b) else tok.eot
    forced = torch.tensor([initial + toks_a[:p_]], dtype=torch.int64).cuda()
    _w, logits = model.get_attentions(window[None], forced, [100], 3, 1.0)
    row = logits[0, -1].float().cpu().numpy()
    gap = abs(float(row[choice_a]) - float(row[choice_b]))
    print("%s: window %d (seek %d) diverges at sampled position %d: tokens %d / %d, teacher-forced logit gap %.3e" % (
        what, k, wa["seek"], p_, choice_a, choice_b, gap))
    assert gap < 1e-3, (what, k, p_, gap)


@pytest.mark.parametrize("words", [False, True], ids=["tokens-only", "word-timestamps"])
def test_batch_equals_each_recording_alone(small, audios, fake_vocab, monkeypatch, words):
    tr, decoding = _m("transcribe"), _m("decoding")
    tok = _m("tokenizer").get_tokenizer(True, language="en", task="transcribe", vocab_path=fake_vocab if words else None)
    kw = dict(language="en", sample_len=24)
    if words:
        kw.update(vocab_path=fake_vocab, word_timestamps=True, topk=4)
    logs_alone, alone = [], []
    for pcm in audios:
        log = _Log(decoding)
        monkeypatch.setattr(decoding, "decode", log)
        alone.append(tr.transcribe(small, pcm, **kw))
        monkeypatch.setattr(decoding, "decode", log.real)
        logs_alone.append(log.rows)
    log = _Log(decoding)
    monkeypatch.setattr(decoding, "decode", log)
    batch = small.transcribe_batch(audios, **kw)
    monkeypatch.setattr(decoding, "decode", log.real)
    assert len(batch) == 3
    # the batch shrinks as recordings end: the first round decodes all three, the last rounds the longest recording only
    assert log.batches[0] == 3 and log.batches[-1] == 1 and all(b <= a for a, b in zip(log.batches, log.batches[1:]))
    assert sum(log.batches) == sum(len(r["windows"]) for r in batch)
    n_excused = 0
    for i, (a, b) in enumerate(zip(alone, batch)):
        what = "recording %d (%d s)" % (i, SECONDS[i])
        content = len(audios[i]) // 160
        assert b["windows"][0]["seek"] == 0 and b["windows"][-1]["seek"] + b["windows"][-1]["advance"] == content, what
        k = _first_difference(a, b)
        print("%s: %d windows alone, %d in the batch, first difference: %s" % (what, len(a["windows"]), len(b["windows"]), k))
        if k is not None:
            n_excused += 1
            _excused(small, tok, small.log_mel_long(torch.from_numpy(audios[i]).cuda()), a, b, k, logs_alone[i], log.rows, what)
            continue
        assert [w["max_frames"] for w in a["windows"]] == [w["max_frames"] for w in b["windows"]], what
        assert len(a["segments"]) == len(b["segments"]) and a["text"] == b["text"], what
        for sa, sb in zip(a["segments"], b["segments"]):
            assert (sa["id"], sa["seek"], sa["start"], sa["end"], sa["tokens"], sa["text"]) == \
                (sb["id"], sb["seek"], sb["start"], sb["end"], sb["tokens"], sb["text"]), what
            assert [(w["word"], w["start"], w["end"]) for w in sa["words"]] == [(w["word"], w["start"], w["end"]) for w in sb["words"]], what
        assert [w["aligned"] for w in a["windows"]] == [w["aligned"] for w in b["windows"]], what
        assert a["windows_without_words"] == b["windows_without_words"], what
    assert n_excused <= 1, n_excused
    if words:
        assert sum(len(s["words"]) for r in batch for s in r["segments"]) > 0
