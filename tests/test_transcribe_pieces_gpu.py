"""transcribe(pieces=3) on the MI355X: one synthetic recording of 150 s on the tiny seeded model of tests/test_transcribe_batch_gpu.py
(seed 5, max_batch 4, sample_len 24), cut at quiet frames (wca_quiet_cuts) and decoded three rows at a time, against the three runs
transcribe(clip_timestamps=[cuts[k] / 100, cuts[k + 1] / 100]) merged: windows, tokens, segment times and words must be equal. A piece
that differs is excused only by the rule of that file: its first differing window was decoded from the same frames with the same prompt,
and the two token rows part at a position where the teacher-forced logits of the two choices are closer than 1e-3 (the GEMM path, and
with it the fp32 summation order, depends on the number of rows in the batch). At most one piece of the three may be excused.
Measured on the MI355X: the cuts fall at frames 4894 and 9640, every piece has two windows, and all three pieces equal their clips in both
forms, so no excuse is taken."""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

SECONDS = 150


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
def audio():
    return _m("synthetic").synth_audio(33, 16000 * SECONDS + 40)


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


def _brief(window):
    return window["seek"], window["size"], window["advance"], window["skipped"]


def _tokens_by_seek(segments):
    out = {}
    for s in segments:
        out.setdefault(s["seek"], []).extend(s["tokens"])
    return out


def _first_difference(wa, sa, wb, sb):
    """Index of the first window at which the two window lists differ in (seek, size, advance, skipped) or in the kept tokens, or None."""
    ta, tb = _tokens_by_seek(sa), _tokens_by_seek(sb)
    for k in range(max(len(wa), len(wb))):
        if k >= len(wa) or k >= len(wb) or _brief(wa[k]) != _brief(wb[k]) or ta.get(wa[k]["seek"], []) != tb.get(wb[k]["seek"], []):
            return k
    return None


def _excused(model, tok, mel_long, wa, wb, log_a, log_b, what):
    """The window starts from the same state in both runs (everything before it in its piece agrees), so both decoded the same frames
    with the same prompt: the two token rows may differ only from a position at which the teacher-forced logits of the two choices are
    closer than 1e-3."""
    assert (wa["seek"], wa["size"]) == (wb["seek"], wb["size"]), what
    key = _key(model.mel_window(mel_long, wa["seek"], wa["size"]))
    (prompt_a, toks_a, window), (prompt_b, toks_b, _) = log_a[key], log_b[key]
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
    print("%s: window at seek %d diverges at sampled position %d: tokens %d / %d, teacher-forced logit gap %.3e" % (
        what, wa["seek"], p_, choice_a, choice_b, gap))
    assert gap < 1e-3, (what, p_, gap)


@pytest.mark.parametrize("words", [False, True], ids=["tokens-only", "word-timestamps"])
def test_pieces_equal_their_clips_merged(small, audio, fake_vocab, monkeypatch, words):
    tr, decoding = _m("transcribe"), _m("decoding")
    tok = _m("tokenizer").get_tokenizer(True, language="en", task="transcribe", vocab_path=fake_vocab if words else None)
    kw = dict(language="en", sample_len=24)
    if words:
        kw.update(vocab_path=fake_vocab, word_timestamps=True, topk=4)
    log = _Log(decoding)
    monkeypatch.setattr(decoding, "decode", log)
    whole = tr.transcribe(small, audio, pieces=3, **kw)
    monkeypatch.setattr(decoding, "decode", log.real)
    content = len(audio) // 160
    mel_long = small.log_mel_long(torch.from_numpy(audio).cuda())
    cuts, levels = small.quiet_cuts(mel_long, 3)
    assert [(p["start_frame"], p["stop_frame"]) for p in whole["pieces"]] == list(zip(cuts, cuts[1:])) and cuts[0] == 0 and cuts[-1] == content
    assert [p["level"] for p in whole["pieces"]] == [None] + levels
    assert all(abs(c - content * k // 3) <= 500 and c % 2 == 0 for k, c in enumerate(cuts[:-1]))
    # the first round decodes the three pieces' first windows as three rows, and the batch only shrinks
    assert log.batches[0] == 3 and all(b <= a for a, b in zip(log.batches, log.batches[1:]))
    assert sum(log.batches) == len(whole["windows"])
    assert [s["id"] for s in whole["segments"]] == list(range(len(whole["segments"])))
    n_excused, n_segments = 0, 0
    for k in range(3):
        what = "piece %d [%d, %d)" % (k, cuts[k], cuts[k + 1])
        part_log = _Log(decoding)
        monkeypatch.setattr(decoding, "decode", part_log)
        part = tr.transcribe(small, audio, clip_timestamps=[cuts[k] / 100, cuts[k + 1] / 100], **kw)
        monkeypatch.setattr(decoding, "decode", part_log.real)
        assert "pieces" not in part and part["windows"][0]["seek"] == cuts[k], what
        assert part["windows"][-1]["seek"] + part["windows"][-1]["advance"] == cuts[k + 1], what
        mine = [w for w in whole["windows"] if w["piece"] == k]
        seeks = {w["seek"] for w in mine}
        segs = [s for s in whole["segments"] if s["seek"] in seeks]
        assert mine[0]["seek"] == cuts[k] and all(cuts[k] <= w["seek"] and w["seek"] + w["size"] <= cuts[k + 1] for w in mine), what
        d = _first_difference(part["windows"], part["segments"], mine, segs)
        print("%s: %d windows as a clip, %d as a piece, first difference: %s" % (what, len(part["windows"]), len(mine), d))
        if d is not None:
            n_excused += 1
            _excused(small, tok, mel_long, part["windows"][d], mine[d], part_log.rows, log.rows, what)
            n_segments += len(segs)
            continue
        assert [{**w, "piece": k} for w in part["windows"]] == mine, what   # (seek, size, advance, skipped, max_frames, aligned)
        assert len(part["segments"]) == len(segs), what
        for sa, sb in zip(part["segments"], segs):
            assert sb["id"] == n_segments + sa["id"], what   # the pieces' segments are numbered on
            assert (sa["seek"], sa["start"], sa["end"], sa["tokens"], sa["text"]) == (sb["seek"], sb["start"], sb["end"], sb["tokens"], sb["text"]), what
            assert [(w["word"], w["start"], w["end"]) for w in sa["words"]] == [(w["word"], w["start"], w["end"]) for w in sb["words"]], what
        n_segments += len(segs)
    assert n_segments == len(whole["segments"])
    assert n_excused <= 1, n_excused
    if words:
        assert sum(len(s["words"]) for s in whole["segments"]) > 0
