"""`-m gpu`: long-form forced alignment end to end on the tiny seeded model of tests/test_decode_gpu.py's `small` fixture with a fake
vocabulary: the closed last window against the existing single-window path, align_batch(open_end=...) against align_batch(), the window
loop's mechanics on a 70 s recording, and the lock-step driver against the single-recording loop. The model's weights are random, so
the maps hold no alignment: what is pinned here is the mechanics (parity of the path is unpinned: neither the reference nor upstream
aligns a long recording against a given text). The kernel itself is pinned in tests/test_dtw_open_gpu.py."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _m(n):
    return importlib.import_module("whisper-char-alignment_amd." + n)


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("whisper-char-alignment_amd")


@pytest.fixture(scope="module")
def small(pkg):
    dims = pkg.ModelDimensions(80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)
    m = pkg.WhisperAMD(dims, device="cuda:0", max_batch=4, precision="f16")
    m.load_state_dict(_m("synthetic").random_state_dict(dims, seed=5))
    return m


@pytest.fixture(scope="module")
def tok(fake_vocab):
    return _m("tokenizer").get_tokenizer(True, language="en", vocab_path=fake_vocab)


def _text(seed, n_units):
    """Lower-case words of 2-7 letters, about n_units char units with their spaces."""
    rng = np.random.default_rng(seed)
    words, n = [], 0
    while n < n_units:
        w = "".join(rng.choice(list("abcdefghijklmnopqrstuvwxyz"), size=int(rng.integers(2, 8))))
        words.append(w)
        n += len(w) + 1
    return " ".join(words)


def _audio(seed, seconds):
    return _m("synthetic").synth_audio(seed, int(seconds * 16000))


KW = dict(language="en", aligned_unit_type="char", aggr="topk", topk=4, medfilt_width=3)


def test_short_recording_is_one_closed_window_with_the_single_window_times(small, tok, fake_vocab):
    al, tm, rt = _m("align_long"), _m("timing"), _m("retokenize")
    pcm, text = _audio(1, 12), "hello tiny world of words"
    out = al.force_align_long(small, pcm, text, vocab_path=fake_vocab, **KW)
    assert [(w["seek"], w["size"], w["closed"], w["committed"]) for w in out["windows"]] == [(0, 1200, True, 5)]
    assert out["unaligned_words"] == 0 and out["windows_without_words"] == 0
    # the existing single-window path on the same window: encode the cut mel, align_batch without open_end, words_from_jump_frames
    units = rt.encode(rt.remove_punctuation(text), tok, "char")
    tokens = [*tok.sot_sequence, tok.no_timestamps, *units, tok.eot]
    mel = small.log_mel_long(torch.from_numpy(pcm))
    small.encode_batch(mel=small.mel_window(mel, 0, 1200)[None])
    opts = small.make_opts(aggregation="topk", topk=4, sot_len=len(tok.sot_sequence), medfilt_width=3)
    jump, _sel = small.align_batch(None, None, torch.tensor([tokens], device="cuda"), [len(tokens)], [600], opts)
    words, starts, ends = tm.words_from_jump_frames(jump[0], units, tok, "char")
    assert [w["word"] for w in out["words"]] == words[:-1] == ["hello", " tiny", " world", " of", " words"]
    assert [w["start"] for w in out["words"]] == [float(s) for s in starts] and [w["end"] for w in out["words"]] == [float(e) for e in ends]
    assert out["windows"][0]["end_row"] == len(units)   # a closed path ends in the eot row


def test_align_batch_with_every_row_closed_is_align_batch(small, tok):
    rt = _m("retokenize")
    texts = ["one short row", "a second row that is a good deal longer than the first", "mid sized row here"]
    rows = [[*tok.sot_sequence, tok.no_timestamps, *rt.encode(t, tok, "char"), tok.eot] for t in texts]
    n_max = max(len(r) for r in rows)
    toks = torch.full((3, n_max), tok.eot, dtype=torch.int64)
    for b, r in enumerate(rows):
        toks[b, :len(r)] = torch.tensor(r)
    toks = toks.cuda()
    n_samples = [160000, 203217, 96000]
    pcm = torch.zeros(3, max(n_samples))
    for b, n in enumerate(n_samples):
        pcm[b, :n] = torch.from_numpy(_audio(10 + b, n / 16000)[:n])
    pcm = pcm.cuda()
    frames = [n // 320 for n in n_samples]
    opts = small.make_opts(aggregation="topk", topk=4, sot_len=len(tok.sot_sequence), medfilt_width=3)
    args = (pcm, n_samples, toks, [len(r) for r in rows], frames, opts)
    jump0, sel0 = small.align_batch(*args)
    jump1, sel1, end_rows, scores = small.align_batch(*args, open_end=[False] * 3)
    assert np.array_equal(jump0, jump1) and np.array_equal(sel0, sel1)
    assert list(end_rows) == [len(r) - len(tok.sot_sequence) - 2 for r in rows] and np.isfinite(scores).all()
    # with log-probs as well, and one row open: the closed rows keep their result, the open row's tail is -1
    vocab_end = tok.eot
    jump2, sel2, lp2 = small.align_batch(*args, token_logprobs_vocab_end=vocab_end)
    jump3, sel3, lp3, end3, _sc3 = small.align_batch(*args, token_logprobs_vocab_end=vocab_end, open_end=[False, True, False])
    assert np.array_equal(lp2, lp3) and np.array_equal(sel2, sel3) and np.array_equal(jump2, jump0)
    assert np.array_equal(jump3[[0, 2]], jump0[[0, 2]]) and end3[0] == end_rows[0] and end3[2] == end_rows[2]
    n1 = len(rows[1]) - len(tok.sot_sequence) - 1
    assert 0 <= end3[1] < n1 and (jump3[1, :end3[1] + 1] >= 0).all() and (jump3[1, end3[1] + 1:n1] == -1).all() and (jump3[1, n1:] == 0).all()
    small.align_batch(*args, enqueue_only=True)
    with pytest.raises(_m("_lib").WcaError):   # end rows of a batch that was enqueued without them: refused, nothing consumed
        small.fetch(3, n_max, opts, with_end_rows=True)
    small.fetch(3, n_max, opts)


def _check_mechanics(al, out, text, tok, seconds):
    units, starts, words = al.transcript_units(text, tok, "char")
    content = int(seconds * 100)
    wins = out["windows"]
    assert [w["word"] for w in out["words"]] == words   # every word exactly once, in transcript order
    seeks = [w["seek"] for w in wins]
    assert all(b > a for a, b in zip(seeks, seeks[1:])) and seeks[0] == 0
    timed = [w for w in out["words"] if w["start"] is not None]
    assert out["unaligned_words"] == len(words) - len(timed) and all(w["start"] is None for w in out["words"][len(timed):])
    t = [w["start"] for w in timed]
    assert all(b >= a for a, b in zip(t, t[1:])) and all(0 <= w["start"] <= w["end"] <= seconds for w in timed)
    cursor, without = 0, 0
    for k, w in enumerate(wins):
        assert w["w0"] == cursor and w["size"] == min(3000, content - w["seek"])
        rows = [starts[j] - starts[w["w0"]] for j in range(w["w0"], w["w1"] + 1)]
        assert 4 + rows[-1] + 1 <= 448 and 0 <= w["end_row"] < rows[-1] + 1   # the offered rows: the run's units and its eot
        assert w["closed"] == (w["seek"] + w["size"] >= content and w["w1"] == len(words))
        complete = sum(1 for j in range(len(rows) - 1) if rows[j + 1] - 1 <= w["end_row"])
        nxt = wins[k + 1]["seek"] if k + 1 < len(wins) else None
        if w["closed"] or (w["w1"] == len(words) and w["end_row"] == rows[-1]):
            assert w["committed"] == w["w1"] - w["w0"] and nxt is None
        elif w["committed"]:
            assert w["committed"] == complete - 1 >= 1   # all complete words but the last
            assert nxt is None or 0 < nxt - w["seek"] < w["size"]
        else:
            without += 1
            assert nxt is None or nxt - w["seek"] == w["size"]
        cursor += w["committed"]
    assert cursor == len(timed) and without == out["windows_without_words"]
    return len(units)


def test_seventy_second_recording_loop_mechanics(small, tok, fake_vocab):
    al = _m("align_long")
    text = _text(7, 600)
    out = al.force_align_long(small, _audio(2, 70), text, vocab_path=fake_vocab, **KW)
    n_units = _check_mechanics(al, out, text, tok, 70)
    assert 590 <= n_units <= 610 and len(out["windows"]) >= 2
    print("70 s: %d windows, %d unaligned words, %d windows without words" % (len(out["windows"]), out["unaligned_words"],
                                                                              out["windows_without_words"]))


def test_planted_alignment_heads_give_the_planted_end_rows_and_times(pkg, tok, fake_vocab):
    """The one place where the maps hold an alignment: synthetic.aligned_state_dict plants a ridge at 5 encoder frames per decoder
    position into the upper layers' head 0, so in EVERY window DTW row r peaks at frame 5 r. A 3000-frame window (1500 encoder frames)
    then holds rows 0 .. 1499 / 5 = 299.8 of the run it is offered: the open-end DTW must end in row 299 or 300. A row is entered after
    the previous row's peak and not after its own (one more frame for the width-3 median filter), so a word whose first unit is unit u
    of the transcript starts in (0.1 u - 0.1, 0.1 u + 0.02] s in the first window; every later window starts where a held-back word
    was entered, up to one peak spacing (0.1 s) before that word's own peak, and is re-based there."""
    al = _m("align_long")
    dims = pkg.ModelDimensions(80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)
    m = pkg.WhisperAMD(dims, device="cuda:0", max_batch=4, precision="f16")
    m.load_state_dict(_m("synthetic").aligned_state_dict(dims, seed=5, frames_per_token=5.0))
    text = _m("synthetic").synth_text(7, 600)   # 600 units at 0.1 s each: 60 s of text in 70 s of audio
    out = al.force_align_long(m, _audio(2, 70), text, vocab_path=fake_vocab, **KW)
    _check_mechanics(al, out, text, tok, 70)
    _units, starts, words = al.transcript_units(text, tok, "char")
    wins = out["windows"]
    assert len(wins) == 3 and out["unaligned_words"] == 0 and out["windows_without_words"] == 0
    assert [w["size"] for w in wins[:2]] == [3000, 3000] and all(w["end_row"] in (299, 300) for w in wins[:2])
    k, left = 0, wins[0]["committed"]
    for j, w in enumerate(out["words"][:sum(x["committed"] for x in wins[:2])]):   # the words of the two open windows
        while left == 0:
            k, left = k + 1, wins[k + 1]["committed"]
        left -= 1
        assert 0.1 * starts[j] - 0.1 * (k + 1) < w["start"] <= 0.1 * starts[j] + 0.02 + 1e-9, (j, k, w)


def test_lock_step_batch_returns_what_each_recording_gives_alone(small, tok, fake_vocab):
    """Compared in the reference-precision mode: tests/test_batch_invariance_gpu.py pins the jump frames as independent of the batch
    size only there (in the f16 mode the kernel choice by row count moves near-tied DTW steps of random-weight maps)."""
    al = _m("align_long")
    audios = [_audio(3, 20), _audio(4, 45), _audio(2, 70)]
    texts = [_text(8, 150), _text(9, 380), _text(7, 600)]
    small.set_precision("reference")
    try:
        together = al.force_align_long_batch(small, audios, texts, vocab_path=fake_vocab, **KW)
        alone = [al.force_align_long(small, a, t, vocab_path=fake_vocab, **KW) for a, t in zip(audios, texts)]
    finally:
        small.set_precision("f16")
    for k, (got, want, text, seconds) in enumerate(zip(together, alone, texts, (20, 45, 70))):
        _check_mechanics(al, got, text, tok, seconds)
        assert got == want, k


def test_over_long_word_is_refused_before_any_gpu_work(small, fake_vocab):
    al = _m("align_long")
    with pytest.raises(ValueError, match="units"):
        al.force_align_long(small, np.zeros(16000, np.float32), "ok " + "x" * 450, vocab_path=fake_vocab, **KW)
    with pytest.raises(ValueError, match="vocab_path"):
        al.force_align_long(small, np.zeros(16000, np.float32), "ok", vocab_path=None, **KW)


def test_cli_writes_word_times_json(small, fake_vocab, tmp_path):
    import json
    import wave
    al = _m("align_long")
    pcm = _audio(5, 8)
    wav = tmp_path / "rec.wav"
    with wave.open(str(wav), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes((pcm * 32767).astype("<i2").tobytes())
    txt = tmp_path / "rec.txt"
    txt.write_text("Hello, tiny world!")
    args = al.parse_args(["--audio", str(wav), "--text", str(txt), "--vocab", fake_vocab, "--output_dir", str(tmp_path / "out"), "--topk", "4"])
    paths = al.main(args, model=small)
    got = json.load(open(paths[0]))
    assert paths == [str(tmp_path / "out" / "rec.json")] and [w["word"].strip() for w in got["words"]] == ["Hello", "tiny", "world"]
    assert got["unaligned_words"] == 0 and len(got["windows"]) == 1 and got["windows"][0]["closed"]
    scp = tmp_path / "list.scp"
    scp.write_text("%s\t%s\n%s\t%s\n" % (wav, txt, wav, txt))
    args = al.parse_args(["--scp", str(scp), "--batch", "2", "--vocab", fake_vocab, "--output_dir", str(tmp_path / "out2"), "--topk", "4"])
    paths = al.main(args, model=small)
    assert len(paths) == 2 and [w["word"] for w in json.load(open(paths[1]))["words"]] == [w["word"] for w in got["words"]]
