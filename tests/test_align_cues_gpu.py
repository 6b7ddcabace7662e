"""`-m gpu`: row windows in the fused alignment and force_align_cues end to end, on the tiny seeded models of tests/test_align_long_gpu.py
with a fake vocabulary. align_batch(row_windows=...) is pinned against align_batch() (full windows: bit for bit; windows around the
unconstrained path: the same path; restrictive windows: jump frames inside them; open rows beside windowed ones), and force_align_cues
on the planted-ridge checkpoint against cues cut from force_align_long's result for the same recording. The weights are synthetic:
what is pinned is the mechanics, not quality on speech. The kernel itself is pinned in tests/test_dtw_windows_gpu.py."""
import importlib
import math

import numpy as np
import pytest
import torch

import dtw_windows_ref as wref

pytestmark = pytest.mark.gpu

KW = dict(language="en", aligned_unit_type="char", aggr="topk", topk=4, medfilt_width=3)


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
def ridge(pkg):
    """The planted-ridge checkpoint (DTW row r of every window peaks at encoder frame 5 r), two rows per round."""
    dims = pkg.ModelDimensions(80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)
    m = pkg.WhisperAMD(dims, device="cuda:0", max_batch=2, precision="f16")
    m.load_state_dict(_m("synthetic").aligned_state_dict(dims, seed=5, frames_per_token=5.0))
    return m


@pytest.fixture(scope="module")
def tok(fake_vocab):
    return _m("tokenizer").get_tokenizer(True, language="en", vocab_path=fake_vocab)


def _audio(seed, seconds):
    return _m("synthetic").synth_audio(seed, int(seconds * 16000))


# ---------------------------------------------------------------------------------------------- align_batch(row_windows=...)
@pytest.fixture(scope="module")
def batch(small, tok):
    """Three rows of different lengths with their unconstrained result, computed once."""
    rt = _m("retokenize")
    texts = ["one short row", "a second row that is a good deal longer than the first", "mid sized row here"]
    rows = [[*tok.sot_sequence, tok.no_timestamps, *rt.encode(t, tok, "char"), tok.eot] for t in texts]
    n_max = max(len(r) for r in rows)
    toks = torch.full((3, n_max), tok.eot, dtype=torch.int64)
    for b, r in enumerate(rows):
        toks[b, :len(r)] = torch.tensor(r)
    n_samples = [160000, 203217, 96000]
    pcm = torch.zeros(3, max(n_samples))
    for b, n in enumerate(n_samples):
        pcm[b, :n] = torch.from_numpy(_audio(10 + b, n / 16000)[:n])
    frames = [n // 320 for n in n_samples]
    opts = small.make_opts(aggregation="topk", topk=4, sot_len=len(tok.sot_sequence), medfilt_width=3)
    args = (pcm.cuda(), n_samples, toks.cuda(), [len(r) for r in rows], frames, opts)
    n_dtw = [len(r) - len(tok.sot_sequence) - 1 for r in rows]   # DTW rows: the text tokens and the eot
    jump, sel, mean, cells = small.align_batch(*args, path_scores=True)
    return dict(args=args, n_max=n_max, frames=frames, n_dtw=n_dtw, jump=jump, sel=sel, mean=mean, cells=cells)


def _tables(batch, per_row):
    """[B, n_max] window tables from per_row(b, n, F) -> (lo, hi) of row b's n DTW rows; the entries behind them hold rubbish."""
    lo, hi = np.full((3, batch["n_max"]), 12345, np.int32), np.full((3, batch["n_max"]), -7, np.int32)
    for b, (n, F) in enumerate(zip(batch["n_dtw"], batch["frames"])):
        lo[b, :n], hi[b, :n] = per_row(b, n, F)
    return lo, hi


def test_full_windows_are_align_batch_bit_for_bit(small, batch):
    full = _tables(batch, lambda b, n, F: wref.full(n, F))
    jump, sel, mean, cells = small.align_batch(*batch["args"], path_scores=True, row_windows=full)
    assert np.array_equal(jump, batch["jump"]) and np.array_equal(sel, batch["sel"])
    assert np.array_equal(mean, batch["mean"]) and np.array_equal(cells, batch["cells"])   # (f32 means compared as bits: no NaN occurs)
    jump2, sel2 = small.align_batch(*batch["args"], row_windows=full)
    assert np.array_equal(jump2, batch["jump"]) and np.array_equal(sel2, batch["sel"])


@pytest.mark.parametrize("w", [0, 3, 40])
def test_windows_around_the_unconstrained_path_reproduce_it(small, batch, w):
    """Row i of the unconstrained path holds the frames jump[i] .. jump[i+1]; windows of that stretch widened by w on both sides hold
    the whole path, and every cell on it keeps its cost and its move (the costs of other cells can only grow), so the path is the same --
    short of an exact tie between the diagonal and the upper cost, which the real-valued maps of this model do not produce."""
    def around(b, n, F):
        j = batch["jump"][b, :n].astype(np.int64)
        lo, hi = np.maximum(j - w, 0), np.minimum(np.append(j[1:], F - 1) + w, F - 1)
        lo[0], hi[-1] = 0, F - 1
        assert wref.invalid_reason(lo, hi, n, F) is None
        return lo, hi
    jump, sel, mean, cells = small.align_batch(*batch["args"], path_scores=True, row_windows=_tables(batch, around))
    assert np.array_equal(jump, batch["jump"]) and np.array_equal(sel, batch["sel"])
    assert np.array_equal(mean, batch["mean"]) and np.array_equal(cells, batch["cells"])


def test_restrictive_windows_hold_the_jump_frames(small, batch):
    kinds = [lambda b, n, F: wref.band(n, F, 6), lambda b, n, F: wref.staircase(n, F, 4, 5, seed=b), lambda b, n, F: wref.idle_lanes(n, F)]
    for kind in kinds:
        lo, hi = _tables(batch, kind)
        jump, sel, mean, cells = small.align_batch(*batch["args"], path_scores=True, row_windows=(lo, hi))
        assert np.array_equal(sel, batch["sel"])   # everything upstream of the DTW is unchanged
        for b, (n, F) in enumerate(zip(batch["n_dtw"], batch["frames"])):
            j = jump[b, :n]
            assert (lo[b, :n] <= j).all() and (j <= hi[b, :n]).all() and (np.diff(j) >= 0).all() and j[0] == 0, b
            assert (jump[b, n:] == 0).all() and cells[b, :n].sum() >= F and (cells[b, :n] >= 1).all()
            assert (j + cells[b, :n] - 1 <= hi[b, :n]).all()   # the whole stretch of the path in a row, not only where it enters
    assert not np.array_equal(jump, batch["jump"])   # (the last kind does constrain this batch)


def test_one_batch_mixes_an_open_row_with_windowed_rows(small, batch):
    lo, hi = _tables(batch, lambda b, n, F: wref.full(n, F) if b == 1 else wref.band(n, F, 6))
    flags = [False, True, False]
    jump, sel, end_rows, scores = small.align_batch(*batch["args"], open_end=flags, row_windows=(lo, hi))
    jump_open, _sel, end_open, scores_open = small.align_batch(*batch["args"], open_end=flags)
    jump_win, _sel2 = small.align_batch(*batch["args"], row_windows=(lo, hi))
    assert np.array_equal(jump[1], jump_open[1]) and end_rows[1] == end_open[1] and scores[1] == scores_open[1]   # the open row: as without windows
    assert np.array_equal(jump[[0, 2]], jump_win[[0, 2]])                                                         # the windowed rows: as without the open row
    assert [end_rows[0], end_rows[2]] == [batch["n_dtw"][0] - 1, batch["n_dtw"][2] - 1]
    assert np.array_equal(sel, batch["sel"])


def test_bad_windows_are_refused_and_nothing_is_consumed(small, batch):
    err = _m("_lib").WcaError
    band = _tables(batch, lambda b, n, F: wref.band(n, F, 6))
    with pytest.raises(err, match="open"):   # an open end with real windows
        small.align_batch(*batch["args"], open_end=[True, False, False], row_windows=band)
    for kind in wref.INVALID_KINDS:
        def broken(b, n, F, kind=kind):
            return wref.make_invalid(kind, n, F) if b == 2 else wref.full(n, F)
        with pytest.raises(err):
            small.align_batch(*batch["args"], row_windows=_tables(batch, broken))
    with pytest.raises(ValueError, match="row_windows"):
        small.align_batch(*batch["args"], row_windows=(band[0][:, :-1], band[1][:, :-1]))
    with pytest.raises(err):   # nothing was enqueued by any of them
        small.fetch(3, batch["n_max"], batch["args"][5])
    jump, sel = small.align_batch(*batch["args"])
    assert np.array_equal(jump, batch["jump"]) and np.array_equal(sel, batch["sel"])


def test_two_windowed_batches_in_flight(small, batch):
    a = _tables(batch, lambda b, n, F: wref.band(n, F, 6))
    c = _tables(batch, lambda b, n, F: wref.staircase(n, F, 4, 5, seed=b))
    want_a, want_c = small.align_batch(*batch["args"], row_windows=a)[0], small.align_batch(*batch["args"], row_windows=c)[0]
    small.align_batch(*batch["args"], row_windows=a, enqueue_only=True)
    small.align_batch(*batch["args"], row_windows=c, enqueue_only=True)
    got_a = small.fetch(3, batch["n_max"], batch["args"][5])[0]
    got_c = small.fetch(3, batch["n_max"], batch["args"][5])[0]
    assert np.array_equal(got_a, want_a) and np.array_equal(got_c, want_c) and not np.array_equal(want_a, want_c)


# ---------------------------------------------------------------------------------------------- force_align_cues
def _cues_from(result, words_per_cue=6):
    """Cues cut from a force_align_long result: runs of words_per_cue words, from the first one's start to the last one's end."""
    words = result["words"]
    return [(g[0]["start"], g[-1]["end"], "".join(w["word"] for w in g).strip())
            for g in (words[k:k + words_per_cue] for k in range(0, len(words), words_per_cue))]


@pytest.fixture(scope="module")
def long70(ridge, fake_vocab):
    text = _m("synthetic").synth_text(7, 600)   # 600 units at 0.1 s each: 60 s of text in 70 s of audio
    pcm = _audio(2, 70)
    out = _m("align_long").force_align_long(ridge, pcm, text, vocab_path=fake_vocab, **KW)
    assert out["unaligned_words"] == 0
    return pcm, out, _cues_from(out)


def _count_rounds(model, monkeypatch):
    calls = []
    real = model.encode_batch
    monkeypatch.setattr(model, "encode_batch", lambda *a, **k: (calls.append(k["mel"].shape[0]), real(*a, **k))[1])
    return calls


def _check_cue_result(al, out, cues, tok, slack, seconds):
    plan = al.CuePlan(cues, [al.transcript_units(t, tok, "char") for _a, _b, t in cues], len(tok.sot_sequence), cue_slack=slack)
    plan.set_audio(int(seconds * 100) + 3000)
    strip = lambda ws: [{k: v for k, v in w.items() if k != "mean_word_score"} for w in ws]   # noqa: E731
    assert strip(out["windows"]) == strip(plan.windows) and out["unaligned_words"] == 0
    assert [(c["w0"], c["w1"], c["window"]) for c in out["cues"]] == [(c["w0"], c["w1"], c["window"]) for c in plan.cues]
    assert [w["word"] for w in out["words"]] == [w["word"] for w in plan.words]
    for w in out["words"]:
        a, b = cues[w["cue"]][:2]
        assert a - slack - 0.02 - 1e-9 <= w["start"] <= b + slack + 0.02 + 1e-9 and w["start"] <= w["end"] <= seconds + 1e-9, w
    return plan


def test_cues_cut_from_the_sequential_result(ridge, tok, fake_vocab, long70, monkeypatch):
    al = _m("align_long")
    pcm, seq, cues = long70
    calls = _count_rounds(ridge, monkeypatch)
    out = al.force_align_cues(ridge, pcm, cues, vocab_path=fake_vocab, **KW)
    plan = _check_cue_result(al, out, cues, tok, 1.0, 70)
    W = len(plan.windows)
    assert W >= 3 and len(calls) == math.ceil(W / 2) and sum(calls) == W   # rounds of max_batch = 2 rows, not one per window
    assert set(out) == {"words", "cues", "windows", "unaligned_words"} and set(out["words"][0]) == {"word", "start", "end", "cue"}
    # (not asserted, since nothing bounds it but the slack windows checked above: a closed cue window must spend the frames between the end
    # of its ridge and its last frame somewhere, which the open window of the sequential loop did not have to)
    moved = [abs(w["start"] - s["start"]) for w, s in zip(out["words"], seq["words"])]
    print("word starts against the sequential result: moved by at most %.2f s, median %.2f s" % (max(moved), float(np.median(moved))))
    # a tighter slack: more windows fit no better, the words stay inside
    out05 = al.force_align_cues(ridge, pcm, cues, vocab_path=fake_vocab, cue_slack=0.5, **KW)
    _check_cue_result(al, out05, cues, tok, 0.5, 70)


def test_cues_with_word_scores_and_trim_silence(ridge, tok, fake_vocab, long70):
    al = _m("align_long")
    pcm, _seq, cues = long70
    plain = al.force_align_cues(ridge, pcm, cues, vocab_path=fake_vocab, **KW)
    out = al.force_align_cues(ridge, pcm, cues, vocab_path=fake_vocab, word_scores=True, trim_silence=True, **KW)
    assert set(out) == {"words", "cues", "windows", "unaligned_words", "speech_segments"}
    assert all(0.0 <= w["score"] <= 1.0 for w in out["words"]) and all(0.0 <= w["mean_word_score"] <= 1.0 for w in out["windows"])
    scored = al.force_align_cues(ridge, pcm, cues, vocab_path=fake_vocab, word_scores=True, **KW)
    strip = lambda ws, key: [{k: v for k, v in w.items() if k != key} for w in ws]   # noqa: E731
    assert strip(scored["words"], "score") == plain["words"] and strip(scored["windows"], "mean_word_score") == plain["windows"]
    trimmed = _m("timing").trim_words_to_speech(scored["words"], [(s["start_frame"], s["stop_frame"]) for s in out["speech_segments"]])
    assert out["words"] == trimmed
    for a, b in zip(out["words"], scored["words"]):
        assert b["start"] - 1e-9 <= a["start"] <= a["end"] <= b["end"] + 1e-9


def test_srt_file_and_cli(ridge, tok, fake_vocab, long70, tmp_path):
    import json
    al = _m("align_long")
    pcm, _seq, cues = long70
    cues = cues[:8]
    def stamp(t):
        ms = int(round(t * 1000))
        return "%02d:%02d:%02d,%03d" % (ms // 3600000, ms // 60000 % 60, ms // 1000 % 60, ms % 1000)
    srt = tmp_path / "rec.srt"
    srt.write_text("".join("%d\n%s --> %s\n<i>%s</i>\n\n" % (k + 1, stamp(a), stamp(b), t) for k, (a, b, t) in enumerate(cues)), encoding="utf-8")
    parsed = _m("longform").read_cues(str(srt))
    assert [t for _a, _b, t in parsed] == [t for _a, _b, t in cues] and all(abs(p[0] - c[0]) < 1e-3 and abs(p[1] - c[1]) < 1e-3 for p, c in zip(parsed, cues))
    out = al.force_align_cues(ridge, pcm, str(srt), vocab_path=fake_vocab, **KW)
    assert out == al.force_align_cues(ridge, pcm, parsed, vocab_path=fake_vocab, **KW) and out["unaligned_words"] == 0
    npy = tmp_path / "rec.npy"
    np.save(str(npy), pcm)
    args = al.parse_args(["--audio", str(npy), "--cues", str(srt), "--cue_slack", "1.0", "--vocab", fake_vocab, "--output_dir", str(tmp_path / "o"),
                          "--topk", "4"])
    got = json.load(open(al.main(args, model=ridge)[0]))
    assert got["words"] == out["words"] and got["cue_file"] == str(srt) and got["windows"] == out["windows"]


def test_batch_form_equals_the_single_form(ridge, tok, fake_vocab, long70):
    """The comparison chosen: in the reference-precision mode, where tests/test_batch_invariance_gpu.py pins the jump frames as independent
    of the batch size, the whole results are EQUAL (windows, cues, every word time); in the f16 mode the kernel choice by row count may
    move near-tied DTW steps, and only the plans are compared."""
    al = _m("align_long")
    pcm, _seq, cues = long70
    audios = [pcm, pcm[:16000 * 25], _audio(4, 20)]
    cue_lists = [cues, [c for c in cues if c[1] < 24.0], [c for c in cues if c[1] < 50.0]]   # the last one's cues outlast its audio
    together16 = al.force_align_cues_batch(ridge, audios, cue_lists, vocab_path=fake_vocab, **KW)
    ridge.set_precision("reference")
    try:
        together = al.force_align_cues_batch(ridge, audios, cue_lists, vocab_path=fake_vocab, **KW)
        alone = [al.force_align_cues(ridge, a, c, vocab_path=fake_vocab, **KW) for a, c in zip(audios, cue_lists)]
    finally:
        ridge.set_precision("f16")
    for k, (got, want, got16) in enumerate(zip(together, alone, together16)):
        assert got == want, k
        assert got16["windows"] == want["windows"] and got16["cues"] == want["cues"], k
    assert together[0]["unaligned_words"] == together[1]["unaligned_words"] == 0
    assert together[2]["unaligned_words"] > 0   # its second window starts past the 20 s of audio and does not run


def test_refusals_come_before_any_audio_is_read(ridge, fake_vocab):
    al = _m("align_long")
    with pytest.raises(ValueError, match="sorted"):
        al.force_align_cues(ridge, "/no/such/file.wav", [(5.0, 6.0, "ab"), (1.0, 2.0, "cd")], vocab_path=fake_vocab, **KW)
    with pytest.raises(ValueError, match="does not fit"):
        al.force_align_cues(ridge, "/no/such/file.wav", [(0.0, 40.0, "ab")], vocab_path=fake_vocab, **KW)
