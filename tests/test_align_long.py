"""CPU tests of the long-form forced alignment: the numpy restatement of the open-end DTW on planted matrices (tests/dtw_open_ref.py),
and the window loop of align_long.py against a scripted aligner built from a planted truth -- a "recording" whose unit boundaries are
known encoder frames. A window's scripted aligner returns the true jump frames of the offered units and the last row that fits."""
import importlib

import numpy as np
import pytest

import dtw_open_ref as ref

SOT_LEN = 3
UNIT_LIMIT = 448 - SOT_LEN - 2


@pytest.fixture(scope="module")
def al():
    return importlib.import_module("whisper-char-alignment_amd.align_long")


# ---------------------------------------------------------------------------------------------- the numpy reference
@pytest.fixture(scope="module")
def planted_results():
    return [(n0, ref.dtw_open(m)) for m, n0 in ref.planted_cases()]


def test_reference_recovers_the_planted_end_row(planted_results):
    assert len(planted_results) == 5
    for n0, (ti, tj, jump, end_row, score, _un) in planted_results:
        assert end_row == n0
        assert ti[0] == 0 and tj[0] == 0 and ti[-1] == n0 and tj[-1] == len(set(tj)) - 1
        assert (jump[:n0 + 1] >= 0).all() and (np.diff(jump[:n0 + 1]) >= 0).all() and (jump[n0 + 1:] == -1).all()
        assert np.isfinite(score) and score < 0


def test_unnormalised_last_column_minimum_does_not_recover_it(planted_results):
    """Why the kernel carries path lengths: every visited cell adds a non-positive cost, so the longest path always has the smallest
    unnormalised cost and the last row wins whatever the matrix holds."""
    for (m, n0), (_n0, res) in zip(ref.planted_cases(), planted_results):
        assert res[5] == m.shape[0] - 1 != n0


def test_reference_closed_form_is_the_oracle_dtw():
    from oracle import timing_ref
    rng = np.random.default_rng(5)
    for N, M in [(1, 1), (1, 9), (7, 1), (13, 40), (40, 13)]:
        m = rng.random((N, M)).astype(np.float32)
        ti, tj, jump, end_row, _s, _u = ref.dtw_open(m, open_end=False)
        oi, oj = timing_ref.dtw_py(-m.astype(np.float64))
        assert end_row == N - 1 and np.array_equal(ti, oi) and np.array_equal(tj, oj)


def test_reference_ties_go_to_the_lower_row():
    assert ref.dtw_open(np.full((9, 14), 0.25, np.float32))[3] == 0   # every cell ties, every score ties


# ---------------------------------------------------------------------------------------------- planted truth + scripted aligner
class Truth:
    """n_words words of 2..7 units; unit u starts at global encoder frame T[u], the text ends (eot) at T[n_units]."""

    def __init__(self, seconds, n_words, first_frame=10, last_frame=None, seed=0, unit_range=(2, 8)):
        rng = np.random.default_rng(seed)
        self.n_frames = int(seconds * 100) + 3000
        lens = rng.integers(*unit_range, size=n_words)
        self.starts = [int(v) for v in np.pad(np.cumsum(lens), (1, 0))]
        n_units = self.starts[-1]
        last_frame = int(seconds * 50) - 10 if last_frame is None else last_frame
        cuts = np.sort(rng.choice(np.arange(first_frame + 1, last_frame), size=n_units, replace=False))
        self.T = [first_frame] + [int(c) for c in cuts]   # n_units + 1 strictly increasing frames
        self.words = ["w%d" % k for k in range(n_words)]

    def state(self, al):
        return al.AlignState(self.n_frames, self.starts, self.words, SOT_LEN)

    def align(self, st, request):
        seek, size, w0, w1, closed = request
        g0, max_frames = seek // 2, size // 2
        u0, u1 = st.unit_span(w0, w1)
        rel = np.array([self.T[u] - g0 for u in range(u0, u1 + 1)])   # the offered units, then the eot row (the next unit's start)
        assert rel[0] >= 0, "a window never starts after the first unit it is offered"
        if closed:
            return np.minimum(rel, max_frames - 1).astype(np.int32), len(rel) - 1, -1.0
        fits = np.flatnonzero(rel < max_frames)
        end_row = int(fits[-1]) if len(fits) else 0
        jump = np.where(np.arange(len(rel)) <= end_row, np.clip(rel, 0, max_frames - 1), -1).astype(np.int32)
        return jump, end_row, -1.0

    def expected(self, k):
        return self.T[self.starts[k]] * 0.02, self.T[self.starts[k + 1]] * 0.02


def run_one(al, truth, check=None):
    st = truth.state(al)
    requests = []

    def align_rows(live, reqs):
        assert live == [0]
        requests.extend(reqs)
        if check:
            check(st, reqs[0])
        return [truth.align(st, r) for r in reqs]

    return al.align_loop([st], align_rows)[0], requests, st


def assert_planted_times(truth, words):
    for k, w in enumerate(words):
        s, e = truth.expected(k)
        assert w["word"] == truth.words[k]
        assert abs(w["start"] - s) < 1e-9 and abs(w["end"] - e) < 1e-9, (k, w, s, e)
        assert round(w["start"] * 50) == truth.T[truth.starts[k]] and round(w["end"] * 50) == truth.T[truth.starts[k + 1]]


def test_loop_returns_every_word_once_with_the_planted_times(al):
    truth = Truth(100, 330, seed=1)   # about 1480 units in 100 s: both the 448-token limit and the window edge cut runs

    def check(st, req):
        _seek, size, w0, w1, _closed = req
        u0, u1 = st.unit_span(w0, w1)
        assert w1 > w0 and SOT_LEN + 1 + (u1 - u0) + 1 <= 448 and size <= 3000
        assert u0 == truth.starts[w0] and u1 == truth.starts[w1]   # whole words only
        if w1 < st.n_words:   # the longest run: one more word would not fit
            assert truth.starts[w1 + 1] - u0 > UNIT_LIMIT

    out, requests, st = run_one(al, truth, check)
    assert out["unaligned_words"] == 0 and len(out["words"]) == 330
    assert_planted_times(truth, out["words"])
    seeks = [r[0] for r in requests]
    assert all(b > a for a, b in zip(seeks, seeks[1:])) and st.seek == st.content_frames == 10000
    assert [r[4] for r in requests] == [False] * (len(requests) - 1) + [True]
    assert len(out["windows"]) == len(requests) >= 4 and sum(w["committed"] for w in out["windows"]) == 330
    token_bound = [r for r in requests if truth.starts[r[3]] - truth.starts[r[2]] > UNIT_LIMIT - 8]
    assert token_bound and len(token_bound) < len(requests)
    for w in out["windows"]:
        assert set(w) == {"seek", "size", "w0", "w1", "closed", "end_row", "score", "committed"}


def test_window_that_commits_nothing_advances_by_size_and_keeps_the_cursor(al):
    truth = Truth(100, 120, first_frame=2100, seed=2)   # 42 s of silence first
    out, requests, _st = run_one(al, truth)
    assert requests[0][:3] == (0, 3000, 0) and requests[1][:3] == (3000, 3000, 0)
    assert out["windows"][0]["committed"] == 0 and out["windows_without_words"] >= 1
    assert out["unaligned_words"] == 0
    assert_planted_times(truth, out["words"])


def test_text_longer_than_the_audio_leaves_unaligned_words(al):
    truth = Truth(100, 400, last_frame=7400, seed=3)   # the text runs to 148 s, the audio stops at 100 s
    truth.n_frames = 10000 + 3000
    out, requests, st = run_one(al, truth)
    assert st.seek == st.content_frames and out["unaligned_words"] > 0 and len(out["words"]) == 400
    aligned = [w for w in out["words"] if w["start"] is not None]
    assert len(aligned) == 400 - out["unaligned_words"] and all(w["start"] is None and w["end"] is None for w in out["words"][len(aligned):])
    assert_planted_times(truth, aligned)
    assert all(w["end"] <= 100.0 for w in aligned) and not requests[-1][4]


def test_text_that_ends_early_stops_the_loop(al):
    truth = Truth(100, 60, last_frame=1900, seed=4)   # the text ends at 38 s
    out, requests, st = run_one(al, truth)
    assert out["unaligned_words"] == 0 and st.cursor == st.n_words and st.seek < st.content_frames
    assert len(requests) == 2 and not any(r[4] for r in requests)
    assert_planted_times(truth, out["words"])


def test_over_long_word_is_a_value_error(al):
    with pytest.raises(ValueError, match="units"):
        al.AlignState(13000, [0, 3, 3 + UNIT_LIMIT + 1, 3 + UNIT_LIMIT + 4], ["a", "b", "c"], SOT_LEN)
    al.AlignState(13000, [0, 3, 3 + UNIT_LIMIT, 3 + UNIT_LIMIT + 4], ["a", "b", "c"], SOT_LEN)   # exactly the limit fits


def test_remainder_under_one_encoder_frame_ends_the_recording(al):
    st = al.AlignState(3000 + 3001, [0, 2, 4], ["a", "b"], SOT_LEN)
    assert st.request()[:2] == (0, 3000)
    st.receive(np.array([0, -1, -1, -1, -1], np.int32), 0, -1.0)
    assert st.seek == st.content_frames == 3001 and st.done and st.result()["unaligned_words"] == 2


def test_lock_step_driver_returns_what_the_single_loop_returns(al):
    truths = [Truth(100, 330, seed=1), Truth(40, 90, seed=6), Truth(100, 120, first_frame=2100, seed=2), Truth(100, 60, last_frame=1900, seed=4)]
    alone = [run_one(al, t)[0] for t in truths]
    states = [t.state(al) for t in truths]
    rounds = []

    def align_rows(live, reqs):
        rounds.append(len(live))
        return [truths[i].align(states[i], r) for i, r in zip(live, reqs)]

    together = al.align_loop(states, align_rows)
    assert together == alone
    assert rounds[0] == 4 and rounds[-1] < 4 and all(b <= a for a, b in zip(rounds, rounds[1:]))   # the batch shrinks


def test_transcript_units_follow_the_teacher_text_path(al, fake_vocab):
    tk = importlib.import_module("whisper-char-alignment_amd.tokenizer")
    rt = importlib.import_module("whisper-char-alignment_amd.retokenize")
    tok = tk.get_tokenizer(True, language="en", vocab_path=fake_vocab)
    text = "Hello, tiny world! It's 12 o'clock."
    units, starts, words = al.transcript_units(text, tok, "char")
    assert units == rt.encode(rt.remove_punctuation(text), tok, "char")
    assert [w.strip() for w in words] == rt.remove_punctuation(text).split() and starts[0] == 0 and starts[-1] == len(units)
    assert list(starts) == list(rt.char_word_starts(units + [tok.eot], tok))
    assert al.transcript_units(" ,. ", tok, "char") == ([], [0], [])
    with pytest.raises(ValueError, match="units"):
        al.AlignState(13000, *al.transcript_units("a" * 500 + " b", tok, "char")[1:], len(tok.sot_sequence))
