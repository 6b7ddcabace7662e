"""CPU tests of the path-score reference (tests/path_score_ref.py), of the host aggregation above it (timing.word_alignment_scores, the
`score` of align_long.AlignState) and of the command-line flags. The reference walks a path cell by cell; the kernel's route over jump
frames is restated beside it with its possible mistakes as switches, and each mistake is shown to change the result on these inputs."""
import importlib

import numpy as np
import pytest
import torch

import path_score_ref as ps


def _m(name):
    return importlib.import_module("whisper-char-alignment_amd." + name)


def _path(cells):
    return np.array([c[0] for c in cells]), np.array([c[1] for c in cells])


def _ridge(N, M, cells):
    m = np.zeros((N, M), np.float32)
    for i, j in cells:
        m[i, j] = 1.0
    return m


# hand-made paths: (name, N, M, cells, expected cells per row)
DIAGONAL_ENTRY = ("diagonal entry", 3, 5, [(0, 0), (0, 1), (1, 2), (1, 3), (2, 4)], [2, 2, 1])
VERTICAL_ENTRY = ("vertical entry", 3, 5, [(0, 0), (0, 1), (1, 1), (1, 2), (1, 3), (2, 4)], [2, 3, 1])
TALL = ("N > M", 5, 2, [(0, 0), (1, 0), (2, 0), (3, 1), (4, 1)], [1, 1, 1, 1, 1])
ONE_ROW = ("N = 1", 1, 7, [(0, j) for j in range(7)], [7])
LONG_END = ("long end row", 2, 6, [(0, 0), (1, 1), (1, 2), (1, 3), (1, 4), (1, 5)], [1, 5])
HAND = [DIAGONAL_ENTRY, VERTICAL_ENTRY, TALL, ONE_ROW, LONG_END]


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_a_ridge_of_ones_scores_exactly_one(case):
    """On a 0/1 matrix whose ones are the path, every row's mean is exactly 1 and its cell count is the hand count; the jump-frame route
    gives the same. The oracle DTW finds that path once leaving the ridge costs something (on 0 / 1 itself every detour over zeros
    ties, and ties go left)."""
    _name, N, M, cells, want = case
    m = _ridge(N, M, cells)
    ti, tj = ps.closed_path(2 * m - 1)
    assert list(zip(ti.tolist(), tj.tolist())) == cells
    got_cells, total, mean, abs_sum = ps.row_scores(m, ti, tj)
    assert got_cells.tolist() == want and mean.tolist() == [1.0] * N and total.tolist() == [float(c) for c in want]
    assert abs_sum.tolist() == total.tolist() and mean.dtype == np.float32 and got_cells.dtype == np.int32
    jc, jm = ps.from_jumps(m, ti, tj)
    assert jc.tolist() == want and jm.tolist() == [1.0] * N


def test_known_means_on_a_graded_matrix():
    """m[i][j] = 10 i + j: the means are the hand sums; the shared column of a vertical entry counts in both rows."""
    m = (10.0 * np.arange(3)[:, None] + np.arange(5)[None, :]).astype(np.float32)
    cells, _t, mean, _a = ps.row_scores(m, *_path(VERTICAL_ENTRY[3]))
    assert cells.tolist() == [2, 3, 1] and mean.tolist() == [0.5, 12.0, 24.0]
    cells, _t, mean, _a = ps.row_scores(m, *_path(DIAGONAL_ENTRY[3]))
    assert cells.tolist() == [2, 2, 1] and mean.tolist() == [0.5, 12.5, 24.0]


def test_rows_off_the_path_are_zero_and_the_mean_is_rounded_once():
    m = np.full((4, 3), 0.1, np.float32)
    cells, total, mean, _a = ps.row_scores(m, *_path([(0, 0), (1, 1), (1, 2)]), n_rows=6)   # an open end at row 1, two rows of padding
    assert cells.tolist() == [1, 2, 0, 0, 0, 0] and mean[2:].tolist() == [0.0] * 4 and total[2:].tolist() == [0.0] * 4
    assert mean[1] == np.float32((np.float64(np.float32(0.1)) * 2) / 2)
    assert ps.row_scores(m, [], [])[0].tolist() == [0, 0, 0, 0]
    b = ps.bound(cells, ps.row_scores(m, *_path([(0, 0), (1, 1), (1, 2)]), n_rows=6)[3])
    assert b[2:].tolist() == [0.0] * 4 and b[0] == 2.0 ** -23 * np.float64(np.float32(0.1))


def _random_cases():
    rng = np.random.default_rng(5)
    out = []
    # values in [0, 1] (no cell costs anything: the path never moves diagonally, every entry is vertical) and signed ones, where it does
    for lo, (N, M) in ((0, (7, 30)), (0, (30, 7)), (-1, (12, 12)), (-1, (20, 31)), (-1, (1, 9)), (0, (9, 1))):
        m = rng.uniform(lo, 1, (N, M)).astype(np.float32)
        out.append((m,) + ps.closed_path(m))
    return out


def test_the_jump_frame_route_is_the_definition():
    """Cell by cell and by jump frames: the same cells and the same bits, on the hand paths and on oracle paths of random matrices
    (tall ones are full of vertical entries)."""
    cases = [(np.random.default_rng(k).uniform(-1, 1, (N, M)).astype(np.float32),) + _path(cells) for k, (_n, N, M, cells, _w) in enumerate(HAND)]
    n_vertical = n_diagonal = 0
    for m, ti, tj in cases + _random_cases():
        cells, _t, mean, _a = ps.row_scores(m, ti, tj)
        jc, jm = ps.from_jumps(m, ti, tj)
        assert jc.tolist() == cells.tolist() and jm.tobytes() == mean.tobytes()
        assert cells.sum() == len(ti)
        n_vertical += int(np.sum((np.diff(ti) == 1) & (np.diff(tj) == 0)))
        n_diagonal += int(np.sum((np.diff(ti) == 1) & (np.diff(tj) == 1)))
    assert n_vertical > 20 and n_diagonal > 5


@pytest.mark.parametrize("mutation,case", [("always_shared", DIAGONAL_ENTRY), ("never_shared", VERTICAL_ENTRY), ("never_shared", TALL),
                                           ("end_row_cut", LONG_END), ("end_row_cut", ONE_ROW), ("neighbour_span", VERTICAL_ENTRY),
                                           ("neighbour_span", LONG_END)])
def test_each_mistake_of_the_route_is_noticed(mutation, case):
    """The four ways the jump-frame route can go wrong each change cells or means on the hand path that exercises them, by far more
    than the comparison's bound."""
    _name, N, M, cells, _want = case
    m = (1.0 + np.arange(N)[:, None] + 0.25 * np.arange(M)[None, :]).astype(np.float32)
    ti, tj = _path(cells)
    ref_cells, _t, ref_mean, abs_sum = ps.row_scores(m, ti, tj)
    bad_cells, bad_mean = ps.from_jumps(m, ti, tj, mutation)
    worst = np.max(np.abs(bad_mean.astype(np.float64) - ref_mean) - ps.bound(ref_cells, abs_sum))
    assert bad_cells.tolist() != ref_cells.tolist() or worst > 1e-3, (mutation, bad_cells, bad_mean)
    if mutation == "neighbour_span":
        assert bad_cells.tolist() == ref_cells.tolist() and worst > 1e-3   # only the means can show this one


def test_every_mistake_shows_on_random_matrices_too():
    for mutation in ("always_shared", "never_shared", "end_row_cut", "neighbour_span"):
        seen = False
        for m, ti, tj in _random_cases():
            cells, _t, mean, _a = ps.row_scores(m, ti, tj)
            bc, bm = ps.from_jumps(m, ti, tj, mutation)
            seen = seen or bc.tolist() != cells.tolist() or bm.tobytes() != mean.tobytes()
        assert seen, mutation


def test_open_paths_end_early():
    """An open-end path stops at its end row: the rows past it hold no cell."""
    import dtw_open_ref
    m = dtw_open_ref.planted(20, 40, 11, seed=3)
    ti, tj, end = ps.open_path(m)
    assert 0 < end < 19
    cells, _t, mean, _a = ps.row_scores(m, ti, tj)
    assert (cells[:end + 1] > 0).all() and not cells[end + 1:].any() and not mean[end + 1:].any()
    jc, jm = ps.from_jumps(m, ti, tj)
    assert jc.tolist() == cells.tolist() and jm.tobytes() == mean.tobytes()


# ------------------------------------------------------------------------------------------------ the host aggregation
@pytest.fixture(scope="module")
def tok():
    return _m("tokenizer").get_tokenizer(True, language="English")


@pytest.mark.parametrize("text", ["hello tiny world", "i am here", "x y", "don't stop me now", "word"])
def test_word_alignment_scores_use_word_probabilities_slices(tok, text):
    """With one cell per row and exp(log-prob) as the row means, the cell-weighted mean over a word's rows is word_probabilities' list
    slice mean: the two functions cut the same rows. Then with real cell counts against the reference aggregation."""
    tm, rt = _m("timing"), _m("retokenize")
    tt = rt.encode(text, tok, "char")
    rng = np.random.default_rng(len(text))
    lp = np.log(rng.uniform(0.01, 1.0, len(tt))).astype(np.float32)
    probs = tm.word_probabilities(lp, tt, tok, "char")
    row_mean = np.concatenate([np.exp(lp.astype(np.float64)), [0.123]])   # the eot row belongs to no word
    got = tm.word_alignment_scores(row_mean, np.ones(len(tt) + 1, np.int32), tt, tok, "char")
    assert len(got) == len(probs) == len(text.split())
    np.testing.assert_allclose(got, probs, rtol=1e-12, atol=0)
    cells = rng.integers(0, 5, len(tt) + 1).astype(np.int32)
    mean = rng.uniform(0, 1, len(tt) + 1).astype(np.float32)
    wb = tm._word_boundaries(tt, tok, "char")
    got = tm.word_alignment_scores(torch.from_numpy(np.concatenate([mean, np.zeros(5, np.float32)])), np.concatenate([cells, np.zeros(5, np.int32)]),
                                   tt, tok, "char")
    want = ps.word_scores(mean, cells, wb)
    assert len(got) == len(want) and all((g == w) or (g != g and w != w) for g, w in zip(got, want))


def test_word_alignment_scores_edges(tok):
    tm, rt = _m("timing"), _m("retokenize")
    assert tm.word_alignment_scores(np.zeros(1, np.float32), np.zeros(1, np.int32), [], tok, "char") == []
    assert tm.word_probabilities(np.zeros(0, np.float32), [], tok, "char") == []
    tt = rt.encode("ab cd", tok, "char")
    cells = np.array([1, 2, 0, 0, 0, 0], np.int32)   # an open end after the first word
    got = tm.word_alignment_scores(np.array([0.5, 1.0, 0, 0, 0, 0], np.float32), cells, tt, tok, "char")
    assert got[0] == pytest.approx(2.5 / 3, abs=1e-12) and got[1] != got[1] and len(got) == 2
    dropin = open(_m("timing").__file__.replace("timing.py", "dropin/timing.py")).read()
    assert "path_scores = _t.path_scores" in dropin and "word_alignment_scores = _t.word_alignment_scores" in dropin


def test_align_state_scores_follow_the_committed_words():
    """AlignState(word_scores=True): a closed window's words get the cell-weighted mean of their rows, the window their mean; without
    the option neither key exists and receive() takes what it took."""
    al = _m("align_long")
    starts, words = [0, 2, 5, 6], ["ab", "cde", "f"]
    jump = np.array([0, 3, 5, 9, 12, 20, 30])
    mean = np.array([0.5, 1.0, 0.25, 0.5, 0.75, 0.125, 0.9], np.float32)
    cells = np.array([3, 2, 4, 3, 8, 10, 1], np.int32)
    st = al.AlignState(3000 + 100, starts, words, 3, word_scores=True)
    st.receive(jump, 6, 0.0, None, (mean, cells))
    res = st.result()
    assert [w["score"] for w in res["words"]] == ps.word_scores(mean, cells, starts)
    assert res["windows"][0]["mean_word_score"] == pytest.approx(np.mean(ps.word_scores(mean, cells, starts)), abs=1e-15)
    plain = al.AlignState(3000 + 100, starts, words, 3)
    plain.receive(jump, 6, 0.0, None)
    r0 = plain.result()
    assert set(r0["words"][0]) == {"word", "start", "end"} and "mean_word_score" not in r0["windows"][0]
    assert [(w["start"], w["end"]) for w in r0["words"]] == [(w["start"], w["end"]) for w in res["words"]]
    with pytest.raises(ValueError):
        al.AlignState(3000 + 100, starts, words, 3, word_scores=True).receive(jump, 6, 0.0, None)
    # an open window that commits nothing, then the audio ends: unaligned words carry score None
    st = al.AlignState(3000 + 5000, starts, words, 3, word_scores=True)
    assert not st.request()[4]
    st.receive(np.zeros(7, np.int64), 0, 0.0, None, (np.zeros(7, np.float32), np.zeros(7, np.int32)))
    st.seek = st.content_frames
    res = st.result()
    assert [w["score"] for w in res["words"]] == [None] * 3 and res["windows"][0]["mean_word_score"] is None


# ------------------------------------------------------------------------------------------------ command line
def test_flags_parse_and_default_to_off():
    infer, al, tr = _m("infer_ali"), _m("align_long"), _m("transcribe")
    base = ["--output_dir", "x"]
    assert infer.parse_args(base).word_alignment_score is False and infer.parse_args(base + ["--word_alignment_score"]).word_alignment_score is True
    ab = ["--audio", "a.wav", "--text", "a.txt", "--vocab", "v", "--output_dir", "x"]
    assert getattr(al.parse_args(ab), "word_scores", False) is False and al.parse_args(ab + ["--word_scores"]).word_scores is True
    tb = ["--audio", "a.wav", "--output_dir", "x"]
    assert getattr(tr.parse_args(tb), "word_alignment_score", False) is False
    assert tr.parse_args(tb + ["--word_timestamps", "--word_alignment_score"]).word_alignment_score is True
    with pytest.raises(ValueError, match="word_timestamps"):
        tr.transcribe_batch(object(), [], language="en", word_alignment_score=True)


def test_python_signatures_default_to_off(wca):
    import inspect
    eng = wca.WhisperAMD
    assert inspect.signature(eng.align_batch).parameters["path_scores"].default is False
    assert inspect.signature(eng.fetch).parameters["with_path_scores"].default is False
    assert list(inspect.signature(eng.dtw_path_scores).parameters) == ["self", "matrix_dev", "n_rows", "n_cols", "open_end"]
    assert [f[0] for f in wca._lib.AlignDesc._fields_][-1] == "path_scores"
    for name in ("wca_dtw_path_scores", "wca_align_batch_path_scores", "wca_test_align_postproc_scores"):
        assert name in wca._lib.SIGNATURES
