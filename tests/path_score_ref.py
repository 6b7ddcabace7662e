"""Test helper: the per-row score of a DTW path (csrc/path_score.hip) restated in numpy float64, and the word aggregation above it.

For an f32 matrix X [N][M] (NOT negated) and a path (text_idx, time_idx): cells[i] = the number of path cells with text index i, sum[i] =
the float64 sum of X[i][j] over them, mean[i] = float32(sum[i] / cells[i]); rows the path does not visit are (0, 0.0). This file walks the
path cell by cell, so it knows nothing of jump frames or of how a row is entered; `from_jumps` restates the kernel's own route (row i holds
the frames jump[i] .. last[i]) with switches for the ways that route can go wrong, and the tests show that each of them is noticed."""
import numpy as np

BOUND_REL = 2.0 ** -23   # |mean - ref| <= 2^-23 * sum|x| / cells: at most 1500 f64 additions (1500 * 2^-53) and one rounding to f32 (2^-24)


def row_scores(matrix, text_idx, time_idx, n_rows=None):
    """-> (cells [n_rows] int32, sum [n_rows] f64, mean [n_rows] f32, abs_sum [n_rows] f64) of the path on `matrix`; n_rows defaults to the
    matrix's. abs_sum (the sum of |X|) is what the comparison's bound is made of."""
    m = np.ascontiguousarray(matrix, dtype=np.float32)
    n_rows = m.shape[0] if n_rows is None else int(n_rows)
    ti, tj = np.asarray(text_idx, dtype=np.int64), np.asarray(time_idx, dtype=np.int64)
    cells = np.zeros(n_rows, dtype=np.int32)
    total, abs_sum = np.zeros(n_rows, dtype=np.float64), np.zeros(n_rows, dtype=np.float64)
    if len(ti):
        v = m[ti, tj].astype(np.float64)
        np.add.at(cells, ti, 1)
        np.add.at(total, ti, v)
        np.add.at(abs_sum, ti, np.abs(v))
    mean = np.zeros(n_rows, dtype=np.float32)
    hit = cells > 0
    mean[hit] = (total[hit] / cells[hit]).astype(np.float32)
    return cells, total, mean, abs_sum


def bound(cells, abs_sum):
    """The largest |mean - ref| the arithmetic allows, per row (0 where the row holds no cell: those are exact)."""
    out = np.zeros(len(cells), dtype=np.float64)
    hit = np.asarray(cells) > 0
    out[hit] = BOUND_REL * abs_sum[hit] / np.asarray(cells)[hit]
    return out


def word_scores(mean, cells, word_boundaries):
    """The cell-weighted mean of the rows [wb[w], wb[w + 1]) of every word in float64, nan for a word without a cell."""
    mean, cells = np.asarray(mean, dtype=np.float64), np.asarray(cells, dtype=np.float64)
    out = []
    for a, b in zip(word_boundaries[:-1], word_boundaries[1:]):
        c = cells[a:b].sum()
        out.append(float((mean[a:b] * cells[a:b]).sum() / c) if c > 0 else float("nan"))
    return out


def from_jumps(matrix, text_idx, time_idx, mutation=None):
    """(cells, mean) the way the kernel forms them: row i holds the frames jump[i] .. last[i], last = M - 1 for the end row, else jump[i+1]
    where the path enters row i + 1 vertically and jump[i+1] - 1 where it enters diagonally. mutation: None (the definition), or one of
      "always_shared"  last = jump[i+1] whatever the entry,
      "never_shared"   last = jump[i+1] - 1 whatever the entry,
      "end_row_cut"    the end row stops at its jump frame,
      "neighbour_span" the sum is divided by the frame span of the NEXT row (the end row: of the previous one)."""
    m = np.ascontiguousarray(matrix, dtype=np.float32)
    N, M = m.shape
    ti, tj = np.asarray(text_idx, dtype=np.int64), np.asarray(time_idx, dtype=np.int64)
    end = int(ti[-1])
    jump = np.full(N, -1, dtype=np.int64)
    vertical = np.zeros(N, dtype=bool)   # row i is entered from (i - 1, same frame)
    for k in range(len(ti) - 1, -1, -1):
        jump[ti[k]] = tj[k]
    for k in range(1, len(ti)):
        if ti[k] != ti[k - 1]:
            vertical[ti[k]] = tj[k] == tj[k - 1]
    last = np.zeros(N, dtype=np.int64)
    for i in range(end + 1):
        if i == end:
            last[i] = jump[i] if mutation == "end_row_cut" else M - 1
        elif mutation == "always_shared":
            last[i] = jump[i + 1]
        elif mutation == "never_shared":
            last[i] = jump[i + 1] - 1
        else:
            last[i] = jump[i + 1] if vertical[i + 1] else jump[i + 1] - 1
    span = np.maximum(last - jump + 1, 0)
    cells, mean = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.float32)
    for i in range(end + 1):
        if span[i] <= 0:
            continue
        cells[i] = span[i]
        div = span[i]
        if mutation == "neighbour_span":
            div = max(span[i + 1] if i < end else span[i - 1] if i > 0 else span[i], 1)
        mean[i] = np.float32(m[i, jump[i]:last[i] + 1].astype(np.float64).sum() / div)
    return cells, mean


def closed_path(matrix):
    """The closed DTW path of `-matrix` through the oracle: (text_idx, time_idx)."""
    import torch
    from oracle import timing_ref
    ti, tj = timing_ref.dtw(-torch.from_numpy(np.ascontiguousarray(matrix, dtype=np.float32)))
    return np.asarray(ti, dtype=np.int64), np.asarray(tj, dtype=np.int64)


def open_path(matrix):
    """The open-end DTW path through tests/dtw_open_ref.py: (text_idx, time_idx, end_row)."""
    import dtw_open_ref
    ti, tj, _jump, end_row, _score, _ = dtw_open_ref.dtw_open(matrix, True)
    return ti, tj, int(end_row)
