"""`-m gpu`: the open-end DTW kernel (csrc/dtw.hip, OPEN form) against its numpy restatement (tests/dtw_open_ref.py), BIT-EXACT: end row,
path, path length and jump frames with their -1 tail; the diagnostic score to rtol 1e-6. Shapes reach every rows-per-lane instantiation
(N <= 64, 128, ... 512) and the edges of the 16-column trace words; inputs are random matrices, the planted matrices, a constant matrix
(every DP cell and every score ties: end row 0) and a matrix whose two best end rows tie exactly (the lower row wins)."""
import ctypes as C
import importlib
from fractions import Fraction

import numpy as np
import pytest
import torch

import dtw_open_ref as ref

pytestmark = pytest.mark.gpu

_pi = C.POINTER(C.c_int32)
_pf = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def eng():
    e = importlib.import_module("whisper-char-alignment_amd.engine").default_engine(0)
    e._bind_stream()
    return e


def _check(code):
    importlib.import_module("whisper-char-alignment_amd._lib").check(code)


def _host_open(eng, m):
    """wca_dtw_open on a host matrix -> (text_idx, time_idx, end_row, score)."""
    m = np.ascontiguousarray(m, dtype=np.float32)
    N, M = m.shape
    ti, tj = np.zeros(N + M, np.int32), np.zeros(N + M, np.int32)
    n, end_row, score = C.c_int32(0), C.c_int32(-7), C.c_float(0)
    _check(eng._lib.wca_dtw_open(eng._h, m.ctypes.data_as(_pf), N, M, ti.ctypes.data_as(_pi), tj.ctypes.data_as(_pi), C.byref(n),
                                 C.byref(end_row), C.byref(score)))
    return ti[:n.value].astype(np.int64), tj[:n.value].astype(np.int64), end_row.value, np.float32(score.value)


def _batch_open(eng, mats, open_flags, n_rows=None, n_cols=None):
    """wca_dtw_batch_dev_open on [P][N][M] -> (jump [P][N], end_row [P], score [P])."""
    mats = np.ascontiguousarray(mats, dtype=np.float32)
    P, N, M = mats.shape
    md = torch.from_numpy(mats).cuda()
    jf, er, sc = np.full((P, N), -9, np.int32), np.full(P, -9, np.int32), np.zeros(P, np.float32)
    i32 = importlib.import_module("whisper-char-alignment_amd._lib").i32_array
    _check(eng._lib.wca_dtw_batch_dev_open(eng._h, C.c_void_p(md.data_ptr()), P, N, M, i32(n_rows) if n_rows is not None else None,
                                           i32(n_cols) if n_cols is not None else None, i32(open_flags), jf.ctypes.data_as(_pi),
                                           er.ctypes.data_as(_pi), sc.ctypes.data_as(_pf)))
    return jf, er, sc


def _assert_matches(eng, m, name):
    ti, tj, jump, end_row, score, _un = ref.dtw_open(m)
    gi, gj, g_end, g_score = _host_open(eng, m)
    assert g_end == end_row, (name, g_end, end_row)
    assert len(gi) == len(ti) and np.array_equal(gi, ti) and np.array_equal(gj, tj), name
    np.testing.assert_allclose(g_score, score, rtol=1e-6, err_msg=name)
    jf, er, sc = _batch_open(eng, m[None], [1])   # the batched entry agrees with the host-matrix one
    assert er[0] == end_row and np.array_equal(jf[0], jump), name
    assert (jf[0][end_row + 1:] == -1).all() and (jf[0][:end_row + 1] >= 0).all()
    np.testing.assert_allclose(sc[0], score, rtol=1e-6, err_msg=name)
    return end_row


SHAPES = [(1, 1), (1, 17), (2, 15), (2, 100), (63, 16), (63, 1500), (64, 17), (64, 100), (65, 1), (65, 1500), (128, 15), (128, 100),
          (129, 16), (129, 1500), (257, 17), (257, 100), (385, 15), (385, 1500), (449, 16), (449, 1500), (512, 1), (512, 100), (512, 1500)]


@pytest.mark.parametrize("N,M", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_open_end_random_bit_exact(eng, N, M):
    m = np.random.default_rng(N * 4099 + M).random((N, M), dtype=np.float32)
    _assert_matches(eng, m, "rand%dx%d" % (N, M))


def test_open_end_recovers_the_planted_end_rows(eng):
    for k, (m, n0) in enumerate(ref.planted_cases()):
        assert _assert_matches(eng, m, "planted%d" % k) == n0


def test_constant_matrix_every_tie_goes_to_row_zero(eng):
    for N, M in [(40, 90), (130, 17), (512, 100)]:
        assert _assert_matches(eng, np.full((N, M), 0.25, np.float32), "const%dx%d" % (N, M)) == 0


def test_two_best_end_rows_tie_exactly_and_the_lower_row_wins(eng):
    """Quarter-valued entries keep every cost exact; in this matrix rows 18 and 48 reach the same cost per path cell, -7/12, over paths
    of 51 and 81 cells: equal only as exact fractions (neither -7/12 nor the two quotients are representable)."""
    N, M = 70, 33
    m = (np.random.default_rng(160).integers(0, 4, size=(N, M)) / 4).astype(np.float32)
    Ct, Lt, _T = ref.fill(m)
    sc = [Fraction(float(Ct[i + 1, M])) / int(Lt[i + 1, M]) for i in range(N)]
    order = sorted(range(N), key=lambda i: (sc[i], i))
    assert order[:2] == [18, 48] and sc[18] == sc[48] == Fraction(-7, 12) and (Lt[19, M], Lt[49, M]) == (51, 81)
    assert _assert_matches(eng, m, "tie") == 18


def test_ragged_launch_mixing_open_and_closed_problems(eng):
    rng = np.random.default_rng(9)
    P, N, M = 8, 200, 300
    n_rows = [200, 1, 64, 65, 130, 77, 199, 128]
    n_cols = [300, 40, 1, 17, 300, 16, 33, 250]
    flags = [1, 0, 1, 0, 1, 1, 0, 0]
    mats = rng.random((P, N, M), dtype=np.float32)
    n0 = 40
    mats[4, :130, :300] = ref.planted(130, 300, n0, seed=3)
    jf, er, sc = _batch_open(eng, mats, flags, n_rows, n_cols)
    for p in range(P):
        n, mm = n_rows[p], n_cols[p]
        corner = np.ascontiguousarray(mats[p, :n, :mm])
        assert (jf[p, n:] == 0).all(), p   # rows beyond the problem's own are defined as 0
        if flags[p]:
            _ti, _tj, jump, end_row, score, _un = ref.dtw_open(corner)
            assert er[p] == end_row and np.array_equal(jf[p, :n], jump), p
            np.testing.assert_allclose(sc[p], score, rtol=1e-6)
        else:   # exactly today's closed result, through today's entry point
            want = np.full((1, n), -9, np.int32)
            md = torch.from_numpy(corner).cuda()
            _check(eng._lib.wca_dtw_batch_dev(eng._h, C.c_void_p(md.data_ptr()), 1, n, mm, want.ctypes.data_as(_pi)))
            assert er[p] == n - 1 and np.array_equal(jf[p, :n], want[0]), p
            assert np.array_equal(want[0], ref.dtw_open(corner, open_end=False)[2]), p
    assert er[4] == n0
    # all-closed flags through the open entry: every problem is the closed result
    jf0, er0, _sc0 = _batch_open(eng, mats, [0] * P, n_rows, n_cols)
    assert list(er0) == [n - 1 for n in n_rows]
    for p in range(P):
        if not flags[p]:
            assert np.array_equal(jf0[p], jf[p])


def test_timing_dtw_open_wrapper(eng):
    tm = importlib.import_module("whisper-char-alignment_amd.timing")
    m, n0 = ref.planted(64, 100, 38, seed=2), 38
    ti, tj, end_row, score = tm.dtw_open(torch.from_numpy(-m))   # takes the already negated matrix, like timing.dtw
    want = ref.dtw_open(m)
    assert end_row == n0 == want[3] and np.array_equal(ti, want[0]) and np.array_equal(tj, want[1])
    assert ti.dtype == np.int64 and abs(score - float(want[4])) <= 1e-6 * abs(float(want[4]))


def test_open_entry_points_refuse_bad_shapes(eng):
    m = np.zeros((4, 4), np.float32)
    md = torch.zeros(1, 4, 4).cuda()
    out = np.zeros(4, np.int32)
    i32 = importlib.import_module("whisper-char-alignment_amd._lib").i32_array
    n = C.c_int32(0)
    assert eng._lib.wca_dtw_open(eng._h, m.ctypes.data_as(_pf), 513, 4, out.ctypes.data_as(_pi), out.ctypes.data_as(_pi), C.byref(n), C.byref(n), None) < 0
    for rows, cols in (([5], None), ([0], None), (None, [5]), (None, [0])):
        rc = eng._lib.wca_dtw_batch_dev_open(eng._h, C.c_void_p(md.data_ptr()), 1, 4, 4, i32(rows) if rows else None, i32(cols) if cols else None,
                                             i32([1]), out.ctypes.data_as(_pi), out.ctypes.data_as(_pi), None)
        assert rc < 0, (rows, cols)
