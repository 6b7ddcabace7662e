"""`-m gpu`: the windowed DTW kernel (csrc/dtw.hip, WIN form) against its numpy restatement (tests/dtw_windows_ref.py), BIT-EXACT: path,
path length and jump frames. Shapes are test_dtw_open_gpu.SHAPES (every rows-per-lane instantiation, the edges of the 16-column trace
words); window kinds: full (= wca_dtw exactly), a diagonal band, a staircase as cues produce it, lo == hi chains with one path known in
closed form, windows that idle whole lanes, windows with edges at j % 16 in {0, 15}, and quarter-valued matrices with exact zeros planted
at the windows' left edges (the exception to the tie rule). Every invalid condition is refused with WCA_ERR_INVALID before a launch."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import dtw_open_ref as open_ref
import dtw_windows_ref as ref
from test_dtw_open_gpu import SHAPES

pytestmark = pytest.mark.gpu

_pi = C.POINTER(C.c_int32)
_pf = C.POINTER(C.c_float)
WCA_ERR_INVALID = -1


def _m(n):
    return importlib.import_module("whisper-char-alignment_amd." + n)


@pytest.fixture(scope="module")
def eng():
    e = _m("engine").default_engine(0)
    e._bind_stream()
    return e


def _host(eng, m, lo, hi):
    """wca_dtw_windows on a host matrix -> (rc, text_idx, time_idx)."""
    m = np.ascontiguousarray(m, dtype=np.float32)
    lo, hi = np.ascontiguousarray(lo, np.int32), np.ascontiguousarray(hi, np.int32)
    N, M = m.shape
    ti, tj = np.full(N + M, -9, np.int32), np.full(N + M, -9, np.int32)
    n = C.c_int32(-9)
    rc = eng._lib.wca_dtw_windows(eng._h, m.ctypes.data_as(_pf), N, M, lo.ctypes.data_as(_pi), hi.ctypes.data_as(_pi), ti.ctypes.data_as(_pi),
                                  tj.ctypes.data_as(_pi), C.byref(n))
    return rc, ti[:max(n.value, 0)].astype(np.int64), tj[:max(n.value, 0)].astype(np.int64)


def _batch(eng, mats, lo, hi, n_rows=None, n_cols=None):
    """wca_dtw_batch_dev_windows on [P][N][M] -> (rc, jump [P][N]); the jump frames start as -9."""
    mats = np.ascontiguousarray(mats, dtype=np.float32)
    P, N, M = mats.shape
    md = torch.from_numpy(mats).cuda()
    lo, hi = np.ascontiguousarray(lo, np.int32), np.ascontiguousarray(hi, np.int32)
    jf = np.full((P, N), -9, np.int32)
    i32 = _m("_lib").i32_array
    rc = eng._lib.wca_dtw_batch_dev_windows(eng._h, C.c_void_p(md.data_ptr()), P, N, M, i32(n_rows) if n_rows is not None else None,
                                            i32(n_cols) if n_cols is not None else None, lo.ctypes.data_as(_pi), hi.ctypes.data_as(_pi),
                                            jf.ctypes.data_as(_pi))
    return rc, jf


def _cases(N, M):
    """(name, matrix, lo, hi) for one shape: every window kind the shape admits."""
    rng = np.random.default_rng(N * 4099 + M)
    real = rng.random((N, M), dtype=np.float32)
    quarter = (rng.integers(0, 4, size=(N, M)) / 4).astype(np.float32)
    stairs = ref.staircase(N, M, 6, 3, seed=N + M)
    out = [("full", real, *ref.full(N, M)), ("band", real, *ref.band(N, M, 4)), ("staircase", real, *stairs),
           ("idle", real, *ref.idle_lanes(N, M)), ("edges", real, *ref.word_edges(N, M, seed=N)),
           ("zeros-staircase", ref.plant_zeros_at_left_edges(quarter, stairs[0]), *stairs),
           ("zeros-band", ref.plant_zeros_at_left_edges(quarter, ref.band(N, M, 1)[0]), *ref.band(N, M, 1))]
    if N >= M:
        out.append(("chain", quarter, *ref.chain(N, M, seed=M)))
    return out


@pytest.mark.parametrize("N,M", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_windowed_dtw_bit_exact(eng, N, M):
    cases = _cases(N, M)
    want = [ref.dtw_windows(m, lo, hi) for _n, m, lo, hi in cases]
    for (name, m, lo, hi), (ti, tj, _jump, _c) in zip(cases, want):
        assert ref.invalid_reason(lo, hi, N, M) is None, name
        rc, gi, gj = _host(eng, m, lo, hi)
        assert rc == 0 and len(gi) == len(ti) and np.array_equal(gi, ti) and np.array_equal(gj, tj), name
        if name == "chain":   # the one path, in closed form
            assert np.array_equal(gi, np.arange(N)) and np.array_equal(gj, lo), name
        if name == "full":   # exactly wca_dtw, and the closed restatement
            fi, fj = _m("timing")._dtw_host(eng, m)
            oi, oj = open_ref.dtw_open(m, open_end=False)[:2]
            assert np.array_equal(gi, fi) and np.array_equal(gj, fj) and np.array_equal(gi, oi) and np.array_equal(gj, oj)
    # all kinds as one launch, then in reverse order: the jump frames, whatever a problem's position
    mats, los, his = (np.stack([c[k] for c in cases]) for k in (1, 2, 3))
    rc, jf = _batch(eng, mats, los, his)
    assert rc == 0
    for p, (case, w) in enumerate(zip(cases, want)):
        assert np.array_equal(jf[p], w[2]), case[0]
    rc, jr = _batch(eng, mats[::-1], los[::-1], his[::-1])
    assert rc == 0 and np.array_equal(jr[::-1], jf)


def test_exception_case_and_planted_zeros(eng):
    m, lo, hi = ref.exception_case()
    rc, gi, gj = _host(eng, m, lo, hi)
    assert rc == 0 and list(zip(gi, gj)) == [(0, 0), (0, 1), (1, 1)]
    # a larger problem in which the rule without the exception demonstrably fails
    rng = np.random.default_rng(11)
    hit = 0
    for k in range(12):
        N, M = int(rng.integers(20, 140)), int(rng.integers(20, 90))
        lo, hi = ref.random_valid(N, M, rng)
        mq = ref.plant_zeros_at_left_edges((rng.integers(0, 4, size=(N, M)) / 4).astype(np.float32), lo)
        try:
            hit += not np.isfinite(ref.dtw_windows(mq, lo, hi, exception=False)[3])
        except AssertionError:
            hit += 1
        ti, tj, _j, _c = ref.dtw_windows(mq, lo, hi)
        rc, gi, gj = _host(eng, mq, lo, hi)
        assert rc == 0 and np.array_equal(gi, ti) and np.array_equal(gj, tj), k
    assert hit > 0


def test_ragged_launch_mixing_windowed_and_full_problems(eng):
    rng = np.random.default_rng(9)
    P, N, M = 8, 200, 300
    n_rows = [200, 1, 64, 65, 130, 77, 199, 128]
    n_cols = [300, 40, 1, 17, 300, 16, 33, 250]
    kinds = ["band", "full", "full", "staircase", "full", "edges", "idle", "band"]
    mats = rng.random((P, N, M), dtype=np.float32)
    lo, hi = np.full((P, N), 7, np.int32), np.full((P, N), -3, np.int32)   # (entries past a problem's rows are not read)
    for p, kind in enumerate(kinds):
        n, mm = n_rows[p], n_cols[p]
        w = {"band": lambda: ref.band(n, mm, 5), "full": lambda: ref.full(n, mm), "staircase": lambda: ref.staircase(n, mm, 4, 2, seed=p),
             "edges": lambda: ref.word_edges(n, mm, seed=p), "idle": lambda: ref.idle_lanes(n, mm)}[kind]()
        lo[p, :n], hi[p, :n] = w
    rc, jf = _batch(eng, mats, lo, hi, n_rows, n_cols)
    assert rc == 0
    for p in range(P):
        n, mm = n_rows[p], n_cols[p]
        corner = np.ascontiguousarray(mats[p, :n, :mm])
        assert np.array_equal(jf[p, :n], ref.dtw_windows(corner, lo[p, :n], hi[p, :n])[2]), p
        assert (jf[p, n:] == 0).all(), p
        if kinds[p] == "full":   # exactly the closed kernel's result
            want = np.full((1, n), -9, np.int32)
            md = torch.from_numpy(corner).cuda()
            assert eng._lib.wca_dtw_batch_dev(eng._h, C.c_void_p(md.data_ptr()), 1, n, mm, want.ctypes.data_as(_pi)) == 0
            assert np.array_equal(jf[p, :n], want[0]), p


@pytest.mark.parametrize("kind", ref.INVALID_KINDS)
def test_invalid_windows_are_refused_before_any_launch(eng, kind):
    for N, M in [(3, 3), (70, 20)]:
        m = np.random.default_rng(5).random((N, M), dtype=np.float32)
        lo, hi = ref.make_invalid(kind, N, M)
        assert ref.invalid_reason(lo, hi, N, M) is not None
        n = C.c_int32(-9)
        ti = np.full(N + M, -9, np.int32)
        rc = eng._lib.wca_dtw_windows(eng._h, m.ctypes.data_as(_pf), N, M, lo.ctypes.data_as(_pi), hi.ctypes.data_as(_pi), ti.ctypes.data_as(_pi),
                                      ti.ctypes.data_as(_pi), C.byref(n))
        assert rc == WCA_ERR_INVALID and n.value == -9 and (ti == -9).all(), (kind, rc)
        # as the second problem of a batch whose first is fine: the whole call is refused and nothing is written
        los, his = np.stack([ref.full(N, M)[0], lo]), np.stack([ref.full(N, M)[1], hi])
        rc, jf = _batch(eng, np.stack([m, m]), los, his)
        assert rc == WCA_ERR_INVALID and (jf == -9).all(), (kind, rc)
    # the break only counts inside a problem's own rows
    lo, hi = ref.make_invalid(kind, 70, 20)
    lo2, hi2 = np.concatenate([ref.full(5, 20)[0], lo]), np.concatenate([ref.full(5, 20)[1], hi])
    rc, jf = _batch(eng, np.random.default_rng(6).random((1, 75, 20), dtype=np.float32), lo2[None], hi2[None], n_rows=[5])
    assert rc == 0 and (jf[0, 5:] == 0).all()


def test_null_windows_and_bad_shapes_are_refused(eng):
    m = np.zeros((4, 4), np.float32)
    lo, hi = ref.full(4, 4)
    out = np.zeros(8, np.int32)
    n = C.c_int32(0)
    args = (out.ctypes.data_as(_pi), out.ctypes.data_as(_pi), C.byref(n))
    assert eng._lib.wca_dtw_windows(eng._h, m.ctypes.data_as(_pf), 4, 4, None, hi.ctypes.data_as(_pi), *args) == WCA_ERR_INVALID
    assert eng._lib.wca_dtw_windows(eng._h, m.ctypes.data_as(_pf), 513, 4, lo.ctypes.data_as(_pi), hi.ctypes.data_as(_pi), *args) == WCA_ERR_INVALID
    for rows, cols in (([5], None), ([0], None), (None, [5]), (None, [0])):
        rc, _jf = _batch(eng, m[None], lo[None], hi[None], rows, cols)
        assert rc == WCA_ERR_INVALID, (rows, cols)


def test_python_wrappers(eng):
    tm = _m("timing")
    N, M = 64, 100
    m = np.random.default_rng(3).random((N, M), dtype=np.float32)
    lo, hi = ref.band(N, M, 6)
    ti, tj, jump, _c = ref.dtw_windows(m, lo, hi)
    gi, gj = tm.dtw_windows(torch.from_numpy(-m), lo, hi)   # takes the already negated matrix, like timing.dtw
    assert gi.dtype == np.int64 and np.array_equal(gi, ti) and np.array_equal(gj, tj)
    assert np.array_equal(eng.dtw_windows(torch.from_numpy(m)[None], lo[None], hi[None])[0], jump)
    with pytest.raises(_m("_lib").WcaError):
        tm.dtw_windows(torch.from_numpy(-m), lo + 1, hi)
