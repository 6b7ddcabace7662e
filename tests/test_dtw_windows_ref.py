"""CPU tests of the windowed DTW's numpy restatement (tests/dtw_windows_ref.py): full windows are the closed DTW bit for bit, valid
windows always hold the path, the one exception to the tie rule is reached by a planted case that fails without it, and the validity
check rejects each broken condition."""
import numpy as np
import pytest

import dtw_open_ref as open_ref
import dtw_windows_ref as ref


def _matrices(N, M, rng):
    """A quarter-valued matrix (exact costs, many ties, exact zeros) and a real-valued one."""
    return (rng.integers(0, 4, size=(N, M)) / 4).astype(np.float32), rng.random((N, M), dtype=np.float32)


def test_full_windows_are_the_closed_dtw_bit_for_bit():
    rng = np.random.default_rng(1)
    for N, M in [(1, 1), (1, 9), (7, 1), (13, 40), (40, 13), (65, 33), (30, 100)]:
        for m in _matrices(N, M, rng):
            C, T = ref.fill(m, *ref.full(N, M))
            Co, _Lo, To = open_ref.fill(m)
            assert np.array_equal(C, Co) and np.array_equal(T[1:, 1:], To[1:, 1:]), (N, M)
            ti, tj, jump, _c = ref.dtw_windows(m, *ref.full(N, M))
            oi, oj, ojump = open_ref.dtw_open(m, open_end=False)[:3]
            assert np.array_equal(ti, oi) and np.array_equal(tj, oj) and np.array_equal(jump, ojump), (N, M)


def test_random_valid_windows_hold_the_path():
    rng = np.random.default_rng(2)
    for k in range(120):
        N, M = int(rng.integers(1, 40)), int(rng.integers(1, 60))
        lo, hi = ref.random_valid(N, M, rng)
        assert ref.invalid_reason(lo, hi, N, M) is None
        for m in _matrices(N, M, rng):
            m = ref.plant_zeros_at_left_edges(m, lo) if k % 2 else m
            ti, tj, jump, cost = ref.dtw_windows(m, lo, hi)
            assert np.isfinite(cost)
            assert (ti[0], tj[0]) == (0, 0) and (ti[-1], tj[-1]) == (N - 1, M - 1)
            assert (lo[ti] <= tj).all() and (tj <= hi[ti]).all()
            assert (np.diff(ti) >= 0).all() and (np.diff(tj) >= 0).all() and ((np.diff(ti) + np.diff(tj)) >= 1).all()
            assert (lo <= jump).all() and (jump <= hi).all()


def test_generators_give_valid_windows():
    for N, M in [(1, 1), (2, 15), (63, 16), (65, 1500), (129, 16), (512, 100)]:
        gens = [ref.full(N, M), ref.band(N, M, 3), ref.staircase(N, M, 5, 4), ref.idle_lanes(N, M), ref.word_edges(N, M)]
        if N >= M:
            gens.append(ref.chain(N, M))
        for lo, hi in gens:
            assert ref.invalid_reason(lo, hi, N, M) is None, (N, M)


def test_chain_windows_leave_one_path():
    rng = np.random.default_rng(3)
    for N, M in [(1, 1), (9, 9), (40, 13), (64, 17)]:
        lo, hi = ref.chain(N, M, seed=N)
        for m in _matrices(N, M, rng):
            ti, tj, jump, _c = ref.dtw_windows(m, lo, hi)
            assert np.array_equal(ti, np.arange(N)) and np.array_equal(tj, lo) and np.array_equal(jump, lo)


def test_planted_case_reaches_the_exception_and_fails_without_it():
    m, lo, hi = ref.exception_case()
    assert ref.invalid_reason(lo, hi, 2, 2) is None
    C0, _T0 = ref.fill(m, lo, hi, exception=False)
    assert np.isinf(C0[2, 2])   # upstream's rule alone: tie -> left, and left is not allowed: the end cell is infinite
    with pytest.raises(AssertionError):
        ref.dtw_windows(m, lo, hi, exception=False)
    C1, T1 = ref.fill(m, lo, hi)
    assert C1[2, 2] == np.float32(-0.75) and T1[2, 2] == 1   # with it: up
    ti, tj, jump, cost = ref.dtw_windows(m, lo, hi)
    assert list(zip(ti, tj)) == [(0, 0), (0, 1), (1, 1)] and list(jump) == [0, 1] and cost == np.float32(-0.75)


def test_exception_is_needed_on_random_quarter_valued_matrices():
    """Among random valid windows with zeros planted at the window edges, some fail without the exception and none with it."""
    rng = np.random.default_rng(4)
    failed = 0
    for _k in range(80):
        N, M = int(rng.integers(2, 30)), int(rng.integers(2, 40))
        lo, hi = ref.random_valid(N, M, rng)
        m = ref.plant_zeros_at_left_edges(_matrices(N, M, rng)[0], lo)
        assert np.isfinite(ref.fill(m, lo, hi)[0][N, M])
        try:
            failed += not np.isfinite(ref.dtw_windows(m, lo, hi, exception=False)[3])
        except AssertionError:
            failed += 1
    assert failed > 0


@pytest.mark.parametrize("kind", ref.INVALID_KINDS)
def test_each_invalid_condition_is_rejected(kind):
    for N, M in [(3, 3), (5, 9), (70, 20)]:
        lo, hi = ref.make_invalid(kind, N, M)
        assert ref.invalid_reason(lo, hi, N, M) is not None, (kind, N, M)
    assert ref.invalid_reason(*ref.full(5, 9), 5, 9) is None
