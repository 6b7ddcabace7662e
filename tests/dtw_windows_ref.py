"""Test helper: a numpy restatement of the windowed DTW (csrc/dtw.hip, WIN form), its validity check and window generators.

The recurrence is dtw_open_ref.fill's -- anti-diagonal fill, the tie rule of dtw_cpu (diagonal only if strictly smallest, else up only if
strictly smallest, else left), C[i][j] = float32(float64(-m[i][j]) + float64(c)) -- with two additions: a cell (i, j) outside its row's
window lo[i] <= j <= hi[i] stores C = +inf, and ONE exception to the tie rule: where the rule chose left, c2 is +inf and c0 == c1 is finite
(the left edge of a row's window under an exact 0), the move is up. `exception=False` switches it off, to show what it is for."""
import numpy as np

INVALID_KINDS = ["lo_negative", "hi_past_end", "lo_above_hi", "lo0_not_zero", "hi_last_not_end", "lo_decreasing", "hi_decreasing", "gap"]


def invalid_reason(lo, hi, n, m):
    """None if (lo, hi) are valid windows of an n x m problem, else the first condition that fails."""
    lo, hi = [int(v) for v in lo[:n]], [int(v) for v in hi[:n]]
    for i in range(n):
        if not 0 <= lo[i] <= hi[i] <= m - 1:
            return "0 <= lo[%d] <= hi[%d] <= M-1" % (i, i)
        if i and (lo[i] < lo[i - 1] or hi[i] < hi[i - 1]):
            return "non-decreasing at row %d" % i
        if i and lo[i] > hi[i - 1] + 1:
            return "lo[%d] <= hi[%d] + 1" % (i, i - 1)
    if lo[0] != 0:
        return "lo[0] == 0"
    if hi[n - 1] != m - 1:
        return "hi[N-1] == M-1"
    return None


def fill(matrix, lo, hi, exception=True):
    """(C [N+1][M+1] f32, T [N+1][M+1] int8) of the windowed DTW of `-matrix`, with the border row / column 0 of dtw_cpu. T of a cell that
    is not allowed is -1."""
    m = np.ascontiguousarray(matrix, dtype=np.float32)
    N, M = m.shape
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    x = (-m).astype(np.float64)
    C = np.full((N + 1, M + 1), np.inf, dtype=np.float32)
    T = np.full((N + 1, M + 1), -1, dtype=np.int8)
    C[0, 0] = 0
    for d in range(2, N + M + 1):
        i = np.arange(max(1, d - M), min(N, d - 1) + 1)
        j = d - i
        c0, c1, c2 = C[i - 1, j - 1], C[i - 1, j], C[i, j - 1]
        t = np.where((c0 < c1) & (c0 < c2), 0, np.where((c1 < c0) & (c1 < c2), 1, 2))
        if exception:
            t = np.where((t == 2) & np.isinf(c2) & (c0 == c1) & np.isfinite(c0), 1, t)
        c = np.where(t == 0, c0, np.where(t == 1, c1, c2))
        allowed = (lo[i - 1] <= j - 1) & (j - 1 <= hi[i - 1])
        with np.errstate(invalid="ignore"):
            v = (x[i - 1, j - 1] + c.astype(np.float64)).astype(np.float32)
        C[i, j] = np.where(allowed, v, np.float32(np.inf))
        T[i, j] = np.where(allowed, t, -1)
    return C, T


def dtw_windows(matrix, lo, hi, exception=True):
    """-> (text_indices, time_indices, jump_frames [N], end_cost f32): the path from (N-1, M-1) back along the moves. Raises
    AssertionError if the backtrace meets a cell that is not allowed (only possible with exception=False or invalid windows)."""
    C, T = fill(matrix, lo, hi, exception)
    N, M = C.shape[0] - 1, C.shape[1] - 1
    T = T.copy()
    T[0, :] = 2
    T[:, 0] = 1
    i, j = N, M
    path = []
    while i > 0 or j > 0:
        path.append((i - 1, j - 1))
        assert T[i, j] >= 0, "the backtrace left the windows at (%d, %d)" % (i - 1, j - 1)
        if T[i, j] == 0:
            i, j = i - 1, j - 1
        elif T[i, j] == 1:
            i -= 1
        else:
            j -= 1
    path = np.array(path[::-1], dtype=np.int64)
    jump = np.full(N, -1, dtype=np.int32)
    for ti, tj in path[::-1]:
        jump[ti] = tj
    return path[:, 0], path[:, 1], jump, C[N, M]


# ---------------------------------------------------------------------------------------------- window generators
def full(N, M):
    return np.zeros(N, np.int32), np.full(N, M - 1, np.int32)


def _finish(lo, hi, M):
    """Any (lo, hi) made valid: clipped, monotone, the corners pinned, no gap between consecutive rows."""
    lo, hi = np.clip(np.asarray(lo, np.int64), 0, M - 1), np.clip(np.asarray(hi, np.int64), 0, M - 1)
    lo, hi = np.maximum.accumulate(lo), np.maximum.accumulate(hi)
    lo[0], hi[-1] = 0, M - 1
    hi = np.maximum(hi, lo)
    for i in range(1, len(lo)):
        lo[i] = min(lo[i], hi[i - 1] + 1)
    lo = np.minimum(lo, hi)
    return lo.astype(np.int32), hi.astype(np.int32)


def band(N, M, width):
    """A diagonal band: row i may sit within `width` frames of the straight line from (0, 0) to (N-1, M-1)."""
    c = np.round(np.arange(N) * ((M - 1) / max(N - 1, 1))).astype(np.int64)
    return _finish(c - width, c + width, M)


def staircase(N, M, n_cues, slack, seed=0):
    """Windows as cues produce them: the rows fall into n_cues runs, run k shares one interval [start_k - slack, end_k + slack], and
    the last row (an eot) has [end - slack, M - 1]."""
    rng = np.random.default_rng(seed)
    n_cues = max(1, min(n_cues, N, M))
    row_cut = np.sort(rng.choice(np.arange(1, N), size=min(n_cues - 1, max(N - 1, 0)), replace=False)) if N > 1 else np.array([], np.int64)
    col_cut = np.sort(rng.integers(0, M, size=len(row_cut)))
    starts, ends = np.concatenate([[0], col_cut]), np.concatenate([col_cut, [M - 1]])
    cue = np.searchsorted(row_cut, np.arange(N), side="right")
    lo, hi = starts[cue] - slack, ends[cue] + slack
    lo[cue == 0] = 0
    hi[cue == cue[-1]] = M - 1
    if N > 1:
        lo[-1] = M - 1 - slack
    return _finish(lo, hi, M)


def chain(N, M, seed=0):
    """lo == hi in every row: exactly one path, row i at frame lo[i] only. Needs N >= M (every frame is some row's) -- for N < M use
    chain_path on the transposed roles. Returns (lo, hi): lo rises by 0 or 1 per row from 0 to M - 1."""
    assert N >= M
    rng = np.random.default_rng(seed)
    steps = np.zeros(N - 1, np.int64)
    steps[rng.choice(N - 1, size=M - 1, replace=False)] = 1
    lo = np.concatenate([[0], np.cumsum(steps)]).astype(np.int32)
    return lo, lo.copy()


def idle_lanes(N, M):
    """Windows that leave whole lanes idle for long stretches: the first half of the rows is held in the first few frames and the second
    half in the last few, so for most of the sweep the lanes of either half own no allowed cell."""
    k = max(1, min(M // 8, 4))
    h = N // 2
    lo = np.where(np.arange(N) < h, 0, M - 1 - k)
    hi = np.where(np.arange(N) < h, k, M - 1)
    return _finish(lo, hi, M)


def word_edges(N, M, seed=0):
    """Windows whose edges sit at j % 16 in {0, 15}: the edges of the 16-column trace words."""
    rng = np.random.default_rng(seed)
    edges0 = np.arange(0, M, 16)
    edges15 = np.minimum(np.arange(15, M + 15, 16), M - 1)
    lo = np.sort(rng.choice(edges0, size=N))
    hi = np.sort(rng.choice(edges15, size=N))
    return _finish(lo, np.maximum(hi, lo + 15), M)


def random_valid(N, M, rng):
    lo = np.sort(rng.integers(0, M, size=N))
    hi = lo + rng.integers(0, max(2, M // 3), size=N)
    return _finish(lo, hi, M)


def plant_zeros_at_left_edges(matrix, lo):
    """Quarter-valued matrix with an exact 0 at (i - 1, lo[i]) for every row i whose window starts right of the row above's: the cell above
    a window's left edge adds nothing, so the diagonal and the upper cost there can tie -- the exception's case."""
    m = np.array(matrix, dtype=np.float32)
    for i in range(1, len(lo)):
        if lo[i] > lo[i - 1]:
            m[i - 1, lo[i]] = 0.0
    return m


def make_invalid(kind, N, M):
    """Full windows of an N x M problem (N, M >= 3) broken in exactly the named way."""
    lo, hi = full(N, M)
    if kind == "lo_negative":
        lo[0] = -1
    elif kind == "hi_past_end":
        hi[N - 1] = M
    elif kind == "lo_above_hi":
        lo[1:], hi[1] = 2, 1
        hi[0] = 1
    elif kind == "lo0_not_zero":
        lo[:] = 1
    elif kind == "hi_last_not_end":
        hi[:] = M - 2
    elif kind == "lo_decreasing":
        lo[1], lo[2] = 1, 0
    elif kind == "hi_decreasing":
        hi[0], hi[1] = M - 1, M - 2
        hi[2:] = M - 1
    elif kind == "gap":
        hi[0], lo[1:] = 0, 2
    else:
        raise KeyError(kind)
    return lo, hi


def exception_case():
    """The named planted case: 2 x 2, row 1 may only sit at frame 1, and the entry above its window's left edge is an exact 0.
    C[0][0] = -0.25 and C[0][1] = -0.25 + 0 tie as the diagonal and upper cost of cell (1, 1), whose left neighbour is not allowed."""
    m = np.array([[0.25, 0.0], [0.5, 0.5]], np.float32)
    return m, np.array([0, 1], np.int32), np.array([1, 1], np.int32)
