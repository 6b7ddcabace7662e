"""Test helper: a numpy restatement of the open-end DTW (csrc/dtw.hip, OPEN form) and the planted matrices it is checked on.

The closed DTW's restatement lives in oracle/ (dtw_cpu + backtrace); the open-end form has no counterpart in the reference or upstream,
so it is restated here with the same arithmetic: the recurrence and tie rule of dtw_cpu (diagonal only if strictly smallest, else up only
if strictly smallest, else left), C[i][j] = float32(float64(-m[i][j]) + float64(c)), a path length L per cell (cells on the chosen path,
the cell included), and the end row n* = argmin C[i][M-1] / L[i][M-1] decided on the exact cross-multiplied products (row a beats row b
iff C_a * L_b < C_b * L_a in float64, where both products are exact), the lower row on ties. The table is filled one anti-diagonal at a
time (the cells of one anti-diagonal do not depend on each other), which keeps a 512 x 1500 problem well under a second."""
import numpy as np

PLANTED_SHAPES = [(120, 200), (300, 1500), (64, 100), (130, 300), (200, 750)]


def fill(matrix):
    """Cost, path-length and move tables of the DTW of `-matrix`: (C [N+1][M+1] f32, L [N+1][M+1] int64, T [N+1][M+1] int8), with the
    border row / column 0 of dtw_cpu."""
    m = np.ascontiguousarray(matrix, dtype=np.float32)
    N, M = m.shape
    x = (-m).astype(np.float64)
    C = np.full((N + 1, M + 1), np.inf, dtype=np.float32)
    L = np.zeros((N + 1, M + 1), dtype=np.int64)
    T = np.full((N + 1, M + 1), -1, dtype=np.int8)
    C[0, 0] = 0
    for d in range(2, N + M + 1):
        i = np.arange(max(1, d - M), min(N, d - 1) + 1)
        j = d - i
        c0, c1, c2 = C[i - 1, j - 1], C[i - 1, j], C[i, j - 1]
        t = np.where((c0 < c1) & (c0 < c2), 0, np.where((c1 < c0) & (c1 < c2), 1, 2))
        c = np.where(t == 0, c0, np.where(t == 1, c1, c2))
        C[i, j] = (x[i - 1, j - 1] + c.astype(np.float64)).astype(np.float32)
        L[i, j] = np.where(t == 0, L[i - 1, j - 1], np.where(t == 1, L[i - 1, j], L[i, j - 1])) + 1
        T[i, j] = t
    return C, L, T


def end_row(C, L):
    """argmin over rows of C[i][M] / L[i][M], exact, the lower row on ties (0-based row)."""
    best = 0
    for i in range(1, C.shape[0] - 1):
        a, b = float(C[i + 1, -1]) * int(L[best + 1, -1]), float(C[best + 1, -1]) * int(L[i + 1, -1])
        if a < b:
            best = i
    return best


def dtw_open(matrix, open_end=True):
    """-> (text_indices, time_indices, jump_frames [N] (-1 past the end row), end_row, score f32, unnormalised_end_row).
    open_end=False: the closed DTW (end row N - 1) through the same tables. unnormalised_end_row: the row of the smallest C[i][M-1],
    the lower row on ties -- what a selection without path lengths would pick."""
    C, L, T = fill(matrix)
    N, M = C.shape[0] - 1, C.shape[1] - 1
    n_star = end_row(C, L) if open_end else N - 1
    T[0, :] = 2
    T[:, 0] = 1
    i, j = n_star + 1, M
    path = []
    while i > 0 or j > 0:
        path.append((i - 1, j - 1))
        if T[i, j] == 0:
            i, j = i - 1, j - 1
        elif T[i, j] == 1:
            i -= 1
        else:
            j -= 1
    path = np.array(path[::-1], dtype=np.int64)
    jump = np.full(N, -1, dtype=np.int32)
    for ti, tj in path[::-1]:
        jump[ti] = tj   # the backtrace's last visit of a row is the frame at which the path enters it
    score = np.float32(np.float64(C[n_star + 1, M]) / np.float64(L[n_star + 1, M]))
    return path[:, 0], path[:, 1], jump, n_star, score, int(np.argmin(C[1:, M]))


def planted(N, M, n0, seed=0, noise=0.02):
    """An attention-like matrix [N][M] f32: a diagonal band over rows 0..n0 (row i peaks where the straight line from (0, 0) to
    (n0, M - 1) crosses it), the remaining rows uniform noise; every column is then divided by its L2 norm, like the aggregated maps."""
    rng = np.random.default_rng(seed)
    m = rng.uniform(0.0, noise, size=(N, M))
    cols = np.arange(M)
    centre = cols * (n0 / max(M - 1, 1))
    rows = np.arange(n0 + 1)[:, None]
    m[:n0 + 1] += np.exp(-0.5 * ((rows - centre[None, :]) / 0.7) ** 2)
    m /= np.linalg.norm(m, axis=0, keepdims=True)
    return m.astype(np.float32)


def planted_cases():
    """The five planted matrices: (matrix, n0), n0 at about 60 % of the rows."""
    return [(planted(N, M, (3 * N) // 5, seed=k), (3 * N) // 5) for k, (N, M) in enumerate(PLANTED_SHAPES)]
