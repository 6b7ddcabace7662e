"""Test helper: a numpy restatement of the quiet-cut definition (include/wca.h: wca_quiet_cuts), written from the definition and not from
the kernel (csrc/quiet_cuts.hip), as tests/dtw_open_ref.py restates the open-end DTW.

    q(x)  = rint(4096 clamp(x, -8, 8)), ties to even; a NaN counts as 8
    e[t]  = sum over the mel rows of q(mel[m][t])
    s[t]  = sum over j in [-half_width, half_width] of e[clamp(t + j, 0, content_frames - 1)]
    g_k   = floor(k content_frames / n_pieces), k = 1 .. n_pieces - 1
    cut_k = the even t in [g_k - radius, g_k + radius] with the smallest (s[t], |t - g_k|, t)

Everything after q is Python / int64 integer arithmetic, so the result does not depend on any summation order. The whole s is computed
(from a prefix sum over an edge-padded e), which is not how a kernel that looks at 3201 frames per cut would do it."""
import numpy as np

N_PIECES_MAX, RADIUS_MAX, HALF_WIDTH_MAX = 4096, 1500, 100


def valid(content_frames, ld, n_pieces, radius, half_width):
    """The argument ranges outside which wca_quiet_cuts returns WCA_ERR_INVALID."""
    return (2 <= n_pieces <= N_PIECES_MAX and 1 <= radius <= RADIUS_MAX and 0 <= half_width <= HALF_WIDTH_MAX and content_frames <= ld
            and content_frames < 2 ** 31 and content_frames // n_pieces >= 2 * radius + 2)


def quantise(x):
    """q of the definition: float32 array -> int64 array."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    x = np.where(np.isnan(x), 8.0, np.clip(x, -8.0, 8.0))
    return np.rint(4096.0 * x).astype(np.int64)   # (np.rint rounds half to even; 4096 x is exact in float64)


def smoothed_level(mel, content_frames, half_width):
    """s [content_frames] int64 of mel [n_mels][>= content_frames]."""
    e = quantise(np.asarray(mel)[:, :content_frames]).sum(axis=0)
    padded = np.concatenate([np.full(half_width, e[0]), e, np.full(half_width, e[-1])])
    prefix = np.concatenate([[0], np.cumsum(padded)])
    return prefix[2 * half_width + 1:] - prefix[:content_frames]


def quiet_cuts(mel, n_pieces, radius=500, half_width=12, content_frames=None):
    """-> (cuts: n_pieces + 1 ints, levels: n_pieces - 1 ints). mel [n_mels][T] float32; content_frames defaults to T - 3000."""
    mel = np.asarray(mel)
    if content_frames is None:
        content_frames = mel.shape[1] - 3000
    if not valid(content_frames, mel.shape[1], n_pieces, radius, half_width):
        raise ValueError("invalid arguments")
    s = smoothed_level(mel, content_frames, half_width)
    cuts, levels = [0], []
    for k in range(1, n_pieces):
        g = k * content_frames // n_pieces
        best = min((int(s[t]), abs(t - g), t) for t in range(g - radius, g + radius + 1) if t % 2 == 0)
        cuts.append(best[2])
        levels.append(best[0])
    return cuts + [content_frames], levels
