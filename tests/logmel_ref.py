"""Test helper: a float64 numpy restatement of the log-mel front end (csrc/logmel.hip: wca_log_mel, the pcm path of phase 1, and
wca_log_mel_long), written from the definition and not from the kernels, as tests/dtw_open_ref.py restates the open-end DTW; and the
signal, sample counts and batches that tests/test_logmel_ref.py pins on the CPU and tests/test_logmel_edges_gpu.py runs on the GPU.

    s      = the ns samples, then zeros up to `total` samples
    frame  = s reflect-padded by 200 at both ends (the mirror at 0 and at total - 1), cut every 160 samples into 400-sample frames
    power  = |rfft(frame * hann)|^2, hann the periodic window 0.5 - 0.5 cos(2 pi n / 400), 201 bins
    logv   = log10(max(filters @ power, 1e-10)), filters = audio.mel_filters(n_mels) (the f32 table the engine loads) taken to float64
    out    = (max(logv, max(logv) - 8) + 4) / 4, ONE maximum over all bins and frames of the row / the recording

The 30 s form has total = 480000 and 3000 frames; the whole-recording form has total = n + 480000 and (n + 480000) // 160 frames.
Everything after the f32 samples and the f32 filter table is float64, with numpy's FFT: no step shares code or summation order with
the kernels' folded 199-term DFT.

What the kernels decide from the sample count alone, restated here as `active_frames` and `last_frame_samples`:

    na = min(ceil((ns + 200) / 160), 3000)       frames that see a sample; the others are exactly log10(1e-10) = -10 before the floor
    k  = ns + 200 - 160 (na - 1)                 samples that fall in frame na - 1 (k = 1: only window index 0, whose Hann weight is 0)
"""
import functools
import importlib

import numpy as np

N_FFT, HOP, N_FRAMES, N_SAMPLES = 400, 160, 3000, 480000

# 0, 1, 2: below one hop; 120: exactly two active frames; 121, 128, 200: a 1-, 8-, 80-sample sliver in frame 2; 199 / 200 / 201: around half a
# window; 99968, 100000, 100120: an 8-, 40- and 160-sample last frame in mid-buffer (100120 + 200 is a multiple of 160); 479640 / 479648: the
# last frame (2999) is inactive / holds 8 samples; 479999 / 480000: the end reflect mirrors the last samples.
SAMPLE_COUNTS = [0, 1, 2, 120, 121, 128, 199, 200, 201, 99968, 100000, 100120, 479640, 479648, 479999, 480000]
QUIET = 0.03          # a quiet row is the same signal times this: its maximum drops by -2 log10(0.03) = 3.05 decades

# The batches of the GPU tests as (sample count, quiet) rows. EDGE_BATCH is cut into launches of four rows by an engine of max_batch 4: every
# launch alternates loud and quiet rows, and every quiet row has inactive frames (479648, 479999 and 480000 have none: they are loud;
# 0 samples have no loud form: quiet). The rows with an 8-sample last frame are loud where they are compared with the reference: times
# 0.03, the lower bins of such a frame fall under the 1e-10 clamp, which is the value of an inactive frame.
EDGE_BATCH = [(480000, False), (0, True), (2, False), (1, True),
              (479999, False), (120, True), (128, False), (199, True),
              (479648, False), (201, True), (121, False), (100000, True),
              (99968, False), (100120, True), (200, False), (479640, True)]
STRIDE_BATCH = [(100120, True), (99968, False), (121, False), (0, True)]        # on a [4, 100120] buffer
MELS128_BATCH = [(128, False), (100000, True), (479648, False), (480000, False)]
IMAGE_BATCH = [(128, False), (99968, True), (479648, False), (480000, False)]
LONG_COUNTS = [0, 1, 2, 121, 128, 201]
LAUNCH_ROWS = 4


def active_frames(ns):
    return min(-(-(ns + 200) // HOP), N_FRAMES)


def last_frame_samples(ns):
    return ns + 200 - HOP * (active_frames(ns) - 1)


def signal(ns, quiet=False):
    """f32 [ns]: 0.05 * standard normal noise (seeded by ns) with clicks of 0.9 at 1 and ns - 1 and of 0.3 at ns - 2, where those exist
    (a later one replaces an earlier one). The click at 1 is mirrored into frame 0 by the start reflect, the one at ns - 2 by the end
    reflect when ns = 480000, the one at ns - 1 makes a thin last-frame sliver visible. The click at ns - 2 is the smaller one on
    purpose: two equal clicks next to each other cancel near the Nyquist frequency, and in an 8-sample sliver, where the rising Hann
    window weighs them 2.2e-3 and 3.0e-3, the top mel bins then come within 0.6 .. 1.0 decades of the floor, whatever the seed; with 0.3
    the lowest bin of such a frame stays 1.6 decades above it (tests/test_logmel_ref.py asserts at least 1). quiet: times QUIET."""
    x = (0.05 * np.random.default_rng(20000 + ns).standard_normal(ns)).astype(np.float32)
    for i, a in ((1, 0.9), (ns - 2, 0.3), (ns - 1, 0.9)):
        if 0 <= i < ns:
            x[i] = a
    return (x * np.float32(QUIET)).astype(np.float32) if quiet else x


@functools.lru_cache(maxsize=None)
def filters(n_mels):
    audio = importlib.import_module("whisper-char-alignment_amd.audio")
    return audio.mel_filters(n_mels).astype(np.float64)


def _log_mel(x, total, n_mels):
    x = np.asarray(x, dtype=np.float32)
    assert x.ndim == 1 and x.shape[0] <= total
    s = np.zeros(total, dtype=np.float64)
    s[:x.shape[0]] = x
    padded = np.pad(s, N_FFT // 2, mode="reflect")
    n_frames = total // HOP
    frames = np.lib.stride_tricks.sliding_window_view(padded, N_FFT)[::HOP][:n_frames]
    hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)
    power = np.abs(np.fft.rfft(frames * hann, axis=-1)) ** 2            # [n_frames][201]
    logv = np.log10(np.maximum(filters(n_mels) @ power.T, 1e-10))       # [n_mels][n_frames]
    out = (np.maximum(logv, logv.max() - 8.0) + 4.0) / 4.0
    return out, logv


def log_mel(x, n_mels=80):
    """The 30 s form of x f32 [ns <= 480000] -> (out [n_mels][3000], logv [n_mels][3000]) float64: the floored and scaled output, and
    the log10 values before the floor."""
    return _log_mel(x, N_SAMPLES, n_mels)


def log_mel_long(x, n_mels=80):
    """The whole-recording form of x f32 [n] -> (out, logv), both [n_mels][(n + 480000) // 160] float64."""
    return _log_mel(x, np.asarray(x).shape[0] + N_SAMPLES, n_mels)


def batch(rows, stride=N_SAMPLES, n_mels=80, junk=np.nan):
    """-> (pcm f32 [len(rows)][stride] with `junk` at and beyond every row's sample count, the sample counts, the reference outputs
    float64 [len(rows)][n_mels][3000])."""
    pcm = np.full((len(rows), stride), junk, dtype=np.float32)
    for b, (ns, quiet) in enumerate(rows):
        pcm[b, :ns] = signal(ns, quiet)
    ref = np.stack([log_mel(signal(ns, quiet), n_mels)[0] for ns, quiet in rows])
    return pcm, [ns for ns, _ in rows], ref
