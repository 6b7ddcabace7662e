"""CPU tests of the float64 log-mel restatement (tests/logmel_ref.py) and of the inputs that tests/test_logmel_edges_gpu.py feeds the
kernels: the restatement agrees with the fp32 oracle (oracle/whisper_ref.py: torch.stft), and on these inputs the `max - 8` floor hides
nothing -- the last active frame of every sample count lies well above the floor, so an off-by-one in the kernels' active-frame count,
their early return, their `t < na` select or their `idx < ns` guard changes values that the GPU comparison sees."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import logmel_ref as ref
from oracle import whisper_ref

ORACLE_TOL = 2e-5   # float64 against the oracle's f32 torch.stft / f32 matmul on the (log10 + 4) / 4 scale; measured: at most 7.6e-6


@pytest.fixture(scope="module")
def cases():
    """{ns: (out, logv)} of the loud signal at every sample count, computed once."""
    return {ns: ref.log_mel(ref.signal(ns)) for ns in ref.SAMPLE_COUNTS}


def test_sample_count_arithmetic():
    assert [ref.active_frames(ns) for ns in ref.SAMPLE_COUNTS] == [2, 2, 2, 2, 3, 3, 3, 3, 3, 627, 627, 627, 2999, 3000, 3000, 3000]
    assert [ref.last_frame_samples(ns) for ns in ref.SAMPLE_COUNTS] == [40, 41, 42, 160, 1, 8, 79, 80, 81, 8, 40, 160, 160, 8, 359, 360]
    for rows in (ref.EDGE_BATCH, ref.STRIDE_BATCH, ref.MELS128_BATCH, ref.IMAGE_BATCH):
        assert all(ns in ref.SAMPLE_COUNTS for ns, _ in rows)
    assert sorted(ns for ns, _ in ref.EDGE_BATCH) == ref.SAMPLE_COUNTS
    assert [q for _, q in ref.EDGE_BATCH] == [False, True] * 8          # alternate rows are quiet
    x = ref.signal(480000)
    assert x.dtype == np.float32 and x[1] == x[479999] == np.float32(0.9) and x[479998] == np.float32(0.3)
    assert ref.signal(0).shape == (0,) and list(ref.signal(1)) == [np.float32(0.9)]
    assert list(ref.signal(2)) == [np.float32(0.3), np.float32(0.9)]
    assert np.array_equal(ref.signal(200, quiet=True), ref.signal(200) * np.float32(ref.QUIET))


def test_reference_agrees_with_the_oracle(cases):
    filt = ref.filters(80).astype(np.float32)
    worst = 0.0
    for ns, (out, _) in cases.items():
        want = whisper_ref.log_mel_spectrogram(whisper_ref.pad_or_trim(torch.from_numpy(ref.signal(ns))), filt).double().numpy()
        assert out.shape == want.shape == (80, 3000)
        err = float(np.abs(out - want).max())
        worst = max(worst, err)
        assert err < ORACLE_TOL, (ns, err)
    print("float64 log-mel against the fp32 oracle, 30 s form: max |d| = %.3g" % worst)
    assert np.all(cases[0][0] == -1.5)                                  # no sample: every bin is log10(1e-10), the floor is 8 below it


def test_long_reference_agrees_with_the_oracle():
    filt = ref.filters(80).astype(np.float32)
    for n in ref.LONG_COUNTS + [46592]:
        x = ref.signal(n)
        out, logv = ref.log_mel_long(x)
        want = whisper_ref.log_mel_spectrogram(F.pad(torch.from_numpy(x), (0, 480000)), filt).double().numpy()
        assert out.shape == logv.shape == want.shape == (80, (n + 480000) // 160)
        err = float(np.abs(out - want).max())
        assert err < ORACLE_TOL, (n, err)
    # the two forms differ only in where the zeros end: same values wherever the 30 s form's end reflect is out of reach
    assert np.allclose(ref.log_mel_long(ref.signal(201))[0][:, :2998], ref.log_mel(ref.signal(201))[0][:, :2998], rtol=0, atol=1e-12)


def test_the_floor_hides_nothing(cases):
    """The last active frame lies at least one decade above the floor in every mel bin, and fewer than 1 % of the bins of the active
    frames sit on the floor. The one exception: a last frame of k = 1 sample (121 here) holds window index 0 only, whose periodic Hann
    weight is 0, so that frame is silent and sits on the floor; it is left out of that row's floor share, and nothing else is exempt."""
    for ns, (out, logv) in cases.items():
        na, k = ref.active_frames(ns), ref.last_frame_samples(ns)
        floorv = logv.max() - 8.0
        assert np.all(logv[:, na:] == -10.0)                            # the inactive frames are exactly the clamp
        if ns >= 2 and k >= 8:
            margin = float((logv[:, na - 1] - floorv).min())
            assert margin >= 1.0, (ns, k, margin)
        else:
            assert ns < 2 or k == 1, (ns, k)
        if k == 1:
            assert ns == 121 and np.all(logv[:, na - 1] == -10.0)
            na -= 1
        share = float((logv[:, :na] <= floorv).mean())
        assert share < 0.01, (ns, share)
    margins = {ns: round(float((logv[:, ref.active_frames(ns) - 1] - (logv.max() - 8.0)).min()), 2) for ns, (_, logv) in cases.items()
               if ns >= 2 and ref.last_frame_samples(ns) >= 8}
    print("decades between the last active frame's lowest bin and the floor: %s" % margins)


@pytest.mark.parametrize("name,n_mels", [("EDGE_BATCH", 80), ("STRIDE_BATCH", 80), ("MELS128_BATCH", 128), ("IMAGE_BATCH", 80)])
def test_quiet_rows_are_quiet(name, n_mels):
    """Every launch (four rows) holds loud and quiet rows; each quiet row's maximum lies at least 2 decades below that of every loud row
    of the batch, and the quiet row has inactive frames. Those frames hold the clamp, -10, which lies above the quiet row's own floor (its maximum is below -2); a floor taken from a
    loud row's maximum m lifts them to m - 8, that is by (m + 2) / 4 on the output scale: at least 0.05 here, 250 times the tolerance of
    the GPU comparison (not the 2 / 4 = 0.5 that two floors 2 decades apart would give if the clamp were not in between)."""
    rows = getattr(ref, name)
    outs = [ref.log_mel(ref.signal(ns, q), n_mels) for ns, q in rows]
    peak = [float(logv.max()) for _, logv in outs]
    loud = min(p for p, (_, q) in zip(peak, rows) if not q)             # over the whole batch: whichever loud row a launch holds
    for b0 in range(0, len(rows), ref.LAUNCH_ROWS):
        kinds = [q for _, q in rows[b0:b0 + ref.LAUNCH_ROWS]]
        assert True in kinds and False in kinds, (name, b0)
    for p, (ns, q), (out, _) in zip(peak, rows, outs):
        if q:
            assert p <= loud - 2.0, (name, ns, p, loud)
            assert ref.active_frames(ns) < ref.N_FRAMES, (name, ns)
            assert p < -2.0 and np.all(out[:, -1] == -1.5)
            assert (loud - 8.0 + 4.0) / 4.0 - (-1.5) >= 0.05, (name, ns, loud)


@pytest.mark.parametrize("name,n_mels", [("EDGE_BATCH", 80), ("STRIDE_BATCH", 80), ("MELS128_BATCH", 128)])
def test_quiet_rows_keep_their_last_frame_visible(name, n_mels):
    """The margin of test_the_floor_hides_nothing is taken on the loud signal. A quiet row's floor lies below the 1e-10 clamp, so what
    could hide its last active frame is the clamp, the value of the inactive frames: in the batches that are compared with the reference,
    every bin of that frame stays a decade above it (and the rows with 8 samples in that frame, which would not, are loud there)."""
    for ns, quiet in getattr(ref, name):
        k = ref.last_frame_samples(ns)
        assert not (quiet and k == 8), (name, ns)
        if quiet and ns >= 2 and k > 1:
            logv = ref.log_mel(ref.signal(ns, True), n_mels)[1]
            assert logv.max() - 8.0 < -10.0 and logv[:, ref.active_frames(ns) - 1].min() >= -9.0, (name, ns)


def test_scaling_shifts_the_unclamped_bins(cases):
    """A row times 0.03 is the same row shifted by 2 log10(0.03) wherever the 1e-10 clamp holds neither."""
    for ns in (2, 128, 100000):
        quiet = ref.log_mel(ref.signal(ns, quiet=True))[1]
        live = quiet > -10.0
        assert live.any() and np.abs(quiet[live] - cases[ns][1][live] - 2.0 * np.log10(ref.QUIET)).max() < 1e-6
