"""`-m gpu`: the log-mel kernels (csrc/logmel.hip) against the float64 restatement tests/logmel_ref.py at the sample counts where the
active-frame arithmetic decides something, on inputs whose last active frame lies above the `max - 8` floor (tests/test_logmel_ref.py
asserts that on the CPU): the batched 30 s form in ragged launches with NaN behind every row's samples and loud and quiet rows side by
side, a row stride of its own, silence, 128 mels, the whole-recording form at short lengths, and the time-major f16 image that the
pcm path writes for the conv stem, observed through detect_language bit for bit against the mel path.

Both precision modes run: "f16" (f32 DFT) and "reference" (f64 accumulation of the f32 products)."""
import importlib

import numpy as np
import pytest
import torch

import logmel_ref as ref

pytestmark = pytest.mark.gpu

TOL = 2e-4   # tests/test_kernels_gpu.py::test_logmel_vs_oracle: direct-sum DFT against FFT on the (log10 + 4) / 4 scale
SOT = 50258  # <|startoftranscript|> of the multilingual vocabulary; the language tokens follow it
PRECISIONS = ["f16", "reference"]


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("whisper-char-alignment_amd")


def _engine(pkg, n_mels, n_vocab):
    syn = importlib.import_module("whisper-char-alignment_amd.synthetic")
    dims = pkg.ModelDimensions(n_mels, 1500, 256, 4, 2, n_vocab, 448, 256, 4, 2)
    m = pkg.WhisperAMD(dims, device="cuda:0", max_batch=ref.LAUNCH_ROWS, precision="f16")
    m.load_state_dict(syn.random_state_dict(dims, seed=5))
    return m


@pytest.fixture(scope="module")
def small(pkg):
    return _engine(pkg, 80, 51865)


@pytest.fixture(scope="module")
def mels128(pkg):
    return _engine(pkg, 128, 51866)


@pytest.fixture(scope="module")
def edge_batch():
    return ref.batch(ref.EDGE_BATCH)


def _check_batch(m, precision, rows, pcm, n_samples, want, what):
    """log_mel of the batch in `precision` against the float64 outputs `want`: every row's whole [n_mels][3000], no NaN, an empty row
    exactly -1.5. Returns the largest error."""
    m.set_precision(precision)
    try:
        got = m.log_mel(torch.from_numpy(pcm).cuda(), n_samples=n_samples).cpu().numpy()
    finally:
        m.set_precision("f16")
    assert got.shape == want.shape == (len(rows), m.dims.n_mels, 3000) and got.dtype == np.float32
    assert not np.isnan(got).any(), [ns for b, (ns, _) in enumerate(rows) if np.isnan(got[b]).any()]
    err = np.abs(got.astype(np.float64) - want)
    for b, (ns, quiet) in enumerate(rows):
        mel, t = np.unravel_index(int(err[b].argmax()), err[b].shape)
        assert err[b].max() < TOL, "%s (%s): row %d, %d samples%s (%d active frames): |d| = %.3g at mel %d, frame %d: %.6f, reference %.6f" % (
            what, precision, b, ns, ", quiet" if quiet else "", ref.active_frames(ns), err[b].max(), mel, t, got[b, mel, t], want[b, mel, t])
        if ns == 0:
            assert np.all(got[b] == -1.5)
    print("%s (%s): max |d| against float64 = %.3g" % (what, precision, err.max()))
    return float(err.max())


@pytest.mark.parametrize("precision", PRECISIONS)
def test_edges_of_the_batched_form(small, edge_batch, precision):
    """All 16 sample counts in one call: four launches of four ragged rows, alternate rows quiet, NaN at and beyond every row's count."""
    pcm, n_samples, want = edge_batch
    assert pcm.shape == (16, 480000) and n_samples[:2] == [480000, 0] and not np.isnan(pcm[0]).any() and np.isnan(pcm[1]).all()
    _check_batch(small, precision, ref.EDGE_BATCH, pcm, n_samples, want, "16 sample counts")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_row_stride(small, precision):
    """A [4, 100120] buffer: the row stride is not 480000, row 0 fills its row, the last row is empty."""
    pcm, n_samples, want = ref.batch(ref.STRIDE_BATCH, stride=100120)
    assert pcm.shape == (4, 100120) and n_samples == [100120, 99968, 121, 0]
    _check_batch(small, precision, ref.STRIDE_BATCH, pcm, n_samples, want, "row stride 100120")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_128_mels(mels128, precision):
    pcm, n_samples, want = ref.batch(ref.MELS128_BATCH, n_mels=128)
    _check_batch(mels128, precision, ref.MELS128_BATCH, pcm, n_samples, want, "128 mels")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_silence_and_scale(small, precision):
    """1000 exact zeros are -1.5 everywhere (the clamp, 8 above its own floor), alone and with NaN behind them; a row times 0.03 is the
    row shifted by 2 log10(0.03) / 4 wherever neither the clamp nor a floor holds either of the two."""
    ns = 100000
    loud, quiet = ref.log_mel(ref.signal(ns))[1], ref.log_mel(ref.signal(ns, quiet=True))[1]
    live = (loud > loud.max() - 8.0 + 0.01) & (quiet > max(quiet.max() - 8.0, -10.0) + 0.01)
    assert live[:, :ref.active_frames(ns)].mean() > 0.99 and not live[:, ref.active_frames(ns):].any()
    pcm = np.stack([ref.signal(ns), ref.signal(ns, quiet=True)])
    behind = np.full((1, 4000), np.nan, dtype=np.float32)
    behind[0, :1000] = 0.0
    small.set_precision(precision)
    try:
        silent = small.log_mel(torch.zeros(1000).cuda()).cpu().numpy()
        silent_behind = small.log_mel(torch.from_numpy(behind).cuda(), n_samples=[1000]).cpu().numpy()
        got = small.log_mel(torch.from_numpy(pcm).cuda()).cpu().numpy().astype(np.float64)
    finally:
        small.set_precision("f16")
    assert silent.shape == (80, 3000) and np.all(silent == -1.5)
    assert silent_behind.shape == (1, 80, 3000) and np.all(silent_behind == -1.5)
    shift = np.abs(got[1][live] - got[0][live] - 2.0 * np.log10(ref.QUIET) / 4.0).max()
    print("a row times %.2f (%s): largest departure from the shift %.6f = %.3g" % (ref.QUIET, precision, 2.0 * np.log10(ref.QUIET) / 4.0, shift))
    assert shift < TOL


@pytest.mark.parametrize("precision", PRECISIONS)
def test_whole_recording_form_at_short_lengths(small, precision):
    """wca_log_mel_long below and around one window, the empty recording included (the long and burst inputs: tests/test_transcribe_gpu.py)."""
    small.set_precision(precision)
    worst = 0.0
    try:
        for ns in ref.LONG_COUNTS:
            got = small.log_mel_long(torch.from_numpy(ref.signal(ns)).cuda()).cpu().numpy()
            want = ref.log_mel_long(ref.signal(ns))[0]
            assert got.shape == want.shape == (80, (ns + 480000) // 160), ns
            assert not np.isnan(got).any(), ns
            err = np.abs(got.astype(np.float64) - want)
            mel, t = np.unravel_index(int(err.argmax()), err.shape)
            assert err.max() < TOL, (ns, precision, float(err.max()), int(mel), int(t))
            if ns == 0:
                assert np.all(got == -1.5)
            worst = max(worst, float(err.max()))
    finally:
        small.set_precision("f16")
    print("whole-recording form, %s samples (%s): max |d| against float64 = %.3g" % (ref.LONG_COUNTS, precision, worst))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_image_the_conv_stem_reads(small, precision):
    """The time-major f16 image (zero rows at both ends; hi / lo pairs in the reference mode) is written by logmel_finalize_kernel on the
    pcm path and by mel_to_tm_kernel on the mel path. Both round the same f32 value y = (max(v, floor) + 4) / 4 -- the mel path reads back
    the y that the same finalize kernel stored for log_mel -- so whatever is computed from the encoded state agrees bit for bit: here the
    language token and the 99 language probabilities, then four greedily decoded tokens and the sum of their log-probabilities, of a
    ragged batch with one quiet row and NaN behind every row's samples. That the
    observation is fine enough shows at the end: the mel path with ONE frame of one row replaced, the last active one by the inactive
    value, as an active-frame count one too low would leave it, gives other bits in that row."""
    pcm, n_samples, _ = ref.batch(ref.IMAGE_BATCH)
    dev = torch.from_numpy(pcm).cuda()
    args = dict(sot=SOT, lang_begin=SOT + 1, n_lang=99)
    no_mask = np.zeros(small.dims.n_vocab, dtype=np.uint8)

    def observe(**source):
        """Language token [4] int32 and probabilities [4, 99] f32, then four greedy steps on the state the detection left (which also
        uses that state up: the precision mode cannot change while one waits): tokens [4, 8] int32 and sum of log-probs [4] f32."""
        lang, probs = small.detect_language(**source, **args)
        tokens, _, logprob = small.greedy_decode(None, None, None, [SOT, SOT + 1, SOT + 101, SOT + 105], no_mask, None, sample_len=4,
                                                 eot=SOT - 1, timestamp_begin=SOT + 106, apply_timestamp_rules=False, batch=4)
        return [torch.from_numpy(np.ascontiguousarray(v)) for v in (lang, tokens, probs, logprob)]

    small.set_precision(precision)
    try:
        from_pcm = observe(pcm=dev, n_samples=n_samples)
        mel = small.log_mel(dev, n_samples=n_samples)
        from_mel = observe(mel=mel)
        one_off = mel.clone()
        na = ref.active_frames(n_samples[0])
        one_off[0, :, na - 1] = mel[0, :, na]
        from_one_off = observe(mel=one_off)
    finally:
        small.set_precision("f16")
    probs = from_pcm[2]
    assert probs.shape == (4, 99) and bool(torch.isfinite(probs).all()) and bool(((probs.sum(-1) - 1.0).abs() < 1e-5).all())
    assert from_pcm[1].shape == (4, 8) and bool(torch.isfinite(from_pcm[3]).all())
    differ = int((probs.view(torch.int32) != from_mel[2].view(torch.int32)).sum())
    print("pcm path vs mel path (%s): %d of %d language probabilities differ in their bits (max |dp| = %.3g), sum of log-probs %s / %s" %
          (precision, differ, probs.numel(), float((probs - from_mel[2]).abs().max()), from_pcm[3].tolist(), from_mel[3].tolist()))
    assert torch.equal(from_pcm[0], from_mel[0]) and torch.equal(from_pcm[1], from_mel[1])
    assert torch.equal(probs.view(torch.int32), from_mel[2].view(torch.int32))
    assert torch.equal(from_pcm[3].view(torch.int32), from_mel[3].view(torch.int32))
    assert not torch.equal(from_one_off[2][0].view(torch.int32), from_mel[2][0].view(torch.int32))
