"""CPU tests of the resampler to 16 kHz: the plan arithmetic and the float64 table of the C ABI (wca_resample_plan / wca_resample_table,
host only) against a numpy restatement of the definition in include/wca.h, the properties of that definition on tones, and the routing
of transcribe(): audio that is not at 16 kHz goes through model.resample with its channels. The kernel is tests/test_resample_gpu.py."""
import ctypes as C
import importlib
import math
import wave

import numpy as np
import pytest
import torch

PLANS = {8000: (2, 1, 7, 16), 11025: (640, 441, 7, 16), 22050: (320, 441, 9, 20), 24000: (2, 3, 10, 22), 32000: (1, 2, 13, 28),
         44100: (160, 441, 17, 36), 48000: (1, 3, 19, 40), 44101: (16000, 44101, 17, 36), 384000: (1, 24, 146, 294)}


# ---- the definition, restated in float64 numpy
def ref_plan(sr_in):
    g = math.gcd(sr_in, 16000)
    L, M = 16000 // g, sr_in // g
    W = -(-600 * M // (99 * min(L, M)))
    return L, M, W, 2 * W + 2


def ref_table(sr_in):
    L, M, W, n_taps = ref_plan(sr_in)
    c = 0.99 * min(L, M) / M
    i, p = np.arange(n_taps, dtype=np.float64)[None, :], np.arange(L, dtype=np.float64)[:, None]
    t = np.clip((i - W - p / L) * c, -6.0, 6.0)
    return c * np.sinc(t) * np.cos(np.pi * t / 12.0) ** 2   # np.sinc(t) = sin(pi t) / (pi t), 1 at 0


def ref_resample(x, sr_in):
    """x float64 [n] (the channel mean already taken) -> float64 [ceil(n L / M)]"""
    L, M, W, n_taps = ref_plan(sr_in)
    h = ref_table(sr_in)
    n_out = -(-len(x) * L // M)
    jm = np.arange(n_out, dtype=object) * M   # Python ints: j M passes 2^31
    k0, p = (jm // L).astype(np.int64), (jm % L).astype(np.int64)
    k = k0[:, None] + np.arange(n_taps)[None, :] - W
    inside = (k >= 0) & (k < len(x))
    xg = np.where(inside, np.asarray(x, np.float64)[np.clip(k, 0, max(len(x) - 1, 0))] if len(x) else 0.0, 0.0)
    return (h[p] * xg).sum(axis=1)


@pytest.fixture(scope="module")
def audio():
    return importlib.import_module("whisper-char-alignment_amd.audio")


def test_plan(audio, lib, wca):
    for sr_in, want in PLANS.items():
        assert ref_plan(sr_in) == want, sr_in
        assert audio.resample_plan(sr_in) == want, sr_in
    for sr_in in (1999, 384001):
        with pytest.raises(wca._lib.WcaError):
            audio.resample_plan(sr_in)
        assert lib.wca_resample_plan(sr_in, None, None, None, None) == -1
    assert lib.wca_version() >= 12
    assert lib.wca_resample_plan(2000, None, None, None, None) == 0 and lib.wca_resample_plan(384000, None, None, None, None) == 0
    # no engine: everything that needs one is refused before anything else happens
    n = C.c_int64(-1)
    assert lib.wca_resample_16k(None, None, 1, 0, 0, 48000, None, 0, C.byref(n)) == -1 and b"null" in lib.wca_last_error()


def test_table(lib):
    for sr_in in (8000, 44100, 48000, 44101):
        L, M, W, n_taps = ref_plan(sr_in)
        got = np.full((L, n_taps), np.nan)
        assert lib.wca_resample_table(sr_in, got.ctypes.data_as(C.POINTER(C.c_double))) == 0
        want = ref_table(sr_in)
        err = float(np.abs(got - want).max())
        rows = got.sum(axis=1)
        print("sr_in %d: table [%d, %d], max |C - numpy| %.2e, row sums %.5f .. %.5f, max sum |h| %.4f" % (
            sr_in, L, n_taps, err, rows.min(), rows.max(), np.abs(got).sum(axis=1).max()))
        assert err <= 1e-12
        assert rows.min() >= 1.0 and rows.max() <= 1.0009   # the filter's own DC gain
    assert lib.wca_resample_table(1999, np.zeros(8).ctypes.data_as(C.POINTER(C.c_double))) == -1
    assert lib.wca_resample_table(48000, None) == -1


def test_filter_properties():
    """The definition itself, on 0.25 s of a 44.1 kHz tone: a tone in the pass band comes out as the same tone at 16 kHz, one above
    the new Nyquist frequency is removed."""
    n = 11025
    t_in = np.arange(n) / 44100.0
    y = ref_resample(np.sin(2 * np.pi * 1000.0 * t_in), 44100)
    assert len(y) == 4000
    ideal = np.sin(2 * np.pi * 1000.0 * np.arange(len(y)) / 16000.0)
    mid = slice(50, len(y) - 50)   # away from the zero-extended ends (the filter spans 36 input samples = 13 outputs)
    gain_db = 20 * np.log10(np.dot(y[mid], ideal[mid]) / np.dot(ideal[mid], ideal[mid]))
    err = float(np.abs(y[mid] - ideal[mid]).max())
    stop = ref_resample(np.sin(2 * np.pi * 12000.0 * t_in), 44100)
    stop_db = 20 * np.log10(np.sqrt(np.mean(stop[mid] ** 2)) / np.sqrt(0.5))
    print("1 kHz: gain %.4f dB, max |y - ideal| %.2e; 12 kHz: %.1f dB" % (gain_db, err, stop_db))
    assert abs(gain_db) <= 0.01
    assert err <= 1e-3
    assert stop_db <= -50.0


# ---- routing in transcribe
class _Stub:
    """The calls transcribe makes before its loop, recorded; every window decodes to <|0.00|> a <|1.00|>."""

    def __init__(self, dims):
        self.dims, self.is_multilingual, self.device, self.max_batch = dims, True, torch.device("cpu"), 4
        self.resampled, self.mel_inputs = [], []

    def resample(self, pcm, sr_in):
        out = torch.zeros(-(-pcm.shape[-1] * 16000 // sr_in))
        self.resampled.append((pcm.clone(), sr_in, out))
        return out

    def log_mel_long(self, pcm):
        self.mel_inputs.append(pcm)
        return torch.zeros(self.dims.n_mels, (pcm.shape[0] + 480000) // 160)

    def mel_window(self, mel_long, seek, size):
        return torch.zeros(self.dims.n_mels, 3000)


def _write_wav(path, pcm_i16, rate):
    """pcm_i16 [channels, n] int16"""
    with wave.open(str(path), "wb") as w:
        w.setnchannels(pcm_i16.shape[0])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(pcm_i16.T).astype("<i2").tobytes())


def test_routing(wca, tmp_path):
    tr = importlib.import_module("whisper-char-alignment_amd.transcribe")
    decoding = importlib.import_module("whisper-char-alignment_amd.decoding")
    tok = importlib.import_module("whisper-char-alignment_amd.tokenizer").get_tokenizer(True, language="en", task="transcribe")
    dims = wca.ModelDimensions(80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)
    ts, a = tok.timestamp_begin, tok.encode("a")[0]

    def decode_window(window, prompt):
        return decoding.DecodingResult(language="en", tokens=[ts, a, ts + 50], text="", avg_logprob=-0.3, no_speech_prob=0.1, temperature=0.0,
                                       compression_ratio=1.0)

    rng = np.random.default_rng(0)
    mono8 = rng.integers(-3000, 3000, size=(1, 8000 * 2 + 1)).astype(np.int16)
    stereo44 = rng.integers(-3000, 3000, size=(2, 44100 + 7)).astype(np.int16)
    mono16 = rng.integers(-3000, 3000, size=(1, 16000 * 2)).astype(np.int16)
    for name, pcm, rate in (("t.wav", mono8, 8000), ("s.wav", stereo44, 44100), ("m.wav", mono16, 16000)):
        _write_wav(tmp_path / name, pcm, rate)

    for name, pcm, rate in (("t.wav", mono8, 8000), ("s.wav", stereo44, 44100)):
        m = _Stub(dims)
        res = tr.transcribe(m, str(tmp_path / name), language="en", decode_window=decode_window)
        assert len(m.resampled) == 1 and len(m.mel_inputs) == 1
        got, sr_in, out = m.resampled[0]
        assert sr_in == rate
        want = torch.from_numpy(pcm.astype(np.float32) / 32768.0)
        assert torch.equal(got, want if pcm.shape[0] > 1 else want[0])   # every channel reaches the kernel: [C, n]
        assert m.mel_inputs[0] is out                                     # and what it returns is what the log-mel gets
        n16 = -(-pcm.shape[1] * 16000 // rate)
        assert [(w["seek"], w["size"]) for w in res["windows"]] == [(0, n16 // 160)]

    m = _Stub(dims)
    tr.transcribe(m, str(tmp_path / "m.wav"), language="en", decode_window=decode_window)
    assert m.resampled == [] and m.mel_inputs[0].shape == (32000,)
    tr.transcribe(m, np.zeros(16000, np.float32), language="en", decode_window=decode_window)
    assert m.resampled == []

    # an array with sample_rate= takes the same path
    m = _Stub(dims)
    x = rng.standard_normal(8000 * 3).astype(np.float32)
    res = tr.transcribe(m, x, language="en", decode_window=decode_window, sample_rate=8000)
    assert len(m.resampled) == 1 and m.resampled[0][1] == 8000 and torch.equal(m.resampled[0][0], torch.from_numpy(x))
    assert m.mel_inputs[0] is m.resampled[0][2] and [(w["seek"], w["size"]) for w in res["windows"]] == [(0, 300)]

    # transcribe_batch: one rate for all arrays, or one per recording; a file keeps its own
    def decode_windows(windows, prompts):
        return [decode_window(None, None) for _ in prompts]

    m = _Stub(dims)
    out = tr.transcribe_batch(m, [str(tmp_path / "s.wav"), x, np.zeros(16000, np.float32)], language="en", decode_windows=decode_windows,
                              sample_rate=[16000, 8000, 16000])
    assert [r[1] for r in m.resampled] == [44100, 8000] and len(m.mel_inputs) == 3 and len(out) == 3
    with pytest.raises(ValueError, match="rates"):
        tr.transcribe_batch(m, [x, x], language="en", decode_windows=decode_windows, sample_rate=[8000])
    assert tr.parse_args(["--audio", "x.npy", "--output_dir", "o", "--sample_rate", "8000"]).sample_rate == 8000
    assert tr.parse_args(["--audio", "x.wav", "--output_dir", "o"]).sample_rate == 16000


def test_dropin_exports(audio):
    import os
    import sys
    dropin = os.path.join(os.path.dirname(os.path.abspath(audio.__file__)), "dropin")
    sys.path.insert(0, dropin)
    try:
        whisper = importlib.import_module("whisper")
        assert whisper.audio.resample is audio.resample and whisper.audio.resample_plan(48000) == (1, 3, 19, 40)
    finally:
        sys.path.remove(dropin)
