"""The resampler to 16 kHz on the MI355X (wca_resample_16k, csrc/resample.hip) against a float64 numpy restatement of the definition in
include/wca.h: every table home of the kernel (one uniform row, LDS, global memory), up- and down-sampling, both zero-extended ends,
several tiles with a ragged last one, the 64-bit j M, channels / row stride / alignment, the refusals, the table cache, and transcribe()
of a 48 kHz file end to end on the tiny seeded model of tests/test_transcribe_gpu.py.

Tolerance: the kernel rounds the table and the products to f32 and adds n_taps terms in f32, so
|gpu - ref| <= (n_taps + 2) 2^-24 sum|h| max|x| <= 42 x 5.96e-8 x 1.87 = 4.7e-6 for n_taps <= 40 and |x| <= 1 (sum|h| <= 1.87 over the
rates used here, printed by tests/test_resample.py::test_table); TOL gives that bound a factor of two."""
import ctypes as C
import importlib
import json
import math
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-5
RATES = (8000, 11025, 22050, 24000, 32000, 44100, 48000, 44101)


# ---- the definition, restated in float64 numpy
def ref_plan(sr_in):
    g = math.gcd(sr_in, 16000)
    L, M = 16000 // g, sr_in // g
    W = -(-600 * M // (99 * min(L, M)))
    return L, M, W, 2 * W + 2


_tables = {}


def ref_table(sr_in):
    if sr_in not in _tables:
        L, M, W, n_taps = ref_plan(sr_in)
        c = 0.99 * min(L, M) / M
        i, p = np.arange(n_taps, dtype=np.float64)[None, :], np.arange(L, dtype=np.float64)[:, None]
        t = np.clip((i - W - p / L) * c, -6.0, 6.0)
        _tables[sr_in] = c * np.sinc(t) * np.cos(np.pi * t / 12.0) ** 2
    return _tables[sr_in]


def ref_resample(x, sr_in, j_from=0):
    """x float64 [n] (the channel mean already taken) -> float64 outputs [j_from, ceil(n L / M))"""
    L, M, W, n_taps = ref_plan(sr_in)
    h = ref_table(sr_in)
    n_out = -(-len(x) * L // M)
    jm = np.arange(j_from, n_out, dtype=object) * M   # Python ints: j M passes 2^31
    k0, p = (jm // L).astype(np.int64), (jm % L).astype(np.int64)
    k = k0[:, None] + np.arange(n_taps)[None, :] - W
    inside = (k >= 0) & (k < len(x))
    xg = np.where(inside, np.asarray(x, np.float64)[np.clip(k, 0, len(x) - 1)], 0.0)
    return (h[p] * xg).sum(axis=1)


def _noise(n, seed):
    x = np.random.default_rng(seed).uniform(-1.0, 1.0, n).astype(np.float32)
    x[0], x[n - 1] = 1.0, -1.0   # both zero-extended ends carry full-scale samples (n == 1: the sample is -1)
    return x


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("whisper-char-alignment_amd")


@pytest.fixture(scope="module")
def small(pkg):
    dims = pkg.ModelDimensions(80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)
    m = pkg.WhisperAMD(dims, device="cuda:0", max_batch=4, precision="f16")
    m.load_state_dict(importlib.import_module("whisper-char-alignment_amd.synthetic").random_state_dict(dims, seed=5))
    return m


@pytest.mark.parametrize("sr_in", RATES)
def test_resample_vs_float64(small, sr_in):
    L, M, W, n_taps = ref_plan(sr_in)
    # the n_in that gives n_out = 20001: several tiles and a ragged last one whatever the tile size. Down-sampling, one exists in every
    # interval (20000 M / L, 20001 M / L]; up-sampling (8 kHz doubles: n_out is even) the next n_in gives 20002
    n_tiles_in = 20001 * M // L
    if -(-n_tiles_in * L // M) < 20001:
        n_tiles_in += 1
    n_tiles_out = -(-n_tiles_in * L // M)
    assert (n_tiles_out == 20001 if M >= L else n_tiles_out in (20001, 20002)) and n_tiles_out % 256 != 0
    for n_in in (1, 2, W, W + 1, 4099, n_tiles_in):
        x = _noise(n_in, 1000 + n_in % 977)
        got = small.resample(torch.from_numpy(x), sr_in)
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == (-(-n_in * L // M),)
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref_resample(x.astype(np.float64), sr_in)).max())
        print("sr_in %d n_in %d -> %d: max |gpu - float64| %.2e" % (sr_in, n_in, got.shape[0], err))
        assert err <= TOL, (sr_in, n_in, err)


def test_resample_64bit_index(small):
    sr_in, n_in = 44101, 170000
    L, M, W, n_taps = ref_plan(sr_in)
    x = _noise(n_in, 7)
    got = small.resample(torch.from_numpy(x).cuda(), sr_in).cpu().numpy()
    assert got.shape == (61677,) and (got.shape[0] - 2000) * M > 2 ** 31   # every checked output has j M past 2^31
    want = ref_resample(x.astype(np.float64), sr_in, j_from=got.shape[0] - 2000)
    err = float(np.abs(got[-2000:].astype(np.float64) - want).max())
    print("44101 Hz, outputs %d..%d: max |gpu - float64| %.2e" % (got.shape[0] - 2000, got.shape[0], err))
    assert err <= TOL


def test_resample_channels_and_stride(small):
    n_in, ld = 30001, 30004
    rng = np.random.default_rng(21)
    alloc = torch.from_numpy(rng.uniform(-1.0, 1.0, 1 + 2 * ld).astype(np.float32)).cuda()
    buf = alloc[1:].view(2, ld)        # starts one float into the allocation; rows ld = n_in + 3 apart
    view = buf[:, :n_in]
    assert view.data_ptr() % 16 == 4 and view.stride() == (ld, 1)
    host = view.cpu().numpy()
    got = small.resample(view, 44100).cpu().numpy()
    want = ref_resample(host.astype(np.float64).mean(axis=0), 44100)
    assert got.shape == want.shape
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("[2, %d] rows %d apart at 44100 Hz: max |gpu - float64| %.2e" % (n_in, ld, err))
    assert err <= TOL
    # 16 kHz in: no filter, the f32 mean (a copy for one channel)
    same = small.resample(view, 16000)
    assert torch.equal(same, view.mean(dim=0))
    assert torch.equal(small.resample(view[0], 16000), view[0])
    # a recording without samples
    for sr_in in (16000, 44100):
        empty = small.resample(torch.zeros(2, 0), sr_in)
        assert empty.shape == (0,) and empty.is_cuda
    n_out = C.c_int64(-1)
    assert small._lib.wca_resample_16k(small._h, None, 1, 0, 0, 44100, None, 0, C.byref(n_out)) == 0 and n_out.value == 0


def test_resample_refusals(small):
    lib = small._lib
    x = torch.from_numpy(_noise(4099, 3)).cuda()
    out = torch.full((2000,), 7.0, device="cuda")
    n_out = C.c_int64(-1)

    def call(channels, sr_in, cap):
        return lib.wca_resample_16k(small._h, C.c_void_p(x.data_ptr()), channels, x.shape[0], x.shape[0], sr_in, C.c_void_p(out.data_ptr()), cap,
                                    C.byref(n_out))

    want_n = -(-4099 * 160 // 441)
    for channels, sr_in, cap in ((1, 1999, 2000), (1, 384001, 2000), (0, 44100, 2000), (9, 44100, 2000), (1, 44100, want_n - 1)):
        assert call(channels, sr_in, cap) == -1, (channels, sr_in, cap)   # WCA_ERR_INVALID
        assert lib.wca_last_error()
    assert n_out.value == want_n   # the size is reported even where the buffer is too small
    small.synchronize()
    assert bool((out == 7.0).all())   # nothing was launched
    for rate in (1999, 384001):
        with pytest.raises(importlib.import_module("whisper-char-alignment_amd._lib").WcaError):
            small.resample(x, rate)
    with pytest.raises(ValueError):
        small.resample(torch.zeros(2, 2, 8), 44100)
    assert call(1, 44100, 2000) == 0 and n_out.value == want_n
    small.synchronize()
    err = float(np.abs(out[:want_n].cpu().numpy().astype(np.float64) - ref_resample(x.cpu().numpy().astype(np.float64), 44100)).max())
    assert err <= TOL and bool((out[want_n:] == 7.0).all())


def test_table_cache(small):
    x = torch.from_numpy(_noise(50000, 5)).cuda()
    first = small.resample(x, 44100)
    other = small.resample(x, 48000)
    again = small.resample(x, 44100)
    assert torch.equal(first, again)
    assert float(np.abs(other.cpu().numpy().astype(np.float64) - ref_resample(x.cpu().numpy().astype(np.float64), 48000)).max()) <= TOL


def _write_wav(path, pcm_i16, rate):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm_i16.astype("<i2").tobytes())


def _brief(res):
    return ([(w["seek"], w["size"], w["advance"], w["skipped"]) for w in res["windows"]],
            [(s["seek"], s["start"], s["end"], s["tokens"]) for s in res["segments"]])


def test_transcribe_48k_file(small, tmp_path):
    m = lambda n: importlib.import_module("whisper-char-alignment_amd." + n)   # noqa: E731
    tr, syn = m("transcribe"), m("synthetic")
    pcm_i16 = np.round(syn.synth_audio(41, 48000 * 3) * 32767.0).clip(-32768, 32767).astype(np.int16)
    path = tmp_path / "rec48.wav"
    _write_wav(path, pcm_i16, 48000)
    pcm = torch.from_numpy(pcm_i16.astype(np.float32) / 32768.0)
    pcm16 = small.resample(pcm, 48000)
    assert pcm16.shape == (48000,)
    assert small.log_mel_long(pcm16).shape == (80, (pcm16.shape[0] + 480000) // 160)
    kw = dict(language="en", sample_len=24)
    from_file = tr.transcribe(small, str(path), **kw)
    from_16k = tr.transcribe(small, pcm16.cpu(), **kw)
    same = lambda a, b: json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)   # noqa: E731
    assert same(from_file, from_16k) and len(from_file["windows"]) == 1 and from_file["windows"][0]["size"] == 300
    assert same(tr.transcribe(small, pcm, sample_rate=48000, **kw), from_16k)

    # lock-step with a 16 kHz array: each recording's own result (tests/test_transcribe_batch_gpu.py's rule: equal windows and tokens, or
    # a first difference inside the one window excused by a teacher-forced logit gap below 1e-3, for at most one recording)
    other = syn.synth_audio(42, 16000 * 5 + 40)
    alone = [from_file, tr.transcribe(small, other, **kw)]
    batch = tr.transcribe_batch(small, [str(path), other], sample_rate=[48000, 16000], **kw)
    tok = m("tokenizer").get_tokenizer(True, language="en", task="transcribe")
    mels = [small.log_mel_long(pcm16), small.log_mel_long(torch.from_numpy(other).cuda())]
    n_excused = 0
    for i, (a, b) in enumerate(zip(alone, batch)):
        assert [(w["seek"], w["size"]) for w in a["windows"]] == [(w["seek"], w["size"]) for w in b["windows"]] and len(a["windows"]) == 1
        if _brief(a) == _brief(b):
            continue
        n_excused += 1
        toks_a = [t for s in a["segments"] for t in s["tokens"]]
        toks_b = [t for s in b["segments"] for t in s["tokens"]]
        assert toks_a != toks_b, "the decodes agree: the difference is in the host loop"
        p_ = next(k for k in range(max(len(toks_a), len(toks_b))) if k >= len(toks_a) or k >= len(toks_b) or toks_a[k] != toks_b[k])
        choice_a = toks_a[p_] if p_ < len(toks_a) else tok.eot
        choice_b = toks_b[p_] if p_ < len(toks_b) else tok.eot
        window = small.mel_window(mels[i], 0, a["windows"][0]["size"])
        forced = torch.tensor([list(tok.sot_sequence) + toks_a[:p_]], dtype=torch.int64).cuda()
        _w, logits = small.get_attentions(window[None], forced, [100], 3, 1.0)
        row = logits[0, -1].float().cpu().numpy()
        gap = abs(float(row[choice_a]) - float(row[choice_b]))
        print("recording %d diverges at sampled position %d: tokens %d / %d, teacher-forced logit gap %.3e" % (i, p_, choice_a, choice_b, gap))
        assert gap < 1e-3, (i, p_, gap)
    assert n_excused <= 1
