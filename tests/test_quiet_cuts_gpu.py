"""`-m gpu`: the quiet-cut kernel (csrc/quiet_cuts.hip, C ABI wca_quiet_cuts) against its numpy restatement (tests/quiet_cuts_ref.py),
BIT-EXACT in cuts and levels: the definition is in integers from the first sum on, so no summation order can excuse a difference. The
shapes are the smallest at which the kernel can go wrong: spans that are no multiple of a wave or of the workgroup, the largest LDS span,
windows that reach past either end of the recording, ties across waves, the quantiser's rounding ties and its special values, more
workgroups than compute units, and a target k * content_frames beyond 2^31."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import quiet_cuts_ref as ref

pytestmark = pytest.mark.gpu


def _engine(n_mels):
    pkg = importlib.import_module("whisper-char-alignment_amd")
    n_vocab = 51866 if n_mels == 128 else 51865
    return pkg.WhisperAMD(pkg.ModelDimensions(n_mels, 1500, 128, 2, 1, n_vocab, 448, 128, 2, 1), device="cuda:0", max_batch=1, _register=False,
                          precision="f16")   # (weight-less: the cut runs no forward)


@pytest.fixture(scope="module")
def eng80():
    return _engine(80)


@pytest.fixture(scope="module")
def eng128():
    return _engine(128)


def _random(seed, n_mels, frames):
    return np.random.default_rng(seed).normal(0.5, 0.3, size=(n_mels, frames)).astype(np.float32)


def _check(engine, mel, content_frames, n_pieces, radius, half_width):
    want = ref.quiet_cuts(mel, n_pieces, radius, half_width, content_frames)
    got = engine.quiet_cuts(torch.from_numpy(mel).cuda(), n_pieces, radius, half_width, content_frames)
    assert got[0] == want[0], (content_frames, n_pieces, radius, half_width)
    assert got[1] == want[1], (content_frames, n_pieces, radius, half_width)
    cuts = got[0]
    assert cuts[0] == 0 and cuts[-1] == content_frames and all(a < b for a, b in zip(cuts, cuts[1:])) and all(c % 2 == 0 for c in cuts[1:-1])
    return got


@pytest.mark.parametrize("case, cuts", [((4001, 3, 300, 12), [0, 1332, 2666, 4001]), ((700, 3, 100, 100), [0, 232, 466, 700]),
                                        ((1001, 4, 124, 3), [0, 250, 500, 750, 1001]), ((6010, 2, 1500, 0), [0, 3004, 6010])])
def test_silence_cuts_at_the_even_frame_nearest_the_equal_share(eng80, case, cuts):
    """All zero: every candidate ties in level, on lanes of all four waves; the distance to the target, then the lower frame, decide."""
    got = _check(eng80, np.zeros((80, case[0]), np.float32), *case)
    assert got[0] == cuts and got[1] == [0] * (case[1] - 1)


def test_plateau_edge_nearest_the_target(eng80):
    mel = _random(0, 80, 4001)
    mel[:, 1500:1560] = -1.0
    cuts, levels = _check(eng80, mel, 4001, 3, 300, 12)
    assert cuts[1] == 1512 and levels[0] == -8192000   # the 36-frame tie plateau [1512, 1547]: its edge nearest the target 1333


@pytest.mark.parametrize("seed", range(5))
def test_random_mels(eng80, eng128, seed):
    _check(eng80, _random(seed, 80, 4001), 4001, 3, 300, 12)
    _check(eng128, _random(seed, 128, 3000 + seed), 3000 + seed, 2 + seed, 129, 5)   # 259 candidates + 10: no multiple of 64 or 256


def test_spans(eng80, eng128):
    _check(eng80, _random(10, 80, 4001), 4001, 3, 129, 12)       # a span that is no multiple of 64 or 256
    _check(eng80, _random(11, 80, 6010), 6010, 2, 1500, 100)     # the largest LDS span, 3201 frame levels
    _check(eng128, _random(12, 128, 6004), 6004, 2, 1500, 100)   # ... with the largest levels' row count (content_frames / n = 2 radius + 2 exactly)
    _check(eng80, _random(13, 80, 9), 8, 2, 1, 0)                # the smallest there is: frames 3..5, one even candidate
    _check(eng80, _random(14, 80, 9), 9, 2, 1, 100)              # every window clamps on both sides


def test_window_clamps_at_both_ends_and_reads_nothing_past_content_frames(eng80):
    """400 frames in 4 pieces, radius 49, half width 100: the first range's windows reach below frame 0 and the last one's beyond frame
    399, so both clamps fire; the tensor is 64 frames longer than the content, and what lies there (NaN, inf, huge values) is not read:
    the restatement never sees it."""
    cf = 400
    mel = _random(20, 80, cf + 64)
    mel[:, cf:] = np.nan
    mel[::2, cf + 1::3] = np.inf
    mel[1::2, cf + 2::3] = -1e30
    want = ref.quiet_cuts(mel[:, :cf].copy(), 4, 49, 100, cf)
    got = _check(eng80, mel, cf, 4, 49, 100)
    assert got == want
    # the same content without the tail (ld == content_frames)
    assert eng80.quiet_cuts(torch.from_numpy(mel[:, :cf].copy()).cuda(), 4, 49, 100, cf) == want


def test_quantiser_ties_go_to_even(eng80):
    """Values (k + 0.5) / 4096 are exact in f32 and sit on the quantiser's ties: rint gives the even neighbour, round-half-away another
    level for every even k."""
    k = np.random.default_rng(30).integers(-3000, 3000, size=(80, 2001))
    mel = ((2 * k + 1) / 8192.0).astype(np.float32)
    assert np.array_equal(mel.astype(np.float64) * 4096.0, k + 0.5)
    away = np.where(k >= 0, k + 1, k).sum(axis=0)
    assert not np.array_equal(ref.quantise(mel).sum(axis=0), away)   # (the two roundings do differ on this input)
    _check(eng80, mel, 2001, 3, 300, 12)
    _check(eng80, mel, 2001, 3, 300, 0)   # half_width 0: the level IS one frame's sum of quantised values


def test_special_values_inside_a_range(eng80):
    mel = _random(40, 80, 4001)
    g = 4001 // 3
    for row, dt, v in [(3, 0, np.nan), (5, 2, np.inf), (7, -4, -np.inf), (9, 10, 100.0), (11, -10, -100.0), (13, 20, 8.001), (15, -20, -8.001),
                       (17, 30, 8.0), (19, -30, -8.0), (21, 40, -0.0), (23, -40, 1e-45), (25, 50, 3.4e38), (27, -50, -3.4e38)]:
        mel[row, g + dt] = v
    assert ref.quantise(np.float32(np.nan)) == 32768 and ref.quantise(np.float32(-np.inf)) == -32768
    _check(eng80, mel, 4001, 3, 300, 12)
    _check(eng80, mel, 4001, 3, 300, 0)
    mel[:, g - 2:g + 3] = np.nan   # a whole stretch of NaN is loud: the cut moves away from it
    cuts, _ = _check(eng80, mel, 4001, 3, 300, 1)
    assert abs(cuts[1] - g) > 3
    mel[:] = -np.inf   # the lowest level there is, everywhere: 80 x -32768 x 25 stays inside int32
    assert _check(eng80, mel, 4001, 3, 300, 12)[1] == [-80 * 32768 * 25] * 2


def test_many_pieces_and_a_target_beyond_int32(eng80):
    """4096 pieces: 4095 workgroups, more than the GPU has compute units; and with 524500 frames the product k * content_frames of the
    targets passes 2^31 (4095 x 524500)."""
    _check(eng80, _random(50, 80, 16389), 16389, 4096, 1, 0)
    cf = 524500
    mel = (torch.randn(80, cf, generator=torch.Generator().manual_seed(51)) * 0.3 + 0.5).numpy()
    _check(eng80, mel, cf, 4096, 63, 2)


def test_invalid_arguments_leave_the_cuts_untouched(eng80):
    lib, INVALID = eng80._lib, -1
    mel = torch.zeros(80, 4001, device="cuda")
    bad = [dict(n_pieces=1), dict(n_pieces=4097), dict(n_pieces=0), dict(radius=0), dict(radius=1501), dict(half_width=-1), dict(half_width=101),
           dict(content_frames=4002), dict(content_frames=2 ** 31, ld=2 ** 31), dict(radius=1000), dict(content_frames=0), dict(content_frames=-5),
           dict(n_pieces=7, radius=285)]   # 4001 // 7 = 571 < 2 x 285 + 2
    for change in bad:
        a = dict(ld=4001, content_frames=4001, n_pieces=3, radius=300, half_width=12)
        a.update(change)
        assert not ref.valid(a["content_frames"], a["ld"], a["n_pieces"], a["radius"], a["half_width"]), change
        cuts = np.full(4100, -7, np.int32)
        levels = np.full(4100, -7, np.int32)
        rc = lib.wca_quiet_cuts(eng80._h, ctypes.c_void_p(mel.data_ptr()), a["ld"], a["content_frames"], a["n_pieces"], a["radius"], a["half_width"],
                                cuts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), levels.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        assert rc == INVALID, change
        assert (cuts == -7).all() and (levels == -7).all(), change
    cuts = np.full(4, -7, np.int32)
    assert lib.wca_quiet_cuts(eng80._h, None, 4001, 4001, 3, 300, 12, cuts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None) == INVALID
    assert lib.wca_quiet_cuts(eng80._h, ctypes.c_void_p(mel.data_ptr()), 4001, 4001, 3, 300, 12, None, None) == INVALID and (cuts == -7).all()
    # the boundary itself is valid: 4001 // 7 = 571 >= 2 x 284 + 2; and the levels are optional
    assert lib.wca_quiet_cuts(eng80._h, ctypes.c_void_p(mel.data_ptr()), 4001, 4001, 7, 284, 12, np.zeros(8, np.int32).ctypes.data_as(
        ctypes.POINTER(ctypes.c_int32)), None) == 0
    with pytest.raises(ValueError):
        eng80.quiet_cuts(mel, 3, content_frames=4002)
    with pytest.raises(ValueError):
        eng80.quiet_cuts(torch.zeros(128, 4001, device="cuda"), 3)
