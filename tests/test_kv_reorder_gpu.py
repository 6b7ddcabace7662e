"""The cache reorder of the beam search (csrc/beam.hip kv_reorder through wca_test_kv_reorder) on the MI355X, bit for bit against numpy
indexing: dst[p][r][:n_keep[r]] = src[p][src_idx[r]][:n_keep[r]] for every plane, with ragged n_keep, for the sources a beam step produces
(identity, a permutation, duplicates) and for the broadcast of an audio's prefill to its group (src = r // G, planes of different sizes).
Slots past n_keep are not compared: the copy leaves them alone."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

L, ROWS, T_MAX = 2, 6, 7


@pytest.fixture(scope="module")
def engine():
    pkg = importlib.import_module("whisper-char-alignment_amd")
    return pkg.WhisperAMD(pkg.ModelDimensions(80, 1500, 128, 2, 1, 97, 448, 128, 2, 1), device="cuda:0", max_batch=1, precision="f16")


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


@pytest.mark.parametrize("d", [64, 1024])
@pytest.mark.parametrize("kind", ["identity", "permutation", "duplicates", "broadcast"])
def test_kv_reorder_bit_exact(engine, d, kind):
    _lib = importlib.import_module("whisper-char-alignment_amd._lib")
    rng = np.random.default_rng(d + len(kind))
    G = 3
    rows_src = ROWS // G if kind == "broadcast" else ROWS
    src_idx = {"identity": [0, 1, 2, 3, 4, 5], "permutation": [4, 2, 5, 0, 1, 3], "duplicates": [1, 1, 0, 4, 4, 4],
               "broadcast": [r // G for r in range(ROWS)]}[kind]
    n_keep = np.array([7, 0, 3, 1, 6, 4], dtype=np.int32)   # ragged: full, empty, and in between
    # every element distinct in its low bits: a wrong plane, row, slot or column shows
    src = rng.integers(-2048, 2048, size=(2 * L, rows_src, T_MAX, d)).astype(np.float16)
    sentinel = np.float16(-7.5)
    src_d = torch.from_numpy(src).cuda()
    dst_d = torch.full((2 * L, ROWS, T_MAX, d), float(sentinel), dtype=torch.float16, device="cuda")
    idx_d = None if kind == "broadcast" else torch.tensor(src_idx, dtype=torch.int32, device="cuda")
    keep_d = torch.from_numpy(n_keep).cuda()
    engine._bind_stream()
    _lib.check(engine._lib.wca_test_kv_reorder(engine._h, _vp(src_d), _vp(dst_d), 2 * L, rows_src, ROWS, T_MAX, d, _vp(idx_d),
                                               G if kind == "broadcast" else 1, _vp(keep_d)))
    torch.cuda.synchronize()
    got = dst_d.cpu().numpy()
    for r in range(ROWS):
        want = src[:, src_idx[r], :n_keep[r]]
        assert np.array_equal(got[:, r, :n_keep[r]].view(np.uint16), want.view(np.uint16)), (kind, d, r)
    assert np.array_equal(src_d.cpu().numpy().view(np.uint16), src.view(np.uint16))   # the source is only read


def test_kv_reorder_refuses_what_it_cannot_copy(engine):
    lib = engine._lib
    a = torch.zeros(2 * 6 * 7 * 64, dtype=torch.float16, device="cuda")
    b = torch.zeros_like(a)
    keep = torch.zeros(6, dtype=torch.int32, device="cuda")
    assert lib.wca_test_kv_reorder(engine._h, _vp(a), _vp(a), 2, 6, 6, 7, 64, None, 1, _vp(keep)) < 0     # in place
    assert lib.wca_test_kv_reorder(engine._h, _vp(a), _vp(b), 2, 6, 6, 7, 60, None, 1, _vp(keep)) < 0     # d % 8
    assert lib.wca_test_kv_reorder(engine._h, _vp(a), _vp(b), 2, 6, 6, 7, 64, None, 0, _vp(keep)) < 0     # no sources and no divisor
    assert lib.wca_test_kv_reorder(engine._h, _vp(a), _vp(b), 2, 6, 6, 7, 64, None, 1, None) < 0 and b"null" in lib.wca_last_error()
