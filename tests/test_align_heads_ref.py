"""CPU checks of tests/align_heads_ref.py, the reference that tests/test_align_heads_gpu.py holds the alignment-heads kernels to: its float64
form is torch's softmax / std_mean(unbiased=False) and the oracle's median filter on every scene, no scene rests on 0 / 0, the float32
form's DTW jumps are the float64 form's on the planted-ridge scenes (so the GPU is only asked for what fp32 itself delivers), and the new
C ABI names are declared, bound and refuse null arguments without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import align_heads_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ar.SCENE_NAMES)
def test_float64_form_is_torch_and_the_oracle_filter(name):
    """softmax -> std_mean(unbiased=False) normalisation -> oracle median filter -> mean over the heads -> [sot_len:-1], in torch float64,
    equals the reference's float64 form; the row maximum is the fp32 product's."""
    from oracle import timing_ref
    sc, ref64, _ = ar.scene(name)
    for b, (n, F) in enumerate(zip(sc["n_tok"], sc["n_frames"])):
        x = torch.from_numpy(np.array(sc["qk"][b][list(sc["heads"]), :n, :F]))
        prod = (x * torch.tensor(sc["scale"], dtype=torch.float32)).float()
        assert np.array_equal(ref64[b]["rowmax"], prod.max(dim=-1).values.numpy())
        p = torch.softmax(prod.double(), dim=-1)
        std, mean = torch.std_mean(p, dim=-2, keepdim=True, unbiased=False)
        np.testing.assert_allclose(ref64[b]["mean"], mean[:, 0].numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(ref64[b]["std"], std[:, 0].numpy(), rtol=1e-9, atol=1e-300)
        if F == 1:
            assert np.isnan(ref64[b]["matrix"]).all()
            continue
        z = timing_ref.median_filter((p - mean) / std, sc["w"])
        matrix = z.mean(dim=0)[sc["sot_len"]:-1].numpy()
        np.testing.assert_allclose(ref64[b]["matrix"], matrix, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("name", ar.SCENE_NAMES)
def test_no_scene_rests_on_a_zero_std(name):
    """Every column of every utterance with F >= 2 keeps std >= STD_FLOOR * mean (build_scene asserts it; restated here on the shared
    scene), an F = 1 utterance has std == 0 and a NaN matrix, everything outside a corner is NaN, and the float32 form's distance from
    float64 is a finite, non-zero yardstick for the matrix."""
    sc, ref64, ref32 = ar.scene(name)
    for b, (n, F) in enumerate(zip(sc["n_tok"], sc["n_frames"])):
        assert np.isnan(sc["qk"][b, :, n:, :]).all() and np.isnan(sc["qk"][b, :, :, F:]).all() and np.isfinite(sc["qk"][b, :, :n, :F]).all()
        if F > 1:
            assert float((ref64[b]["std"] / ref64[b]["mean"]).min()) >= ar.STD_FLOOR
            assert np.isfinite(ref32[b]["matrix"]).all()
    d = sc["distance32"]
    assert all(np.isfinite(v) for v in d.values()) and 0 < d["matrix"] < 1e-2 and d["rowsum"] < 1e-5 and d["std"] < 1e-3, d


@pytest.mark.parametrize("name", ar.RIDGE_SCENES)
def test_float32_jumps_are_the_float64_jumps_on_the_ridge_scenes(name):
    sc, ref64, ref32 = ar.scene(name)
    for b, (n, F) in enumerate(zip(sc["n_tok"], sc["n_frames"])):
        if F == 1 or n - sc["sot_len"] - 1 < 1:
            continue
        j64, j32 = ar.jumps(ref64[b]["matrix"]), ar.jumps(ref32[b]["matrix"])
        assert np.array_equal(j64, j32), (b, j64, j32)
        assert len(set(j64.tolist())) > min(len(j64), F) // 2, (b, "the ridge spreads the rows over the frames")


def test_reference_notices_a_wrong_order_of_operations():
    """The reference's order (softmax, normalise, THEN filter) against the step-by-step route's (filter the logits first): the two differ by
    far more than the yardstick on a filtered scene, so the comparison can tell them apart."""
    sc, ref64, _ = ar.scene("ragged6_w7")
    b, n, F = 4, sc["n_tok"][4], sc["n_frames"][4]
    x = np.array(sc["qk"][b][list(sc["heads"]), :n, :F])
    wrong = ar.postproc(ar.median_reflect(x, sc["w"]), 1, sc["scale"], sc["sot_len"])
    assert np.max(np.abs(wrong["matrix"] - ref64[b]["matrix"])) > 1e3 * ar.BOUND_FACTOR * sc["distance32"]["matrix"]


def test_new_entry_points_are_declared_bound_and_refuse_null(wca):
    """wca_align_batch_enqueue_heads, wca_align_batch_heads, wca_test_align_heads_postproc: in the header, in the binding with the header's
    descriptor fields in the header's order, exported, and refused with a message that says `null` before any HIP call."""
    lib, L = wca._lib.load(), wca._lib
    header = open(os.path.join(ROOT, "include", "wca.h")).read()
    for name in ("wca_align_batch_enqueue_heads", "wca_align_batch_heads", "wca_test_align_heads_postproc"):
        assert name in header and name in L.SIGNATURES and hasattr(lib, name)
    body = re.search(r"typedef struct \{([^{}]*)\} wca_test_heads_postproc_desc;", header, flags=re.S).group(1)
    names = [n for decl in re.findall(r"([\w ,*]+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) for n in re.findall(r"(\w+)\s*(?:,|$)", decl)]
    assert names == [f[0] for f in L.HeadsPostprocDesc._fields_]
    assert lib.wca_version() >= 21
    ad, ar_, hd = L.AlignDesc(), L.AlignResult(), L.HeadsPostprocDesc()
    heads = (ctypes.c_int32 * 1)(0)
    for fn, args in ((lib.wca_align_batch_enqueue_heads, (None, None, None, 0)), (lib.wca_align_batch_enqueue_heads, (None, ctypes.byref(ad), heads, 1)),
                     (lib.wca_align_batch_heads, (None, None, None, 0, None)), (lib.wca_align_batch_heads, (None, ctypes.byref(ad), heads, 1, ctypes.byref(ar_))),
                     (lib.wca_test_align_heads_postproc, (None, None)), (lib.wca_test_align_heads_postproc, (None, ctypes.byref(hd)))):
        assert lib.wca_test_set_switch(b"no_such_switch", 1) < 0 and b"null" not in lib.wca_last_error()
        assert fn(*args) < 0 and b"null" in lib.wca_last_error(), fn.__name__
