"""CPU checks of tests/postproc_ref.py, the float64 reference that tests/test_postproc_gpu.py holds the post-processing kernels to: it
reproduces the oracle on uniform shapes, the scenes it builds separate their scores, and the comparison the GPU file makes would notice
each of the ways such a kernel goes wrong on a ragged batch."""
import numpy as np
import pytest
import torch

import postproc_ref as pr
from oracle import timing_ref


def _uniform(n, F, w, scale, weights, topk, seed, sot_len=3):
    spec = dict(name="uniform", seed0=seed, w=w, scale=scale, weights=weights, topk=topk, sot_len=sot_len, n_frames_max=F, ld=F + 3, n_tok_max=n,
                n_frames=[F], n_tok=[n])
    return pr.build_scene(spec)


@pytest.mark.parametrize("n,F,w,scale,weights,topk", [(12, 50, 7, 1.0, (1.0, 1.0, 0.0), 3), (9, 130, 3, 0.37, (1.0, 1.0, 1.0), 6),
                                                     (6, 3, 9, 0.37, (1.0, 0.0, 0.0), 8), (20, 65, 1, 1.0, (0.0, 1.0, 1.0), 0),
                                                     (7, 40, 11, 0.37, (1.0, 1.0, 0.0), 0)])
def test_reference_reproduces_the_oracle_on_uniform_shapes(n, F, w, scale, weights, topk):
    """One utterance, every head of the same shape: the oracle's fp32 torch pipeline (median filter, softmax, filter_attention, aggregate)
    against the float64 numpy one, within fp32 noise; the selection is the same list."""
    sc, ref = _uniform(n, F, w, scale, weights, topk, seed=n + F)
    r = ref[0]
    qk = torch.from_numpy(sc["qk"][0].reshape(pr.L, pr.H, n, sc["ld"]).copy())
    A = timing_ref.attention_weights(qk, F, w, scale)
    st = pr.head_stats(sc["qk"][0][:, :, :F], w, scale, weights)
    np.testing.assert_allclose(A.reshape(pr.LH, n, F).numpy(), st["A"], rtol=1e-5, atol=1e-9)
    full = timing_ref.filter_attention(A, pr.LH, *weights)[1]
    for s, (l, h), _ in full:
        assert abs(s - r["scores"][l * pr.H + h]) <= pr.score_bound(s)
    matrix, scores = timing_ref.aggregate(A, "topk" if topk else "mean", topk, *weights)
    np.testing.assert_allclose(matrix[sc["sot_len"]:-1].numpy(), r["matrix"], rtol=pr.MATRIX_RTOL, atol=pr.MATRIX_ATOL)
    if topk:
        want = [l * pr.H + h for _, (l, h), _ in scores]
        assert list(r["sel"]) == want + [-1] * (topk - len(want))


@pytest.mark.parametrize("name", pr.SCENE_NAMES)
def test_scene_scores_are_separated(name):
    """The condition the selection assertion of the GPU file rests on, for every scene it uses: consecutive reference scores are ten score
    bounds apart, the planted ties are exact; and the scene holds what it says (lengths inside the buffers, plants in place)."""
    sc, ref = pr.scene(name)
    assert pr.gaps_ok(sc, ref)
    for b, r in enumerate(ref):
        n, F = sc["n_tok"][b], sc["n_frames"][b]
        assert r["rowmax"].shape == (pr.LH, n) and r["colnorm"].shape == (pr.LH, F) and r["matrix"].shape == (max(n - sc["sot_len"] - 1, 0), F)
        assert np.isfinite(r["matrix"]).all() and np.isfinite(r["scores"]).all() and (r["colnorm"] > 0).all()
        if F == 1:
            assert len(set(r["scores"].tolist())) == 1
    if sc.get("twin") is not None:
        b, h0, h1 = sc["twin"]
        assert ref[b]["scores"][h0] == ref[b]["scores"][h1] and len(set(ref[b]["scores"].tolist())) == pr.LH - 1


def test_scenes_cover_the_required_shapes():
    scs = [pr.scene(n)[0] for n in pr.SCENE_NAMES]
    assert {512, 513, 1024, 1025, 1500} <= {s["n_frames_max"] for s in scs}
    assert {1, 3, 5, 7, 9, 11} == {s["w"] for s in scs} and {1.0, 0.37} == {s["scale"] for s in scs}
    assert {(1.0, 1.0, 0.0), (1.0, 1.0, 1.0)} == {s["weights"] for s in scs}
    ks = {s["topk"] for s in scs}
    assert 0 in ks and pr.LH in ks and any(0 < k < pr.LH for k in ks) and any(k > pr.LH for k in ks)
    assert any(s["ld"] == s["n_frames_max"] for s in scs) and any(s["ld"] > s["n_frames_max"] and s["ld"] % 4 == 0 for s in scs)
    frames = {(f if f != s["n_frames_max"] else "max") for s in scs for f in s["n_frames"]}
    assert {1, 2, 63, 64, 65, "max"} <= frames
    for s in scs:
        if s["w"] > 1:
            assert {s["w"] // 2, s["w"] // 2 + 1} <= set(s["n_frames"]), s["name"]
        assert len(s["n_tok"]) <= 6 and s["n_tok_max"] <= 40 and s["n_tok_max"] in s["n_tok"]
    toks = [(n, s["sot_len"]) for s in scs for n in s["n_tok"]]
    assert any(n == sl + 1 for n, sl in toks) and any(n == sl + 2 for n, sl in toks) and {n % 4 for n, _ in toks} == {0, 1, 2, 3}
    plants = [p[-1] for s in scs for p in s.get("plant", ())]
    assert float("-inf") in plants and 1.0e4 in plants


def _moved(sc, ref, mut):
    """What the GPU file's comparison would see between the reference and its mutation `mut`: the largest deviation of each compared
    quantity in units of its bound, and whether a selected head changed."""
    bad = pr.reference(sc, mut)
    worst, sel_changed = 0.0, False
    for r, m in zip(ref, bad):
        worst = max(worst, float(np.max(np.abs(m["scores"] - r["scores"]) / [pr.score_bound(s) for s in r["scores"]])))
        worst = max(worst, float(np.max(np.abs(m["colnorm"] - r["colnorm"]) / (pr.COLNORM_RTOL * r["colnorm"]))))
        rows = min(len(m["rowsum"][0]), len(r["rowsum"][0]))
        if rows:
            worst = max(worst, float(np.max(np.abs(m["rowsum"][:, :rows] - r["rowsum"][:, :rows]) / (pr.ROWSUM_RTOL * r["rowsum"][:, :rows]))))
            if not np.array_equal(m["rowmax"][:, :rows], r["rowmax"][:, :rows]):
                worst = np.inf
        N = min(len(m["matrix"]), len(r["matrix"]))
        if N:
            worst = max(worst, float(np.max(np.abs(m["matrix"][:N] - r["matrix"][:N]) / (pr.MATRIX_ATOL + pr.MATRIX_RTOL * np.abs(r["matrix"][:N])))))
        if r["sel"] is not None and list(r["sel"]) != list(m["sel"]):
            sel_changed = True
    return worst, sel_changed


@pytest.mark.parametrize("mut,name", [("reflect_at_fmax", "f512_w7_top3"), ("neighbour_colnorm", "f513_w3_top6"), ("row_trim", "f1025_w9_mean"),
                                      ("stats_ntokmax", "f1024_w5_top8"), ("head_lo", "f1025_w9_mean"), ("cnt", "f1024_w5_top8")])
def test_mutations_are_noticed(mut, name):
    """Each way a ragged post-processing kernel goes wrong -- the filter reflecting at n_frames_max instead of n_frames[b], a neighbouring
    utterance's column norms, the row range off by one, statistics over n_tok_max rows, the mean's first head off by one layer, the
    head count not reduced when topk > L*H -- moves a compared quantity by at least ten bounds, or changes a selected head."""
    sc, ref = pr.scene(name)
    worst, sel_changed = _moved(sc, ref, mut)
    assert worst >= 10.0 or sel_changed, (mut, worst)


def test_scaling_before_the_median_is_the_same_function():
    """The seventh candidate, a median taken after the scaling with a NEGATIVE scale, is not a defect a test can see: the filter widths are
    odd, and for an odd window rounding(x * s) is monotone in x (non-increasing for s < 0), so the middle element stays the middle one and
    median(round(x s)) == round(median(x) s) to the bit -- reflect padding included. Shown here on a ragged scene instead of assumed."""
    spec = dict(next(s for s in pr.SPECS if s["name"] == "f512_w7_top3"), scale=-0.37, name="negative_scale")
    sc, ref = pr.build_scene(spec)
    bad = pr.reference(sc, "scale_then_median")
    for r, m in zip(ref, bad):
        for key in ("rowmax", "rowsum", "colnorm", "scores", "matrix"):
            assert r[key].tobytes() == m[key].tobytes(), key


def test_hook_is_declared_bound_and_refuses_null_without_a_gpu(wca):
    """wca_test_align_postproc: the ctypes descriptor has the header's fields in the header's order, and no engine / no descriptor are
    refused before any HIP call."""
    import ctypes
    import os
    import re
    lib, L = wca._lib.load(), wca._lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wca.h")).read()
    body = re.search(r"typedef struct \{([^{}]*)\} wca_test_postproc_desc;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in L.PostprocDesc._fields_]
    assert ctypes.sizeof(L.PostprocDesc) == 11 * 8 + 6 * 4
    d = L.PostprocDesc()
    for args in ((None, None), (None, ctypes.byref(d))):
        assert lib.wca_test_set_switch(b"no_such_switch", 1) < 0 and b"null" not in lib.wca_last_error()
        assert lib.wca_test_align_postproc(*args) < 0 and b"null" in lib.wca_last_error()
    assert lib.wca_test_last_colnorm(None, 1, None) < 0 and b"null" in lib.wca_last_error()
