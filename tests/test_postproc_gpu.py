"""The post-processing half of the batched alignment on logits we choose (run on the MI355X with `-m gpu`): wca_test_align_postproc runs
the functions wca_align_batch_enqueue runs behind its decoder -- metadata staging, head statistics on logits with the row (max, sum)
kept, top-k, the aggregation that re-materialises the selected heads, the ragged DTW -- and every output is compared with the float64
reference of tests/postproc_ref.py, with the step-by-step API, with the general head-statistics kernel, and with itself under padding,
recycled workspaces and another batch order. Every comparison runs over each utterance's own n_tok[b] x n_frames[b] corner."""
import ctypes as C

import numpy as np
import pytest
import torch

import postproc_ref as pr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(wca):
    # no weights: neither the hook nor the step-by-step calls need any, and they take L and H as arguments, not from the engine's model
    dims = wca.ModelDimensions(80, 1500, 128, 2, 2, 51865, 448, 128, 2, 2)
    m = wca.WhisperAMD(dims, device="cuda:0", max_batch=6, precision="f16", _register=False)
    m._bind_stream()
    return m


def _opts(eng, sc):
    return eng.make_opts(aggregation="topk" if sc["topk"] else "mean", topk=sc["topk"] if sc["topk"] else -1, w_colnorm=sc["weights"][0],
                         w_rownorm=sc["weights"][1], w_coverage=sc["weights"][2], sot_len=sc["sot_len"], medfilt_width=sc["w"],
                         qk_scale=sc["scale"])


def _run(eng, sc, qk=None, order=None):
    """The hook on the scene (or on `qk` in its place, or on its utterances in another order), cut to the corners: per utterance a dict of
    rowstats [LH][n][2], colnorm [LH][F], scores [LH], sel [k] or None, matrix [N][F], jump [n_tok_max] (whole row: zero past N)."""
    qk = torch.from_numpy(np.array(sc["qk"] if qk is None else qk))
    n_tok, n_frames = list(sc["n_tok"]), list(sc["n_frames"])
    if order is not None:
        qk, n_tok, n_frames = qk[list(order)], [n_tok[i] for i in order], [n_frames[i] for i in order]
    out = eng.align_postproc(qk.cuda(), n_tok, n_frames, _opts(eng, sc), pr.L, pr.H, n_frames_max=sc["n_frames_max"])
    res = []
    for b, (n, F) in enumerate(zip(n_tok, n_frames)):
        N = max(n - sc["sot_len"] - 1, 0)
        res.append({"rowstats": out["rowstats"][b, :, :n].copy(), "colnorm": out["colnorm"][b, :, :F].copy(), "scores": out["scores"][b].copy(),
                    "sel": out["sel"][b].copy() if out["sel"] is not None else None, "matrix": out["matrix"][b, :N, :F].copy(),
                    "jump": out["jump"][b].copy()})
    return res


def _same_bits(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        for key in x:
            if x[key] is None:
                assert y[key] is None
                continue
            assert x[key].shape == y[key].shape and x[key].tobytes() == y[key].tobytes(), (what, "utterance", i, key)


@pytest.fixture(scope="module")
def results(eng):
    """The hook's results per scene, computed once (no test changes them)."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _run(eng, pr.scene(name)[0])
        return cache[name]
    return get


# ------------------------------------------------------------------------------- a .. d: against float64
@pytest.mark.parametrize("name", pr.SCENE_NAMES)
def test_statistics_selection_matrix_and_jumps_against_float64(eng, results, name):
    """(a) row maximum == the fp32 product's maximum exactly, row sums and column norms within their measured bounds, scores within
    2e-5 * max(1, |s|); (b) the selection is the reference's at every position, planted ties in index order, -1 past L*H; (c) the matrix
    within rtol 2e-5 / atol 1e-7; (d) the jump frames are the oracle DTW's on the GPU's own matrix, zero from n_tok - sot_len - 1 on."""
    from oracle import timing_ref
    sc, ref = pr.scene(name)
    got = results(name)
    worst_sum = worst_cn = worst_sc = 0.0
    for b, (g, r) in enumerate(zip(got, ref)):
        n, F = sc["n_tok"][b], sc["n_frames"][b]
        assert g["rowstats"][..., 0].tobytes() == r["rowmax"].tobytes(), (b, "row maximum")
        worst_sum = max(worst_sum, float(np.max(np.abs(g["rowstats"][..., 1] - r["rowsum"]) / r["rowsum"])))
        worst_cn = max(worst_cn, float(np.max(np.abs(g["colnorm"] - r["colnorm"]) / r["colnorm"])))
        worst_sc = max(worst_sc, float(np.max(np.abs(g["scores"] - r["scores"]) / np.maximum(1.0, np.abs(r["scores"])))))
    print("postproc %s: worst relative deviation row sums %.3g, column norms %.3g, scores %.3g (seed tries %d)"
          % (name, worst_sum, worst_cn, worst_sc, sc["tries"]))
    assert worst_sum <= pr.ROWSUM_RTOL and worst_cn <= pr.COLNORM_RTOL and worst_sc <= pr.SCORE_RTOL
    for b, (g, r) in enumerate(zip(got, ref)):
        n, F = sc["n_tok"][b], sc["n_frames"][b]
        N = max(n - sc["sot_len"] - 1, 0)
        if sc["topk"]:
            assert list(g["sel"]) == list(r["sel"]), (b, "selection")
        np.testing.assert_allclose(g["matrix"], r["matrix"], rtol=pr.MATRIX_RTOL, atol=pr.MATRIX_ATOL, err_msg="utterance %d" % b)
        if N:
            ti, tj = timing_ref.dtw(-torch.from_numpy(g["matrix"]))
            jumps = np.pad(np.diff(ti), (1, 0), constant_values=1).astype(bool)
            assert np.array_equal(g["jump"][:N], tj[jumps]), (b, "jump frames")
        assert not g["jump"][N:].any(), (b, "jump row past the DTW rows")


def test_refusals(eng, lib):
    """n_frames_max above the 1536 frames of the widest head-statistics instance is refused (1500 is the model's limit), as are the
    lengths and options wca_align_batch_enqueue refuses; nothing is launched."""
    sc = pr.scene("f130_w1_top1")[0]
    qk = torch.zeros(1, pr.LH, 8, 1540).cuda()

    def refused(n_tok, n_frames, fmax, **kw):
        with pytest.raises(Exception):
            eng.align_postproc(kw.pop("qk", qk), n_tok, n_frames, _opts(eng, dict(sc, **kw)), pr.L, pr.H, n_frames_max=fmax)

    refused([8], [1500], 1537)
    refused([8], [1537], 1537)
    refused([9], [100], 100)            # n_tok above n_tok_max
    refused([8], [0], 100)
    refused([8], [100], 99)             # n_frames_max below an utterance's frames
    refused([8], [100], 1500, qk=qk[..., :1499].contiguous())   # ld below n_frames_max
    refused([8], [100], 100, w=4)
    refused([8], [100], 100, w=35)
    refused([8] * 7, [100] * 7, 100, qk=torch.zeros(7, pr.LH, 8, 100).cuda())   # above max_batch
    assert lib.wca_test_align_postproc(eng._h, None) < 0 and b"null" in lib.wca_last_error()
    out = eng.align_postproc(qk, [8], [1500], _opts(eng, sc), pr.L, pr.H, n_frames_max=1500)   # and the limit itself is taken
    assert np.isfinite(out["scores"]).all()


# ------------------------------------------------------------------------------- e: the two routes agree bit for bit
def _stepwise(eng, lib, wca, sc, b):
    """Utterance b alone through the step-by-step API: wca_attention_weights on its logit slice, then wca_filter_attention (scores; its
    head statistics leave the column norms) and wca_force_align on the dense maps."""
    n, F, ld = sc["n_tok"][b], sc["n_frames"][b], sc["ld"]
    o = _opts(eng, sc)
    qk = torch.from_numpy(np.array(sc["qk"][b, :, :n])).cuda().contiguous()
    ws = torch.empty(pr.LH, n, F, device="cuda", dtype=torch.float32)
    eng._bind_stream()
    vp = lambda t: C.c_void_p(t.data_ptr())
    pf, pi = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    wca._lib.check(lib.wca_attention_weights(eng._h, vp(qk), pr.L, pr.H, n, ld, F, sc["w"], sc["scale"], vp(ws)))
    scores = np.zeros(pr.LH, np.float32)
    wca._lib.check(lib.wca_filter_attention(eng._h, vp(ws), pr.L, pr.H, n, F, 1, *sc["weights"], scores.ctypes.data_as(pf), None, None))
    colnorm = np.zeros((pr.LH, F), np.float32)
    wca._lib.check(lib.wca_test_last_colnorm(eng._h, pr.LH * F, colnorm.ctypes.data_as(pf)))
    N = n - sc["sot_len"] - 1
    res = {"scores": scores, "colnorm": colnorm}
    if N >= 1:   # (wca_force_align refuses an utterance without DTW rows)
        mat = np.zeros((N, F), np.float32)
        ti, tj = np.zeros(N + F, np.int32), np.zeros(N + F, np.int32)
        plen = C.c_int32(0)
        k = max(sc["topk"], 1)
        sel, ssc = np.full(k, -1, np.int32), np.zeros(k, np.float32)
        wca._lib.check(lib.wca_force_align(eng._h, vp(ws), pr.L, pr.H, n, F, C.byref(o), mat.ctypes.data_as(pf), ti.ctypes.data_as(pi),
                                           tj.ctypes.data_as(pi), C.byref(plen), sel.ctypes.data_as(pi), ssc.ctypes.data_as(pf)))
        ti, tj = ti[:plen.value], tj[:plen.value]
        res.update(matrix=mat, sel=sel if sc["topk"] else None, jump=tj[np.pad(np.diff(ti), (1, 0), constant_values=1).astype(bool)])
    return res


@pytest.mark.parametrize("name", pr.SCENE_NAMES)
def test_batched_route_equals_the_stepwise_api_bit_for_bit(eng, lib, wca, results, name):
    """(e) Each utterance alone through wca_attention_weights -> wca_force_align on dense maps gives the hook's matrix, selected heads
    and path, and its scores and column norms, to the bit: the re-materialised weight is the value whose (max, sum) and column norms
    were stored, at qk_scale = 0.37 (inexact products) as at 1.0, and no reduction order depends on the batch."""
    sc, _ = pr.scene(name)
    got = results(name)
    for b, g in enumerate(got):
        s = _stepwise(eng, lib, wca, sc, b)
        N = max(sc["n_tok"][b] - sc["sot_len"] - 1, 0)
        assert s["scores"].tobytes() == g["scores"].tobytes(), (b, "scores")
        assert s["colnorm"].tobytes() == g["colnorm"].tobytes(), (b, "column norms")
        if N:
            if sc["topk"]:
                assert list(s["sel"]) == list(g["sel"]), (b, "selection")
            diff = np.abs(s["matrix"].astype(np.float64) - g["matrix"])
            assert s["matrix"].tobytes() == g["matrix"].tobytes(), (b, "matrix", "%d elements differ, worst %.3g" % ((diff > 0).sum(), diff.max()))
            assert np.array_equal(s["jump"], g["jump"][:N]), (b, "path")


# ------------------------------------------------------------------------------- f: lean against general on every output
@pytest.mark.parametrize("name", [s["name"] for s in pr.SPECS if s["w"] <= 9])
def test_lean_kernel_equals_general_on_every_output(eng, switch, results, name):
    """(f) head_stats_fast_kernel against head_stats_kernel: row statistics, column norms, scores, selection, matrix and jump frames."""
    sc, _ = pr.scene(name)
    switch("head_stats_general", 1)
    general = _run(eng, sc)
    switch("head_stats_general", 0)
    _same_bits(results(name), general, "lean vs general")


# ------------------------------------------------------------------------------- g: nothing outside a corner is read
@pytest.mark.parametrize("name", pr.SCENE_NAMES)
def test_nothing_outside_a_corner_is_read(eng, results, name):
    """(g) NaN in the pad columns [n_frames[b], ld) and the rows [n_tok[b], n_tok_max): every output is finite and has the bits of the
    run on a zero-filled copy (and of the run on the scene's own random padding)."""
    sc, _ = pr.scene(name)
    runs = []
    for fill in (np.nan, 0.0):
        qk = np.array(sc["qk"])
        for b, (n, F) in enumerate(zip(sc["n_tok"], sc["n_frames"])):
            qk[b, :, n:, :] = fill
            qk[b, :, :, F:] = fill
        runs.append(_run(eng, sc, qk=qk))
    for r in runs[0]:
        for key, v in r.items():
            assert v is None or np.isfinite(v).all(), key
    _same_bits(runs[0], runs[1], "NaN padding vs zero padding")
    _same_bits(runs[0], results(name), "NaN padding vs the scene's padding")


# ------------------------------------------------------------------------------- h: recycled workspaces
def test_recycled_workspaces(eng, results):
    """(h) A large batch, a small one, the large one again: each has the bits of its stand-alone result, and the small one's jump rows
    are zero beyond their DTW rows although the buffer held the large batch's frames."""
    big, small = "f1500_w11_top2", "f130_w1_top1"
    alone_big, alone_small = results(big), results(small)
    first = _run(eng, pr.scene(big)[0])
    mid = _run(eng, pr.scene(small)[0])
    again = _run(eng, pr.scene(big)[0])
    _same_bits(first, alone_big, "large, first")
    _same_bits(mid, alone_small, "small after large")
    _same_bits(again, alone_big, "large again")
    sc = pr.scene(small)[0]
    assert any(r["jump"].any() for r in first)
    for b, r in enumerate(mid):
        assert not r["jump"][max(sc["n_tok"][b] - sc["sot_len"] - 1, 0):].any()


# ------------------------------------------------------------------------------- i: batch position
@pytest.mark.parametrize("name", ["f1024_w5_top8", "f1025_w9_mean", "f513_w3_top6"])
def test_batch_position(eng, results, name):
    """(i) Permuting the utterances of a batch permutes every result, bit for bit."""
    sc, _ = pr.scene(name)
    B = len(sc["n_tok"])
    order = [(3 * i + 2) % B if B % 3 else (B - 1 - i) for i in range(B)]
    assert sorted(order) == list(range(B)) and order != list(range(B))
    got = _run(eng, sc, order=order)
    _same_bits(got, [results(name)[i] for i in order], "permuted batch")
