"""The alignment-heads post-processing of the batched alignment on logits we choose (run on the MI355X with `-m gpu`):
wca_test_align_heads_postproc runs the functions wca_align_batch_enqueue_heads runs behind its decoder -- metadata staging, the three
passes of csrc/align_heads.hip, the ragged DTW -- and every output is compared with the float64 reference of tests/align_heads_ref.py
within 8 x the float32 restatement's own distance from float64 on the same scene, with the oracle DTW, with the single-utterance route at
width 1, and with itself under another batch order, recycled workspaces and other bytes outside the corners. Every comparison runs over
each utterance's own n_tok[b] x n_frames[b] corner; everything outside it is NaN in the scenes."""
import ctypes as C

import numpy as np
import pytest
import torch

import align_heads_ref as ar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(wca):
    # no weights: the hook and the step-by-step calls take L and H as arguments, not from the engine's model (the engine of test_postproc_gpu.py)
    dims = wca.ModelDimensions(80, 1500, 128, 2, 2, 51865, 448, 128, 2, 2)
    m = wca.WhisperAMD(dims, device="cuda:0", max_batch=6, precision="f16", _register=False)
    m._bind_stream()
    return m


def _opts(eng, sc):
    return eng.make_opts(sot_len=sc["sot_len"], medfilt_width=sc["w"], qk_scale=sc["scale"])


def _run(eng, sc, qk=None, order=None, heads=None):
    """The hook on the scene (or on `qk` in its place, or on its utterances in another order), cut to the corners: per utterance a dict of
    rowmax / rowsum [S][n], mean / std [S][F], matrix [N][F], jump [n_tok_max] (whole row: zero past N)."""
    qk = torch.from_numpy(np.array(sc["qk"] if qk is None else qk))
    n_tok, n_frames = list(sc["n_tok"]), list(sc["n_frames"])
    if order is not None:
        qk, n_tok, n_frames = qk[list(order)], [n_tok[i] for i in order], [n_frames[i] for i in order]
    out = eng.align_heads_postproc(qk.cuda(), n_tok, n_frames, _opts(eng, sc), ar.L, ar.H, sc["heads"] if heads is None else heads,
                                   n_frames_max=sc["n_frames_max"])
    res = []
    for b, (n, F) in enumerate(zip(n_tok, n_frames)):
        N = max(n - sc["sot_len"] - 1, 0)
        res.append({"rowmax": out["rowstats"][b, :, :n, 0].copy(), "rowsum": out["rowstats"][b, :, :n, 1].copy(),
                    "mean": out["colstats"][b, :, :F, 0].copy(), "std": out["colstats"][b, :, :F, 1].copy(),
                    "matrix": out["matrix"][b, :N, :F].copy(), "jump": out["jump"][b].copy()})
    return res


def _same_bits(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        for key in x:
            assert x[key].shape == y[key].shape and x[key].tobytes() == y[key].tobytes(), (what, "utterance", i, key)


@pytest.fixture(scope="module")
def results(eng):
    """The hook's results per scene, computed once (no test changes them)."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _run(eng, ar.scene(name)[0])
        return cache[name]
    return get


# ------------------------------------------------------------------------------- a .. d: against float64 and the oracle DTW
@pytest.mark.parametrize("name", ar.SCENE_NAMES)
def test_statistics_matrix_and_jumps_against_float64(eng, results, name):
    """(a) the row maximum is the fp32 product's maximum to the bit; row sums, column means and column stds (relative) and (b) the matrix
    (absolute) lie within BOUND_FACTOR = 8 float32-restatement distances of float64, over each utterance's corner; an F = 1 utterance
    has std == 0 and a NaN matrix, as defined; (c) the jump frames are the oracle DTW's on the GPU's own matrix, zero from
    n_tok - sot_len - 1 on; (d) on the planted-ridge scenes they are also the float64 reference's."""
    sc, ref64, _ = ar.scene(name)
    got = results(name)
    for b, (g, r) in enumerate(zip(got, ref64)):
        assert g["rowmax"].tobytes() == r["rowmax"].tobytes(), (b, "row maximum")
        if sc["n_frames"][b] == 1:
            assert (g["std"] == 0).all() and (g["mean"] == 1).all() and np.isnan(g["matrix"]).all(), (b, "F = 1")
        else:
            assert np.isfinite(g["matrix"]).all() and np.isfinite(g["std"]).all(), (b, "finite")
    for g in got:
        assert np.isfinite(g["rowsum"]).all() and np.isfinite(g["mean"]).all(), "row sums and column means are finite in every scene"
    dist, yard = ar.distances(ref64, got), sc["distance32"]
    ratios = {k: (dist[k] / (ar.BOUND_FACTOR * yard[k]) if yard[k] > 0 else float(dist[k] > 0)) for k in dist}
    print("align-heads %s: deviation from float64 / (8 x the float32 form's): row sums %.3g, column means %.3g, column stds %.3g, matrix %.3g"
          "  [float32 form: %.3g %.3g %.3g %.3g]" % (name, ratios["rowsum"], ratios["mean"], ratios["std"], ratios["matrix"], yard["rowsum"],
                                                     yard["mean"], yard["std"], yard["matrix"]))
    assert all(r <= 1.0 for r in ratios.values()), ratios   # (a NaN ratio fails)
    for b, (g, r) in enumerate(zip(got, ref64)):
        n, F = sc["n_tok"][b], sc["n_frames"][b]
        N = max(n - sc["sot_len"] - 1, 0)
        assert not g["jump"][N:].any(), (b, "jump row past the DTW rows")
        if N and F > 1:   # (F = 1: a DTW over NaN, which nobody defines)
            assert np.array_equal(g["jump"][:N], ar.jumps(g["matrix"])), (b, "jump frames against the oracle DTW on the GPU's matrix")
            if sc["ridge"] > 0:
                assert np.array_equal(g["jump"][:N], ar.jumps(r["matrix"])), (b, "jump frames against the float64 reference's")


# ------------------------------------------------------------------------------- e: bit-identical under what must not matter
@pytest.mark.parametrize("name", ["ragged6_w7", "f257_w3_sot1", "n129_f513_w7"])
def test_batch_order(eng, results, name):
    """(e1) Permuting the utterances of a batch permutes every result, bit for bit."""
    sc = ar.scene(name)[0]
    B = len(sc["n_tok"])
    order = [(B - 1 - i) for i in range(B)]
    _same_bits(_run(eng, sc, order=order), [results(name)[i] for i in order], "permuted batch")


def test_recycled_workspaces(eng, results):
    """(e2) A large scene, a small one, the large one again: each has the bits of its stand-alone result, and the small one's jump rows
    are zero beyond their DTW rows although the buffer held the large scene's frames."""
    big, small = "n448_f1500_w7", "f130_w1"
    alone_big, alone_small = results(big), results(small)
    first = _run(eng, ar.scene(big)[0])
    mid = _run(eng, ar.scene(small)[0])
    again = _run(eng, ar.scene(big)[0])
    _same_bits(first, alone_big, "large, first")
    _same_bits(mid, alone_small, "small after large")
    _same_bits(again, alone_big, "large again")
    sc = ar.scene(small)[0]
    assert any(r["jump"].any() for r in first)
    for b, r in enumerate(mid):
        assert not r["jump"][max(sc["n_tok"][b] - sc["sot_len"] - 1, 0):].any()


@pytest.mark.parametrize("name", ar.SCENE_NAMES)
def test_nothing_outside_a_corner_matters(eng, results, name):
    """(e3) The scenes hold NaN in the pad columns [n_frames[b], ld) and the rows [n_tok[b], n_tok_max), and noise in the heads that are not
    selected; zeros in all three places, and large finite values, give the same bits."""
    sc = ar.scene(name)[0]
    for fill in (0.0, 1.0e30):
        qk = np.array(sc["qk"])
        for b, (n, F) in enumerate(zip(sc["n_tok"], sc["n_frames"])):
            qk[b, :, n:, :] = fill
            qk[b, :, :, F:] = fill
            qk[b, [h for h in range(ar.LH) if h not in sc["heads"]]] = fill
        _same_bits(_run(eng, sc, qk=qk), results(name), "padding %g vs NaN padding" % fill)


def test_head_order_is_the_summing_order(eng, results):
    """The heads are summed in list order: the reversed list gives the reversed statistics to the bit and a matrix within the bound."""
    name = "ragged6_w7"
    sc, ref64, _ = ar.scene(name)
    rev = _run(eng, sc, heads=list(reversed(sc["heads"])))
    for g, r in zip(results(name), rev):
        for key in ("rowmax", "rowsum", "mean", "std"):
            assert g[key][::-1].tobytes() == r[key].tobytes(), key
    assert ar.distances(ref64, rev)["matrix"] <= ar.BOUND_FACTOR * sc["distance32"]["matrix"]


# ------------------------------------------------------------------------------- f: width 1 against the single-utterance route
def test_width_one_agrees_with_the_single_utterance_route(eng, lib, wca, results):
    """(f) At width 1 the filter drops out and the order of operations no longer matters: wca_attention_weights (width 1) and then
    wca_default_find_alignment, one utterance at a time, give the hook's matrix within the bound of (b) and its jump frames."""
    name = "f130_w1"
    sc, ref64, _ = ar.scene(name)
    got = results(name)
    bound = ar.BOUND_FACTOR * sc["distance32"]["matrix"]
    vp = lambda t: C.c_void_p(t.data_ptr())
    pf, pi = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    heads = np.ascontiguousarray(sc["heads"], dtype=np.int32)
    for b, (n, F) in enumerate(zip(sc["n_tok"], sc["n_frames"])):
        N = n - sc["sot_len"] - 1
        qk = torch.from_numpy(np.array(sc["qk"][b, :, :n])).cuda().contiguous()
        ws = torch.empty(ar.LH, n, F, device="cuda", dtype=torch.float32)
        eng._bind_stream()
        wca._lib.check(lib.wca_attention_weights(eng._h, vp(qk), ar.L, ar.H, n, sc["ld"], F, 1, sc["scale"], vp(ws)))
        mat = np.zeros((N, F), np.float32)
        ti, tj = np.zeros(N + F, np.int32), np.zeros(N + F, np.int32)
        plen = C.c_int32(0)
        wca._lib.check(lib.wca_default_find_alignment(eng._h, vp(ws), ar.L, ar.H, n, F, heads.ctypes.data_as(pi), len(heads), sc["sot_len"], None,
                                                      mat.ctypes.data_as(pf), ti.ctypes.data_as(pi), tj.ctypes.data_as(pi), C.byref(plen)))
        ti, tj = ti[:plen.value], tj[:plen.value]
        worst = float(np.max(np.abs(mat.astype(np.float64) - ref64[b]["matrix"])))
        apart = float(np.max(np.abs(got[b]["matrix"].astype(np.float64) - mat)))
        print("align-heads %s utterance %d: the hook's matrix and the single-utterance route's are %.3g apart, the latter %.3g from float64 "
              "(bound %.3g)" % (name, b, apart, worst, bound))
        assert np.isfinite(mat).all() and apart <= bound and worst <= bound
        assert np.array_equal(tj[np.pad(np.diff(ti), (1, 0), constant_values=1).astype(bool)], got[b]["jump"][:N])


# ------------------------------------------------------------------------------- g: refusals
def test_refusals(eng, lib, wca):
    """(g) A head out of range, an empty or over-long head list, a null descriptor and the lengths and widths wca_align_batch_enqueue
    refuses are refused by the hook; wca_align_batch_enqueue_heads refuses path_scores and open_end_host before anything is enqueued (the
    engine has no weights: a call that got past the checks would say so, not `path scores` / `open-ended`)."""
    sc = ar.scene("f130_w1")[0]
    qk = torch.zeros(1, ar.LH, 8, 100).cuda()

    def refused(what, heads, n_tok=(8,), n_frames=(100,), fmax=100, **kw):
        with pytest.raises(wca._lib.WcaError) as err:
            eng.align_heads_postproc(kw.pop("qk", qk), list(n_tok), list(n_frames), _opts(eng, dict(sc, **kw)), ar.L, ar.H, heads, n_frames_max=fmax)
        assert what in str(err.value), err.value

    refused("outside", [0, ar.LH])
    refused("outside", [-1])
    refused("empty", [])
    refused("alignment heads for a model", list(range(ar.LH)) + [0])
    refused("n_tok", [0], n_tok=(9,))
    refused("max_frames", [0], n_frames=(0,))
    refused("n_frames_max", [0], fmax=99)
    refused("ld", [0], fmax=101, n_frames=(100,))
    refused("median filter width", [0], w=4)
    refused("median filter width", [0], w=35)
    refused("batch", [0], n_tok=(8,) * 7, n_frames=(100,) * 7, qk=torch.zeros(7, ar.LH, 8, 100).cuda())
    assert lib.wca_test_align_heads_postproc(eng._h, None) < 0 and b"null" in lib.wca_last_error()
    out = eng.align_heads_postproc(torch.randn(1, ar.LH, 8, 100).cuda(), [8], [100], _opts(eng, sc), ar.L, ar.H, [ar.LH - 1])   # the limit is taken
    assert np.isfinite(out["matrix"][0, :4]).all()

    L_ = wca._lib
    tokens = torch.zeros(1, 8, dtype=torch.int64).cuda()
    nt, mf, oe, hd = L_.i32_array([8]), L_.i32_array([100]), L_.i32_array([0]), L_.i32_array([0])
    o = _opts(eng, sc)
    base = dict(pcm_dev=None, n_samples_host=None, tokens_dev=C.c_void_p(tokens.data_ptr()), n_tok_host=C.cast(nt, C.c_void_p),
                max_frames_host=C.cast(mf, C.c_void_p), opts=C.pointer(o), pcm_stride=0, n_tok_max=8, batch=1, vocab_end=0)
    for what, extra in ((b"path scores", dict(path_scores=1)), (b"open-ended", dict(open_end_host=C.cast(oe, C.c_void_p)))):
        d = L_.AlignDesc(**base, **extra)
        assert lib.wca_align_batch_enqueue_heads(eng._h, C.byref(d), hd, 1) < 0 and what in lib.wca_last_error(), lib.wca_last_error()
    d = L_.AlignDesc(**base)
    assert lib.wca_align_batch_enqueue_heads(eng._h, C.byref(d), L_.i32_array([4]), 1) < 0 and b"outside" in lib.wca_last_error()   # 2 x 2 heads
    assert lib.wca_align_batch_enqueue_heads(eng._h, C.byref(d), hd, 0) < 0 and b"empty" in lib.wca_last_error()
    with pytest.raises(ValueError):
        eng.align_batch(None, None, tokens, [8], [100], o, alignment_heads=[(0, 0)], path_scores=True)
    with pytest.raises(ValueError):
        eng.align_batch(None, None, tokens, [8], [100], o, alignment_heads=True, open_end=[False])
    with pytest.raises(ValueError):
        eng.align_batch(None, None, tokens, [8], [100], o, alignment_heads=[(2, 0)])
