"""`-m gpu`: the per-row score of the DTW path (csrc/path_score.hip) against its float64 restatement (tests/path_score_ref.py) on the oracle's
path -- cell counts exactly, means within the derived bound 2^-23 * sum|x| / cells -- through every layer that carries it: the step API
(wca_dtw_path_scores), the post-processing hook (wca_test_align_postproc_scores), the fused alignment (align_batch(path_scores=True)),
force_align_long(word_scores=True), transcribe(word_alignment_score=True) and infer_ali.py --word_alignment_score. Everything the calls
returned before is compared bit for bit with the call without the option. Each test prints the largest |mean - ref| / bound it saw."""
import ctypes as C
import glob
import importlib
import json
import os

import numpy as np
import pytest
import torch

import dtw_open_ref
import path_score_ref as ps
import postproc_ref as pr

pytestmark = pytest.mark.gpu

_pi = C.POINTER(C.c_int32)
_pf = C.POINTER(C.c_float)


def _m(n):
    return importlib.import_module("whisper-char-alignment_amd." + n)


@pytest.fixture(scope="module")
def eng():
    e = _m("engine").default_engine(0)
    e._bind_stream()
    return e


def _reference(corner, is_open):
    """(cells, mean, bound, jump, end_row) of one problem on the oracle's path: oracle.timing_ref.dtw for a closed problem,
    tests/dtw_open_ref.py for an open one."""
    if is_open:
        ti, tj, end = ps.open_path(corner)
    else:
        ti, tj = ps.closed_path(corner)
        end = corner.shape[0] - 1
    cells, _total, mean, abs_sum = ps.row_scores(corner, ti, tj)
    jump = np.full(corner.shape[0], -1, np.int32)
    for k in range(len(ti) - 1, -1, -1):
        jump[ti[k]] = tj[k]
    return cells, mean, ps.bound(cells, abs_sum), jump, end


def _worst_ratio(got_mean, ref_mean, bound):
    """The largest |mean - ref| / bound over the rows with cells; rows without must be exact and are asserted by the caller."""
    hit = bound > 0
    if not hit.any():
        return 0.0
    return float(np.max(np.abs(got_mean[hit].astype(np.float64) - ref_mean[hit].astype(np.float64)) / bound[hit]))


def _batch_open(eng, mats, n_rows, n_cols, flags):
    P, N, M = mats.shape
    md = torch.from_numpy(mats).cuda()
    jf, er = np.full((P, N), -9, np.int32), np.full(P, -9, np.int32)
    i32 = _m("_lib").i32_array
    _m("_lib").check(eng._lib.wca_dtw_batch_dev_open(eng._h, C.c_void_p(md.data_ptr()), P, N, M, i32(n_rows), i32(n_cols), i32(flags),
                                                     jf.ctypes.data_as(_pi), er.ctypes.data_as(_pi), None))
    return jf, er


def _check_launch(eng, name, mats, n_rows, n_cols, flags):
    """One wca_dtw_path_scores launch against wca_dtw_batch_dev_open (jump frames, end rows: bit for bit) and the reference (cells exactly,
    means within the bound, rows off the path exactly (0, 0.0)). Returns (jump, end_rows, mean, cells)."""
    mats = np.ascontiguousarray(mats, dtype=np.float32)
    P, N, M = mats.shape
    jump, end_rows, mean, cells = eng.dtw_path_scores(torch.from_numpy(mats).cuda(), n_rows, n_cols, flags)
    assert jump.shape == mean.shape == cells.shape == (P, N) and mean.dtype == np.float32 and cells.dtype == np.int32
    live = [p for p in range(P) if n_rows[p] >= 1 and n_cols[p] >= 1]   # (the older entry point refuses an empty problem)
    jf, er = _batch_open(eng, mats[live], [n_rows[p] for p in live], [n_cols[p] for p in live], [flags[p] for p in live])
    assert jump[live].tobytes() == jf.tobytes() and end_rows[live].tobytes() == er.tobytes(), name
    worst = 0.0
    for p in range(P):
        n, mm = n_rows[p], n_cols[p]
        if n < 1 or mm < 1:
            assert end_rows[p] == -1 and not cells[p].any() and not mean[p].any() and not jump[p].any(), (name, p)
            continue
        ref_cells, ref_mean, bound, ref_jump, end = _reference(mats[p, :n, :mm], flags[p])
        assert end_rows[p] == end and np.array_equal(jump[p, :n], ref_jump), (name, p, "the DTW itself")
        assert np.array_equal(cells[p, :n], ref_cells), (name, p, "cells", cells[p, :n], ref_cells)
        off = np.ones(N, bool)
        off[:end + 1] = False
        assert not cells[p, off].any() and mean[p, off].tobytes() == np.zeros(int(off.sum()), np.float32).tobytes(), (name, p, "rows off the path")
        ratio = _worst_ratio(mean[p, :n], ref_mean, bound)
        assert ratio <= 1.0, (name, p, ratio)
        worst = max(worst, ratio)
    print("path-score %s: largest |mean - ref| / bound = %.3g" % (name, worst))
    return jump, end_rows, mean, cells


def _scene(N, M, seed):
    """Four problems of N x M: values in [0, 1] closed, signed closed, a planted band (column-normalised, like the aggregated maps) open,
    signed open."""
    rng = np.random.default_rng(seed)
    mats = np.zeros((4, N, M), np.float32)
    mats[0] = rng.random((N, M), dtype=np.float32)
    mats[1] = rng.standard_normal((N, M)).astype(np.float32)
    mats[2] = dtw_open_ref.planted(N, M, (3 * N) // 5, seed=seed)
    mats[3] = rng.standard_normal((N, M)).astype(np.float32)
    return mats, [N] * 4, [M] * 4, [0, 0, 1, 1]


ROWS = [(1, 37), (2, 37), (64, 90), (65, 90), (512, 130)]
COLS = [(9, 1), (9, 2), (9, 16), (9, 17), (40, 1500)]
EDGES = [(65, 3), (1, 1500), (512, 2), (512, 1500)]


@pytest.mark.parametrize("N,M", ROWS + COLS + EDGES, ids=["%dx%d" % s for s in ROWS + COLS + EDGES])
def test_step_api_against_the_reference(eng, N, M):
    """N_max on both sides of the DTW's rows-per-lane instances and of the score kernel's 4 rows per workgroup, M on both sides of the
    16-column trace words and of the 64 lanes, one row of 1500 frames and 512 rows over two or three frames; open and closed problems,
    values in [0, 1] (every entry vertical) and signed (diagonal entries) in one launch."""
    _check_launch(eng, "%dx%d" % (N, M), *_scene(N, M, 1000 * N + M))


def test_ragged_launch_with_empty_and_single_row_problems(eng):
    rng = np.random.default_rng(12)
    P, N, M = 9, 70, 100
    n_rows = [70, 0, 1, 1, 64, 65, 33, 5, 70]
    n_cols = [100, 50, 100, 1, 17, 16, 0, 1, 63]
    flags = [1, 0, 1, 0, 0, 1, 1, 0, 0]
    mats = np.where(np.arange(P)[:, None, None] % 2 == 0, rng.random((P, N, M)), rng.standard_normal((P, N, M))).astype(np.float32)
    mats[0] = dtw_open_ref.planted(N, M, 30, seed=4)
    mats[1] = np.nan   # an empty problem is not read
    mats[6] = np.nan
    _jump, end_rows, _mean, cells = _check_launch(eng, "ragged", mats, n_rows, n_cols, flags)
    assert end_rows[0] == 30 and cells[0, :31].all() and not cells[0, 31:].any()
    assert cells[7, :5].tolist() == [1] * 5   # one frame shared by five rows: every entry vertical


def test_same_bits_at_every_batch_position_and_on_every_run(eng):
    rng = np.random.default_rng(3)
    N, M = 130, 700
    one = rng.standard_normal((N, M)).astype(np.float32)
    mats = rng.random((7, N, M), dtype=np.float32)
    mats[0] = mats[6] = one
    flags = [1, 0, 1, 0, 1, 0, 1]
    a = eng.dtw_path_scores(torch.from_numpy(mats).cuda(), [N] * 7, [M] * 7, flags)
    b = eng.dtw_path_scores(torch.from_numpy(mats).cuda(), [N] * 7, [M] * 7, flags)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
        assert x[0].tobytes() == x[6].tobytes()
    alone = eng.dtw_path_scores(torch.from_numpy(one[None]).cuda(), None, None, [1])
    for x, y in zip(a, alone):
        assert x[0].tobytes() == y[0].tobytes()
    closed = eng.dtw_path_scores(torch.from_numpy(one[None]).cuda())   # no flags: every problem closed
    assert closed[1][0] == N - 1 and closed[3][0].all()


def test_timing_path_scores_wrapper(eng):
    tm = _m("timing")
    m = np.random.default_rng(8).standard_normal((23, 60)).astype(np.float32)
    ti, tj = ps.closed_path(m)
    for arg in (m, torch.from_numpy(m), torch.from_numpy(m).cuda()):
        gi, gj, mean, cells = tm.path_scores(arg)
        assert np.array_equal(gi, ti) and np.array_equal(gj, tj) and gi.dtype == np.int64
        ref_cells, _t, ref_mean, abs_sum = ps.row_scores(m, ti, tj)
        assert np.array_equal(cells, ref_cells) and _worst_ratio(mean, ref_mean, ps.bound(ref_cells, abs_sum)) <= 1.0
    dropin = open(os.path.join(os.path.dirname(tm.__file__), "dropin", "timing.py")).read()
    assert "path_scores = _t.path_scores" in dropin


def test_step_api_refusals(eng, lib):
    md = torch.zeros(1, 4, 4).cuda()
    out, outf = np.zeros(4, np.int32), np.zeros(4, np.float32)
    i32 = _m("_lib").i32_array
    args = lambda N, rows: (eng._h, C.c_void_p(md.data_ptr()), 1, N, 4, i32(rows) if rows else None, None, None, out.ctypes.data_as(_pi),
                            out.ctypes.data_as(_pi), outf.ctypes.data_as(_pf), out.ctypes.data_as(_pi))
    assert lib.wca_dtw_path_scores(*args(513, None)) < 0
    assert lib.wca_dtw_path_scores(*args(4, [5])) < 0 and lib.wca_dtw_path_scores(*args(4, [-1])) < 0
    assert lib.wca_dtw_path_scores(*args(4, [4])[:10], None, None) < 0 and b"null" in lib.wca_last_error()
    assert lib.wca_dtw_path_scores(*args(4, [4])) == 0


# ------------------------------------------------------------------------------------------------ the post-processing hook
@pytest.fixture(scope="module")
def hook_eng(wca):
    dims = wca.ModelDimensions(80, 1500, 128, 2, 2, 51865, 448, 128, 2, 2)
    m = wca.WhisperAMD(dims, device="cuda:0", max_batch=6, precision="f16", _register=False)
    m._bind_stream()
    return m


def _hook(eng, sc, path_scores):
    o = eng.make_opts(aggregation="topk" if sc["topk"] else "mean", topk=sc["topk"] if sc["topk"] else -1, w_colnorm=sc["weights"][0],
                      w_rownorm=sc["weights"][1], w_coverage=sc["weights"][2], sot_len=sc["sot_len"], medfilt_width=sc["w"], qk_scale=sc["scale"])
    out = eng.align_postproc(torch.from_numpy(np.array(sc["qk"])).cuda(), list(sc["n_tok"]), list(sc["n_frames"]), o, pr.L, pr.H,
                             n_frames_max=sc["n_frames_max"], path_scores=path_scores)
    res = []
    for b, (n, F) in enumerate(zip(sc["n_tok"], sc["n_frames"])):   # only an utterance's own corner of an output is defined
        N = max(n - sc["sot_len"] - 1, 0)
        r = {"rowstats": out["rowstats"][b, :, :n], "colnorm": out["colnorm"][b, :, :F], "scores": out["scores"][b],
             "sel": out["sel"][b] if out["sel"] is not None else np.zeros(0), "matrix": out["matrix"][b, :N, :F], "jump": out["jump"][b]}
        if path_scores:
            r.update(path_mean=out["path_mean"][b], path_cells=out["path_cells"][b])
        res.append({k: np.ascontiguousarray(v) for k, v in r.items()})
    return res


@pytest.mark.parametrize("name", pr.SCENE_NAMES)
def test_postproc_hook_scores_and_everything_else_unchanged(hook_eng, name):
    """wca_test_align_postproc_scores: every output wca_test_align_postproc also gives has its bits; the scores are the reference's on
    the GPU's own matrix and the oracle path; the rows past an utterance's DTW rows (an utterance without any among them) are (0, 0.0)."""
    sc, _ = pr.scene(name)
    plain, got = _hook(hook_eng, sc, False), _hook(hook_eng, sc, True)
    worst = 0.0
    for b, (p, g) in enumerate(zip(plain, got)):
        for key in p:
            assert p[key].shape == g[key].shape and p[key].tobytes() == g[key].tobytes(), (name, b, key)
        N = max(sc["n_tok"][b] - sc["sot_len"] - 1, 0)
        assert not g["path_cells"][N:].any() and g["path_mean"][N:].tobytes() == np.zeros(len(g["path_mean"]) - N, np.float32).tobytes()
        if N:
            cells, mean, bound, jump, _end = _reference(g["matrix"], False)
            assert np.array_equal(g["jump"][:N], jump) and np.array_equal(g["path_cells"][:N], cells), (name, b)
            ratio = _worst_ratio(g["path_mean"][:N], mean, bound)
            assert ratio <= 1.0, (name, b, ratio)
            worst = max(worst, ratio)
    print("path-score postproc %s: largest |mean - ref| / bound = %.3g" % (name, worst))


def test_postproc_hook_refuses_null_outputs(hook_eng, lib):
    assert lib.wca_test_align_postproc_scores(hook_eng._h, None, None, None) < 0 and b"null" in lib.wca_last_error()


# ------------------------------------------------------------------------------------------------ the fused alignment
def _utt(tok, uid, n_samples, n_chars):
    syn, rt = _m("synthetic"), _m("retokenize")
    tt = rt.encode(syn.synth_text(uid, n_chars), tok, "char")
    return syn.synth_audio(uid, n_samples), tt, [*tok.sot_sequence, tok.no_timestamps, *tt, tok.eot]


def _batch(utts):
    eot = utts[0][2][-1]
    n_max, smax = max(len(u[2]) for u in utts), max(len(u[0]) for u in utts)
    pb = np.zeros((len(utts), smax), dtype=np.float32)
    tarr = np.full((len(utts), n_max), eot, dtype=np.int64)
    for i, (p, _tt, toks) in enumerate(utts):
        pb[i, :len(p)] = p
        tarr[i, :len(toks)] = toks
    return (torch.from_numpy(pb).cuda(), [len(u[0]) for u in utts], torch.from_numpy(tarr).cuda(), [len(u[2]) for u in utts],
            [len(u[0]) // 320 for u in utts])


@pytest.fixture(scope="module")
def small(wca):
    """The 256-wide 3 + 3-layer model of test_token_logprobs_gpu.py, a ragged batch of 3, contract mode."""
    dims = wca.ModelDimensions(80, 1500, 256, 4, 3, 51865, 448, 256, 4, 3)
    model = wca.WhisperAMD(dims, device="cuda:0", max_batch=3, precision="reference").load_state_dict(
        _m("synthetic").random_state_dict(dims, seed=5, cross_qk_std=0.08))
    tok = _m("tokenizer").get_tokenizer(True, language="English")
    utts = [_utt(tok, u, n, c) for u, n, c in [(31, 48000, 25), (32, 80000, 40), (33, 32000, 12)]]
    opts = model.make_opts(aggregation="topk", topk=4, sot_len=len(tok.sot_sequence), medfilt_width=3)
    return dict(model=model, tok=tok, utts=utts, batch=_batch(utts), opts=opts)


@pytest.fixture(scope="module")
def step_matrices(small):
    """wca_force_align's matrix of every row of the batch (the step-by-step route on the same engine), computed once."""
    model, tok, tm = small["model"], small["tok"], _m("timing")
    pcm, ns, tarr, n_tok, frames = small["batch"]
    w, _logits = model.get_attentions(model.log_mel(pcm, ns), tarr, frames, medfilt_width=3, n_tok=n_tok, want_logits=False)
    out = []
    for i, (_p, tt, _toks) in enumerate(small["utts"]):
        matrix = tm.force_align(w[i][:, :, :n_tok[i], :frames[i]].contiguous(), tt, tok, "char", "topk", topk=4)[3]
        out.append(np.ascontiguousarray(matrix.numpy()))
    return out


def _check_rows(name, small, step_matrices, jump, mean, cells, flags):
    worst = 0.0
    for i, m in enumerate(step_matrices):
        N = m.shape[0]
        ref_cells, ref_mean, bound, ref_jump, _end = _reference(m, flags[i])
        assert np.array_equal(jump[i, :N], ref_jump), (name, i, "jump frames")
        assert np.array_equal(cells[i, :N], ref_cells) and not cells[i, N:].any() and not mean[i, N:].any(), (name, i)
        ratio = _worst_ratio(mean[i, :N], ref_mean, bound)
        assert ratio <= 1.0, (name, i, ratio)
        worst = max(worst, ratio)
    print("path-score engine %s: largest |mean - ref| / bound = %.3g" % (name, worst))


def test_align_batch_scores_and_alignment_unchanged(small, step_matrices):
    model, tok, opts, args = small["model"], small["tok"], small["opts"], small["batch"]
    j0, s0 = model.align_batch(*args, opts)
    j1, s1, mean, cells = model.align_batch(*args, opts, path_scores=True)
    assert j0.tobytes() == j1.tobytes() and s0.tobytes() == s1.tobytes() and mean.shape == cells.shape == j0.shape
    _check_rows("closed", small, step_matrices, j1, mean, cells, [0, 0, 0])
    # open-end rows and token log-probs as well: every earlier value keeps its bits and its place, the scores come last
    flags = [False, True, True]
    base = model.align_batch(*args, opts, token_logprobs_vocab_end=tok.eot, open_end=flags)
    full = model.align_batch(*args, opts, token_logprobs_vocab_end=tok.eot, open_end=flags, path_scores=True)
    assert len(base) == 5 and len(full) == 7
    for x, y in zip(base, full):
        assert x.tobytes() == y.tobytes()
    _check_rows("open", small, step_matrices, full[0], full[5], full[6], flags)
    assert full[0][0].tobytes() == j0[0].tobytes() and full[5][0].tobytes() == mean[0].tobytes() and full[6][0].tobytes() == cells[0].tobytes()
    for i in (1, 2):   # rows past an open end row are off the path
        assert not full[6][i, full[3][i] + 1:].any()


def test_two_batches_in_flight_each_fetch_returns_its_own(small, wca, lib):
    model, opts, a = small["model"], small["opts"], small["batch"]
    b = _batch(small["utts"][1:])
    ja, sa, ma, ca = model.align_batch(*a, opts, path_scores=True)
    jb, sb = model.align_batch(*b, opts)
    model.align_batch(*a, opts, enqueue_only=True, path_scores=True)
    model.align_batch(*b, opts, enqueue_only=True)
    got = model.fetch(3, a[2].shape[1], opts, with_path_scores=True)
    for x, y in zip(got, (ja, sa, ma, ca)):
        assert x.tobytes() == y.tobytes()
    n_max = b[2].shape[1]
    mean, cells = np.full((2, n_max), 7, np.float32), np.full((2, n_max), 7, np.int32)
    assert lib.wca_align_batch_path_scores(model._h, 2, n_max, mean.ctypes.data_as(_pf), cells.ctypes.data_as(_pi)) == -4   # WCA_ERR_STATE
    assert (mean == 7).all() and (cells == 7).all()
    with pytest.raises(wca._lib.WcaError) as ei:
        model.fetch(2, n_max, opts, with_path_scores=True)
    assert ei.value.code == -4
    jb2, sb2 = model.fetch(2, n_max, opts)   # nothing was consumed by the refused calls
    assert jb2.tobytes() == jb.tobytes() and sb2.tobytes() == sb.tobytes()
    assert lib.wca_align_batch_path_scores(model._h, 2, n_max, mean.ctypes.data_as(_pf), cells.ctypes.data_as(_pi)) == -4   # nothing pending
    # the other order: the scores of the second batch are read after the first was fetched; reading twice consumes nothing
    model.align_batch(*b, opts, enqueue_only=True)
    model.align_batch(*a, opts, enqueue_only=True, path_scores=True)
    assert model.fetch(2, n_max, opts)[0].tobytes() == jb.tobytes()
    m2, c2 = np.zeros_like(ma), np.zeros_like(ca)
    for _ in range(2):
        assert lib.wca_align_batch_path_scores(model._h, 3, a[2].shape[1], m2.ctypes.data_as(_pf), c2.ctypes.data_as(_pi)) == 0
        assert m2.tobytes() == ma.tobytes() and c2.tobytes() == ca.tobytes()
    assert model.fetch(3, a[2].shape[1], opts)[0].tobytes() == ja.tobytes()


def test_recycled_workspaces(small):
    """A large batch, a small one, the large one again: each has the bits of its stand-alone result, and the small one's rows are zero
    past their DTW rows although the buffer held the large batch's scores."""
    model, opts, big = small["model"], small["opts"], small["batch"]
    little = _batch(small["utts"][2:])
    alone = model.align_batch(*little, opts, path_scores=True)
    first = model.align_batch(*big, opts, path_scores=True)
    mid = model.align_batch(*little, opts, path_scores=True)
    again = model.align_batch(*big, opts, path_scores=True)
    for x, y in zip(first, again):
        assert x.tobytes() == y.tobytes()
    for x, y in zip(alone, mid):
        assert x.tobytes() == y.tobytes()
    N = little[3][0] - 4
    assert mid[3][0, :N].all() and not mid[3][0, N:].any() and not mid[2][0, N:].any()
    # (reference mode: a row's PATH does not depend on the batch it rides in -- tests/test_batch_invariance_gpu.py; its matrix, and so
    # its means, may move in the last bit with the GEMM route the batch size selects)
    assert mid[0][0, :N + 1].tobytes() == first[0][2, :N + 1].tobytes() and mid[3][0, :N].tobytes() == first[3][2, :N].tobytes()
    np.testing.assert_allclose(mid[2][0, :N], first[2][2, :N], rtol=1e-5)


# ------------------------------------------------------------------------------------------------ the top layers
@pytest.fixture(scope="module")
def planted(wca):
    """The planted-ridge checkpoint of test_align_long_gpu.py: DTW row r peaks at encoder frame 5 r."""
    dims = wca.ModelDimensions(80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)
    m = wca.WhisperAMD(dims, device="cuda:0", max_batch=4, precision="f16")
    m.load_state_dict(_m("synthetic").aligned_state_dict(dims, seed=5, frames_per_token=5.0))
    return m


class _Recorder:
    """Wraps model.align_batch: keeps every call's token rows and results."""

    def __init__(self, model):
        self.model, self.inner, self.calls = model, model.align_batch, []
        model.align_batch = self

    def __call__(self, pcm, n_samples, tokens, n_tok, *rest, **kw):
        res = self.inner(pcm, n_samples, tokens, n_tok, *rest, **kw)
        self.calls.append((tokens.cpu().numpy(), list(n_tok), kw, res))
        return res

    def close(self):
        del self.model.align_batch


def _in_range(s):
    return s != s or 0.0 <= s <= 1.0 + 1e-6


def test_force_align_long_word_scores(planted, fake_vocab):
    al, tm = _m("align_long"), _m("timing")
    tok = _m("tokenizer").get_tokenizer(True, language="en", vocab_path=fake_vocab)
    text = _m("synthetic").synth_text(7, 340)   # 34 s of text in 40 s of audio: an open window, then a closed one
    pcm = _m("synthetic").synth_audio(2, 40 * 16000)
    kw = dict(language="en", aligned_unit_type="char", aggr="topk", topk=4, medfilt_width=3, vocab_path=fake_vocab)
    plain = al.force_align_long(planted, pcm, text, **kw)
    rec = _Recorder(planted)
    try:
        out = al.force_align_long(planted, pcm, text, word_scores=True, **kw)
    finally:
        rec.close()
    assert all(set(w) == {"word", "start", "end"} for w in plain["words"]) and all("mean_word_score" not in w for w in plain["windows"])
    strip = lambda r: dict(r, words=[{k: v for k, v in w.items() if k != "score"} for w in r["words"]],
                           windows=[{k: v for k, v in w.items() if k != "mean_word_score"} for w in r["windows"]])
    assert strip(out) == plain and len(out["windows"]) == len(rec.calls) >= 2 and out["unaligned_words"] == 0
    k = 0
    for win, (tokens, n_tok, call_kw, res) in zip(out["windows"], rec.calls):
        assert call_kw.get("path_scores") is True and len(res) == 6
        run = [int(t) for t in tokens[0, 4:n_tok[0] - 1]]
        want = tm.word_alignment_scores(res[4][0], res[5][0], run, tok, "char")[:win["committed"]]
        got = [w["score"] for w in out["words"][k:k + win["committed"]]]
        assert got == want and all(_in_range(s) for s in got) and len(got) == win["committed"] > 0
        assert win["mean_word_score"] == pytest.approx(float(np.mean([s for s in got if s == s])), abs=1e-12)
        k += win["committed"]
    assert k == len(out["words"])
    # the planted ridge: above the level of heads that do not tell a word's units from any other token, 1 / sqrt(n_tok) of the
    # smallest window (a column of equal entries has that value after the division by its L2 norm)
    chance = max(1.0 / np.sqrt(min(n_tok[0] for _t, n_tok, _k, _r in rec.calls)), 0.0)
    assert np.nanmean([w["score"] for w in out["words"]]) > chance
    print("path-score force_align_long: %d words, mean score %.3f" % (k, np.nanmean([w["score"] for w in out["words"]])))


def test_transcribe_word_alignment_score(planted, fake_vocab):
    tr, decoding, tm, rt = _m("transcribe"), _m("decoding"), _m("timing"), _m("retokenize")
    tk = _m("tokenizer").get_tokenizer(True, language="en", task="transcribe", vocab_path=fake_vocab)
    pcm = torch.from_numpy(_m("synthetic").synth_audio(5, 16000 * 38))
    ts = tk.timestamp_begin
    script = [[ts, *tk.encode(" hello tiny world again"), ts + 700], [ts, *tk.encode(" some more words"), ts + 300]]

    def run(**kw):
        calls = []

        def decode_window(mel_window, prompt):
            real = decoding.decode(planted, mel_window, decoding.DecodingOptions(language="en", prompt=list(prompt) or None, vocab_path=fake_vocab,
                                                                                 sample_len=4))
            calls.append(1)
            return decoding.DecodingResult(language="en", tokens=list(script[len(calls) - 1]), text="", avg_logprob=real.avg_logprob,
                                           no_speech_prob=real.no_speech_prob, temperature=0.0, compression_ratio=1.0)
        return tr.transcribe(planted, pcm, language="en", vocab_path=fake_vocab, word_timestamps=True, no_speech_threshold=None, topk=4,
                             decode_window=decode_window, **kw)

    plain = run()
    rec = _Recorder(planted)
    try:
        out = run(word_alignment_score=True)
    finally:
        rec.close()
    words0 = [w for seg in plain["segments"] for w in seg["words"]]
    words1 = [w for seg in out["segments"] for w in seg["words"]]
    assert len(words0) == len(words1) >= 5 and all(set(w) == {"word", "start", "end", "probability"} for w in words0)
    assert [{k: v for k, v in w.items() if k != "alignment_score"} for w in words1] == words0
    want = []
    for tokens, n_tok, call_kw, res in rec.calls:
        assert call_kw.get("path_scores") is True and len(res) == 4
        want += tm.word_alignment_scores(res[2][0], res[3][0], [int(t) for t in tokens[0, 4:n_tok[0] - 1]], tk, "char")
    got = [w["alignment_score"] for w in words1]
    assert got == want and all(_in_range(s) for s in got)
    with pytest.raises(ValueError):
        tr.transcribe(planted, pcm, language="en", vocab_path=fake_vocab, word_alignment_score=True)


def test_cli_word_alignment_score(tmp_path, wca):
    """infer_ali.py --word_alignment_score (the helper pattern of test_cli_gpu.py / test_token_logprobs_gpu.py): the records gain
    word_align_scores_hat, the result JSON mean_word_align_score, and nothing else moves."""
    import joblib
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    pcm = np.load(os.path.join(gold, "sample_pcm_int16.npy"))
    words = "the quick brown fox jumps over the lazy dog".split()
    lines = []
    for u in range(3):
        x = np.roll(pcm, 1000 * u)[: len(pcm) - 2000 * u]
        head = ("NIST_1A\n   1024\nsample_count -i %d\nsample_rate -i 16000\nchannel_count -i 1\nsample_n_bytes -i 2\n"
                "sample_byte_format -s2 01\nsample_coding -s3 pcm\nend_head\n" % len(x)).encode()
        wav = tmp_path / ("utt%d.wav" % u)
        wav.write_bytes(head + b" " * (1024 - len(head)) + x.astype("<i2").tobytes())
        w = words[: 9 - 2 * u]
        step = len(x) // (len(w) + 1)
        (tmp_path / ("utt%d.wrd" % u)).write_text("".join("%d %d %s\n" % (i * step, (i + 1) * step, t) for i, t in enumerate(w)))
        lines.append("utt%d %s\n" % (u, wav))
    scp = tmp_path / "test.scp"
    scp.write_text("".join(lines))
    infer, tm = _m("infer_ali"), _m("timing")
    dims = wca.dims_for("tiny")
    model = wca.WhisperAMD(dims, device="cuda:0", max_batch=2).load_state_dict(_m("synthetic").random_state_dict(dims, seed=0))
    model.use_official_alignment_heads("tiny")
    argv = ["--model", "tiny", "--random_init", "--dataset", "TIMIT", "--scp", str(scp), "--aggr", "topk", "--topk", "5",
            "--aligned_unit_type", "char", "--medfilt_width", "3", "--batch_size", "2", "--save_prediction", "--teacher", "text"]
    recs, res = {}, {}
    for flag in (False, True):
        out = tmp_path / ("out%d" % flag)
        infer.infer_dataset(infer.parse_args(argv + ["--output_dir", str(out)] + (["--word_alignment_score"] if flag else [])), model=model)
        res[flag] = json.load(open(glob.glob(str(out / "*.json"))[0]))
        recs[flag] = joblib.load(glob.glob(str(out / "*-predictions.pkl"))[0])
    base = {"starts", "ends", "texts", "starts_hat", "ends_hat", "predwords", "fids"}
    assert set(res[True]) - set(res[False]) == {"mean_word_align_score", "word_alignment_score"}
    tok = _m("tokenizer").get_tokenizer(True, language="English")
    opts = model.make_opts(aggregation="topk", topk=5, sot_len=3, medfilt_width=3)
    ds = infer.DATASET["TIMIT"](str(scp), n_mels=80, device="cuda:0", model=model, compute_mel=False)
    every = []
    for n, p in recs[True].items():
        assert set(recs[False][n]) == base and set(p) == base | {"word_align_scores_hat"}
        assert np.array_equal(p["ends_hat"], recs[False][n]["ends_hat"]) and np.array_equal(p["starts_hat"], recs[False][n]["starts_hat"])
        assert len(p["word_align_scores_hat"]) == len(p["ends_hat"]) > 0 and all(0.0 <= v <= 1.0 + 1e-6 for v in p["word_align_scores_hat"])
        every += list(p["word_align_scores_hat"])
        x, duration, _texts, _s, _e, _f = ds.read(n)
        tt = _m("retokenize").encode(" ".join(p["texts"]), tok, "char")
        toks = [*tok.sot_sequence, tok.no_timestamps, *tt, tok.eot]
        xb = torch.from_numpy(np.asarray(x, dtype=np.float32)[None]).cuda()
        jump, _sel, mean, cells = model.align_batch(xb, [xb.shape[1]], torch.tensor([toks]).cuda(), [len(toks)], [duration // 320], opts,
                                                    path_scores=True)
        # (the contract mode: a row's result does not depend on the batch it rides in)
        assert np.array_equal(tm.words_from_jump_frames(jump[0], tt, tok, "char")[2], p["ends_hat"])
        np.testing.assert_allclose(p["word_align_scores_hat"], tm.word_alignment_scores(mean[0], cells[0], tt, tok, "char"), rtol=1e-5)
    assert res[True]["mean_word_align_score"] == pytest.approx(float(np.mean(every)), rel=1e-9)
