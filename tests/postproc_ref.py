"""Float64 reference, in plain numpy, of the post-processing half of the batched alignment (csrc/postproc.hip behind
wca_align_batch_enqueue): head statistics on the captured logits of a ragged batch, top-k, the aggregation of the selected heads and
the row range handed to the DTW. Independent of oracle/timing_ref.py and of the kernels; tests/test_postproc_ref.py checks it against
the oracle on uniform shapes, tests/test_postproc_gpu.py checks the kernels against it through wca_test_align_postproc.

What is DEFINED in fp32 (the kernels and this file agree to the bit): the reflect-padded median over the utterance's own F = n_frames[b]
(skipped when w <= 1 or F <= w // 2; a median is one of its inputs), the product with the fp32 scale rounded to fp32, and the row maximum
of those products. Everything behind it is float64 here: softmax, row sums, column norms, scores, the aggregated matrix.

Bounds (relative to the float64 value, over every utterance's own corner):
  scores     2e-5 * max(1, |s|)   the project's bound for a head score (tests/test_kernels_gpu.py::test_filter_attention)
  matrix     rtol 2e-5, atol 1e-7 the project's bound for the aggregated matrix (test_force_align_matrix_and_path)
  row sums   ROWSUM_RTOL  = 6e-7  measured on the MI355X over SPECS: worst 1.46e-7 (scene f1025_w9_mean); x 4, one significant digit up
  col norms  COLNORM_RTOL = 2e-6  measured on the MI355X over SPECS: worst 4.36e-7 (scene f130_w1_top1); x 4, one significant digit up
Both stay below 2e-5: a score is a sum of column norms and must itself meet 2e-5. (Measured with them, not bounds of their own: the
scores deviate by at most 4.0e-6 of max(1, |s|), scene f1024_w5_top8.)
"""
import functools

import numpy as np

SCORE_RTOL = 2e-5
MATRIX_RTOL, MATRIX_ATOL = 2e-5, 1e-7
ROWSUM_RTOL = 6e-7    # 4 x the measured 1.46e-7
COLNORM_RTOL = 2e-6   # 4 x the measured 4.36e-7
GAP_FACTOR = 10.0     # consecutive reference scores of an utterance differ by at least GAP_FACTOR score bounds (planted ties apart)

L, H = 2, 3
LH = L * H


def score_bound(s):
    return SCORE_RTOL * max(1.0, abs(float(s)))


# ------------------------------------------------------------------------------------------------------------------ the operations
def median_reflect(x, w):
    """Sliding median of odd width w along the last axis with reflect padding; x unchanged when w <= 1 or F <= w // 2."""
    F = x.shape[-1]
    pad = w // 2
    if w <= 1 or F <= pad:
        return x
    xp = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(pad, pad)], mode="reflect")
    win = np.lib.stride_tricks.sliding_window_view(xp, w, axis=-1)
    return np.sort(win, axis=-1)[..., pad]


def head_stats(x, w, scale, weights, scale_first=False):
    """x [LH][n][F] fp32 logits of one utterance's corner -> dict: prod (fp32), rowmax (fp32), rowsum, A, colnorm, scores (float64)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    s32 = np.float32(scale)
    if scale_first:   # (mutation) scale, then filter
        prod = median_reflect((x * s32).astype(np.float32), w)
    else:
        prod = (median_reflect(x, w) * s32).astype(np.float32)
    rowmax = prod.max(axis=-1)
    with np.errstate(invalid="ignore"):
        e = np.exp(prod.astype(np.float64) - rowmax.astype(np.float64)[..., None])
    rowsum = e.sum(axis=-1)
    A = e / rowsum[..., None]
    colnorm = np.sqrt((A * A).sum(axis=-2))
    rownorm = np.sqrt((A * A).sum(axis=-1))
    w_col, w_row, w_cov = weights
    F = x.shape[-1]
    scores = np.zeros(x.shape[0], dtype=np.float64)
    if w_col > 0:
        scores += w_col * colnorm.sum(axis=-1)
    if w_row > 0:
        scores += w_row * rownorm.sum(axis=-1)
    if w_cov > 0:
        scores -= w_cov * (np.maximum(A.sum(axis=-2), 0.5).sum(axis=-1) - 0.5 * F)
    return {"prod": prod, "rowmax": rowmax, "rowsum": rowsum, "A": A, "colnorm": colnorm, "scores": scores}


def topk_ascending(scores, k):
    """The last k of the heads sorted by (score, index) tuples, ascending; -1 past the number of heads."""
    order = [i for _, i in sorted((float(s), i) for i, s in enumerate(scores))]
    keff = min(k, len(order))
    return np.array(order[len(order) - keff:] + [-1] * (k - keff), dtype=np.int32)


def aggregate(A, colnorm, heads, cnt, row_lo, row_hi):
    """mean over `heads` of A / ||A||_col, rows [row_lo, row_hi); cnt = what the sum is divided by"""
    acc = np.zeros(A.shape[1:], dtype=np.float64)
    for hd in heads:
        acc += A[hd] / colnorm[hd][None, :]
    return (acc / cnt)[row_lo:max(row_hi, row_lo)]


MUTATIONS = ("reflect_at_fmax", "neighbour_colnorm", "row_trim", "stats_ntokmax", "head_lo", "cnt", "scale_then_median")


def reference(scene, mut=None):
    """Per utterance: rowmax [LH][n] fp32, rowsum [LH][n], colnorm [LH][F], scores [LH], sel [k] (top-k) or None, heads, matrix
    [n - sot_len - 1][F]. mut: one of MUTATIONS, a deliberately wrong variant (tests/test_postproc_ref.py shows that the comparison
    would notice it)."""
    assert mut is None or mut in MUTATIONS
    qk, o = scene["qk"], scene
    B = len(o["n_tok"])
    stats = []
    for b in range(B):
        n, F = o["n_tok"][b], o["n_frames"][b]
        rows = o["n_tok_max"] if mut == "stats_ntokmax" else n
        if mut == "reflect_at_fmax":   # the filter sees the columns of the longest utterance, the softmax the utterance's own
            full = median_reflect(qk[b, :, :rows, :o["n_frames_max"]], o["w"])[..., :F]
            st = head_stats(full, 1, o["scale"], o["weights"])
        else:
            st = head_stats(qk[b, :, :rows, :F], o["w"], o["scale"], o["weights"], scale_first=(mut == "scale_then_median"))
        stats.append(st)
    out = []
    for b in range(B):
        n, st = o["n_tok"][b], stats[b]
        cn = stats[(b + 1) % B]["colnorm"] if mut == "neighbour_colnorm" else st["colnorm"]
        F = o["n_frames"][b]
        if cn.shape[-1] < F:
            cn = np.concatenate([cn, np.ones((LH, F - cn.shape[-1]))], axis=-1)
        cn = cn[:, :F]
        if o["topk"] > 0:
            sel = topk_ascending(st["scores"], o["topk"])
            heads = [int(h) for h in sel if h >= 0]
            cnt = o["topk"] if mut == "cnt" else len(heads)
        else:
            sel = None
            lo = (L // 2 - 1 if mut == "head_lo" else L // 2) * H
            heads = list(range(lo, LH))
            cnt = len(heads)
        row_lo = o["sot_len"] + (1 if mut == "row_trim" else 0)
        out.append({"rowmax": st["rowmax"][:, :n], "rowsum": st["rowsum"][:, :n], "colnorm": st["colnorm"], "scores": st["scores"], "sel": sel,
                    "heads": heads, "matrix": aggregate(st["A"][:, :n], cn, heads, cnt, row_lo, n - 1)})
    return out


# ------------------------------------------------------------------------------------------------------------------ the scenes
def planted_ties(scene, b):
    """The pairs of heads of utterance b whose scores tie exactly on purpose: every pair when F = 1 (all weights are 1), the twins of the
    twin utterance."""
    if scene["n_frames"][b] == 1:
        return {frozenset((i, j)) for i in range(LH) for j in range(i)}
    if scene.get("twin") is not None and scene["twin"][0] == b:
        return {frozenset(scene["twin"][1:])}
    return set()


def gaps_ok(scene, ref):
    """Every pair of consecutive reference scores of every utterance: exactly equal if planted, else GAP_FACTOR score bounds apart."""
    for b, r in enumerate(ref):
        ties = planted_ties(scene, b)
        order = sorted((float(s), i) for i, s in enumerate(r["scores"]))
        for (s0, i0), (s1, i1) in zip(order, order[1:]):
            if frozenset((i0, i1)) in ties:
                if s0 != s1:
                    return False
            elif s1 - s0 < GAP_FACTOR * score_bound(s1):
                return False
    return True


def _fill(spec, seed):
    rng = np.random.default_rng(seed)
    B = len(spec["n_tok"])
    qk = rng.standard_normal((B, LH, spec["n_tok_max"], spec["ld"])).astype(np.float32)
    qk *= (1.0 + 0.6 * np.arange(LH, dtype=np.float32))[None, :, None, None]   # a logit scale per head: the scores separate
    if spec.get("twin") is not None:
        b, h0, h1 = spec["twin"]
        qk[b, h1] = qk[b, h0]
    for b, hd, t, f0, f1, val in spec.get("plant", ()):   # columns [f0, f1) of one row set to val (-inf, an outlier)
        qk[b, hd, t, f0:f1] = val
    return qk


def build_scene(spec, max_tries=200):
    """The spec with seeded logits qk [B][LH][n_tok_max][ld]: re-seeded until gaps_ok holds, so that the selection is decided by the
    inputs at every position (a condition on the inputs; no position is left out of the comparison)."""
    spec = dict(spec)
    assert spec["n_frames_max"] >= max(spec["n_frames"]) and spec["ld"] >= spec["n_frames_max"] and spec["n_tok_max"] >= max(spec["n_tok"])
    for k in range(max_tries):
        spec["seed"] = spec["seed0"] + 1000 * k
        spec["qk"] = _fill(spec, spec["seed"])
        ref = reference(spec)
        if gaps_ok(spec, ref):
            spec["tries"] = k + 1
            return spec, ref
    raise AssertionError("no seed separates the scores of scene %s" % spec["name"])


NEG_INF = float("-inf")
# name, filter width, fp32 scale, score weights, topk (0 = mean), ragged lengths. Together: n_frames_max on both sides of the kernels'
# values-per-lane instances (512 | 513, 1024 | 1025) and 1500; n_frames in {1, 2, w // 2, w // 2 + 1, 63, 64, 65, n_frames_max};
# n_tok = sot_len + 1 (no DTW rows), sot_len + 2, every residue mod 4, n_tok_max; ld == n_frames_max and ld padded past it;
# widths 1, 3, 5, 7, 9 and 11 (general kernel, generic median); topk below, at and above L*H, and the mean; -inf and 1e4 plants.
SPECS = [
    dict(name="f512_w7_top3", seed0=1, w=7, scale=0.37, weights=(1.0, 1.0, 0.0), topk=3, sot_len=3, n_frames_max=512, ld=512, n_tok_max=40,
         n_frames=[512, 1, 2, 3, 4, 64], n_tok=[40, 4, 5, 17, 18, 19]),
    dict(name="f513_w3_top6", seed0=2, w=3, scale=1.0, weights=(1.0, 1.0, 1.0), topk=6, sot_len=3, n_frames_max=513, ld=516, n_tok_max=38,
         n_frames=[513, 63, 65, 1, 2, 300], n_tok=[7, 38, 12, 4, 5, 22], twin=(5, 1, 4)),
    dict(name="f1024_w5_top8", seed0=3, w=5, scale=0.37, weights=(1.0, 1.0, 1.0), topk=8, sot_len=3, n_frames_max=1024, ld=1024, n_tok_max=40,
         n_frames=[1024, 2, 3, 64, 700], n_tok=[6, 40, 9, 4, 23],
         plant=((4, 1, 5, 10, 11, NEG_INF), (4, 1, 6, 100, 103, NEG_INF), (4, 2, 7, 350, 353, 1.0e4), (3, 0, 2, 5, 6, 1.0e4))),
    dict(name="f1025_w9_mean", seed0=4, w=9, scale=0.37, weights=(1.0, 1.0, 0.0), topk=0, sot_len=3, n_frames_max=1025, ld=1028, n_tok_max=30,
         n_frames=[1025, 4, 5, 63, 1], n_tok=[8, 11, 5, 30, 14]),
    dict(name="f1500_w11_top2", seed0=5, w=11, scale=0.37, weights=(1.0, 1.0, 0.0), topk=2, sot_len=3, n_frames_max=1500, ld=1500, n_tok_max=21,
         n_frames=[1500, 5, 6, 65], n_tok=[10, 5, 4, 21]),
    dict(name="f130_w1_top1", seed0=6, w=1, scale=1.0, weights=(1.0, 1.0, 1.0), topk=1, sot_len=2, n_frames_max=130, ld=132, n_tok_max=13,
         n_frames=[130, 64, 1], n_tok=[13, 5, 4], plant=((0, 3, 4, 20, 21, NEG_INF), (0, 5, 9, 77, 78, 1.0e4), (1, 2, 1, 63, 64, 1.0e4))),
]
SCENE_NAMES = [s["name"] for s in SPECS]


@functools.lru_cache(maxsize=None)
def scene(name):
    """(scene, reference) of one of SPECS, built once and shared; callers leave both unchanged."""
    sc, ref = build_scene(next(s for s in SPECS if s["name"] == name))
    sc["qk"].setflags(write=False)
    return sc, ref
