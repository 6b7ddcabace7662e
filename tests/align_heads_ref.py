"""Reference, in plain numpy, of the alignment-heads post-processing of the batched alignment (csrc/align_heads.hip behind
wca_align_batch_enqueue_heads): openai-whisper's find_alignment on the captured logits of a ragged batch, over a fixed list of heads.
For utterance b, head s, its n rows and F frames:
  1. p = softmax_f(qk[:, :F] * scale)     the product with the fp32 scale ROUNDED to fp32 and its row maximum are DEFINED in fp32 (the
                                          kernels and this file agree to the bit); everything behind is float64 in `reference`
  2. z = (p - mean_t p) / std_t p         per frame over the n rows, population std, a plain division
  3. y = reflect-padded median of z over `w` frames; y = z where w <= 1 or F <= w // 2
  4. matrix = mean over the heads, in list order, of y[sot_len : n - 1]
`reference(scene)` is that in float64, `reference(scene, np.float32)` the same steps in float32 arithmetic: the float32 form's distance from
the float64 form (`distances`) is the yardstick the GPU is held to -- 8 x that distance on the same scene, the factor
tests/test_forward_widths_gpu.py grants the contract mode over its fp32 oracle -- because the division by std amplifies fp32 noise by a
factor that depends on the scene. tests/test_align_heads_ref.py checks this file against torch and the oracle; tests/test_align_heads_gpu.py
checks the kernels against it through wca_test_align_heads_postproc.

F = 1 is a case of its own: the softmax of one frame is 1 in every row, so mean = 1 and std = 0 exactly and every z is 0 / 0 = NaN, in
upstream as here (no guard). Such an utterance keeps its place in the batch: its row and column statistics and the NaN of its whole matrix
corner are compared, its jump frames (a DTW over NaN, which nobody defines) are not. Every other column of every scene keeps
std >= STD_FLOOR * mean (asserted by build_scene), so no other comparison rests on 0 / 0.
"""
import functools

import numpy as np

L, H = 2, 3
LH = L * H
STD_FLOOR = 1e-2      # std_f >= STD_FLOOR * mean_f in every column of every utterance with F >= 2
BOUND_FACTOR = 8.0    # the GPU may be this many float32-restatement distances away from float64


def median_reflect(x, w):
    """Sliding median of odd width w along the last axis with reflect padding; x unchanged when w <= 1 or F <= w // 2."""
    F = x.shape[-1]
    pad = w // 2
    if w <= 1 or F <= pad:
        return x
    xp = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(pad, pad)], mode="reflect")
    win = np.lib.stride_tricks.sliding_window_view(xp, w, axis=-1)
    return np.sort(win, axis=-1)[..., pad]


def postproc(x, w, scale, sot_len, dtype=np.float64):
    """x [S][n][F] fp32 logits of one utterance's corner, the selected heads in list order -> dict: rowmax [S][n] (fp32), rowsum [S][n],
    mean [S][F], std [S][F], matrix [max(n - sot_len - 1, 0)][F], all but rowmax in `dtype` arithmetic."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    S, n, F = x.shape
    prod = (x * np.float32(scale)).astype(np.float32)
    rowmax = prod.max(axis=-1)
    e = np.exp(prod.astype(dtype) - rowmax.astype(dtype)[..., None])
    rowsum = e.sum(axis=-1, dtype=dtype)
    p = e / rowsum[..., None]
    mean = p.sum(axis=-2, dtype=dtype) / dtype(n)
    d = p - mean[:, None, :]
    std = np.sqrt((d * d).sum(axis=-2, dtype=dtype) / dtype(n))
    with np.errstate(invalid="ignore", divide="ignore"):
        z = d / std[:, None, :]
    y = median_reflect(z, w)
    acc = np.zeros((n, F), dtype=dtype)
    for s in range(S):
        acc = acc + y[s]
    matrix = (acc / dtype(S))[sot_len:max(n - 1, sot_len)]
    return {"rowmax": rowmax, "rowsum": rowsum, "mean": mean, "std": std, "matrix": matrix}


def reference(scene, dtype=np.float64):
    """One postproc dict per utterance of the scene, on its own n_tok[b] x n_frames[b] corner of the heads scene["heads"]."""
    qk = scene["qk"]
    return [postproc(qk[b][list(scene["heads"]), :n, :F], scene["w"], scene["scale"], scene["sot_len"], dtype)
            for b, (n, F) in enumerate(zip(scene["n_tok"], scene["n_frames"]))]


def jumps(matrix):
    """The frames at which the oracle DTW's path on -matrix enters each text row ([N] ints)."""
    import torch
    from oracle import timing_ref
    ti, tj = timing_ref.dtw(-torch.from_numpy(np.ascontiguousarray(matrix, dtype=np.float64)))
    return tj[np.pad(np.diff(ti), (1, 0), constant_values=1).astype(bool)]


def distances(ref64, ref32):
    """The float32 restatement's distance from float64 over a scene: the largest relative deviation of the row sums, column means and
    column stds, and the largest absolute deviation of the matrix, over every utterance's corner (an F = 1 utterance's NaN matrix and
    zero std are compared for equality by the callers, not here)."""
    d = {"rowsum": 0.0, "mean": 0.0, "std": 0.0, "matrix": 0.0}

    def widen(key, dev):   # (np.max and np.maximum hand a NaN on, where Python's max(0.0, nan) would drop it: a NaN deviation stays NaN)
        d[key] = float(np.maximum(d[key], np.max(dev)))
    for a, b in zip(ref64, ref32):
        widen("rowsum", np.abs(b["rowsum"] - a["rowsum"]) / a["rowsum"])
        widen("mean", np.abs(b["mean"] - a["mean"]) / a["mean"])
        if a["mean"].shape[-1] == 1:
            continue
        widen("std", np.abs(b["std"] - a["std"]) / a["std"])
        if a["matrix"].size:
            widen("matrix", np.abs(b["matrix"] - a["matrix"]))
    return d


# ------------------------------------------------------------------------------------------------------------------ the scenes
def _fill(spec, seed):
    """Seeded logits [B][LH][n_tok_max][ld]: noise with a scale per head, plus (ridge > 0) a planted monotone ridge -- row t of every head
    is raised around frame (t + 0.5) F / n -- so that the DTW path is decided by the input, not by rounding. Everything outside an
    utterance's n_tok[b] x n_frames[b] corner is NaN: no result may depend on it."""
    rng = np.random.default_rng(seed)
    B = len(spec["n_tok"])
    qk = rng.standard_normal((B, LH, spec["n_tok_max"], spec["ld"])).astype(np.float32)
    qk *= (1.0 + 0.3 * np.arange(LH, dtype=np.float32))[None, :, None, None]
    for b, (n, F) in enumerate(zip(spec["n_tok"], spec["n_frames"])):
        if spec["ridge"] > 0 and n > 0:
            centre = (np.arange(n, dtype=np.float64)[:, None] + 0.5) * F / n
            width = max(1.0, 0.75 * F / n)
            bump = spec["ridge"] * np.exp(-0.5 * ((np.arange(F, dtype=np.float64)[None, :] - centre) / width) ** 2)
            qk[b, :, :n, :F] += bump.astype(np.float32)[None]
        qk[b, :, n:, :] = np.nan
        qk[b, :, :, F:] = np.nan
    return qk


def build_scene(spec):
    """The spec with its seeded logits, its float64 and float32 references and the float32 form's distances; asserts the std floor."""
    spec = dict(spec)
    assert spec["n_frames_max"] >= max(spec["n_frames"]) and spec["ld"] >= spec["n_frames_max"] and spec["n_tok_max"] >= max(spec["n_tok"])
    assert 1 <= len(spec["heads"]) <= LH and all(0 <= h < LH for h in spec["heads"])
    spec["qk"] = _fill(spec, spec["seed"])
    ref64, ref32 = reference(spec), reference(spec, np.float32)
    for b, r in enumerate(ref64):
        if spec["n_frames"][b] == 1:
            assert (r["std"] == 0).all() and np.isnan(r["matrix"]).all()
        else:
            assert (r["std"] >= STD_FLOOR * r["mean"]).all(), (spec["name"], b, float((r["std"] / r["mean"]).min()))
            assert np.isfinite(r["matrix"]).all()
    spec["distance32"] = distances(ref64, ref32)
    return spec, ref64, ref32


# name, filter width, fp32 scale, sot_len, the head list (flat indices, in summing order), ragged lengths, ridge height (0: noise only).
# Together: F in {1, 3 (<= pad at width 7), 4 (pad + 1), 63, 64, 65, 255, 256, 257, 1500 at ld 1500} and ld > F; n_tok in {sot_len + 3,
# odd mid sizes, 448} and on both sides of the column pass's rows-per-wave instances (64 | 65, 128 | 129, 256 | 257); F on both sides of
# the final pass's columns-per-lane instances (256 | 257, 512 | 513, 1024 | 1025); sot_len 3 and 1; S in {1, 3, every head}, lists that are
# not ascending; widths 1, 3, 7 and 33 (the largest check_medfilt takes); qk_scale 1.0 and 0.37; ld a multiple of 4 (16-byte loads) and not
# (the 4-byte form); one ragged batch of six at max_batch = 6.
SPECS = [
    dict(name="ragged6_w7", seed=11, w=7, scale=0.37, sot_len=3, heads=[4, 1, 5, 0, 3, 2], ridge=6.0, n_frames_max=65, ld=68, n_tok_max=41,
         n_frames=[1, 3, 4, 63, 64, 65], n_tok=[6, 41, 17, 6, 23, 9]),
    dict(name="f257_w3_sot1", seed=12, w=3, scale=1.0, sot_len=1, heads=[5, 2], ridge=6.0, n_frames_max=257, ld=260, n_tok_max=65,
         n_frames=[255, 256, 257, 64], n_tok=[23, 4, 65, 64]),
    dict(name="f130_w1", seed=13, w=1, scale=1.0, sot_len=3, heads=[3, 0, 4], ridge=6.0, n_frames_max=130, ld=132, n_tok_max=13,
         n_frames=[130, 64], n_tok=[13, 6]),
    dict(name="ld67_w5_noise", seed=14, w=5, scale=0.37, sot_len=3, heads=[2], ridge=0.0, n_frames_max=65, ld=67, n_tok_max=12,
         n_frames=[65, 33], n_tok=[9, 12]),
    dict(name="n129_f513_w7", seed=15, w=7, scale=0.37, sot_len=3, heads=[1, 0], ridge=6.0, n_frames_max=513, ld=516, n_tok_max=129,
         n_frames=[513, 512, 300], n_tok=[129, 65, 128]),
    dict(name="n257_f1025_w3", seed=16, w=3, scale=1.0, sot_len=3, heads=[4], ridge=6.0, n_frames_max=1025, ld=1028, n_tok_max=257,
         n_frames=[1025, 1024], n_tok=[257, 256]),
    dict(name="n448_f1500_w7", seed=17, w=7, scale=0.37, sot_len=3, heads=[3], ridge=6.0, n_frames_max=1500, ld=1500, n_tok_max=448,
         n_frames=[1500], n_tok=[448]),
    dict(name="f1500_w33_all", seed=18, w=33, scale=1.0, sot_len=3, heads=[0, 1, 2, 3, 4, 5], ridge=6.0, n_frames_max=1500, ld=1500,
         n_tok_max=21, n_frames=[1500, 16, 17], n_tok=[21, 7, 20]),
]
SCENE_NAMES = [s["name"] for s in SPECS]
RIDGE_SCENES = [s["name"] for s in SPECS if s["ridge"] > 0]


@functools.lru_cache(maxsize=None)
def scene(name):
    """(scene, float64 reference, float32 reference) of one of SPECS, built once and shared; callers leave all three unchanged."""
    sc, ref64, ref32 = build_scene(next(s for s in SPECS if s["name"] == name))
    sc["qk"].setflags(write=False)
    return sc, ref64, ref32
