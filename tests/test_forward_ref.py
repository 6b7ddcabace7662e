"""tests/forward_ref.py without a GPU: (a) the float64 restatement of the forward agrees with the fp32 oracle to fp32 noise, (b) the census of
the GEMM plans of a forward at the five Whisper widths -- the batches next to which a site's kernel, split, grid form or fused-LayerNorm
eligibility changes, from which tests/test_forward_widths_gpu.py takes its cases -- holds the kernel switches derived by hand from
csrc/gemm_plan.cpp, and (c) every forward-level wiring mutation of the reference moves an asserted observable by at least 10 of its bounds."""
import importlib

import numpy as np
import pytest
import torch

import forward_ref as fr


def _mods():
    return (importlib.import_module("whisper-char-alignment_amd.synthetic"), importlib.import_module("whisper-char-alignment_amd.audio"))


@pytest.fixture(scope="module")
def small(wca):
    """The 128-wide 2 + 2 layer model on two distinct utterances: inputs, the float64 observables, the fp32 oracle's and the f16-operand
    statement's distances from them. Computed once; no test changes it."""
    from oracle import whisper_ref
    syn, audio = _mods()
    dims = fr.model_dims(wca, 128)
    sd = fr.model_state_dict(dims, seed=3)
    filt = audio.mel_filters(80)
    mel = torch.stack([whisper_ref.log_mel_spectrogram(whisper_ref.pad_or_trim(torch.from_numpy(syn.synth_audio(700 + b, n))), filt)
                       for b, n in enumerate((48000, 400000))])    # 3 s and 25 s: the two utterances differ in most frames
    tokens = torch.randint(0, 50257, (2, 12), generator=torch.Generator().manual_seed(5))
    ref = fr.observables(fr.ForwardRef(sd, dims).forward(mel, tokens))
    w = whisper_ref.WhisperRef(sd, dims)
    enc32 = w.encoder(mel)
    logits32, qk32 = w.decoder(tokens, enc32)
    d32 = fr.distance(fr.observables({"enc": enc32, "qk": qk32, "logits": logits32}), ref)
    d16 = fr.distance(fr.observables(fr.ForwardRef(sd, dims, f16_operands=True).forward(mel, tokens)), ref)
    return {"dims": dims, "sd": sd, "mel": mel, "tokens": tokens, "ref": ref, "d32": d32, "d16": d16}


def test_restatement_agrees_with_the_fp32_oracle(small):
    """(a) fp32 noise: a few 1e-7 on LayerNorm-ed outputs of order 1; the bound is 20 fp32 spacings at 1 (2.4e-6) for the encoder output and
    the logits (relative to the largest) and 1e-7 for the maps, whose values are below 0.02 here."""
    d = small["d32"]
    print("float64 restatement against WhisperRef (fp32), 128 wide, B = 2: encoder %.3g, maps %.3g, logits %.3g rel" %
          (d["enc"][0], d["maps"][0], d["logits"][0]))
    assert small["ref"]["maps"].max().item() < 0.02
    assert d["enc"][0] < 2.4e-6 and d["logits"][0] < 2.4e-6 and d["maps"][0] < 1e-7
    # and the f16-operand statement is the same forward with roundings: orders of magnitude further away, nowhere near wrong
    f = small["d16"]
    print("f16-operand statement against float64: encoder %.3g (mean %.3g), maps %.3g, logits %.3g rel" % (f["enc"][0], f["enc"][1], f["maps"][0], f["logits"][0]))
    assert 20 * d["enc"][0] < f["enc"][0] < 5e-3 and 20 * d["logits"][0] < f["logits"][0] < 5e-3


# ------------------------------------------------------------------------------------------------------------------ (b) the census
# derived by hand from gemm_plan.cpp (a site leaves the 128 x 128 kernel where it has 192 tiles of 256 x 256; M = 1500 B, conv1 3000 B)
HAND_KERNEL_SWITCH = {384: {"fc1": 6, "qkv": 7, "conv1": 9, "out": 17, "fc2": 17, "conv2": 17},
                      512: {"fc1": 4, "qkv": 6, "conv1": 9, "out": 17, "fc2": 17, "conv2": 17},
                      768: {"fc1": 3, "qkv": 4, "conv1": 6, "out": 11, "fc2": 11, "conv2": 11},
                      1024: {"fc1": 2, "qkv": 3, "conv1": 5, "out": 9, "fc2": 9, "conv2": 9},
                      1280: {"fc1": 2, "qkv": 3, "conv1": 4, "out": 7, "fc2": 7, "conv2": 7}}
HAND_FC2_SPLITK_ENDS = {384: None, 512: 3, 768: 2, 1024: 2, 1280: 2}     # the first batch without split-K; 384: K = 1536 never splits
# ... on single operands. The plan corrected the list for pair operands: below the pair kernel's threshold fc2 is the [W | W] call with
# K = 8 d >= 2048, so the 384-wide model splits too, while d / 128 x ceil(1500 B / 128) tiles stay within 128: B = 1 .. 3
HAND_FC2_SPLITK_ENDS_PAIR = {384: 4, 512: 3, 768: 2, 1024: 2, 1280: 2}


@pytest.mark.parametrize("d", fr.WIDTHS)
def test_plan_census(lib, d):
    """(b) every GEMM site of the forward, asked of plan_gemm / plan_dec_gemm with the arguments engine_forward.hip gives it, B = 1 .. 20,
    pair and single operands. The GPU cases are fr.case_batches(lib, d): both sides of every switch up to the width's largest batch."""
    changes = fr.census(lib, d, fr.TOKEN_COUNTS)
    b_max = fr.b_max(lib, d)
    print("width %d: switch batches %s, run up to B = %d: %s" % (d, sorted(changes), b_max, fr.case_batches(lib, d)))
    for B in sorted(changes):
        for (mode, site), (before, after) in sorted(changes[B].items()):
            print("   B = %2d  %-8s %-14s %s -> %s" % (B, mode, site, " ".join(map(str, before)), " ".join(map(str, after))))
    for pair in (False, True):
        plans = {B: fr.site_plans(lib, d, B, 40, pair) for B in range(1, 21)}
        for site, first in HAND_KERNEL_SWITCH[d].items():
            got = min(B for B in plans if plans[B][site][1] != "t128")
            assert got == first, (d, site, pair, got, first)
            assert all(plans[B][site][1] == "t128" for B in range(1, first)) and all(plans[B][site][1] != "t128" for B in range(first, 21))
            assert first in changes and first <= b_max
        # pair operands: the SPLITW kernel from the switch on, the [W | W] call before it; the conv stem is K-doubled throughout
        if pair:
            for site in ("qkv", "fc1", "out", "fc2", "cross_kv"):
                assert {plans[B][site][0] for B in plans if plans[B][site][1] == "t128"} <= {"doubled"}
                assert {plans[B][site][:2] for B in plans if plans[B][site][1] != "t128"} == {("pair", "pair3")}
            assert {plans[B][s][0] for B in plans for s in ("conv1", "conv2")} == {"doubled"}
        else:   # the fused residual + LayerNorm form exists exactly where the site has left the 128 x 128 kernel and N is whole tiles
            for site in ("out", "fc2"):
                for B in plans:
                    assert (plans[B][site][4] == "fusable") == (plans[B][site][1] != "t128" and d % 256 == 0), (d, site, B)
        ends = (HAND_FC2_SPLITK_ENDS_PAIR if pair else HAND_FC2_SPLITK_ENDS)[d]
        splits = [B for B in plans if plans[B]["fc2"][2] > 1]
        assert splits == (list(range(1, ends)) if ends else []), (d, pair, splits)
        # the out-projection has K >= 2048 only as the [W | W] call of the two widest models, at one utterance
        assert [B for B in plans if plans[B]["out"][2] > 1] == ([1] if pair and d >= 1024 else []), (d, pair)
    # the decoder at M = B n: the few-row kernel up to 128 rows in the f16 mode, both sides of it among the cases of every width
    batches = fr.case_batches(lib, d)
    rows = [B * n for B in batches for n in fr.TOKEN_COUNTS]
    assert min(rows) <= fr.DEC_ROWS_MAX < max(rows)
    for B in batches:
        for n in fr.TOKEN_COUNTS:
            p = fr.site_plans(lib, d, B, n, False)
            # (the projections fed by a LayerNorm stay separate launches at 384 and 1280: gemm_rows_supported)
            assert all((p[s][1] == "rows") == (B * n <= fr.DEC_ROWS_MAX) for s in ("dec_out", "dec_co", "dec_fc2")), (d, B, n)
    # every switch batch of the census is run on both sides; only the ceilings of 17 (384 / 512 wide) and 7 (1280 wide) cut it
    ceiling = fr.B_CEILING.get(d, fr.CENSUS_B)
    assert batches == sorted({b for S in changes if S <= ceiling for b in (S - 1, S)}) and max(batches) == b_max
    assert fr.B_CEILING == {384: 17, 512: 17, 1280: 7} and (d in fr.B_CEILING or max(changes) == b_max)
    # ... so that out / fc2 run as one tile per workgroup AND as the tile walk wherever the ceiling allows: 768 (B = 15) and 1024 (B = 11)
    if d in (768, 1024):
        for pair in (False, True):
            forms = {fr.site_plans(lib, d, B, 40, pair)[s][3] for B in batches for s in ("out", "fc2")}
            assert forms == {"one", "walk"}, (d, pair, forms)


# ------------------------------------------------------------------------------------------------------------------ the batched route's rows
def _grid(N, F, path):
    M = np.zeros((N, F))
    for i, j in path:
        M[i, j] = 1.0
    return M


def test_jump_decisions_on_small_matrices():
    """The rule that says which jump frames hang on more than the bounds (fr.jump_decisions), on matrices small enough to enumerate: a path
    of ones in near-zeros is decided at every row and is the oracle DTW's; on 3 x 5 matrices every monotone path is enumerated and the
    rule's verdict compared with the direct statement of it."""
    from oracle import timing_ref
    path = [(0, 0), (0, 1), (1, 2), (2, 2), (2, 3), (3, 4), (3, 5)]
    M = _grid(4, 6, path) - 0.5 + 0.01 * np.random.default_rng(0).random((4, 6))       # (a cell off the path costs: no detour pays)
    jump, decided = fr.jump_decisions(M, 2e-5, 1e-7)
    ti, tj = timing_ref.dtw(-torch.from_numpy(M))
    assert jump.tolist() == [0, 2, 2, 4] == tj[np.pad(np.diff(ti), (1, 0), constant_values=1).astype(bool)].tolist() and decided.all()
    # brute force on random 3 x 5 matrices with entries on a coarse grid plus noise of the bound's size (near-ties are frequent): a row is
    # decided exactly when no competing path reaches the float64 path on the matrix within eps that favours it the most
    rng = np.random.default_rng(1)

    def paths(i, j, N, F):
        if (i, j) == (N - 1, F - 1):
            yield [(i, j)]
            return
        for di, dj in ((0, 1), (1, 0), (1, 1)):
            if i + di < N and j + dj < F:
                for rest in paths(i + di, j + dj, N, F):
                    yield [(i, j)] + rest
    all_paths = list(paths(0, 0, 3, 5))
    seen = {True: 0, False: 0}
    for _ in range(200):
        M = rng.integers(0, 4, (3, 5)) * 0.25 + rng.uniform(-3e-5, 3e-5, (3, 5))
        rtol, atol = 2e-5, 1e-7
        jump, decided = fr.jump_decisions(M, rtol, atol)
        eps = rtol * np.abs(M) + atol + 2.0 ** -24 * 1.01 * np.abs(fr._dp(-M)).max()
        best = min(all_paths, key=lambda p: -sum(M[c] for c in p))
        for i in range(1, 3):
            movable = False
            for p in all_paths:
                if min(j for r, j in p if r == i) == jump[i]:
                    continue
                Mp = M - eps      # the matrix within eps that favours p the most against the float64 path
                for c in p:
                    Mp[c] = M[c] + eps[c]
                movable |= sum(Mp[c] for c in p) >= sum(Mp[c] for c in best)
            assert decided[i] == (not movable), (M, i)
            seen[bool(decided[i])] += 1
    assert min(seen.values()) >= 20, seen


@pytest.mark.parametrize("d", fr.WIDTHS)
def test_batched_route_rows_are_decided(wca, d):
    """The condition on the seeds of the GPU test's batched route, from the reference alone: of the jump frames of the width's batched batch
    (float64 forward on the CPU, fr.alignment_reference with the project's bounds: a head score 2e-5 of max(1, |s|), the aggregated matrix
    rtol 2e-5 / atol 1e-7) at most 2 % hang on less than the bounds."""
    import postproc_ref as pr
    dims = fr.model_dims(wca, d)
    mel, tokens, lengths = fr.inputs(d, fr.BATCHED_B)
    out = fr.ForwardRef(fr.model_state_dict(dims, seed=fr.MODEL_SEED[d]), dims).forward(mel, tokens)
    qk = torch.stack(out["qk"], dim=1).numpy()
    rows = fr.alignment_reference(qk.reshape(fr.BATCHED_B, -1, qk.shape[-2], qk.shape[-1]), [n // 320 for n in lengths],
                                  pr.SCORE_RTOL, pr.MATRIX_RTOL, pr.MATRIX_ATOL, pr.GAP_FACTOR)
    undecided, total = sum(int((~r["decided"]).sum()) for r in rows), sum(len(r["decided"]) for r in rows)
    print("width %d batched route, %d utterances of %s frames: %d of %d jump frames undecided; selections decided: %s; distinct jump frames %s"
          % (d, len(rows), [n // 320 for n in lengths], undecided, total, [r["selection_decided"] for r in rows], [len(set(r["jump"].tolist())) for r in rows]))
    assert total == fr.BATCHED_B * (fr.N_LONG - len(fr.SOT) - 1) and undecided * 50 <= total
    # the paths are no trivial ones: every utterance's tokens enter at several distinct frames
    assert all(len(set(r["jump"].tolist())) >= 4 for r in rows)


# ------------------------------------------------------------------------------------------------------------------ (c) the mutations
def test_every_mutation_is_seen(small, wca):
    """(c) each mutation of the reference against the unmutated one, in units of the bounds the GPU test asserts: the contract mode's
    max(8 x fp32 distance, floor), and the f16 mode's 4 x the f16-operand statement's distance (maximum and mean). Every mutation is at
    least 10 contract bounds away in some observable (the smallest: the lo halves dropped at ONE product, 16). The wiring mutations are
    also at least 2 f16-mode bounds away: an engine with that wiring, as close to the mutated forward as a right engine must be to the right
    one (1 bound), is still more than a bound from the reference. The f16 mode's bounds are coarse at 128 wide -- the encoder output's is
    4e-3, mostly the f16 rounding of the stored output itself -- so the smallest wiring separation there is 5.7 (mlp_ln_before_out, which
    is 2400 contract bounds)."""
    dims, mel, tokens, ref = small["dims"], small["mel"], small["tokens"], small["ref"]
    cb, fb = fr.contract_bounds(small["d32"]), fr.f16_bounds(small["d16"])
    print("bounds at 128 wide: contract %s; f16 mode (max, mean) %s" % ({k: "%.3g" % v for k, v in cb.items()}, {k: "%.3g / %.3g" % v for k, v in fb.items()}))
    sd_x = fr.model_state_dict(dims, seed=3, inexact=True)
    ref_x = fr.observables(fr.ForwardRef(sd_x, dims).forward(mel, tokens))
    for mut in fr.MUTATIONS:
        base, sd = (ref_x, sd_x) if mut == "w_lo_left_out" else (ref, small["sd"])
        dist = fr.distance(fr.observables(fr.ForwardRef(sd, dims, mutation=mut).forward(mel, tokens)), base)
        sep_c = {k: dist[k][0] / cb[k] for k in cb}
        sep_f = {k: max(dist[k][0] / fb[k][0], dist[k][1] / fb[k][1]) for k in fb}
        print("%-30s contract bounds: enc %8.3g maps %8.3g logits %8.3g | f16 bounds: enc %8.3g maps %8.3g logits %8.3g" %
              (mut, sep_c["enc"], sep_c["maps"], sep_c["logits"], sep_f["enc"], sep_f["maps"], sep_f["logits"]))
        assert max(sep_c.values()) >= 10.0, (mut, sep_c)
        if mut not in fr.PRECISION_MUTATIONS:
            assert max(sep_f.values()) >= 2.0, (mut, sep_f)
