"""CPU proofs about the probe families of tests/gemm_tile_probe_ref.py, which tests/test_gemm_tile_probes_gpu.py runs against the tile GEMMs of
csrc/gemm.hip on the GPU: every family is exact in fp32 in any order of accumulation, the planted LayerNorm image survives the epilogue's fp32
chain, every index error of MUTATIONS moves an asserted output of every launch it applies to by at least the family's quantum, and every launch of
SWEEPS gets the kernel, grid, split, supertile and site instance its entry states (plan_gemm through wca_test_gemm_plan: host code, no GPU)."""
import ctypes

import pytest
import torch

import gemm_tile_probe_ref as ref
from test_gemm_forms_gpu import ERF_BOUNDS

ALL = [L for sweep in ref.SWEEPS.values() for L in sweep]
BATCH_A = 2


def test_sweeps_hold_what_the_gpu_test_needs():
    assert set(ref.SWEEPS) == {"t128", "splitk", "t256", "persist", "pair", "ln", "skinny", "gelu"}
    assert len(set(ALL)) == len(ALL)
    for L in ALL:
        assert ref.exact(L) < 2 ** 24, L
        assert L.out_mode != 0 or L.pair or L.gelu or ref.exact(L) <= 2048, L       # an f16 store of whole numbers up to 2048 is exact
        assert L.out_mode != 4 or L.gelu or ref.exact(L) * ref.LO_Q < 512, L        # ... and an f16 pair holds multiples of 2^-14 below 512 exactly
    # what the persistent sweeps must reach: one, two and at least three tiles per workgroup, both values of the remainders, a short last supertile
    per_wg = {len(seq) for L in ref.SWEEPS["persist"] for seq in ref.walks(L)}
    assert {1, 2, 3} <= per_wg and max(per_wg) >= 10
    nwg = {(ref.tiles(L)[1] * ref.tiles(L)[2]) % L.grid != 0 for L in ref.SWEEPS["persist"]}
    rem8 = {(ref.tiles(L)[1] * ref.tiles(L)[2]) & 7 != 0 for L in ref.SWEEPS["persist"]}
    assert nwg == {True, False} and rem8 == {True, False}
    assert any(L.st == 3 and ref.tiles(L)[1] % 3 for L in ref.SWEEPS["persist"])
    ln = ref.SWEEPS["ln"]
    assert {ref.tiles(L)[1] & 7 != 0 for L in ln} == {True, False}
    assert {(L.grid >> 3) % ref.tiles(L)[2] != 0 for L in ln} == {True, False}                      # PR exact, and with idle workgroups
    assert any(not seq for L in ln for seq in ref.ln_walks(L)) and max(len(seq) for L in ln for seq in ref.ln_walks(L)) >= 3
    for L in ln:
        seen = sorted(t for seq in ref.ln_walks(L) for t in seq)
        assert seen == [(tm, tn) for tm in range(ref.tiles(L)[1]) for tn in range(ref.tiles(L)[2])], L    # every tile once
        assert (min(L.cu_limit or ref.N_CU, ref.N_CU) >> 3) >= L.N // 256
    for L in ref.SWEEPS["persist"] + ref.SWEEPS["pair"]:
        seen = sorted(t for seq in ref.walks(L) for t in seq)
        assert seen == [(tm, tn) for tm in range(ref.tiles(L)[1]) for tn in range(ref.tiles(L)[2])], L


def test_inputs_are_f16_values_and_differ_at_every_stride():
    a, lo = ref.comb_a(600, 1024), ref.lo_a(600, 1024) / ref.LO_Q
    for d in [8, 32] + [64 * j for j in range(1, 9)]:
        assert bool((a[:, d:] != a[:, :-d]).all())
    assert bool((lo[:, 64:] != lo[:, :-64]).all()) and bool((lo[1:] != lo[:-1]).all())
    c = ref.count_a(600, 512)
    s = ref.ln_scales(600)
    for d in (1, 16, 64, 128, 256):
        assert bool((a[d:] != a[:-d]).all()) and bool((c[d:] != c[:-d]).any(1).all()) and bool((s[d:] != s[:-d]).all())
    b = ref.bias_of("std", 1024)
    for d in (1, 8, 16, 64, 256):
        assert bool((b[d:] != b[:-d]).all())
    for t in (a, lo * ref.LO_Q, c, b, ref.dense_w(33, 512), ref.comb_w(264, 256), ref.ln_target(300, 768), ref.ln_image(300, 768), c + lo[:, :512] * ref.LO_Q - c):
        assert torch.equal(t.half().double(), t)
    # lo is a genuine low-order term of hi, and no multiple of it
    assert float((lo * ref.LO_Q).abs().max()) < 2.0 ** -11 and len(set((lo[:, :512] / c).flatten().tolist())) > 2
    # the window form: overlapping rows are shifted copies of one sequence, and differ
    for L in ref.SWEEPS["t256"]:
        if L.window:
            w = ref.a_hi(L)
            _, _, lda, _, _ = ref.window_geometry(L)
            assert lda < L.K and torch.equal(w[0, lda:], w[1, :L.K - lda]) and bool((w[1:] != w[:-1]).any(1).all())
    L = ref.SWEEPS["t128"][0]._replace(M=300, N=264, out_mode=2)
    assert ref.addend(L).unique().numel() == 300 * 264 and float(ref.addend(ref.SWEEPS["pair"][0]._replace(out_mode=2)).abs().max()) < 2 ** 23


def _classes():
    seen = {}
    for L in ALL:
        seen.setdefault((L.fam, L.w, bool(L.pair), L.K, bool(L.window)), L)
    return list(seen.values())


def test_every_family_is_exact_in_fp32_in_any_order():
    """fp32 accumulation one k at a time, in the natural order and three seeded permutations (a pair launch also with the hi and lo steps of each
    64-wide K tile interleaved, as the kernel walks them), equals the float64 product bit for bit -- on the first 48 rows and columns"""
    for L in _classes():
        r, c = slice(0, min(L.M, 48)), slice(0, min(L.N, 48))
        hi, w = ref.a_hi(L)[r], ref.w_of(L)[c]
        terms = [(hi, w)]
        if L.pair:
            terms.append((ref.lo_a(L.M, L.K)[r], w))
        want = sum(a @ b.T for a, b in terms)
        prods = torch.cat([(a.float().unsqueeze(1) * b.float().unsqueeze(0)) for a, b in terms], 2)    # [rows][cols][K or 2 K]: exact in fp32
        assert torch.equal(prods.double(), torch.cat([a.unsqueeze(1) * b.unsqueeze(0) for a, b in terms], 2))
        n = prods.shape[2]
        orders = [torch.arange(n)] + [torch.randperm(n, generator=torch.Generator().manual_seed(s)) for s in (1, 2, 3)]
        if L.pair:   # (tile 0: hi, lo), (tile 1: hi, lo), ...
            k = torch.arange(L.K)
            orders.append(torch.stack([k.view(-1, 64), (k + L.K).view(-1, 64)], 1).reshape(-1))
        for order in orders:
            acc = torch.zeros(prods.shape[:2])
            for i in order.tolist():
                acc += prods[:, :, i]
            assert torch.equal(acc.double(), want), (L, order[:4])
        assert float(want.abs().max()) <= ref.exact(L._replace(out_mode=1, bias="")) * (ref.LO_Q if L.pair else 1.0)


@pytest.mark.parametrize("N", range(256, 2049, 256))
def test_layernorm_image_survives_the_fp32_chain(N):
    """Every sign row under every scale (5 x 1031 rows) through the epilogue's chain in fp32 -- per-64-column two-pass mean / M2, Chan merges over the
    four waves and over the N / 256 tiles (1 / 3 and 1 / 5 inexact), rsqrt one unit in the last place either way: the normalised value stays at
    least 2e-4 from every f16 rounding boundary and rounds to the planted image; the fp32 rounding of the last expression (two products and a sum of
    values up to 5: 1e-6) is far inside that margin. Each tile's own statistics are far from the row's."""
    M = 5 * ref.MASTER_ROWS
    x, image = ref.ln_target(M, N), ref.ln_image(M, N)
    gamma, beta = ref.ln_gamma_beta(N)
    s = ref.ln_scales(M)
    assert bool((x.sum(1) == 0).all()) and torch.equal((x * x).sum(1), N * s * s)
    want = [{192: 0.5, 64: -0.5, 128: 0.0}[p] for p in ref.ln_tile_positives(N)]
    assert torch.equal(x.view(M, N // 256, 256).mean(2), s.view(-1, 1) * torch.tensor(want, dtype=torch.float64))
    assert N == 256 or all(v != 0.0 for i, v in enumerate(want) if not (N // 256 % 2 and i == N // 512))
    assert float(ref.f16_boundary_distance(ref.layernorm64(x, gamma, beta)).min()) >= 2e-4
    for ulps in (-1, 0, 1):
        mean, rstd = ref.ln_chain_f32(x, ulps)
        y = (x - mean.double().view(-1, 1)) * rstd.double().view(-1, 1) * gamma + beta
        assert float(ref.f16_boundary_distance(y).min()) >= 2e-4, (N, ulps)
        assert torch.equal(y.half(), image.half()) and torch.equal(y.float().half(), image.half())


def _value_key(L, mutate):
    """what a mutated reference depends on: launches that differ only in fields the mutation does not read are proven once"""
    k = ref._math_key(L)._replace(out_mode=L.out_mode, gelu=L.gelu, bias=L.bias, splitk=L.splitk)
    if mutate in ref._WALK:
        k = k._replace(form=L.form, grid=L.grid, st=L.st)
    if mutate in ("tail_row_takes_previous", "w_perm_of_other_type") or mutate.startswith("ln_"):
        k = k._replace(form=L.form)
    return k


def _moved(L, true, bent):
    """by how much the bent reference moves an asserted output, in units of what the GPU test resolves there"""
    if L.out_mode == 3:
        dx = (torch.nan_to_num(bent[0]) - true[0]).abs().max() / 0.25
        dy = ((torch.nan_to_num(bent[1]) - true[1]).abs() / ref.spacing_f16(true[1])).max() if bent[1] is not None else 0.0
        return float(max(dx, dy))
    d = (ref.flat(bent) - ref.flat(true)).abs()
    if not L.gelu:
        return float(d.max() / (ref.LO_Q if L.pair else 1.0))
    t = ref.flat(true)
    bound = ref.spacing_f16(t) if L.out_mode == 0 else ERF_BOUNDS[0][2] + ERF_BOUNDS[0][3] * t.abs()     # (the f32 store's bound covers the pair store's)
    return float((d / (2 * bound)).max())


def test_no_index_error_hides_in_any_launch():
    """(The residual + LayerNorm launches: an error of the product is looked for in x alone, over the whole launch; an error of the hand-off moves no x
    and is looked for in the first 1024 rows of ln_out, whose statistics are taken where the whole launch takes them -- a block of the full reference.)"""
    hits = dict.fromkeys(ref.MUTATIONS, 0)
    done = set()
    for L in ALL:
        true = true_ln = None
        for mutate in ref.MUTATIONS:
            if not ref.applies(mutate, L):
                continue
            hits[mutate] += 1
            key = (_value_key(L, mutate), mutate)
            if key in done:
                continue
            done.add(key)
            if L.out_mode == 3 and mutate in ref._LN_MUT:
                if true_ln is None:
                    true_ln = ref.reference(L, ln_rows=1024)
                assert _moved(L, true_ln, ref.reference(L, mutate, ln_rows=1024)) >= 1.0, (mutate, L)
                continue
            if true is None:
                true = ref.reference(L, ln=False)
            assert _moved(L, true, ref.reference(L, mutate, ln=False)) >= 1.0, (mutate, L)
    assert all(hits.values()), hits
    print(hits)


def test_the_plan_gives_every_launch_what_its_entry_states(lib, switch):
    for L in ALL:
        switch("gemm_ring", L.ring)
        lda = ref.window_geometry(L)[2] if L.window else (2 * L.K if L.pair else L.K) + L.lda_pad
        out = (ctypes.c_int32 * 10)(*([-1] * 10))
        rc = lib.wca_test_gemm_plan(L.M, L.N, ref.k_arg(L), lda, L.out_mode, L.gelu, L.K if L.pair == 1 else 0, L.force_tile, L.site, ref.N_CU, L.cu_limit,
                                    BATCH_A if L.window else 0, ref.SK_BYTES, out)
        assert rc == 0, (L, lib.wca_last_error())
        kernel, grid_x, grid_y, _, _, splitk, supertile, site = list(out)[:8]
        assert (kernel, grid_x, grid_y, splitk, site) == (L.form, L.grid, L.splitk, L.splitk, L.site_used), (L, list(out))
        # (the entry point has no supertile argument: a launch that names its own is pinned on the auto value it overrides)
        assert supertile == ref._plan(L._replace(supertile=0)).st, (L, list(out))
