"""What tests/test_gemm_rows_probes_gpu.py rests on, proved without a GPU: the probe families of tests/gemm_rows_probe_ref.py are exact (f16 values,
partial sums far below 2^24, a LayerNorm image that sits clear of every f16 rounding boundary), every index error of MUTATIONS moves an
asserted output by at least 0.5 in EVERY launch it applies to (a condition on the families, not a measurement of the kernel), and the decoder's
dispatch (plan_dec_gemm through wca_test_dec_gemm_plan) sends the five Whisper widths where the probes look."""
import ctypes

import pytest
import torch

import gemm_rows_probe_ref as ref

WIDTHS = (384, 512, 768, 1024, 1280)
N_VOCAB = 51865


def _distinct(launches):
    """one launch per value of C: the grid shape and the strides do not enter the reference"""
    seen = {}
    for L in launches:
        seen.setdefault(L._replace(groups=0, lda_pad=0, lda32_pad=0, ldw_pad=0, ldc_pad=0, c_rows=0, c_gap=0), L)
    return list(seen.values())


# ------------------------------------------------------------------------------- the families
def test_sweeps_hold_the_shapes_the_kernel_branches_on():
    s = ref.SWEEPS
    assert {L.M for L in s["rows"]} == set(range(1, 131)) | {192, 193} and {(L.a, L.out_mode) for L in s["rows"]} == {(a, om) for a in ("sign", "ln") for om in (0, 1, 2)}
    assert {L.N for L in s["cols"]} == set(range(1, 71)) | {255, 256, 257, 4097, N_VOCAB} and {L.groups for L in s["cols"]} == {0, 1, 2, 3, 4, 13}
    pairs = {(L.K, L.S) for L in s["depth"]}
    assert len(pairs) == 64 and pairs >= {(384, 1), (512, 1), (768, 1), (1024, 1), (1280, 2), (1536, 2), (2048, 2), (3072, 3), (4096, 4), (5120, 5)}
    assert all(L.K % (L.S * 128) == 0 and L.K // L.S <= 1024 for L in s["depth"] + s["ln"])
    assert {(L.K, L.S) for L in s["ln"]} == {(256, 1), (256, 2), (512, 1), (512, 2), (512, 4), (768, 1), (768, 2), (768, 3), (768, 6),
                                             (1024, 1), (1024, 2), (1024, 4), (1024, 8)}
    assert all(ref.pick_splitk(L.K) == L.S for L in s["depth"] if (L.K, L.S) in {(1280, 2), (1536, 2), (2048, 2), (3072, 3), (4096, 4), (5120, 5)})
    assert {(L.N, L.K, L.a) for L in s["gelu"]} == {(4 * d, d, "sign") for d in WIDTHS} | {(4 * d, d, "ln") for d in (512, 768, 1024)}
    assert max(L.M for sw in s.values() for L in sw) <= ref.ROWS_MAX and max(L.K for sw in s.values() for L in sw) <= ref.K_MAX


def test_every_value_is_f16_exact_and_every_partial_sum_fits_fp32():
    rows = {}                                   # the operands of a shape are a prefix of those of the same shape on more rows
    for sw in ref.SWEEPS.values():
        for L in sw:
            key = (L.a, L.w, L.bias, L.N, L.K, L.out_mode == 2)
            rows[key] = max(rows.get(key, 0), L.M)
    assert ref.SUM_BOUND < 2 ** 24
    for (a_name, w_name, b_name, N, K, acc), M in rows.items():
        a, w, bias, c0 = ref.operands(ref.Launch("", M, N, K, a=a_name, w=w_name, bias=b_name, out_mode=2 if acc else 1))
        for t in (a, w, bias):
            assert t is None or torch.equal(t.half().double(), t)
        assert c0 is None or (torch.equal(c0.float().double(), c0) and c0.unique().numel() == c0.numel())     # f32 data, distinct per (m, n)
        assert float(a.abs().min()) >= 1.0      # never 0: a dropped element always shows
        assert float(a.abs().max()) <= 5 and float(w.abs().max()) <= 1 and K * 5 * 2 <= ref.SUM_BOUND
        worst = K * float(a.abs().max()) * float(w.abs().max()) + (float(bias.abs().max()) if bias is not None else 0) + (float(c0.abs().max()) if acc else 0)
        assert worst < 2 ** 24
        # multiples of 0.5: with the bound above every fp32 partial sum is exact in any order
        assert torch.equal((2 * a).round(), 2 * a) and torch.equal(w.round(), w)


def test_comb_code_separates_the_offsets_the_kernel_steps_by():
    a = ref.comb_a(ref.ROWS_MAX, ref.K_MAX)
    for dk in [8] + [32 * j for j in range(1, 9)] + [128 * j for j in range(1, 9)]:
        assert bool((a[:, dk:] != a[:, :-dk]).all()), dk
    for dm in (1, 8, 16, 64):
        assert bool((a[dm:] != a[:-dm]).all()), dm
    w = ref.comb_w(1024)
    assert torch.equal(w.sum(0), torch.ones(1024, dtype=torch.float64)) and torch.equal(w.sum(1), torch.full((128,), 8.0, dtype=torch.float64))


def test_gelu_runs_keep_the_pre_activation_exact_and_small():
    for L in ref.SWEEPS["gelu"]:
        a, w, bias, _ = ref.operands(L)
        v = a @ w.T + bias
        assert float(v.abs().max()) <= 8 and torch.equal((2 * v).round(), 2 * v)
        assert torch.equal((w != 0).sum(1), torch.full((L.N,), 6 if L.a == "sign" else 1))
        assert float(v.min()) < -3 and float(v.max()) > 3            # both tails of the activation are visited


@pytest.mark.parametrize("K", ref.LN_WIDTHS)
def test_layernorm_probe_rounds_to_the_planted_image(K):
    """float64 LayerNorm of the probe rows rounds to +-gamma + beta, at least 2e-4 from every f16 rounding boundary; so does an fp32
    evaluation whose rstd is off by +-64 ulp (a hardware rsqrt and the summation order of the statistics are far inside that)."""
    M = ref.ROWS_MAX
    x, (gamma, beta), image = ref.ln_x(M, K), ref.ln_gamma_beta(K), ref.ln_image(M, K)
    assert torch.equal(x.sum(1), torch.zeros(M, dtype=torch.float64)) and torch.equal((x * x).mean(1), ref.ln_scales(M) ** 2)
    assert torch.equal((x > 0).sum(1), torch.full((M,), K // 2))
    s = ref.ln_scales(M)
    for dm in (1, 8, 16, 64):
        assert bool((s[dm:] != s[:-dm]).all())
    assert float(image.abs().min()) >= 1 and torch.equal(image.half().double(), image)
    y = ref.layernorm64(x, gamma, beta)
    assert torch.equal(y.half().double(), image)
    assert float(ref.f16_boundary_distance(y).min()) >= 2e-4
    assert float((y - image).abs().max()) <= 2 * 8.1e-5
    x32, g32, b32 = x.float(), gamma.float(), beta.float()
    rstd = torch.rsqrt((x32 * x32).sum(1, keepdim=True) * torch.tensor(1.0 / K, dtype=torch.float32) + torch.tensor(ref.LN_EPS, dtype=torch.float32))
    for ulps in (-64, 0, 64):
        r = (rstd.view(torch.int32) + ulps).view(torch.float32)
        y32 = (x32 * r * g32 + b32).double()
        assert torch.equal(y32.half().double(), image) and float(ref.f16_boundary_distance(y32).min()) >= 2e-4, ulps


def test_neighbouring_statistics_are_off_by_a_factor_of_two():
    M, K = 130, 256
    gamma, beta = ref.ln_gamma_beta(K)
    m = torch.arange(M)
    for other in ((m + 1) % M, (m + 8) % M, (m - 1) % M):
        y = ref.layernorm64(ref.ln_x(M, K), gamma, beta, stats_of=other)
        ratio = ((y - beta) / gamma).abs()
        assert bool(((ratio >= 1.99) | (ratio <= 0.501)).all())


# ------------------------------------------------------------------------------- the index errors
@pytest.mark.parametrize("mutate", ref.MUTATIONS)
def test_every_index_error_moves_an_asserted_output(mutate):
    n, hidden = 0, []
    for sweep, launches in ref.SWEEPS.items():
        for L in _distinct(launches):
            if not ref.applies(mutate, L):
                continue
            moved = float((ref.flat(ref.reference(L, mutate)) - ref.flat(ref.reference(L))).abs().max())
            if not moved >= 0.5:
                hidden.append((moved, L))
            n += 1
    assert not hidden, (len(hidden), hidden[:8])
    assert n >= 8, n


def test_every_sweep_meets_the_errors_it_is_there_for():
    hit = {sweep: {m for m in ref.MUTATIONS for L in launches if ref.applies(m, L)} for sweep, launches in ref.SWEEPS.items()}
    assert hit["depth"] >= {"drop_last_k_step", "read_quarter_twice", "swap_split_slices", "swap_split_partials", "lose_split_partial", "accumulate_twice"}
    assert hit["rows"] >= {"tail_row_takes_previous", "ln_stats_of_neighbour", "bias_shift_one", "accumulate_twice"}
    assert hit["cols"] >= {"column_group_shift_16", "bias_shift_one"}
    assert hit["ln"] >= {"ln_stats_of_neighbour", "swap_split_slices", "lose_split_partial"}
    assert hit["kv"] >= {"kv_t_off_by_one", "kv_neighbour_row", "kv_planes_swapped"}


def test_kv_tables_cover_the_clamp():
    for M in (1, 5, 64, 65, 128):
        L = ref.Launch("kv", M, 48, 256, kv_d=16, kv_t="clamp")
        want, slot = ref.kv_positions(L), ref.kv_slots(L)
        assert int(slot.min()) >= 0 and int(slot.max()) <= ref.T_MAX - 1
        assert int(want[0]) == -1 and int(slot[0]) == 0
        if M > 1:
            assert int(want[1]) == ref.T_MAX and int(slot[1]) == ref.T_MAX - 1
    assert sorted(ref.kv_slots(ref.Launch("kv", 7, 48, 256, kv_d=16, kv_t="perm")).tolist()) == list(range(7))


# ------------------------------------------------------------------------------- the decoder's dispatch
@pytest.fixture(scope="module")
def plan(lib):
    def call(d, M, N, K, ln=0, kv=0):
        out = (ctypes.c_int64 * 8)(*([-1] * 8))
        assert lib.wca_test_dec_gemm_plan(d, M, N, K, ln, kv, out) == 0
        return dict(zip(("few_row", "splitk", "groups", "grid_x", "grid_y", "lds", "ws", "cap"), out))
    return call


def _sites(d):
    """(name, N, K, LayerNorm-fed, KV append) of every GEMM of a decoder forward"""
    return [("qkv_step", 3 * d, d, 1, 1), ("qkv", 3 * d, d, 1, 0), ("out", d, d, 0, 0), ("cross_q", d, d, 1, 0), ("cross_out", d, d, 0, 0),
            ("fc1", 4 * d, d, 1, 0), ("fc2", d, 4 * d, 0, 0), ("logits", N_VOCAB, d, 1, 0)]


# width -> the split of (a plain K = d launch, fc2), and whether the LayerNorm-fed projections fuse (K % 256 == 0, K <= 1024)
EXPECT = {384: (1, 2, False), 512: (1, 2, True), 768: (1, 3, True), 1024: (1, 4, True), 1280: (2, 5, False)}


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("M", (1, 64, 65, 128, 129))
def test_dispatch_table(plan, d, M):
    s_plain, s_fc2, ln_fuses = EXPECT[d]
    for name, N, K, ln, kv in _sites(d):
        p = plan(d, M, N, K, ln, kv)
        assert p["cap"] == 2 * ((d + 15) // 16) * max(s_plain, s_fc2) * 64 * 16 * 4
        want_few = M <= 128 and (ln_fuses or not ln)
        assert p["few_row"] == int(want_few), (name, p)
        if not want_few:
            assert [p[k] for k in ("splitk", "groups", "grid_x", "grid_y", "lds", "ws")] == [0] * 6
            continue
        S = s_fc2 if name == "fc2" else s_plain
        assert p["splitk"] == S, (name, p)
        NG = (N + 15) // 16
        groups = 1 if S > 1 else (NG + 255) // 256
        assert p["groups"] == groups and p["grid_x"] == -(-NG // groups) * S and p["grid_y"] == (M + 63) // 64
        assert p["grid_x"] // S <= 256 or S > 1
        assert p["lds"] == 64 * (K // S + 8) * 2 + 4 * 4 * 4 * 64 * 4 + 16 and p["lds"] <= 160 * 1024
        assert p["ws"] == (0 if S == 1 else ((M + 63) // 64) * NG * S * 64 * 16 * 4) and p["ws"] <= p["cap"]
    assert plan(d, M, N_VOCAB, d, 1)["groups"] in (0, 13)


def test_dispatch_refuses_what_the_workspace_or_the_kernel_cannot_take(plan):
    # a split-K launch takes no KV append; a K that no split of at most 8 brings to 1024 leaves the few-row path; so do more columns than the
    # workspace was carved for
    assert plan(1280, 8, 3 * 1280, 1280, 0, 1)["few_row"] == 0 and plan(1280, 8, 3 * 1280, 1280, 0, 0)["few_row"] == 0
    assert plan(1280, 8, 1280, 1280)["few_row"] == 1
    assert plan(1024, 8, 1024, 8192 + 128)["few_row"] == 0 and plan(1024, 8, 1024, 8192)["few_row"] == 1 and plan(1024, 8, 1024, 8192)["splitk"] == 8
    assert plan(1024, 128, 1024 + 16, 4096)["few_row"] == 0 and plan(1024, 64, 1024 + 16, 4096)["few_row"] == 1
    assert plan(1024, 8, 1024, 320)["few_row"] == 0
