"""The attention layouts of the forward (csrc/engine_forward.hip) at kernel level, on the MI355X (`-m gpu`): Q / K / V as column blocks of one
interleaved buffer, K / V as caches longer than the keys in use with per-row key counts, the logit capture into one layer's slice of a larger
buffer -- built through wca_test_attention_ex, which opens every stride. The reference is a float64 attention on the CPU from the SAME buffers;
tolerances are test_attention's in f16 (4e-3 on the output, 1e-4 on captured logits) and test_split_attention_is_fp32_accurate's on pairs (3e-6;
logits 4e-7 max|logit| + 1e-6). Every strided result is also, bit for bit, what the dense wca_test_attention* call gives on repacked copies."""
import ctypes as C
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

F16_SENTINEL, F32_SENTINEL = -777.0, -777.25


@pytest.fixture(scope="module")
def eng(wca):
    syn = importlib.import_module("whisper-char-alignment_amd.synthetic")
    dims = wca.ModelDimensions(80, 1500, 384, 6, 2, 51865, 448, 384, 6, 2)
    m = wca.WhisperAMD(dims, device="cuda:0", max_batch=2, precision="f16")
    m.load_state_dict(syn.random_state_dict(dims, seed=1))
    m._bind_stream()
    return m


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _ptr(t, off=0):
    return None if t is None else t.data_ptr() + off * t.element_size()


def _attention(eng, lib, wca, q, k, v, o, B, H, nq, nk, q_off=0, k_off=0, v_off=0, o_off=0, cap=None, cap_off=0, nk_rows=None, **kw):
    d = wca._lib.AttnDesc()
    d.q, d.k, d.v, d.o, d.cap, d.nk_rows = _ptr(q, q_off), _ptr(k, k_off), _ptr(v, v_off), _ptr(o, o_off), _ptr(cap, cap_off), _ptr(nk_rows)
    d.B, d.H, d.nq, d.nk = B, H, nq, nk
    for name, val in kw.items():
        assert hasattr(d, name), name
        setattr(d, name, val)
    wca._lib.check(lib.wca_test_attention_ex(eng._h, C.byref(d)))
    torch.cuda.synchronize()


def _ref64(q, k, v, H, causal=False, counts=None):
    """float64 attention of [B][n][H * 64] operands, scale 1/8; counts: keys per batch row. Returns the output and the scaled logits."""
    B, nq, d = q.shape
    nk = k.shape[1]
    qh = q.double().reshape(B, nq, H, 64).permute(0, 2, 1, 3)
    kh = k.double().reshape(B, nk, H, 64).permute(0, 2, 1, 3)
    vh = v.double().reshape(B, nk, H, 64).permute(0, 2, 1, 3)
    qk = (qh @ kh.transpose(-1, -2)) * 0.125
    s = qk.clone()
    if causal:
        s = s + torch.full((nq, nk), float("-inf"), dtype=torch.float64).triu_(1)
    if counts is not None:
        for b, n in enumerate(counts):
            s[b, :, :, n:] = float("-inf")
    p = torch.softmax(s, -1)
    vh = torch.where(torch.isfinite(vh), vh, torch.zeros_like(vh))   # (rows no probability reaches)
    return (p @ vh).permute(0, 2, 1, 3).reshape(B, nq, d), qk


def _pairs(x):
    """fp32 [..., w] -> f16 hi, lo halves"""
    hi = x.half()
    return hi, (x - hi.float()).half()


# ------------------------------------------------------------------------------- interleaved QKV
@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("n", [150, 200])
def test_interleaved_qkv_f16(eng, lib, wca, n, variant):
    """Encoder self-attention of run_encoder: Q, K and V are the column blocks 0, d, 2 d of one [B][n][3 d] buffer (row stride 3 d), O is [B][n][d];
    on both f16 kernels (variant 1 the 16x16x32 one, 2 the 32x32x16 one the encoder takes). n = 150 and 200: ragged query blocks and key tiles."""
    B, H = 2, 3
    d = H * 64
    g = torch.Generator().manual_seed(n + variant)
    qkv = torch.randn(B, n, 3 * d, generator=g).half()
    qkv[:, n // 2, :64] *= 4.0      # a few large logits: the running-maximum update
    q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
    ref, _ = _ref64(q, k, v, H)
    qkv_d = qkv.cuda()
    o = torch.full((B, n, d), F16_SENTINEL, dtype=torch.float16, device="cuda")
    _attention(eng, lib, wca, qkv_d, qkv_d, qkv_d, o, B, H, n, n, k_off=d, v_off=2 * d, q_bs=n * 3 * d, k_bs=n * 3 * d, v_bs=n * 3 * d, o_bs=n * d,
               q_rs=3 * d, k_rs=3 * d, v_rs=3 * d, o_rs=d, variant=variant)
    assert torch.equal(qkv_d.cpu(), qkv)
    torch.testing.assert_close(o.cpu().double(), ref, rtol=4e-3, atol=4e-3)
    dense = torch.full((B, n, d), F16_SENTINEL, dtype=torch.float16, device="cuda")
    qd, kd, vd = q.contiguous().cuda(), k.contiguous().cuda(), v.contiguous().cuda()
    wca._lib.check(lib.wca_test_attention(eng._h, _vp(qd), _vp(kd), _vp(vd), _vp(dense), None, 0, 0, B, H, n, n, variant << 8))
    torch.cuda.synchronize()
    assert torch.equal(o, dense)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("n", [150, 200])
def test_interleaved_qkv_pairs(eng, lib, wca, switch, n, variant):
    """The same in reference precision: rows [q k v hi (3 d) | q k v lo (3 d)] of stride 6 d with q_lo = k_lo = v_lo = 3 d, O rows [hi (d) | lo (d)] with
    o_lo = d; both pair kernels (variant 0 the launcher's 32x32x16 choice, 1 the 16x16x32 one)."""
    B, H = 2, 3
    d = H * 64
    g = torch.Generator().manual_seed(n + variant)
    x = torch.randn(B, n, 3 * d, generator=g)
    x[:, n // 2, :64] *= 4.0
    hi, lo = _pairs(x)
    qkv = torch.cat([hi, lo], dim=-1).contiguous()          # [B][n][6 d]
    val = hi.double() + lo.double()
    q, k, v = val[..., :d], val[..., d:2 * d], val[..., 2 * d:]
    ref, _ = _ref64(q, k, v, H)
    qkv_d = qkv.cuda()
    o = torch.full((B, n, 2 * d), F16_SENTINEL, dtype=torch.float16, device="cuda")
    _attention(eng, lib, wca, qkv_d, qkv_d, qkv_d, o, B, H, n, n, k_off=d, v_off=2 * d, q_bs=n * 6 * d, k_bs=n * 6 * d, v_bs=n * 6 * d, o_bs=n * 2 * d,
               q_rs=6 * d, k_rs=6 * d, v_rs=6 * d, o_rs=2 * d, split=1, q_lo=3 * d, k_lo=3 * d, v_lo=3 * d, o_lo=d, variant=variant)
    assert torch.equal(qkv_d.cpu(), qkv)
    oc = o.cpu()
    got = oc[..., :d].double() + oc[..., d:].double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item()
    assert err < 3e-6, err
    # the dense entry point on repacked [hi (d) | lo (d)] rows
    rep = lambda a, b: torch.cat([hi[..., a:b], lo[..., a:b]], dim=-1).contiguous().cuda()   # noqa: E731
    qd, kd, vd = rep(0, d), rep(d, 2 * d), rep(2 * d, 3 * d)
    dense = torch.full((B, n, 2 * d), F16_SENTINEL, dtype=torch.float16, device="cuda")
    switch("attn_split_variant", variant)
    wca._lib.check(lib.wca_test_attention_split(eng._h, _vp(qd), _vp(kd), _vp(vd), _vp(dense), None, 0, 0, B, H, n, n, 0))
    torch.cuda.synchronize()
    assert torch.equal(o, dense)


# ------------------------------------------------------------------------------- caches with per-row key counts
POISON = (float("nan"), float("inf"), float("-inf"))


def test_cache_layout_with_per_row_key_counts_ignores_what_lies_past_a_row(eng, lib, wca):
    """Self-attention of a decode step (self_attn_args of engine_forward.hip, p.cache): one query per row out of a [B][3 d] QKV row, K and V caches
    [B][T_max][d] with nk = T_max and per-row key counts (1, 17, 40, 33). What a cache holds past a row's count is whatever the buffer held: with NaN
    and +-inf there the output must be, bit for bit, the one with finite filler -- a kernel that multiplies masked rows into its sums turns them
    into NaN. Each row also equals a dense call on its own prefix."""
    B, H, T_max = 4, 4, 40
    d = H * 64
    counts = (1, 17, 40, 33)
    g = torch.Generator().manual_seed(40)
    qkv = torch.randn(B, 3 * d, generator=g).half()
    kc = torch.randn(B, T_max, d, generator=g).half()
    vc = torch.randn(B, T_max, d, generator=g).half()
    ref, _ = _ref64(qkv[:, None, :d], kc, vc, H, counts=counts)
    nkd = torch.tensor(counts, dtype=torch.int32, device="cuda")
    qd = qkv.cuda()
    outs = []
    for poison in (None,) + POISON:
        k2, v2 = kc.clone(), vc.clone()
        if poison is not None:
            for b, n in enumerate(counts):
                k2[b, n:] = poison
                v2[b, n:] = poison
        o = torch.full((B, d), F16_SENTINEL, dtype=torch.float16, device="cuda")
        _attention(eng, lib, wca, qd, k2.cuda(), v2.cuda(), o, B, H, 1, T_max, nk_rows=nkd, q_bs=3 * d, k_bs=T_max * d, v_bs=T_max * d, o_bs=d, q_rs=3 * d,
                   k_rs=d, v_rs=d, o_rs=d)
        outs.append(o)
    torch.testing.assert_close(outs[0].cpu().double()[:, None], ref, rtol=4e-3, atol=4e-3)
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    for b, n in enumerate(counts):
        dense = torch.full((1, d), F16_SENTINEL, dtype=torch.float16, device="cuda")
        qb, kb, vb = qkv[b:b + 1, :d].contiguous().cuda(), kc[b, :n].contiguous().cuda(), vc[b, :n].contiguous().cuda()
        wca._lib.check(lib.wca_test_attention(eng._h, _vp(qb), _vp(kb), _vp(vb), _vp(dense), None, 0, 0, 1, H, 1, n, 0))
        torch.cuda.synchronize()
        assert torch.equal(dense[0], outs[0][b])


def test_causal_prefill_against_a_longer_cache_ignores_the_unused_rows(eng, lib, wca):
    """The prefill of a prompted decode with its keys read from the cache planes: nq = nk = 37 of T_max = 40 cached rows, causal; cache rows 37 .. 39
    poisoned with NaN and +-inf change nothing, and the result is the dense causal call's."""
    B, H, T_max, n = 4, 4, 40, 37
    d = H * 64
    g = torch.Generator().manual_seed(37)
    q = torch.randn(B, n, d, generator=g).half()
    kc = torch.randn(B, T_max, d, generator=g).half()
    vc = torch.randn(B, T_max, d, generator=g).half()
    ref, _ = _ref64(q, kc[:, :n], vc[:, :n], H, causal=True)
    qd = q.cuda()
    outs = []
    for poison in (None,) + POISON:
        k2, v2 = kc.clone(), vc.clone()
        if poison is not None:
            k2[:, n:] = poison
            v2[:, n:] = poison
        o = torch.full((B, n, d), F16_SENTINEL, dtype=torch.float16, device="cuda")
        _attention(eng, lib, wca, qd, k2.cuda(), v2.cuda(), o, B, H, n, n, causal=1, q_bs=n * d, k_bs=T_max * d, v_bs=T_max * d, o_bs=n * d, q_rs=d, k_rs=d,
                   v_rs=d, o_rs=d)
        outs.append(o)
    torch.testing.assert_close(outs[0].cpu().double(), ref, rtol=4e-3, atol=4e-3)
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    dense = torch.full((B, n, d), F16_SENTINEL, dtype=torch.float16, device="cuda")
    kd, vd = kc[:, :n].contiguous().cuda(), vc[:, :n].contiguous().cuda()
    wca._lib.check(lib.wca_test_attention(eng._h, _vp(qd), _vp(kd), _vp(vd), _vp(dense), None, 0, 0, B, H, n, n, 1))
    torch.cuda.synchronize()
    assert torch.equal(outs[0], dense)


# ------------------------------------------------------------------------------- capture into a layer's slice
@pytest.mark.parametrize("pair", [False, True])
def test_capture_into_one_layers_slice(eng, lib, wca, pair):
    """Cross-attention of decoder layer 1 of 3 (cross_attn_args of engine_forward.hip): the logits of the first 145 keys go to that layer's slice of a
    [B][L][H][nq][Fpad = 152] buffer (cap_bs = L H nq Fpad). Layers 0 and 2 and the columns 145 .. 151 keep the sentinel. f16 and pair operands."""
    B, L, H, nq, nk, Fpad, cols = 2, 3, 2, 69, 1500, 152, 145
    d = H * 64
    g = torch.Generator().manual_seed(69 + pair)
    q = torch.randn(B, nq, d, generator=g)
    k = torch.randn(B, nk, d, generator=g)
    v = torch.randn(B, nk, d, generator=g)
    q[:, nq // 2, :64] *= 4.0
    cap = torch.full((B, L, H, nq, Fpad), F32_SENTINEL, device="cuda")
    dense_cap = torch.full((B, H, nq, Fpad), F32_SENTINEL, device="cuda")
    w = 2 * d if pair else d
    o = torch.full((B, nq, w), F16_SENTINEL, dtype=torch.float16, device="cuda")
    dense = torch.full((B, nq, w), F16_SENTINEL, dtype=torch.float16, device="cuda")
    strides = dict(q_bs=nq * w, k_bs=nk * w, v_bs=nk * w, o_bs=nq * w, q_rs=w, k_rs=w, v_rs=w, o_rs=w, cap_off=H * nq * Fpad, cap_bs=L * H * nq * Fpad,
                   cap_hs=nq * Fpad, cap_ld=Fpad, cap_cols=cols)
    if pair:
        (qh, ql), (kh, kl), (vh, vl) = _pairs(q), _pairs(k), _pairs(v)
        ref, qk = _ref64(qh.double() + ql.double(), kh.double() + kl.double(), vh.double() + vl.double(), H)
        qd, kd, vd = (torch.cat(p, dim=-1).contiguous().cuda() for p in ((qh, ql), (kh, kl), (vh, vl)))
        _attention(eng, lib, wca, qd, kd, vd, o, B, H, nq, nk, cap=cap, split=1, q_lo=d, k_lo=d, v_lo=d, o_lo=d, **strides)
        wca._lib.check(lib.wca_test_attention_split(eng._h, _vp(qd), _vp(kd), _vp(vd), _vp(dense), _vp(dense_cap), Fpad, cols, B, H, nq, nk, 0))
        oc = o.cpu()
        err = (oc[..., :d].double() + oc[..., d:].double() - ref).abs().max().item()
        assert err < 3e-6, err
        cerr = (cap[:, 1, :, :, :cols].cpu().double() - qk[..., :cols]).abs().max().item()
        assert cerr < 4e-7 * qk.abs().max().item() + 1e-6, cerr
    else:
        qd, kd, vd = q.half().cuda(), k.half().cuda(), v.half().cuda()
        ref, qk = _ref64(q.half(), k.half(), v.half(), H)
        _attention(eng, lib, wca, qd, kd, vd, o, B, H, nq, nk, cap=cap, **strides)
        wca._lib.check(lib.wca_test_attention(eng._h, _vp(qd), _vp(kd), _vp(vd), _vp(dense), _vp(dense_cap), Fpad, cols, B, H, nq, nk, 0))
        torch.testing.assert_close(o.cpu().double(), ref, rtol=4e-3, atol=4e-3)
        torch.testing.assert_close(cap[:, 1, :, :, :cols].cpu().double(), qk[..., :cols], rtol=1e-4, atol=1e-4)
    torch.cuda.synchronize()
    assert torch.equal(o, dense) and torch.equal(cap[:, 1, :, :, :cols], dense_cap[..., :cols])
    assert bool((cap[:, 0] == F32_SENTINEL).all()) and bool((cap[:, 2] == F32_SENTINEL).all()) and bool((cap[:, 1, :, :, cols:] == F32_SENTINEL).all())
