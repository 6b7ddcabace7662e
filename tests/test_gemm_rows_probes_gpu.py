"""The index arithmetic of the few-row GEMM (csrc/gemm_rows.hip) on the MI355X (`-m gpu`), with the exact probe families of
tests/gemm_rows_probe_ref.py at every shape where an index expression of the kernel changes value: tail tiles and the wave-to-row map, the register
ring over column groups and the clamped weight rows past N, the scalar-store path of odd N / ldc, every (K, splitk) up to 8 x 1024 -- the quarters of a
slice, the steps of a wave, the split-K hand-off and its self-cleaning counters --, the LayerNorm prologue with 1 .. 4 vectors per lane on whole and
split images, the GELU of fc1, the KV-cache append at a scalar position and at per-row positions with their clamp, and every leading dimension.
tests/test_gemm_rows_probe_ref.py proves on the CPU that the families are exact and hide none of sixteen index errors.

Every launch goes through wca_test_gemm_rows_ex on operands built once per module on the device; the output buffer is refilled with a sentinel (NaN;
the addend for out_mode 2) before each launch and must keep it outside the written region.

Bounds, from the references and the number formats (never from the kernel): every comparison without GELU is torch.equal against the float64
reference cast to the output type -- every partial sum is exact in fp32, and one f16 rounding of an exact value is the reference's `.half()`; with
GELU |got - gelu64(v)| <= one f16 spacing at the reference (2^-24 below 2^-14): v is exact, the fp32 activation is within half a spacing, the
store rounds once. The standalone LayerNorm kernels on the probe rows: the f16 output and the pair's hi half EQUAL the planted image, hi + lo is
within 3e-6 of float64, the project's pair bound."""
import ctypes as C
import importlib

import pytest
import torch

import gemm_rows_probe_ref as ref

pytestmark = pytest.mark.gpu

A_POISON, W_POISON, X_POISON, GAP = 99.0, 77.0, 1.0e4, -555.0   # the padding of strided operands; the gaps of a strided out_mode 2 buffer
PAIR_TOL = 3e-6
INVALID = -1


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


@pytest.fixture(scope="module")
def eng(wca):
    syn = importlib.import_module("whisper-char-alignment_amd.synthetic")
    dims = wca.ModelDimensions(80, 1500, 384, 6, 2, 51865, 448, 384, 6, 2)
    m = wca.WhisperAMD(dims, device="cuda:0", max_batch=2, precision="f16")
    m.load_state_dict(syn.random_state_dict(dims, seed=1))
    m._bind_stream()
    return m


class Operands:
    """The device operands of every launch, built once: A rows and LayerNorm rows for ROWS_MAX rows (a launch addresses the first M), W, bias and
    the references, keyed by what they depend on."""

    def __init__(self):
        self.cache = {}
        self.launches = {}

    def get(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    @staticmethod
    def _padded(t, pad, poison, dtype):
        out = torch.full((t.shape[0], t.shape[1] + pad), poison, dtype=dtype)
        out[:, :t.shape[1]] = t
        return out.cuda()

    def a16(self, name, K, pad):
        return self.get(("a", name, K, pad), lambda: self._padded({"comb": ref.comb_a, "sign": ref.sign_a}[name](ref.ROWS_MAX, K), pad, A_POISON, torch.float16))

    def x32(self, K, pad):
        return self.get(("x", K, pad), lambda: self._padded(ref.ln_x(ref.ROWS_MAX, K), pad, X_POISON, torch.float32))

    def gamma_beta(self, K):
        return self.get(("gb", K), lambda: tuple(t.float().cuda() for t in ref.ln_gamma_beta(K)))

    def w16(self, L):
        return self.get(("w", L.w, L.N, L.K, L.ldw_pad), lambda: self._padded(ref.operands(L._replace(M=1))[1], L.ldw_pad, W_POISON, torch.float16))

    def bias(self, L):
        return self.get(("bias", L.bias, L.N), lambda: ref.bias_of(L.bias, L.N).float().cuda()) if L.bias else None

    def want(self, L):
        """the float64 reference cast to the output type, on the device (a tuple c, kc, vc for a KV launch)"""
        def make():
            r = ref.reference(L)
            cast = (lambda t: t.half().cuda()) if L.out_mode == 0 and not L.gelu else (lambda t: t.float().cuda()) if not L.gelu else (lambda t: t.cuda())
            return tuple(cast(t) for t in r) if isinstance(r, tuple) else cast(r)
        return self.get(("want", L._replace(sweep="", groups=0, lda_pad=0, lda32_pad=0, ldw_pad=0, ldc_pad=0, c_rows=0, c_gap=0)), make)

    def addend(self, L):
        return self.get(("c0", L.M, L.N), lambda: ref.addend(L.M, L.N).float().cuda())


@pytest.fixture(scope="module")
def ops():
    return Operands()


def _c_layout(L):
    """(ldc, c_batch_stride, elements of the buffer, int64 [M] offset of every logical row)"""
    ldc = L.N + L.ldc_pad
    m = torch.arange(L.M)
    if L.c_rows:
        stride = L.c_rows * ldc + L.c_gap
        return ldc, stride, -(-L.M // L.c_rows) * stride, (m // L.c_rows) * stride + (m % L.c_rows) * ldc
    return ldc, 0, L.M * ldc, m * ldc


def _launch(eng, lib, wca, ops, L, kv=None, t_rows=None, expect=0):
    """One launch. Returns the output buffer (flat, with its sentinels)."""
    ldc, c_bs, c_len, _ = _c_layout(L)
    dtype = torch.float16 if L.out_mode == 0 else torch.float32
    if L.out_mode == 2:
        c = torch.full((c_len,), GAP, dtype=dtype, device="cuda")
        _live(L, c).copy_(ops.addend(L))
    else:
        c = torch.full((c_len,), float("nan"), dtype=dtype, device="cuda")
    d = wca._lib.GemmRowsDesc()
    if L.a == "ln":
        x = ops.x32(L.K, L.lda32_pad)
        gamma, beta = ops.gamma_beta(L.K)
        d.x, d.gamma, d.beta, d.lda32 = x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), L.K + L.lda32_pad
    else:
        d.a, d.lda = ops.a16(L.a, L.K, L.lda_pad).data_ptr(), L.K + L.lda_pad
    d.w, d.ldw = ops.w16(L).data_ptr(), L.K + L.ldw_pad
    bias = ops.bias(L)
    d.bias = bias.data_ptr() if bias is not None else None
    d.c, d.ldc, d.c_rows_per_batch, d.c_batch_stride = c.data_ptr(), ldc, L.c_rows, c_bs
    d.M, d.N, d.K, d.gelu, d.out_mode, d.splitk, d.groups = L.M, L.N, L.K, L.gelu, L.out_mode, L.S, L.groups
    if kv is not None:
        d.kv_k, d.kv_v, d.kv_tmax = kv[0].data_ptr(), kv[1].data_ptr(), ref.T_MAX
        if t_rows is not None:
            d.kv_t_rows = t_rows.data_ptr()
        else:
            d.kv_t = int(L.kv_t)
    rc = lib.wca_test_gemm_rows_ex(eng._h, C.byref(d))
    assert rc == expect, (rc, lib.wca_last_error(), L)
    ops.launches[L.sweep] = ops.launches.get(L.sweep, 0) + 1
    return c


def _live(L, c):
    """the [M][N] view of the written region of a flat output buffer (a gather for batch-strided rows)"""
    ldc, _, _, off = _c_layout(L)
    if not L.c_rows:
        return c.view(L.M, ldc)[:, :L.N]
    idx = (off.view(-1, 1) + torch.arange(L.N).view(1, -1)).cuda()
    return _Gathered(c, idx)


class _Gathered:
    """rows of a batch-strided buffer: read by gather, written by scatter"""

    def __init__(self, c, idx):
        self.c, self.idx = c, idx

    def copy_(self, src):
        self.c[self.idx] = src.to(self.c.dtype)

    def value(self):
        return self.c[self.idx]


def _got(L, c):
    v = _live(L, c)
    return v.value() if isinstance(v, _Gathered) else v


def _same(got, want, L, what="C"):
    if not torch.equal(got, want):
        bad = (got != want) & ~(torch.isnan(got) & torch.isnan(want))
        i = bad.nonzero()[0].tolist()
        raise AssertionError("%s of %s: %d of %d elements differ, first at %s: got %r, want %r" %
                             (what, L, int(bad.sum()), bad.numel(), i, got[tuple(i)].item(), want[tuple(i)].item()))


def _gaps_untouched(L, c):
    """every element of the buffer outside the rows' N columns still holds its sentinel"""
    ldc, _, c_len, off = _c_layout(L)
    if c_len == L.M * L.N:
        return
    live = torch.zeros(c_len, dtype=torch.bool)
    live[(off.view(-1, 1) + torch.arange(L.N).view(1, -1)).reshape(-1)] = True
    rest = c[(~live).cuda()]
    assert bool((rest == GAP).all() if L.out_mode == 2 else torch.isnan(rest).all()), L


def _run(eng, lib, wca, ops, L):
    c = _launch(eng, lib, wca, ops, L)
    want = ops.want(L)
    if L.gelu:
        got = _got(L, c).double()
        err = (got - want).abs() / ref.spacing_f16(want)
        assert bool(torch.isfinite(got).all()) and float(err.max()) <= 1.0, (L, float(err.max()))
        return float(err.max())
    _same(_got(L, c), want, L)
    _gaps_untouched(L, c)
    if ref.splitk(L) > 1:
        # the same workspace again: the counters cleaned themselves and the partials are added in slice order
        _same(_got(L, _launch(eng, lib, wca, ops, L)), want, L, "the second launch's C")
    return 0.0


@pytest.mark.parametrize("sweep", ["rows", "cols", "depth", "ln", "strides"])
def test_sweep_equals_float64(eng, lib, wca, ops, sweep):
    for L in ref.SWEEPS[sweep]:
        _run(eng, lib, wca, ops, L)
    print("%s: %d launches" % (sweep, ops.launches[sweep]))


def test_gelu_runs_within_one_f16_spacing(eng, lib, wca, ops):
    worst = [(_run(eng, lib, wca, ops, L), L.K, L.a) for L in ref.SWEEPS["gelu"]]
    print("gelu: %d launches, worst error in f16 spacings at the reference (K, rows): %s" % (ops.launches["gelu"], ["%.3f (%d, %s)" % w for w in worst]))


def test_kv_append_routing_at_every_position(eng, lib, wca, ops):
    """q columns to C, k / v columns to plane, row and slot -- a scalar position, or a per-row table (a permutation, all equal, one asking for -1
    and T_max, which the kernel clamps to [0, T_max - 1]); everything else keeps its sentinel."""
    plain = {}
    for L in ref.SWEEPS["kv"]:
        d = L.kv_d
        kc = torch.full((L.M, ref.T_MAX, d), ref.K_SENTINEL, dtype=torch.float16, device="cuda")
        vc = torch.full((L.M, ref.T_MAX, d), ref.V_SENTINEL, dtype=torch.float16, device="cuda")
        t_rows = ref.kv_positions(L).int().cuda() if L.kv_t in ref.KV_TABLES else None
        c = _launch(eng, lib, wca, ops, L, kv=(kc, vc), t_rows=t_rows).view(L.M, L.N)
        want_c, want_k, want_v = ops.want(L)
        _same(c[:, :d], want_c[:, :d], L, "the q columns")
        assert bool(torch.isnan(c[:, d:]).all()), L               # the k / v columns of C are not written
        _same(kc, want_k, L, "the K cache")
        _same(vc, want_v, L, "the V cache")
        key = (L.M, L.N, L.a)
        if key not in plain:
            plain[key] = _launch(eng, lib, wca, ops, L._replace(kv_d=0, kv_t=None)).view(L.M, L.N)
        slot = ref.kv_slots(L).cuda()
        row = torch.arange(L.M, device="cuda")
        _same(c[:, :d], plain[key][:, :d], L, "the q columns against the plain launch")
        _same(kc[row, slot], plain[key][:, d:2 * d], L, "the appended K rows against the plain launch")
        _same(vc[row, slot], plain[key][:, 2 * d:], L, "the appended V rows against the plain launch")
    print("kv: %d launches" % ops.launches["kv"])


def test_refused_launches_write_nothing(eng, lib, wca, ops):
    base = ref.Launch("refused", 5, 48, 256, out_mode=0)
    kv = tuple(torch.full((5, ref.T_MAX, 16), s, dtype=torch.float16, device="cuda") for s in (ref.K_SENTINEL, ref.V_SENTINEL))
    t_rows = torch.zeros(5, dtype=torch.int32, device="cuda")
    cases = [(base._replace(K=320), None, None),                        # no split brings K to whole 128-wide slices
             (base._replace(K=512, S=3), None, None), (base._replace(K=2048, S=1), None, None),
             (base._replace(ldw_pad=4), None, None), (base._replace(lda_pad=4), None, None),
             (base._replace(a="ln", K=384), None, None), (base._replace(a="ln", lda32_pad=2), None, None),
             (base._replace(out_mode=3), None, None), (base._replace(out_mode=1, gelu=1), None, None),
             (base._replace(out_mode=1, kv_t=0), kv, None), (base._replace(N=64, kv_t=0), kv, None), (base._replace(kv_t=ref.T_MAX), kv, None),
             (base._replace(kv_t=-1), kv, None), (base._replace(gelu=1, kv_t="equal"), kv, t_rows), (base._replace(c_rows=2, kv_t=0), kv, None)]
    for L, k, t in cases:
        c = _launch(eng, lib, wca, ops, L, kv=k, t_rows=t, expect=INVALID)
        torch.cuda.synchronize()
        assert bool(torch.isnan(c).all()), L
    assert bool((kv[0] == ref.K_SENTINEL).all()) and bool((kv[1] == ref.V_SENTINEL).all())
    assert lib.wca_test_gemm_rows_ex(eng._h, C.byref(wca._lib.GemmRowsDesc())) == INVALID and b"null" in lib.wca_last_error()


# ------------------------------------------------------------------------------- the standalone LayerNorm kernels on the probe rows
@pytest.mark.parametrize("d", ref.LN_WIDTHS)
def test_layernorm_kernels_on_the_probe_rows(eng, lib, wca, d):
    """csrc/elementwise.hip at all seven widths, rows 1 .. 9 (every partial four-row block): the single output and the pair's hi half equal the
    planted image, hi + lo is within 3e-6 of float64. The pair form runs on an output 16 bytes aligned (from 512 on: the eight-wide kernel) and
    on one 8 bytes past that, which sends d >= 512 to the four-wide fallback."""
    gamma, beta = ref.ln_gamma_beta(d)
    gd, bd = gamma.float().cuda(), beta.float().cuda()
    for rows in range(1, 10):
        x = ref.ln_x(rows, d)
        image, y64 = ref.ln_image(rows, d).half().cuda(), ref.layernorm64(x, gamma, beta).cuda()
        xd = x.float().cuda()
        out = torch.full((rows + 1, d), float("nan"), dtype=torch.float16, device="cuda")
        wca._lib.check(lib.wca_test_layernorm(eng._h, _vp(xd), _vp(gd), _vp(bd), _vp(out), rows, d))
        torch.cuda.synchronize()
        assert torch.equal(out[:rows], image) and bool(torch.isnan(out[rows]).all()), (d, rows)
        for shift in (0, 4):
            buf = torch.full(((rows + 1) * 2 * d + 8,), float("nan"), dtype=torch.float16, device="cuda")
            assert buf.data_ptr() % 16 == 0
            out2 = buf[shift:shift + (rows + 1) * 2 * d].view(rows + 1, 2 * d)
            wca._lib.check(lib.wca_test_layernorm_split(eng._h, _vp(xd), _vp(gd), _vp(bd), C.c_void_p(out2.data_ptr()), rows, d))
            torch.cuda.synchronize()
            assert torch.equal(out2[:rows, :d], image), (d, rows, shift)
            err = float((out2[:rows, :d].double() + out2[:rows, d:].double() - y64).abs().max())
            assert err <= PAIR_TOL, (d, rows, shift, err)
            assert bool(torch.isnan(out2[rows]).all()) and bool(torch.isnan(buf[:shift]).all()) and bool(torch.isnan(buf[shift + (rows + 1) * 2 * d:]).all())
