"""The index arithmetic of the four tile GEMM forms of csrc/gemm.hip on the MI355X (`-m gpu`), with the exact probe families of
tests/gemm_tile_probe_ref.py at every shape where an index expression of a kernel changes value: the 128 x 128 kernel with its scalar-store paths
and its split-K reduce at splits 4, 3, 2 and 1; the two-barrier 256 x 256 kernel with the conv stem's overlapping windows; the persistent kernel on
tile grids of 1 .. 50 tiles walked by 1 .. 9 workgroups under three supertile heights, in both W-row permutations; its pair forms on three A slots
and on two-slot rings; its residual + LayerNorm epilogue at every panel width the plan accepts, with idle workgroups and several rounds; the skinny
kernel. tests/test_gemm_tile_probe_ref.py proves on the CPU that the families are exact, that the plan gives every launch the kernel and grid its
entry states, and that none of twenty-eight index errors hides in a launch it applies to.

Every launch goes through wca_test_gemm_ex on operands built once per module on the device (poison in the ld padding and behind the operand) and
asserts the planned kernel and grid. Every output buffer is refilled with a sentinel before each launch (NaN; for the accumulating modes -555 around
the addend / x0) and must keep it in the ld gaps, the rows from M on, the columns from N on and behind the lo half of a pair row.

Bounds, from the references and the number formats (never from the kernels): every comparison without GELU is equality with the float64 reference
cast to the output type -- every partial sum is exact in fp32, one f16 rounding of an exact value is the reference's `.half()`; a pair store's hi half
equals `.half()` and hi + lo is within the project's pair bound of float64 (3e-6, test_gemm_rows_probes_gpu.PAIR_TOL; the values here fit a pair
exactly); a GELU run is within one f16 spacing at the reference for an f16 store and within the bounds of gelu_erf / gelu_erfc2 that
test_gemm_forms_gpu.py takes from csrc/wca_common.h for the f32 and the pair store; ln_out EQUALS the planted image and x the target."""
import ctypes as C
import importlib
import time

import pytest
import torch

import gemm_tile_probe_ref as ref
from test_gemm_forms_gpu import ERF_BOUNDS, ERFC2_BOUNDS, FP32_MIN_NORMAL, PAIR_ABS, PAIR_REL
from test_gemm_rows_probes_gpu import PAIR_TOL

pytestmark = pytest.mark.gpu

A_POISON, W_POISON, GAP = 99.0, 77.0, -555.0
TAIL = 64      # poisoned elements behind every operand, sentinel elements behind every output


@pytest.fixture(scope="module")
def eng(wca):
    syn = importlib.import_module("whisper-char-alignment_amd.synthetic")
    dims = wca.ModelDimensions(80, 1500, 384, 6, 2, 51865, 448, 384, 6, 2)
    m = wca.WhisperAMD(dims, device="cuda:0", max_batch=2, precision="f16")
    m.load_state_dict(syn.random_state_dict(dims, seed=1))
    m._bind_stream()
    assert torch.cuda.get_device_properties(0).multi_processor_count == ref.N_CU
    return m


def _rows(t, ld, poison, dtype=torch.float16):
    """t [R][C] as a flat device buffer of rows ld apart, poison in the padding and in TAIL elements behind the last row"""
    out = torch.full((t.shape[0] * ld + TAIL,), poison, dtype=dtype)
    out[:t.shape[0] * ld].view(t.shape[0], ld)[:, :t.shape[1]] = t
    return out.cuda()


class Operands:
    """The device operands and references, built once and keyed by what they depend on"""

    def __init__(self):
        self.cache, self.launches, self.worst, self.met = {}, {}, {}, 0

    def get(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    def a16(self, L):
        """(buffer, lda)"""
        if L.window:
            return self.get(("a", L.window, L.K), lambda: torch.cat([ref.window_flat(L), torch.full((TAIL,), A_POISON, dtype=torch.float64)]).half().cuda()), ref.window_geometry(L)[2]
        lda = (2 * L.K if L.pair else L.K) + L.lda_pad

        def make():
            a = ref.a_hi(L)
            return _rows(torch.cat([a, ref.lo_a(L.M, L.K)], 1) if L.pair else a, lda, A_POISON)
        return self.get(("a", L.fam == "comb", bool(L.pair), L.M, L.K, lda), make), lda

    def w16(self, L):
        ldw = (2 * L.K if L.pair == 2 else L.K) + L.ldw_pad

        def make():
            w = ref.w_of(L)
            return _rows(torch.cat([w, w], 1) if L.pair == 2 else w, ldw, W_POISON)
        return self.get(("w", L.w, L.pair == 2, L.N, L.K, ldw), make), ldw

    def bias(self, L):
        return self.get(("bias", L.bias, L.N), lambda: ref.bias_of(L.bias, L.N).float().cuda()) if L.bias else None

    def gamma_beta(self, N):
        return self.get(("gb", N), lambda: tuple(t.float().cuda() for t in ref.ln_gamma_beta(N)))

    def want(self, L):
        """the float64 reference on the device (for the LayerNorm form: x, ln_out, x0), once per set of value-determining fields"""
        key = ref._math_key(L)._replace(out_mode=L.out_mode if L.out_mode in (2, 3) else 1, gelu=L.gelu, bias=L.bias)
        return self.get(("want", key), lambda: ref.reference(L, dev="cuda"))


@pytest.fixture(scope="module")
def ops():
    return Operands()


def _layout(L):
    """(ldc, c_lo, rows of the buffer): two sentinel rows behind the output; a pair row is [hi | gap | lo | gap]"""
    if L.out_mode == 4:
        return 2 * (L.N + L.ldc_pad), L.N + L.ldc_pad, L.M + 2
    return L.N + L.ldc_pad, 0, L.M + 2


def _launch(eng, lib, wca, ops, L, c, ln_out=None):
    a, lda = ops.a16(L)
    w, ldw = ops.w16(L)
    ldc, c_lo, _ = _layout(L)
    d = wca._lib.GemmDesc()
    d.a, d.w, d.c = a.data_ptr(), w.data_ptr(), c.data_ptr()
    bias = ops.bias(L)
    d.bias = bias.data_ptr() if bias is not None else None
    d.M, d.N, d.K, d.lda, d.ldw, d.ldc = L.M, L.N, ref.k_arg(L), lda, ldw, ldc
    d.a_lo, d.c_lo = (L.K if L.pair == 1 else 0), c_lo
    if L.window:
        _, T, _, bs, _ = ref.window_geometry(L)
        d.a_rows_per_batch, d.a_batch_stride = T, bs
    d.gelu, d.out_mode, d.force_tile, d.site, d.cu_limit, d.supertile = L.gelu, L.out_mode, L.force_tile, L.site, L.cu_limit, L.supertile
    if L.out_mode == 3:
        gamma, beta = ops.gamma_beta(L.N)
        d.ln_gamma, d.ln_beta, d.ln_out, d.ln_ld = gamma.data_ptr(), beta.data_ptr(), ln_out.data_ptr(), L.N + L.ln_ld_pad
    plan = (C.c_int32 * 2)(-1, -1)
    rc = lib.wca_test_gemm_ex(eng._h, C.byref(d), plan)
    assert rc == 0, (rc, lib.wca_last_error(), L)
    assert (plan[0], plan[1]) == (L.form, L.grid), "planned kernel %d on %d workgroups, meant %d on %d: %s" % (plan[0], plan[1], L.form, L.grid, L)
    ops.launches[L.sweep] = ops.launches.get(L.sweep, 0) + 1


def _same(got, want, L, what):
    ok = (got == want) | (torch.isnan(got) & torch.isnan(want))
    if not bool(ok.all()):
        i = (~ok).nonzero()[0].tolist()
        raise AssertionError("%s of %s: %d of %d elements differ, first at %s: got %r, want %r" %
                             (what, L, int((~ok).sum()), ok.numel(), i, got[tuple(i)].item(), want[tuple(i)].item()))


def _kept(t, sentinel, L, what):
    ok = torch.isnan(t) if sentinel != sentinel else t == sentinel
    assert bool(ok.all()), "%s of %s: %d elements outside the output were written" % (what, L, int((~ok).sum()))


def _buffer(L, rows, ld, dtype, sentinel, live=None):
    buf = torch.full((rows * ld + TAIL,), sentinel, dtype=dtype, device="cuda")
    if live is not None:
        buf[:rows * ld].view(rows, ld)[:L.M, :L.N] = live.to(dtype)
    return buf


def _gaps(L, buf, rows, ld, sentinel, what, c_lo=0):
    v = buf[:rows * ld].view(rows, ld)
    _kept(v[L.M:], sentinel, L, what + " (rows from M on)")
    _kept(buf[rows * ld:], sentinel, L, what + " (behind the buffer)")
    if c_lo:
        _kept(v[:L.M, L.N:c_lo], sentinel, L, what + " (between hi and lo)")
        _kept(v[:L.M, c_lo + L.N:], sentinel, L, what + " (behind lo)")
    else:
        _kept(v[:L.M, L.N:], sentinel, L, what + " (columns from N on)")
    return v


def _gelu_within(x, got, want, bounds, pair):
    """the per-interval bounds of test_gemm_forms_gpu.py on the points of this launch (an interval without points, or without a bound, asks nothing)"""
    ok = True
    for _, select, abs_b, rel_b in bounds:
        sel = select(x)
        if not bool(sel.any()):
            continue
        r = want[sel].abs()
        err = (got[sel] - want[sel]).abs()
        if pair:
            err = (err - PAIR_REL * r - PAIR_ABS).clamp_min(0.0)
        norm = r >= FP32_MIN_NORMAL
        ok &= abs_b is None or float(err.max()) <= abs_b
        ok &= rel_b is None or not bool(norm.any()) or float((err[norm] / r[norm]).max()) <= rel_b
    return ok


def _note(ops, L, name, value):
    ops.worst[(L.sweep, name)] = max(ops.worst.get((L.sweep, name), 0.0), float(value))


def _run(eng, lib, wca, ops, L, kept):
    """One launch with its checks. kept: the pair stores of the three-slot ring, for the two-slot ring to meet bit for bit."""
    ldc, c_lo, rows = _layout(L)
    want = ops.want(L)
    nan = float("nan")
    if L.out_mode == 3:
        x_want, ln_want, x0 = want
        ln_ld = L.N + L.ln_ld_pad
        for again in (0, 1):                      # twice on the same statistics workspace and arrival counters
            x = _buffer(L, rows, ldc, torch.float32, GAP, x0)
            ln_out = _buffer(L, rows, ln_ld, torch.float16, nan)
            _launch(eng, lib, wca, ops, L, x, ln_out)
            _same(_gaps(L, x, rows, ldc, GAP, "x")[:L.M, :L.N], x_want.float(), L, "x" + " of the second launch" * again)
            _same(_gaps(L, ln_out, rows, ln_ld, nan, "ln_out")[:L.M, :L.N], ln_want.half(), L, "ln_out" + " of the second launch" * again)
        return
    dtype = torch.float16 if L.out_mode in (0, 4) else torch.float32
    for again in range(2 if L.splitk > 1 else 1):  # a split launch twice: the partials are added in slice order from a workspace that is written anew
        c = _buffer(L, rows, ldc, dtype, GAP, ref.addend(L).cuda()) if L.out_mode == 2 else _buffer(L, rows, ldc, dtype, nan)
        _launch(eng, lib, wca, ops, L, c)
        v = _gaps(L, c, rows, ldc, GAP if L.out_mode == 2 else nan, "C", c_lo)
        got = v[:L.M, :L.N]
        if L.out_mode == 4:
            both = got.double() + v[:L.M, c_lo:c_lo + L.N].double()
            key = (ref._math_key(L), L.gelu, L.bias)
            if L.ring == 0 and L.form == ref.PAIR3:
                kept[key] = v[:L.M].clone()
            elif L.ring == 1 and key in kept:
                assert torch.equal(v[:L.M].view(torch.int16), kept[key].view(torch.int16)), "the two rings differ: %s" % (L,)
                ops.met += 1
        if L.gelu:
            pre = ops.want(L._replace(gelu=0))
            if L.out_mode == 0:
                err = ((got.double() - want).abs() / ref.spacing_f16(want)).max()
                assert bool(torch.isfinite(got).all()) and float(err) <= 1.0, (L, float(err))
                _note(ops, L, "GELU f16 store, f16 spacings at the reference", err)
            else:
                g = both if L.out_mode == 4 else got.double()
                assert bool(torch.isfinite(g).all())
                assert _gelu_within(pre.reshape(-1), g.reshape(-1), want.reshape(-1), ERFC2_BOUNDS if L.out_mode == 4 else ERF_BOUNDS, L.out_mode == 4), L
                _note(ops, L, "GELU out_mode %d, abs" % L.out_mode, (g - want).abs().max())
        elif L.out_mode == 4:
            _same(got, want.half(), L, "the hi halves")
            err = (both - want).abs().max()
            assert float(err) <= PAIR_TOL, (L, float(err))
            _note(ops, L, "hi + lo against float64", err)
        else:
            _same(got, want.to(dtype), L, "C" + " of the second launch" * again)


@pytest.mark.parametrize("sweep", list(ref.SWEEPS))
def test_sweep_equals_float64(eng, lib, wca, ops, switch, sweep):
    t0 = time.time()
    kept = {}
    launches = sorted(ref.SWEEPS[sweep], key=lambda L: L.ring)      # the three-slot ring's pair stores first: the two-slot ring must meet them
    for L in launches:
        switch("gemm_ring", L.ring)
        _run(eng, lib, wca, ops, L, kept)
        if L.sweep in ("pair", "ln", "gelu"):
            ops.cache = {k: v for k, v in ops.cache.items() if k[0] != "want" or (k[1].M, k[1].N, k[1].K) == (L.M, L.N, L.K)}   # (the large references: one shape at a time)
    if sweep == "pair":
        assert ops.met >= 3      # pair stores of the two-slot rings that met the three-slot ring's bit for bit
        assert {L.ring for L in launches} == {0, 1}
    torch.cuda.synchronize()
    print("%s: %d launches of %d entries, %.1f s; everything but the following EQUALS float64 cast to the output type, sentinels intact" %
          (sweep, ops.launches[sweep], len(launches), time.time() - t0))
    for (s, name), v in sorted(ops.worst.items()):
        if s == sweep:
            print("  %s: %s: %.3g" % (sweep, name, v))
