"""plan_gemm (csrc/gemm_plan.cpp): which kernel, grid and LDS launch_gemm gives a GEMM, pinned without a GPU through wca_test_gemm_plan.
The expected values were read off launch_gemm as it stood before the plan was split from it (and a seeded differential run of that
code against plan_gemm found no difference: profiles/gemm_plan_ab.txt); none is copied from plan_gemm's output."""
import ctypes
import itertools

import pytest

NONE, SKINNY, TILE128, TILE256, PERSIST, PAIR2, PAIR3, LN = range(8)
ADDEND, BATCH_A, POS, BATCH_C, NO_LN_BUFFERS, NO_C_LO = 1, 2, 4, 8, 16, 32
LDS_128, LDS_256 = 64 * 1024, 128 * 1024
LDS_256P = LDS_256 + 2 * 256 * 4
LDS_256P_LN = LDS_256P + (2 * 512 + 2560) * 4
N_CU = 256
D = 1024            # whisper-medium
M64 = 64 * 1500     # the encoder rows of a batch of 64


@pytest.fixture(scope="module")
def plan(lib):
    def call(M, N, K, out_mode=0, gelu=0, pair=False, lda=None, a_lo=None, force_tile=0, site=0, n_cu=N_CU, cu_limit=0, flags=0, sk_bytes=0):
        """dict of the plan, or None where the arguments are refused. pair: [hi | lo] rows against the plain W (a_lo = K, lda = 2 K)"""
        if a_lo is None:
            a_lo = K if pair else 0
        if lda is None:
            lda = 2 * K if pair else K
        out = (ctypes.c_int32 * 10)(*([-1] * 10))
        rc = lib.wca_test_gemm_plan(M, N, K, lda, out_mode, gelu, a_lo, force_tile, site, n_cu, cu_limit, flags, sk_bytes, out)
        if rc != 0:
            assert b"GEMM refused" in lib.wca_last_error()
            assert list(out) == [-1] * 10
            return None
        names = ("kernel", "grid_x", "grid_y", "block", "lds", "splitk", "supertile", "site", "a_bytes", "w_bytes")
        return dict(zip(names, out))
    return call


# (name, N, K, out_mode on pair operands, out_mode on single operands, gelu, site, supertile)
MEDIUM_B64 = [("qkv", 3 * D, D, 4, 0, 0, 1, 8), ("out", D, D, 2, 2, 0, 1, 8), ("fc1", 4 * D, D, 4, 0, 1, 1, 8), ("fc2", D, 4 * D, 2, 2, 0, 4, 1),
              ("cross_kv", 24 * 2 * D, D, 4, 0, 0, 3, 1), ("logits", 51865, D, 1, 1, 0, 3, 1)]


@pytest.mark.parametrize("name,N,K,om_pair,om_single,gelu,site,supertile", MEDIUM_B64)
def test_medium_batch_64_takes_the_persistent_kernel(plan, name, N, K, om_pair, om_single, gelu, site, supertile):
    p = plan(M64, N, K, om_pair, gelu, pair=True, site=site)
    assert (p["kernel"], p["grid_x"], p["grid_y"], p["block"], p["lds"], p["splitk"]) == (PAIR3, N_CU, 1, 512, LDS_256P, 1)
    assert p["supertile"] == supertile and p["site"] == site
    assert p["a_bytes"] == M64 * 2 * K * 2 and p["w_bytes"] == N * K * 2
    s = plan(M64, N, K, om_single, gelu, site=site)
    assert (s["kernel"], s["grid_x"], s["grid_y"], s["block"], s["lds"], s["splitk"]) == (PERSIST, N_CU, 1, 512, LDS_256P, 1)
    assert s["supertile"] == supertile and s["site"] == site
    assert s["a_bytes"] == M64 * K * 2 and s["w_bytes"] == N * K * 2


def test_supertile_rule(plan):
    # 8 where the K of the launch (2 K on pair operands) is at most 2048 and the row has at most 32 tiles
    assert plan(M64, 32 * 256, 2048, 0)["supertile"] == 8 and plan(M64, 33 * 256, 2048, 0)["supertile"] == 1
    assert plan(M64, 4096, 2048 + 128, 0)["supertile"] == 1
    assert plan(M64, 4096, 1024, 4, pair=True)["supertile"] == 8 and plan(M64, 4096, 1024 + 128, 4, pair=True)["supertile"] == 1


@pytest.mark.parametrize("N,K,site", [(D, D, 1), (D, 4 * D, 4)])
def test_residual_layernorm_form(plan, N, K, site):
    p = plan(M64, N, K, 3, site=site)
    assert (p["kernel"], p["grid_x"], p["grid_y"], p["block"], p["lds"], p["site"]) == (LN, N_CU & ~7, 1, 512, LDS_256P_LN, site)
    assert plan(M64, N, K, 3, site=2)["site"] == 1           # the form exists for sites 1 and 4
    assert plan(M64, N, K, 3, n_cu=100)["grid_x"] == 96
    assert plan(M64, N, K, 3, cu_limit=64)["grid_x"] == 64
    assert plan(M64, N, K, 3, n_cu=24) is None               # a round of n_cu / 8 workgroups must hold a whole panel of N / 256 tiles


def test_conv_stem_takes_the_two_barrier_kernel(plan):
    for M, K, om, flags in ((64 * 3000, 256, 0, BATCH_A | BATCH_C), (M64, 3 * D, 1, BATCH_A | POS)):
        p = plan(M, D, K, om, 1, site=3, flags=flags)
        assert (p["kernel"], p["grid_x"], p["grid_y"], p["block"], p["lds"], p["site"]) == (TILE256, (M // 256) * 4, 1, 512, LDS_256, 3)
    # split mode: the K-doubled operands, and the addend of an inexact checkpoint's W_lo term
    p = plan(M64, D, 6 * D, 1, 1, site=3, flags=BATCH_A | POS | ADDEND)
    assert (p["kernel"], p["grid_x"]) == (TILE256, 1500)
    # a flat launch with an addend keeps the generic epilogue too
    assert plan(M64, 3 * D, 2 * D, 4, flags=ADDEND)["kernel"] == TILE256


def test_small_batches_take_the_128_kernel(plan):
    p = plan(1500, 3 * D, D, 0, site=1)      # 6 x 12 = 72 big tiles
    assert (p["kernel"], p["grid_x"], p["grid_y"], p["block"], p["lds"], p["splitk"]) == (TILE128, 12 * 24, 1, 256, LDS_128, 1)
    p = plan(1500, 4 * D, D, 0, 1, site=1)   # 96
    assert (p["kernel"], p["grid_x"], p["grid_y"]) == (TILE128, 12 * 32, 1)
    assert plan(3000, 3 * D, D, 0)["kernel"] == TILE128                        # 144
    assert plan(3000, 3 * D, D, 4, pair=True) is None                          # ... and no pair form there: the caller takes [W | W]
    p = plan(3000, 4 * D, D, 0, 1)                                             # exactly 192
    assert (p["kernel"], p["grid_x"]) == (PERSIST, 192)
    assert (plan(3000, 4 * D, D, 4, 1, pair=True)["kernel"], plan(3000, 4 * D, D, 4, 1, pair=True)["grid_x"]) == (PAIR3, 192)
    # the threshold from both sides
    assert plan(3072, 4096, D, 0)["kernel"] == PERSIST and plan(2816, 4096, D, 0)["kernel"] == TILE128
    assert plan(3072, 4096, D, 4, pair=True)["kernel"] == PAIR3 and plan(2816, 4096, D, 4, pair=True) is None


def test_split_k_of_the_small_batch_fc2(plan):
    M, N, K = 1500, D, 4 * D
    part = M * N * 4
    p = plan(M, N, K, 2, site=4, sk_bytes=4 * part)
    assert (p["kernel"], p["grid_x"], p["grid_y"], p["splitk"]) == (TILE128, 8 * 12, 4, 4)
    assert plan(M, N, K, 2, sk_bytes=4 * part - 1)["splitk"] == 2       # (three slices do not divide 64 K tiles)
    for small in (0, 1 << 20, 2 * part - 1):
        p = plan(M, N, K, 2, sk_bytes=small)
        assert (p["kernel"], p["grid_y"], p["splitk"]) == (TILE128, 1, 1)
    assert plan(M, N, K, 1, sk_bytes=4 * part)["splitk"] == 1           # the accumulating mode only
    assert plan(M, N, 1024, 2, sk_bytes=4 * part)["splitk"] == 1        # K >= 2048
    assert plan(M, N, K, 2, sk_bytes=4 * part, n_cu=190)["splitk"] == 1  # at most n_cu / 2 tiles
    assert plan(M, N, K, 2, sk_bytes=4 * part, cu_limit=64)["splitk"] == 1


def test_skinny_kernel(plan):
    for M, N, K, om in ((64, 51865, 1024, 1), (1, 3 * D, D, 0), (8, D, 4 * D, 2)):
        p = plan(M, N, K, om)
        assert (p["kernel"], p["grid_x"], p["grid_y"], p["block"], p["lds"], p["splitk"]) == (SKINNY, (N + 15) // 16, 1, 256, 0, 1)
    assert plan(65, D, D, 0)["kernel"] == TILE128
    assert plan(8, D, 768, 0)["kernel"] == TILE128           # K % 512
    assert plan(8, D, D, 0, force_tile=128)["kernel"] == TILE128
    assert plan(8, D, D, 0, force_tile=64)["kernel"] == SKINNY
    assert plan(8, D, D, 0, flags=POS)["kernel"] == TILE128
    assert plan(8, D, D, 2, 1) is None


def test_refusals(plan):
    big = dict(M=M64, N=D, K=D)
    assert plan(**big, out_mode=0) is not None
    assert plan(M64, D, 96, 0) is None and plan(M64, D, 0, 0) is None                  # K % 64
    assert plan(M64, D, D, 0, lda=D + 4) is None                                       # lda % 8
    assert plan(**big, out_mode=4, flags=NO_C_LO) is None
    assert plan(**big, out_mode=2, flags=ADDEND) is None
    assert plan(**big, out_mode=3, flags=ADDEND) is None
    assert plan(**big, out_mode=4, pair=True, flags=ADDEND) is None                    # addend with a_lo
    assert plan(**big, out_mode=4, pair=True) is not None
    assert plan(**big, out_mode=4, pair=True, force_tile=128) is None
    assert plan(**big, out_mode=4, pair=True, force_tile=256) is None
    assert plan(**big, out_mode=4, pair=True, flags=BATCH_A) is None
    assert plan(M64, D, 192, 4, pair=True) is None and plan(M64, D, 64, 4, pair=True) is None   # pair K % 128
    assert plan(M64, D, 192, 0) is not None
    assert plan(**big, out_mode=3, pair=True) is None
    assert plan(**big, out_mode=3) is not None
    assert plan(**big, out_mode=3, gelu=1) is None
    assert plan(M64, 1152, D, 3) is None                                               # N % 256
    assert plan(M64, 2304, D, 3) is None and plan(M64, 2048, D, 3) is not None         # N > 2048
    assert plan(**big, out_mode=3, force_tile=258) is None
    assert plan(**big, out_mode=3, force_tile=256) is None and plan(**big, out_mode=3, force_tile=257) is not None
    assert plan(**big, out_mode=3, flags=NO_LN_BUFFERS) is None
    assert plan(**big, out_mode=3, flags=POS) is None and plan(**big, out_mode=3, flags=BATCH_C) is None
    assert plan(M64, D, 192, 3) is None                                                # an even number of K tiles
    assert plan(1500, D, D, 3) is None                                                 # too few tiles
    assert plan(65, D, D, 0, force_tile=64) is None and plan(8, D, 768, 0, force_tile=64) is None
    assert plan(**big, out_mode=2, gelu=1) is None
    assert plan(**big, out_mode=5) is None and plan(**big, out_mode=-1) is None
    assert plan(0, D, D, 0)["kernel"] == NONE and plan(M64, 0, D, 0)["kernel"] == NONE  # nothing to launch is not an error


def test_cu_limit_and_forced_tiles(plan):
    assert plan(M64, D, D, 0, cu_limit=64)["grid_x"] == 64
    assert plan(M64, D, D, 4, pair=True, cu_limit=64)["grid_x"] == 64
    assert plan(M64, D, D, 0, cu_limit=300)["grid_x"] == N_CU
    tiles = 375 * 4
    p = plan(M64, D, D, 0, force_tile=258)
    assert (p["kernel"], p["grid_x"], p["lds"]) == (PERSIST, tiles, LDS_256P)
    p = plan(M64, D, D, 0, force_tile=256)
    assert (p["kernel"], p["grid_x"], p["lds"]) == (TILE256, tiles, LDS_256)
    p = plan(M64, D, D, 0, force_tile=128)
    assert (p["kernel"], p["grid_x"], p["lds"]) == (TILE128, 750 * 8, LDS_128)
    p = plan(1500, 3 * D, D, 0, force_tile=257)     # 72 tiles, fewer than CUs: one each
    assert (p["kernel"], p["grid_x"], p["block"]) == (PERSIST, 72, 512)
    assert plan(M64, D, 192, 0)["grid_x"] == tiles  # an odd number of K tiles: the ring parity does not carry over, one tile per workgroup
    assert plan(M64, D, 64, 0)["grid_x"] == tiles


def test_pair_ring_switch_and_site_folding(plan, switch):
    for site, used in ((0, 1), (1, 1), (2, 2), (3, 3), (4, 4), (7, 1)):
        p = plan(M64, D, D, 4, pair=True, site=site)
        assert (p["kernel"], p["site"]) == (PAIR3, used)
    switch("gemm_ring", 1)
    for site, used in ((0, 1), (1, 1), (2, 1), (3, 1), (4, 4)):
        p = plan(M64, D, D, 4, pair=True, site=site)
        assert (p["kernel"], p["site"], p["grid_x"], p["lds"]) == (PAIR2, used, N_CU, LDS_256P)
    assert plan(M64, D, D, 0, site=2)["kernel"] == PERSIST and plan(M64, D, D, 0, site=2)["site"] == 2


def _splitw_supported(M, N, K, lda, out_mode):
    """gemm_splitw_supported as launch_gemm's callers used it"""
    if M < 1 or N < 1 or K < 128 or K % 128:
        return False
    if out_mode not in (0, 1, 2, 4):
        return False
    if ((M + 255) // 256) * ((N + 255) // 256) < 192:
        return False
    return ((M - 1) * lda + 2 * K) * 2 < 0x7fffffff and ((N - 1) * K + K) * 2 < 0x7fffffff


def _ln_supported(M, N, K, n_cu):
    """gemm_ln_supported likewise"""
    if N % 256 or N > 2048 or K % 128 or M < 1:
        return False
    if ((M + 255) // 256) * (N // 256) < 192:
        return False
    return (n_cu >> 3) >= N // 256


SWEEP_M, SWEEP_N, SWEEP_K = (1, 64, 65, 1500, 3000, 3072, 12000), (384, 1024, 3072, 4096), (64, 128, 384, 1024, 4096)
SWEEP = list(itertools.product(SWEEP_M, SWEEP_N, SWEEP_K))
# no shape of that sweep has 192 tiles in rows of at most 2048 columns: the LayerNorm form is swept over these as well
SWEEP_LN = SWEEP + list(itertools.product((12288, 96000), SWEEP_N + (256, 2048), SWEEP_K)) + list(itertools.product(SWEEP_M, (256, 2048), SWEEP_K))


def test_the_callers_predicates_are_the_plan(plan):
    """What the engine used to ask before it built a launch is what the plan of that launch says: pair operands are kept exactly where
    the launch with a_lo = K gets a pair kernel, the LayerNorm is fused exactly where the out_mode 3 launch gets its kernel."""
    n_pair = n_ln = 0
    for (M, N, K), om in itertools.product(SWEEP, (0, 1, 2, 4)):
        p = plan(M, N, K, om, pair=True)
        assert (p is not None and p["kernel"] in (PAIR2, PAIR3)) == _splitw_supported(M, N, K, 2 * K, om), (M, N, K, om)
        assert p is None or p["kernel"] == PAIR3
        n_pair += p is not None
    for (M, N, K), n_cu in itertools.product(SWEEP_LN, (256, 64, 24)):
        p = plan(M, N, K, 3, n_cu=n_cu)
        assert (p is not None and p["kernel"] == LN) == _ln_supported(M, N, K, n_cu), (M, N, K, n_cu)
        assert p is None or p["kernel"] == LN
        n_ln += p is not None
    assert n_pair >= 40 and n_ln >= 8     # both answers occur
