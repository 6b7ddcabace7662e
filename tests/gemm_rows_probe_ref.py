"""Test helper: input families made for the INDEX arithmetic of the few-row GEMM (csrc/gemm_rows.hip), their float64 references written from
the definition C = epilogue(A W^T), the launches that tests/test_gemm_rows_probe_ref.py pins on the CPU and tests/test_gemm_rows_probes_gpu.py
runs on the GPU, and the index errors (MUTATIONS) those launches must tell from the truth. With randn operands at K = 1024 .. 5120 one dropped
32-wide k step moves an output by about 3 % of its spread, inside an f16 tolerance for part of the columns. Here every input value is exactly
representable in f16 and every partial sum of every product is an integer (or a multiple of 0.5) far below 2^24: |sum| <= K max|a| max|w| <=
8192 * 5 * 2 (SUM_BOUND), so the fp32 accumulation is exact in any order. The kernel's f32 result must EQUAL the float64 reference and its
f16 result the reference rounded once (`.half()`); only a GELU leaves one f16 spacing.

comb (identifies k): W [128][K] with W[n][k] = 1 where k % 128 == n, else 0; A[m][k] = CODE[(k // 8 + 2 (k % 8) + m) % 9], nine distinct values
of +-{1 .. 5}. The code differs between k and k +- 8, k +- 32 j (j = 1 .. 8: every K quarter of a slice of 128 .. 1024), k +- 128 j (every split
slice), and between rows m and m +- 1, 8, 16, 64 (none of these offsets, over 8, is a multiple of 9). C[m][n] is the sum of row m over tooth n.
A symmetric exchange of two A slices is the one thing a W of period 128 cannot see, so the depth sweep runs the count family as well.

count (identifies rows, columns, bias, accumulation): A is +-1 per (m, k), W in {-1, 0, +1} per (n, k), both seeded; bias[n] = (7 n) % 17 - 8
(neighbours differ); the out_mode 2 addend c0[m][n] = m N + n - (M N) // 2, distinct per element.

LayerNorm probe (A_MODE 1, an exact image): row m of x holds +-s_m with exactly K / 2 of each sign, shuffled per row; s_m cycles through
{0.25, 0.5, 1, 2, 4} in a seeded order (m and m +- 1, 8, 16, 64 differ); gamma[k] in {0.5, 1, 2}, beta[k] in {-3, +3}. Mean 0 and variance
s_m^2 are exact, LN(x)[m][k] = +-gamma (1 - eps') + beta with eps' <= 8e-5 rounds to the f16 value +-gamma[k] + beta[k] (|.| >= 1: never the
0 that beta in -2 .. 2 would need reproduced). A row that takes another row's statistics is off by a factor of 2 or more. The GEMM on the image
runs with the count W: sums are multiples of 0.5 below 2^13.

GELU runs (fc1's form): f16 rows of +-1 against a W of six +-1 per row and bias (7 n) % 5 - 2, or the LayerNorm image against a W of ONE +-1
per row, so that the pre-activation v is exact and |v| <= 8; |got - gelu64(v)| <= one f16 spacing at the reference (2^-24 below 2^-14).

A launch is a Launch tuple; SWEEPS lists, per sweep, the smallest shapes at which each index expression of the kernel changes value."""
import functools
import math
from typing import NamedTuple

import torch

from attention_probe_ref import spacing_f16  # noqa: F401  (the GELU bound of the GPU test)

SEED = 0
TEETH = 128
CODE = (1.0, -2.0, 3.0, -4.0, 5.0, -1.0, 2.0, -3.0, 4.0)
SCALES = (0.25, 0.5, 1.0, 2.0, 4.0)
ROWS_MAX, K_MAX = 193, 8192
SUM_BOUND = K_MAX * 5 * 2
LN_EPS = 1e-5
T_MAX = 7
K_SENTINEL, V_SENTINEL = -777.0, -778.0          # what the caches hold before a launch; C holds NaN
LN_WIDTHS = (128, 256, 384, 512, 768, 1024, 1280)   # what launch_layernorm_f16 takes


class Launch(NamedTuple):
    sweep: str
    M: int
    N: int
    K: int
    a: str = "sign"          # "comb" / "sign" f16 rows, "ln" the LayerNorm prologue on the probe rows
    w: str = "dense"         # "comb", "dense" (count family), "sparse6" / "sparse1" (GELU runs)
    S: int = 0               # splitk, 0 = the launcher's choice
    groups: int = 0
    out_mode: int = 1
    gelu: int = 0
    bias: str = "std"        # "std", "small" (GELU runs), "" none
    lda_pad: int = 0         # elements added to the tight leading dimension
    lda32_pad: int = 0
    ldw_pad: int = 0
    ldc_pad: int = 0
    c_rows: int = 0          # c_rows_per_batch
    c_gap: int = 0           # c_batch_stride = c_rows * ldc + c_gap
    kv_d: int = 0            # > 0: KV append with caches [M][T_MAX][kv_d]
    kv_t: object = None      # a scalar position, or the name of a per-row table (KV_TABLES)


def pick_splitk(K):
    """gemm_rows_pick_splitk: the smallest split with K / S a multiple of 128 up to 1024"""
    for s in range(1, 9):
        if K % (s * 128) == 0 and K // s <= 1024:
            return s
    return 0


def splitk(L):
    return L.S or pick_splitk(L.K)


def accepted_splits(K):
    return [s for s in range(1, 9) if K % (s * 128) == 0 and K // s <= 1024]


KV_TABLES = ("perm", "equal", "clamp")


def kv_positions(L):
    """int64 [M]: the position row m asks for (a table may ask for -1 or T_MAX: kv_slots clamps)"""
    m = torch.arange(L.M)
    if L.kv_t == "perm":
        return torch.randperm(T_MAX, generator=torch.Generator().manual_seed(SEED + 31))[m % T_MAX]
    if L.kv_t == "equal":
        return torch.full((L.M,), 4)
    if L.kv_t == "clamp":
        return torch.tensor([-1, T_MAX, 2, T_MAX + 5, -9, 0, T_MAX - 1, 3])[m % 8]
    return torch.full((L.M,), int(L.kv_t))


def kv_slots(L):
    return kv_positions(L).clamp(0, T_MAX - 1)


def _sweeps():
    s = {}
    s["rows"] = [Launch("rows", M, 40, 256, a=a, out_mode=om) for M in list(range(1, 131)) + [192, 193] for a in ("sign", "ln") for om in (0, 1, 2)]
    s["cols"] = [Launch("cols", M, N, 128, groups=g, out_mode=om, bias="std" if om == 0 else "")        # (the logits launch has no bias)
                 for N in list(range(1, 71)) + [255, 256, 257, 4097, 51865] for M in (5, 17) for om in (0, 1) for g in (0, 1, 2, 3, 4, 13)]
    s["depth"] = [Launch("depth", M, TEETH, S * ks, a=a, w=w, S=S, out_mode=om)
                  for S in range(1, 9) for ks in range(128, 1025, 128) for M in (3, 67) for a, w in (("comb", "comb"), ("sign", "dense")) for om in (1, 2)]
    s["ln"] = [Launch("ln", M, 40, K, a="ln", S=S, lda32_pad=pad) for K in (256, 512, 768, 1024) for S in accepted_splits(K)
               for M in (1, 8, 9, 63, 64, 65, 128) for pad in (0, 4)]
    s["gelu"] = ([Launch("gelu", 33, 4 * d, d, w="sparse6", out_mode=0, gelu=1, bias="small") for d in (384, 512, 768, 1024, 1280)] +
                 [Launch("gelu", 33, 4 * d, d, a="ln", w="sparse1", out_mode=0, gelu=1, bias="small") for d in (512, 768, 1024)])
    s["kv"] = [Launch("kv", M, 3 * d, 256, a=a, out_mode=0, kv_d=d, kv_t=t) for d in (16, 48, 256) for M in (1, 5, 64, 65, 128)
               for t in (0, 3, 6) + KV_TABLES for a in ("sign", "ln")]
    s["strides"] = [Launch("strides", 37, 40, 384, out_mode=om, lda_pad=8, ldw_pad=8, ldc_pad=pad, c_rows=cr, c_gap=24 if cr else 0)
                    for om in (0, 1, 2) for pad in (1, 4) for cr in (0, 5)]
    return s


SWEEPS = _sweeps()


# ------------------------------------------------------------------------------- inputs (float64 tensors of f16-exact values)
def _gen(salt):
    return torch.Generator().manual_seed(SEED + salt)


def comb_a(M, K):
    m, k = torch.arange(M).view(-1, 1), torch.arange(K).view(1, -1)
    return torch.tensor(CODE, dtype=torch.float64)[(k // 8 + 2 * (k % 8) + m) % 9]


@functools.lru_cache(maxsize=None)
def _sign_master():
    return torch.randint(0, 2, (ROWS_MAX, K_MAX), generator=_gen(1)).double() * 2 - 1


def sign_a(M, K):
    return _sign_master()[:M, :K]


def comb_w(K):
    return (torch.arange(K).view(1, -1) % TEETH == torch.arange(TEETH).view(-1, 1)).double()


@functools.lru_cache(maxsize=None)
def dense_w(N, K):
    return torch.randint(-1, 2, (N, K), generator=_gen(1000003 * N + K)).double()


@functools.lru_cache(maxsize=None)
def sparse_w(N, K, nnz):
    g = _gen(2000003 * N + K + nnz)
    idx = torch.rand(N, K, generator=g).topk(nnz, dim=1).indices
    w = torch.zeros(N, K, dtype=torch.float64)
    w.scatter_(1, idx, torch.randint(0, 2, (N, nnz), generator=g).double() * 2 - 1)
    return w


def bias_of(name, N):
    n = torch.arange(N)
    return {"std": ((7 * n) % 17 - 8).double(), "small": ((7 * n) % 5 - 2).double(), "": None}[name]


def addend(M, N):
    return (torch.arange(M).view(-1, 1) * N + torch.arange(N).view(1, -1) - (M * N) // 2).double()


def ln_scales(M):
    order = torch.randperm(5, generator=_gen(3))
    return torch.tensor(SCALES, dtype=torch.float64)[order[torch.arange(M) % 5]]


@functools.lru_cache(maxsize=None)
def ln_signs(K):
    """[ROWS_MAX][K] of +-1 with exactly K / 2 of each in every row"""
    rank = torch.rand(ROWS_MAX, K, generator=_gen(5000 + K)).argsort(dim=1)
    return torch.where(rank < K // 2, 1.0, -1.0).double()


@functools.lru_cache(maxsize=None)
def ln_gamma_beta(K):
    g = _gen(7000 + K)
    gamma = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (K,), generator=g)]
    beta = torch.randint(0, 2, (K,), generator=g).double() * 6 - 3
    return gamma, beta


def ln_x(M, K):
    return ln_signs(K)[:M] * ln_scales(M).view(-1, 1)


def ln_image(M, K):
    """the f16 values the LayerNorm of ln_x must round to"""
    gamma, beta = ln_gamma_beta(K)
    return ln_signs(K)[:M] * gamma + beta


def layernorm64(x, gamma, beta, stats_of=None):
    """whisper's LayerNorm from the definition in float64 (biased variance, eps inside the root); stats_of [M]: the row whose statistics row m uses"""
    mean, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
    if stats_of is not None:
        mean, var = mean[stats_of], var[stats_of]
    return (x - mean) / torch.sqrt(var + LN_EPS) * gamma + beta


def gelu64(v):
    """v Phi(v), through erfc (no cancellation in the negative tail)"""
    return 0.5 * v * torch.erfc(-v / math.sqrt(2.0))


def operands(L):
    """The host operands of a launch, float64: a [M][K] (the planted image for the LayerNorm prologue), w [N][K], bias [N] or None, c0 [M][N] or None"""
    a = {"comb": comb_a, "sign": sign_a, "ln": ln_image}[L.a](L.M, L.K)
    w = comb_w(L.K) if L.w == "comb" else dense_w(L.N, L.K) if L.w == "dense" else sparse_w(L.N, L.K, int(L.w[6:]))
    assert w.shape == (L.N, L.K)
    return a, w, bias_of(L.bias, L.N), addend(L.M, L.N) if L.out_mode == 2 else None


# ------------------------------------------------------------------------------- index errors
# name -> what the kernel would have done wrong; each is applied to the reference's own index arguments (reference(L, mutate))
MUTATIONS = (
    "drop_last_k_step",          # wave (slice 0, quarter 1) stops one 32-wide step early
    "read_quarter_twice",        # wave (slice 0, quarter 2) multiplies quarter 1 again
    "a_next_quarter",            # the A fragment of every wave comes from the next quarter of its slice (W from the right one)
    "a_shift_8",                 # ... from 8 columns on (the lane group's offset)
    "a_shift_32",                # ... from the next k step
    "swap_split_slices",         # the images of slices 0 and 1 change places (W stays)
    "swap_split_partials",       # the partial tiles (column group 0, slice 1) and (column group 1, slice 0) change places in the workspace
    "lose_split_partial",        # the last slice's partial is not added
    "tail_row_takes_previous",   # in the last 16-row tile, row m holds row m - 1
    "column_group_shift_16",     # column n holds the product of column n + 16 (the next ring slot)
    "bias_shift_one",            # bias[n + 1] on column n
    "accumulate_twice",          # out_mode 2 adds the result twice
    "ln_stats_of_neighbour",     # LayerNorm row m uses the statistics of row m + 8 (m - 1 in the last eight)
    "kv_t_off_by_one",           # cache position t + 1 (t - 1 from the last slot)
    "kv_neighbour_row",          # rows 2 j and 2 j + 1 append to each other's cache row
    "kv_planes_swapped",         # k columns to the V plane and back
)


def applies(mutate, L):
    S = splitk(L)
    # What the comb cannot see, and the count family of the same depth launch does: a rotation of A by a multiple of 128 inside a slice keeps
    # every tooth's sum; and where K is a multiple of 9 * 128 every tooth of every row holds whole cycles of CODE (separating k from k +- 128 j
    # for every j up to 8 takes nine classes that a tooth walks in turn), so every output is 5 K / 1152 and only a k that is lost or counted twice shows
    whole = L.w == "comb" and L.K % (9 * TEETH) == 0
    return {
        "drop_last_k_step": True, "read_quarter_twice": True, "a_shift_8": not whole, "a_shift_32": not whole,
        "a_next_quarter": not whole and (L.w != "comb" or (L.K // S // 4) % TEETH != 0),
        "swap_split_slices": S > 1 and L.w != "comb",
        "swap_split_partials": S > 1 and L.N >= 32 and not whole,
        "lose_split_partial": S > 1,
        "tail_row_takes_previous": L.M >= 2 and not whole,
        "column_group_shift_16": L.N > 16 and not whole,
        "bias_shift_one": bool(L.bias) and L.N >= 2,
        "accumulate_twice": L.out_mode == 2,
        "ln_stats_of_neighbour": L.a == "ln" and L.M >= 2,
        "kv_t_off_by_one": L.kv_d > 0,
        "kv_neighbour_row": L.kv_d > 0 and L.M >= 2,
        "kv_planes_swapped": L.kv_d > 0,
    }[mutate]


def _product(L, a, w, mutate):
    """sum_k a[m][k] w[n][k] in float64 -- with the k, row and column index maps a mutation bends"""
    M, N, K, S = L.M, L.N, L.K, splitk(L)
    Ks = K // S
    Kw = Ks // 4
    k = torch.arange(K)
    in_slice = k % Ks
    if mutate == "drop_last_k_step":
        a = a.clone()
        a[:, 2 * Kw - 32:2 * Kw] = 0
    elif mutate == "read_quarter_twice":
        a, w = a.clone(), w.clone()
        a[:, 2 * Kw:3 * Kw] = a[:, Kw:2 * Kw]
        w[:, 2 * Kw:3 * Kw] = w[:, Kw:2 * Kw]
    elif mutate == "a_next_quarter":
        a = a[:, k - in_slice + (in_slice + Kw) % Ks]
    elif mutate == "a_shift_8":
        a = a[:, k - in_slice + (in_slice + 8) % Ks]
    elif mutate == "a_shift_32":
        a = a[:, k - in_slice + (in_slice + 32) % Ks]
    elif mutate == "swap_split_slices":
        a = torch.cat([a[:, Ks:2 * Ks], a[:, :Ks], a[:, 2 * Ks:]], 1)
    elif mutate == "lose_split_partial":
        a = a[:, :K - Ks]
        w = w[:, :K - Ks]
    elif mutate == "tail_row_takes_previous":
        rows = torch.arange(M)
        tail = rows >= (M - 1) // 16 * 16
        a = a[torch.where(tail & (rows > 0), rows - 1, rows)]
    elif mutate == "column_group_shift_16":
        w = w[(torch.arange(N) + 16).clamp(max=N - 1)]
    p = a @ w.T
    if mutate == "swap_split_partials":
        # (group 2 where the slices are 1024 deep and there is one: the comb's code walks 2 classes per column group and 7 per 128 k, so that there
        # the partial of (group 1, slice 0) IS that of (group 0, slice 1))
        g = 32 if Ks == 1024 and N >= 48 else 16
        s0 = a[:, :Ks] @ w[:, :Ks].T
        s1 = a[:, Ks:2 * Ks] @ w[:, Ks:2 * Ks].T
        p[:, 0:16] += s0[:, g:g + 16] - s1[:, 0:16]
        p[:, g:g + 16] += s1[:, 0:16] - s0[:, g:g + 16]
    return p


@functools.lru_cache(maxsize=None)
def _true_product(L):
    a, w, _, _ = operands(L)
    return _product(L, a, w, None)


def _math_key(L):
    """the fields the value of C depends on (not the grid shape, the strides or the cache routing)"""
    return L._replace(sweep="", S=splitk(L), groups=0, lda_pad=0, lda32_pad=0, ldw_pad=0, ldc_pad=0, c_rows=0, c_gap=0, kv_d=0, kv_t=None,
                      out_mode=0, gelu=0, bias="")


def reference(L, mutate=None):
    """float64: c [M][N] = epilogue(A W^T), and for a KV launch (c with NaN in the k / v columns, kc, vc [M][T_MAX][d] with the sentinels where nothing
    lands). mutate: one of MUTATIONS, bending the index arguments of this very computation."""
    assert mutate is None or (mutate in MUTATIONS and applies(mutate, L)), (mutate, L)
    a, w, bias, c0 = operands(L)
    if mutate == "ln_stats_of_neighbour":
        m = torch.arange(L.M)
        a = layernorm64(ln_x(L.M, L.K), *ln_gamma_beta(L.K), stats_of=torch.where(m + 8 < L.M, m + 8, (m - 1).clamp(min=0)))
    if mutate in (None, "bias_shift_one", "accumulate_twice", "kv_t_off_by_one", "kv_neighbour_row", "kv_planes_swapped"):
        v = _true_product(_math_key(L)).clone()
    else:
        v = _product(L, a, w, mutate)
    if bias is not None:
        v = v + (bias[(torch.arange(L.N) + 1).clamp(max=L.N - 1)] if mutate == "bias_shift_one" else bias)
    if L.gelu:
        v = gelu64(v)
    if L.out_mode == 2:
        v = c0 + (2 * v if mutate == "accumulate_twice" else v)
    if not L.kv_d:
        return v
    d = L.kv_d
    slot = kv_slots(L)
    if mutate == "kv_t_off_by_one":
        slot = torch.where(slot + 1 < T_MAX, slot + 1, slot - 1)
    row = torch.arange(L.M)
    if mutate == "kv_neighbour_row":
        row = torch.where((row ^ 1) < L.M, row ^ 1, row)
    kc = torch.full((L.M, T_MAX, d), K_SENTINEL, dtype=torch.float64)
    vc = torch.full((L.M, T_MAX, d), V_SENTINEL, dtype=torch.float64)
    kpart, vpart = v[:, d:2 * d], v[:, 2 * d:]
    if mutate == "kv_planes_swapped":
        kpart, vpart = vpart, kpart
    kc[row, slot], vc[row, slot] = kpart, vpart
    c = v.clone()
    c[:, d:] = float("nan")
    return c, kc, vc


def flat(ref):
    """every asserted output of a launch as one vector (NaN, the untouched C of a KV launch, as 0)"""
    parts = ref if isinstance(ref, tuple) else (ref,)
    return torch.cat([torch.nan_to_num(p, nan=0.0).reshape(-1) for p in parts])


def f16_boundary_distance(y):
    """how far each float64 value is from the nearest point where its f16 rounding changes"""
    h = y.half().double()
    up = spacing_f16(h) / 2
    pow2 = torch.frexp(h.abs())[0] == 0.5
    down = torch.where(pow2, up / 2, up)
    d = y.abs() - h.abs()
    return torch.where(d >= 0, up - d, down + d)
