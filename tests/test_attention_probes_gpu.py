"""The index arithmetic of every attention kernel instance (csrc/attention.hip, csrc/attention_split.hip) on the MI355X (`-m gpu`), with the two
exact probes of tests/attention_probe_ref.py at every key count, query count and causal size where an index expression changes value:
the clamp of staged key rows, the tail / diagonal masks, nk_eff under the causal mask, the one-query kernel's key partition, the XCD remap of
the grid, the capture's column tail. tests/test_attention_probe_ref.py proves on the CPU that the probes hide none of these errors.

Every launch goes through wca_test_attention_ex and addresses a PREFIX of master buffers allocated once: K / V planes [B][1500 + 8][H * 64]
whose rows past a launch's nk are live data (a leaked key is counted by the uniform probe; the last 8 rows hold K = 0, V = 64), Q and O
[B][448][H * 64]. O and the capture buffer are refilled with a sentinel before each launch and must keep it outside the written region.
Pair operands are the same values with zero lo halves; the `-lo` runs give every lo half +-2^-13 and the reference takes hi + lo.

Bounds, from the references and the number formats (never from the kernels):
  uniform probe, f16 kernels   |got - ref| <= one f16 spacing at |ref|, and got == 0 where ref == 0: p = exp2(0) = 1, the row sum and the P.V sums
                               are exact integers; one fp32 reciprocal-multiply (or division) and one f16 rounding remain
  uniform probe, pair kernels  |hi + lo - ref| <= 3e-6, the project's pair bound
  peaked probe, f16 kernels    <= 4e-3 against float64, the project's f16 bound: |v| <= 2, one f16 rounding of P and one of O at 2^-11 each,
                               leaked mass at most 1e-5
  peaked probe, pair kernels   <= 3e-6
  capture                      the captured logits EQUAL the float64 q.k / 8 on [0, cap_cols) (integers, exact in every pass); sentinel everywhere
                               else: pad columns, the other layers' slices. The `-lo` run's logits are no integers: 4e-7 max|logit| + 1e-6, the
                               bound of test_attention_forms_gpu.py. Under the causal mask a logit above the diagonal is read by nothing: there
                               the buffer holds the raw logit or the sentinel (a 128-row query block does not visit key tiles past its last row)
Each test prints its instance's maxima (`-s`). Measured on the MI355X over all sweeps: uniform probe 0.499 f16 spacings on every f16 instance (the
one rounding) and 2.4e-7 on the pair ones; peaked probe 1.2e-6 (f16; 3.1e-6 on one per-row decode launch) and 3.2e-7 (pairs); every capture
equal, 7.5e-8 in the `-lo` run."""
import ctypes as C
import importlib

import pytest
import torch

import attention_probe_ref as ref

pytestmark = pytest.mark.gpu

O_SENTINEL, CAP_SENTINEL = -777.0, -777.25
HD = ref.H * ref.HEAD
LAYERS = 3                      # the capture goes to layer 1's slice of a [B][LAYERS][H][nq][cap_ld] buffer
F16_TOL, PAIR_TOL = 4e-3, 3e-6

# label -> the descriptor fields that select the instance (launch_attention / launch_attention_split, restated in _taken)
INSTANCES = {
    "f16-16": dict(variant=1),                                  # attn_kernel<false, false>
    "f16-causal": dict(causal=1),                               # attn_kernel<true, false>
    "f16-cap": dict(cap=True),                                  # attn_kernel<false, true>
    "f16-causal-cap": dict(causal=1, cap=True),                 # attn_kernel<true, true>
    "f16-32": dict(variant=2),                                  # attn32_kernel
    "decode": dict(),                                           # attn_decode_kernel<false> (nq = 1)
    "decode-rows": dict(rows=True),                             # attn_decode_kernel<true>
    "pair-16": dict(split=1, variant=1),                        # attn_split_kernel<false, false>
    "pair-causal": dict(split=1, causal=1),                     # attn_split_kernel<true, false>
    "pair-cap": dict(split=1, cap=True),                        # attn_split_kernel<false, true>
    "pair-32": dict(split=1),                                   # attn_split32_kernel (nq >= 64, variant 0)
}


def _taken(d, has_rows):
    """The kernel instance the launchers pick for a descriptor (csrc/attention.hip launch_attention, csrc/attention_split.hip
    launch_attention_split, with every test switch at 0)."""
    cap = bool(d.cap) and d.cap_cols > 0
    if d.split:
        if not d.causal and not cap and d.nq >= 64 and d.variant != 1 and d.o_rs % 8 == 0 and d.o_lo % 8 == 0:
            return "pair-32"
        return {(0, False): "pair-16", (1, False): "pair-causal", (0, True): "pair-cap", (1, True): "pair-causal-cap"}[(d.causal, cap)]
    if d.nq == 1 and not cap and (not d.causal or d.nk == 1):
        return "decode-rows" if has_rows else "decode"
    if not d.causal and not cap and d.o_rs % 8 == 0 and d.variant != 1 and (d.nq >= 64 or d.variant == 2):
        return "f16-32"
    return {(0, False): "f16-16", (1, False): "f16-causal", (0, True): "f16-cap", (1, True): "f16-causal-cap"}[(d.causal, cap)]


@pytest.fixture(scope="module")
def eng(wca):
    syn = importlib.import_module("whisper-char-alignment_amd.synthetic")
    dims = wca.ModelDimensions(80, 1500, 384, 6, 2, 51865, 448, 384, 6, 2)
    m = wca.WhisperAMD(dims, device="cuda:0", max_batch=2, precision="f16")
    m.load_state_dict(syn.random_state_dict(dims, seed=1))
    m._bind_stream()
    return m


class Planes:
    """The master buffers of one batch size, on the device. Operands are [3][nb][rows][HD] f16: slot 0 the values (the hi halves), slot 1 zero
    lo halves, slot 2 the +-2^-13 lo halves, so that a pair launch names its lo half by an offset of one or two slots."""

    def __init__(self, nb, nk_max, nq_max, cap_floats=0):
        self.nb, self.rows, self.nq_max = nb, nk_max + ref.GUARD, nq_max
        host = {"ku": torch.zeros(nb, self.rows, HD, dtype=torch.float64), "vu": ref.uniform_v(nb, nk_max, ref.H),
                "kp": ref.peaked_k(nb, nk_max, ref.H), "vp": ref.peaked_v(nb, nk_max, ref.H)}
        self.host = {n: torch.stack([x, torch.zeros_like(x), ref.lo_halves(x.shape, n[0])]).half() for n, x in host.items()}   # (exact)
        qlo = ref.lo_halves((nb, nq_max, HD), "q")
        self.host["qu"] = torch.stack([torch.zeros_like(qlo), torch.zeros_like(qlo), qlo]).half()
        self.dev = {n: x.cuda() for n, x in self.host.items()}
        self.dev["qp"] = self.dev["qu"].clone()             # slot 0 is rebuilt on the device for every peaked launch: 4 K[t]
        self.o = torch.empty(2, nb, nq_max, HD, dtype=torch.float16, device="cuda")
        self.o2 = torch.empty_like(self.o)
        self.cap = torch.empty(max(cap_floats, 4), dtype=torch.float32, device="cuda")
        self.refs = {}

    def unchanged(self):
        return all(torch.equal(self.dev[n].cpu(), x) for n, x in self.host.items())


@pytest.fixture(scope="module")
def planes():
    shapes = ref.SWEEPS["capture"] + ref.SWEEPS["causal_capture"]
    return Planes(ref.B, ref.NK_MAX, ref.NQ_MAX, cap_floats=max(ref.B * LAYERS * ref.H * nq * ref.cap_ld(nk) for nq, nk, _ in shapes))


@pytest.fixture(scope="module")
def row_planes():
    return Planes(ref.ROWS_B, ref.ROWS_B, 1)


def _reference(st, probe, nq, nk, causal, lo, counts=None, key=None):
    """(out [nb][nq][HD], logits [nb][H][nq][nk] or None) in float64 on the device, computed once per (probe, shape) and shared by the instances."""
    key = (probe, nq, nk, causal, lo, key)
    if key not in st.refs:
        live = ref.live_counts(nq, nk, causal, counts=counts, nb=st.nb)
        slots = (0, 2) if lo else (0,)
        val = lambda n: sum(st.host[n][s].double() for s in slots)       # noqa: E731
        if probe == "uniform" and not lo:
            out, logits = ref.uniform_ref(val("vu"), ref.H, live), torch.zeros(st.nb, ref.H, nq, ref.cap_cols(nk), dtype=torch.float64)
        else:
            k, v = (val("ku"), val("vu")) if probe == "uniform" else (val("kp"), val("vp"))
            q = torch.zeros(st.nb, nq, HD, dtype=torch.float64) if probe == "uniform" else ref.peaked_q(st.host["kp"][0].double(), ref.targets(probe, live))
            if lo:
                q = q + st.host["qu"][2][:, :nq].double()
            out, logits, _ = ref.peaked_ref(q, k, v, ref.H, live)
        st.refs[key] = (out.cuda(), logits[..., :ref.cap_cols(nk)].contiguous().cuda())
    return st.refs[key]


def _launch(eng, lib, wca, st, inst, probe, nq, nk, lo=False, counts_dev=None, row=None, o=None):
    """One launch of instance `inst` on a prefix of the master buffers (row: batch row `row` alone, as a B = 1 launch on the Q that the launch
    of all rows built). Returns the descriptor."""
    f = INSTANCES[inst]
    causal, split, capture = f.get("causal", 0), f.get("split", 0), f.get("cap", False)
    o = st.o if o is None else o
    kname, vname, qname = ("ku", "vu", "qu") if probe == "uniform" else ("kp", "vp", "qp")
    nb = st.nb if row is None else 1
    if probe != "uniform" and row is None:          # Q = 4 K[t], built where it is used
        base = counts_dev.view(-1, 1) if counts_dev is not None else torch.full((st.nb, 1), nk, dtype=torch.int64, device="cuda")
        live = base.expand(st.nb, nq)
        if causal:
            live = torch.minimum(live, torch.arange(1, nq + 1, device="cuda").view(1, nq))
        st.dev["qp"][0, :, :nq] = ref.peaked_q(st.dev["kp"][0], ref.targets(probe, live))
    d = wca._lib.AttnDesc()
    esz = 2
    for name, t, bs in (("q", st.dev[qname], st.nq_max * HD), ("k", st.dev[kname], st.rows * HD), ("v", st.dev[vname], st.rows * HD),
                        ("o", o, st.nq_max * HD)):
        slot = t[0].numel()
        setattr(d, name, t.data_ptr() + (row or 0) * bs * esz)
        setattr(d, name + "_bs", bs)
        setattr(d, name + "_rs", HD)
        setattr(d, name + "_lo", (slot if name == "o" or not lo else 2 * slot) if split else 0)
    d.B, d.H, d.nq, d.nk, d.causal, d.split, d.variant = nb, ref.H, nq, nk, causal, split, f.get("variant", 0)
    if f.get("rows"):
        d.nk_rows = st.counts32.data_ptr()
    if capture:
        ld = ref.cap_ld(nk)
        assert st.nb * LAYERS * ref.H * nq * ld <= st.cap.numel()
        d.cap = st.cap.data_ptr() + ref.H * nq * ld * 4
        d.cap_bs, d.cap_hs, d.cap_ld, d.cap_cols = LAYERS * ref.H * nq * ld, nq * ld, ld, ref.cap_cols(nk)
    want = "decode" if (inst == "f16-causal" and nq == 1) else inst      # one causal query with one key is a decode step
    assert _taken(d, bool(f.get("rows"))) == want, (inst, nq, nk)
    wca._lib.check(lib.wca_test_attention_ex(eng._h, C.byref(d)))
    return d


def _checked_launch(eng, lib, wca, st, inst, probe, nq, nk, lo=False):
    """Sentinel fill, launch, and the launch's figures as one device vector (no synchronisation):
    [output error, nonzero where the reference is 0, cells outside the written region that lost the sentinel, capture error, capture cells lost]"""
    f = INSTANCES[inst]
    causal, split, capture = bool(f.get("causal", 0)), f.get("split", 0), f.get("cap", False)
    st.o.fill_(O_SENTINEL)
    if capture:
        st.cap.fill_(CAP_SENTINEL)
    _launch(eng, lib, wca, st, inst, probe, nq, nk, lo=lo)
    want, logits = _reference(st, probe, nq, nk, causal, lo)
    got = st.o[0, :, :nq].double() + (st.o[1, :, :nq].double() if split else 0.0)
    err = (got - want).abs()
    zero = torch.zeros((), dtype=torch.float64, device="cuda")
    if probe == "uniform" and not split:
        fig = [(err / ref.spacing_f16(want)).max(), ((want == 0) & (got != 0)).sum().double()]
    else:
        fig = [err.max(), zero]
    fig[0] = torch.where(torch.isfinite(got).all(), fig[0], torch.full_like(fig[0], float("inf")))
    lost = (st.o[:, :, nq:] != O_SENTINEL).sum() + (0 if split else (st.o[1] != O_SENTINEL).sum())
    fig.append(lost.double())
    if capture:
        ld, cols = ref.cap_ld(nk), ref.cap_cols(nk)
        n = st.nb * LAYERS * ref.H * nq * ld
        view = st.cap[:n].view(st.nb, LAYERS, ref.H, nq, ld)
        region = view[:, 1, :, :, :cols].double()
        above = torch.arange(cols, device="cuda").view(1, cols) > torch.arange(nq, device="cuda").view(nq, 1) if causal else None
        if lo:
            cerr = (region - logits).abs()
        else:
            cerr = (region != logits).double()
        if causal:
            cerr = torch.where(above & (region == CAP_SENTINEL), torch.zeros_like(cerr), cerr)
        fig.append(cerr.max())
        rest = st.cap.clone()
        rest[:n].view(st.nb, LAYERS, ref.H, nq, ld)[:, 1, :, :, :cols] = CAP_SENTINEL
        fig.append((rest != CAP_SENTINEL).sum().double())
    else:
        fig += [zero, zero]
    return torch.stack(fig)


def _sweep(eng, lib, wca, switch, st, label, shapes):
    """Every shape of a sweep on one instance (label, or label-lo: the +-2^-13 lo halves), uniform probe and the three target maps."""
    switch("attn_split_variant", 0)
    switch("attn_split_drop", 0)
    lo = label.endswith("-lo")
    inst = label[:-3] if lo else label
    split = INSTANCES[inst].get("split", 0)
    runs = [(probe, nq, nk) for nq, nk, _ in shapes for probe in ("uniform",) + ref.MAPS]
    figs = torch.stack([_checked_launch(eng, lib, wca, st, inst, probe, nq, nk, lo=lo) for probe, nq, nk in runs]).cpu()
    torch.cuda.synchronize()
    worst = {"uniform": 0.0, "peaked": 0.0, "capture": 0.0}
    for (probe, nq, nk), (err, nonzero, lost, cerr, clost) in zip(runs, figs.tolist()):
        kind = "uniform" if probe == "uniform" else "peaked"
        worst[kind], worst["capture"] = max(worst[kind], err), max(worst["capture"], cerr)
    print(f"\n{label}: {len(runs)} launches; uniform probe max {worst['uniform']:.3g} {'(abs)' if split else 'f16 spacings'}; "
          f"peaked probe max {worst['peaked']:.3g}; capture max difference {worst['capture']:.3g}")
    for (probe, nq, nk), (err, nonzero, lost, cerr, clost) in zip(runs, figs.tolist()):
        where = (label, probe, nq, nk, err, nonzero, lost, cerr, clost)
        if probe == "uniform":
            assert err <= (PAIR_TOL if split else 1.0), where       # f16: in f16 spacings of the reference
            assert nonzero == 0, where
        else:
            assert err <= (PAIR_TOL if split else F16_TOL), where
        assert lost == 0 and clost == 0, where
        if lo:
            assert cerr <= 4e-7 * 32 + 1e-6, where
        else:
            assert cerr == 0, where
    assert st.unchanged()


PLAIN = ["f16-16", "f16-32", "pair-16", "pair-32", "pair-16-lo", "pair-32-lo"]


@pytest.mark.parametrize("label", PLAIN)
def test_key_count_sweep(eng, lib, wca, switch, planes, label):
    """nq = 97, every nk in 1 .. 200, then 255, 256, 257, 448, 1499, 1500: the staged-row clamp and the tail mask of the last key tile at every
    fill, one to 24 tiles, with live rows behind the last key."""
    _sweep(eng, lib, wca, switch, planes, label, ref.SWEEPS["key"])


@pytest.mark.parametrize("label", PLAIN)
def test_query_count_sweep(eng, lib, wca, switch, planes, label):
    """nk = 70, every nq in 2 .. 260 (64 .. 260 where the pair launcher takes its 32x32x16 kernel): the clamped query rows of a ragged block, the
    guarded stores, one to three 128-row blocks over the remapped grid."""
    shapes = [s for s in ref.SWEEPS["query"] if s[0] >= 64 or not label.startswith("pair-32")]
    assert len(shapes) == (197 if label.startswith("pair-32") else 259)
    _sweep(eng, lib, wca, switch, planes, label, shapes)


@pytest.mark.parametrize("label", ["f16-causal", "pair-causal", "pair-causal-lo"])
def test_causal_sweep(eng, lib, wca, switch, planes, label):
    """nq = nk = n, every n in 1 .. 260, then 448: the diagonal mask, nk_eff and the tail mask together where 128-row blocks and 64-key tiles meet.
    Every launch reads its keys from planes longer than n, which is the prefill form of a prompted decode (n = 37 among them); n = 1 in f16
    is a decode step and takes the one-query kernel, as in the product."""
    _sweep(eng, lib, wca, switch, planes, label, ref.SWEEPS["causal"])


@pytest.mark.parametrize("label", ["f16-cap", "pair-cap", "pair-cap-lo"])
def test_capture_sweep(eng, lib, wca, switch, planes, label):
    """nq in {5, 69}, every nk in 1 .. 80, then 145, 1500; cap_cols = min(nk, 145) in rows of roundup4(cap_cols) + 4 floats: the float4 stores, the
    group that straddles cap_cols, the pad columns."""
    _sweep(eng, lib, wca, switch, planes, label, ref.SWEEPS["capture"])


def test_causal_capture(eng, lib, wca, switch, planes):
    _sweep(eng, lib, wca, switch, planes, "f16-causal-cap", ref.SWEEPS["causal_capture"])


def test_decode_sweep(eng, lib, wca, switch, planes):
    """One query, every nk in 1 .. 300: the four waves' key ranges (per_wave a multiple of 8), k_hi and the live[u] select of the last step."""
    _sweep(eng, lib, wca, switch, planes, "decode", ref.SWEEPS["decode"])


@pytest.mark.parametrize("shuffled", [False, True])
def test_decode_with_per_row_key_counts(eng, lib, wca, row_planes, shuffled):
    """One launch of 300 batch rows with 1 .. 300 keys (in order, and in a seeded shuffle) out of planes 300 rows long: every row within the
    probes' bounds, and bit for bit the uniform launch of that row alone with nk = its count."""
    st = row_planes
    counts = ref.rows_counts(shuffled)
    st.counts32 = counts.to(torch.int32).cuda()
    counts_dev = counts.cuda()
    nk = ref.ROWS_B
    for probe in ("uniform",) + ref.MAPS:
        st.o.fill_(O_SENTINEL)
        st.o2.fill_(O_SENTINEL)
        _launch(eng, lib, wca, st, "decode-rows", probe, 1, nk, counts_dev=counts_dev)
        for b, n in enumerate(counts.tolist()):
            _launch(eng, lib, wca, st, "decode", probe, 1, n, counts_dev=counts_dev, row=b, o=st.o2)
        want, _ = _reference(st, probe, 1, nk, False, False, counts=counts, key=shuffled)
        got = st.o[0].double()
        assert bool(torch.isfinite(got).all()), probe
        if probe == "uniform":
            err = ((got - want).abs() / ref.spacing_f16(want)).max().item()
            assert err <= 1.0 and bool((got[want == 0] == 0).all()), (probe, err)
        else:
            err = (got - want).abs().max().item()
            assert err <= F16_TOL, (probe, err)
        assert bool((st.o[1] == O_SENTINEL).all())
        assert torch.equal(st.o, st.o2), probe
        print(f"\ndecode-rows shuffled={shuffled} {probe}: max {err:.3g} {'f16 spacings' if probe == 'uniform' else ''}")
    assert st.unchanged()
