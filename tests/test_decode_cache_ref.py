"""CPU: nothing hides behind the bounds of tests/test_decode_cache_gpu.py and tests/test_decode_widths_gpu.py. At every width the planted attention of
tests/decode_cache_ref.py is one-hot at every fed position, every index fault of the decode loop's cache moves a quantity the GPU tests assert by at least
10 times its bound (at the new widths also a missing split-K partial of fc2 and a LayerNorm launch with another site's parameters), the rows of a batch
differ by as much, the reference's own margins decide at least 90 % of the sampled choices, and the float64 reference is the model that
oracle/whisper_ref.py states in fp32. The launches a decode step is made of at each width are pinned as a literal table."""
import hashlib
import importlib

import pytest
import torch

import decode_cache_ref as R

FACTOR = 10.0   # every fault must move an asserted quantity by this many GPU bounds


@pytest.fixture(scope="module")
def sc():
    return R.scene()


@pytest.fixture(scope="module", params=R.NEW_WIDTHS)
def width(request):
    """Module-scoped, so that the tests of one width run together and its scene and bounds are computed once."""
    return request.param


def test_targets_cover_every_kind_at_every_boundary():
    for lo in (1, 63, 127, 255):
        kinds = {R.kind(n - 1) for n in R.LENGTHS if lo <= n <= lo + 3}
        assert kinds == {0, 1, 2}, (lo, kinds)
    assert {R.kind(n - 1) for n in (446, 447, 448)} == {0, 1, 2}
    for p in range(R.DIMS[6]):
        assert 0 <= R.tgt(p) <= p
    # past the first tile the interior targets are the keys next to a tile boundary
    assert [R.tgt(n - 1) for n in (66, 129, 258, 447)] == [63, 64, 255, 384]


def _one_hot(sc):
    pt = sc["p_target"]
    print("width %d p_target: min over layers, rows, heads and the 448 positions %.9f" % (sc["width"], float(pt.min())))
    assert float(pt.min()) >= 1 - 1e-4
    # the step the mutations go through is the forward: the last position of every length, read from the clean cache
    ref, planes = sc["ref"], R.planes_of(sc["K"], sc["V"], 449)
    for n in (1, 65, 448):
        step = ref.step_logits(sc["tokens"][n - 1:n], n - 1, planes, sc["ckv"])
        assert float((step - ref.logits(sc["x"][:, n - 1])).abs().max()) < 1e-10


def test_reference_is_the_fp32_oracle_model(sc):
    """The float64 forward against oracle.whisper_ref.WhisperRef on the same checkpoint and recordings: cache-free logits of 66 positions agree to fp32
    noise (the logits are O(1): a few hundred fp32 roundings of 6e-8 each, amplified by two LayerNorms, stay under 1e-4; an f16 operand is 5e-4)."""
    wref = importlib.import_module("oracle.whisper_ref")
    oracle = wref.WhisperRef({k: v.float() for k, v in sc["sd"].items()}, sc["D"])
    n = 66
    tokens = sc["tokens"][:n][None].expand(R.B, n)
    want = oracle.decoder(tokens, oracle.encoder(sc["mel"][:R.B]))[0].double()
    got = sc["ref"].logits(sc["x"][:, :n])
    err = float((got - want).abs().max())
    print("float64 reference vs fp32 oracle: max |d logits| %.2e over %s (|logits| max %.2f)" % (err, tuple(got.shape), float(got.abs().max())))
    assert err < 1e-4


def test_planted_attention_is_one_hot(sc):
    _one_hot(sc)


def test_planted_attention_is_one_hot_at_width(width):
    _one_hot(R.scene(width))


def test_scene_256_is_the_first_scene():
    """The width argument left the 256-wide scene what it was. The whole state dict and the reference outputs on it were hashed equal before and after
    the change, once, on one CPU (HISTORY.md); pinned here is what no CPU's float arithmetic can move: the constants the 256-wide path reads, and a
    sha256 over the integer-drawn parts of the checkpoint -- the token row, the +-1 codes of the positional embedding, the planted key / query weights."""
    assert R.dims() == R.dims(256) == type(R.dims())(*R.DIMS) and R.scene() is R.scene(256)
    assert R.GAIN_OF[256] == R.GAIN == 2.0 and R.TOKEN_SEED[256] == 0 and R.tol(256) is R.TOL
    sd, h = R.planted_state_dict(), hashlib.sha256()
    h.update(R.token_row(448).numpy().tobytes())
    h.update(sd["decoder.positional_embedding"][:, :2 * R.CODE].numpy().tobytes())
    for li in range(2):
        for name in ("key", "query"):
            h.update(sd["decoder.blocks.%d.attn.%s.weight" % (li, name)].numpy().tobytes())
    assert h.hexdigest() == "a4ca437394f14aa7ae7729b0c4cd35135deb8fdb42d84e104314d3225910d59e"
    for name, v in sd.items():      # the per-site LayerNorm parameters are the new widths' alone
        if name.startswith("decoder.") and "ln" in name.split(".")[-2]:
            assert bool((v == (1.0 if name.endswith(".weight") else 0.0)).all()), name


def test_every_fault_moves_an_asserted_quantity(sc):
    _faults(sc, R.TOL)


def test_every_fault_moves_an_asserted_quantity_at_width(width):
    """The bounds are bounds(width): max(4 x the f16-operand statement's distance from float64, one f16 spacing), from the references alone."""
    b = R.bounds(width)
    print("width %d bounds: %s" % (width, "  ".join("%s yard %.3e floor %.3e tol %.3e" % (q, b["yard"][q], b["floor"][q], b["tol"][q]) for q in b["tol"])))
    _faults(R.scene(width), b["tol"])


def _faults(sc, TOL):
    ref, ckv, tokens, K, V, x = sc["ref"], sc["ckv"], sc["tokens"], sc["K"], sc["V"], sc["x"]
    T = 449
    clean = R.planes_of(K, V, T)
    rows = []   # (fault, quantity, shift)

    def plane_shift(mut, layer0):
        """The smallest, over the slots the edit moved, of the largest element change in the asserted planes of layer 0 (or of the deeper layers)."""
        d = (mut - clean)[:1] if layer0 else (mut - clean)[1:]
        per_slot = d[:, :, :, :448].abs().amax(dim=(0, 1, 4))   # [B, slot]
        moved = per_slot[per_slot > 0]
        return float(moved.min()) if moved.numel() else 0.0

    def logit_shift(n, **kw):
        """The smallest over the rows of the largest last-position logit change at n cached keys."""
        p = n - 1
        return float((ref.step_logits(tokens[p:p + 1], p, clean, ckv, **kw) - ref.logits(x[:, p])).abs().amax(-1).min())

    for name, mut in (("a slot t holds t-1", R.mut_slot_holds_previous(clean)), ("b row stride T_max-1", R.mut_row_stride(clean)),
                      ("c K/V swapped", R.mut_swap_kv(clean)), ("c layers swapped", R.mut_swap_layers(clean))):
        rows.append((name, "plane0", plane_shift(mut, True)))
        rows.append((name, "plane_deep", plane_shift(mut, False)))
    # d. the positional row off by one: the whole forward with row p - 1 at position p (p >= 1)
    Kd, Vd, xd, _ = ref.forward(tokens[None], ckv, pos_shift=-1)
    shifted = R.planes_of(Kd, Vd, T)
    moved = (shifted - clean)[:, :, :, 1:448].abs().amax(dim=(1, 4))   # [L, B, slot]
    rows.append(("d positional row off by one", "plane0", float(moved[0].min())))
    rows.append(("d positional row off by one", "plane_deep", float(moved[1:].amax(0).min())))
    rows.append(("d positional row off by one", "logits", min(logit_shift(n, pos_row=n - 2) for n in R.LENGTHS if n >= 2)))
    newest = [n for n in R.LENGTHS if R.kind(n - 1) == 0 and n > 1]
    interior = [n for n in R.LENGTHS if R.kind(n - 1) == 2]
    assert len(newest) >= 6 and len(interior) >= 6
    rows.append(("e newest key invisible", "logits", min(logit_shift(n, key_idx=R.drop_newest(n)) for n in newest)))
    rows.append(("f key dropped at a tile boundary", "logits", min(logit_shift(n, key_idx=R.drop_key(n, R.tgt(n - 1))) for n in interior)))
    rows.append(("g row b reads row b-1", "logits", min(logit_shift(n, row_map=R.previous_row(R.B)) for n in R.LENGTHS)))
    rows.append(("g row b reads row b-1", "plane_deep", float(min(
        torch.maximum((K[1:, a] - K[1:, b]).abs().amax(dim=(0, 2)), (V[1:, a] - V[1:, b]).abs().amax(dim=(0, 2))).min()
        for a, b in ((0, 1), (1, 2), (0, 2))))))
    lg = ref.logits(x[:, [n - 1 for n in R.LENGTHS]])
    rows.append(("rows differ", "logits", float(min((lg[a] - lg[b]).abs().amax(-1).min() for a, b in ((0, 1), (1, 2), (0, 2))))))
    if sc["width"] != 256:
        # the two faults of the routes only the new widths take, on decoder layer 0: the whole forward with the fault, its layer-1 planes (every
        # slot of every row) and its last-position logits
        s = R.FC2_SPLITK[sc["width"]]
        for name, fault in (("h fc2 split-K partial %d of %d missing" % (s, s), ("fc2_partial", s)),
                            ("i fc1's LayerNorm reads cross_attn_ln", ("fc1_ln", "cross_attn_ln"))):
            bad = R.DecodeRef(sc["sd"], sc["D"], fault=fault)
            Kf, Vf, xf, _ = bad.forward(tokens[None], ckv)
            moved = torch.maximum((Kf - K)[1:].abs().amax(dim=(0, 3)), (Vf - V)[1:].abs().amax(dim=(0, 3)))   # [B, slot]
            rows.append((name, "plane_deep", float(moved.min())))
            last = [n - 1 for n in R.LENGTHS]
            rows.append((name, "logits", float((bad.logits(xf[:, last]) - ref.logits(x[:, last])).abs().amax(-1).min())))
    print("%-40s %-11s %10s %10s %8s" % ("width %d fault" % sc["width"], "quantity", "shift", "GPU bound", "ratio"))
    for name, q, shift in rows:
        print("%-40s %-11s %10.3e %10.3e %8.1f" % (name, q, shift, TOL[q], shift / TOL[q]))
    # a-d move a cache element, d-g a last-position logit, the rows differ in the layer-1 planes and in the logits: every line of the table holds
    for name, q, shift in rows:
        assert shift >= FACTOR * TOL[q], (name, q, shift, TOL[q])


# width, rows, step / prefill -> the route of qkv, out, cross_q, cross_out, fc1, fc2, logits (decode_cache_ref.routes through format_route).
# rows 3: a step of the uniform decodes; 6: the prefill's logits rows (last + <|sot|>); 126 / 129 / 390: B n of the prefill lengths.
ROUTES = {
    (384, 3, "step"): ("t128 ln:separate kv:launch", "rows", "t128 ln:separate", "rows", "t128 ln:separate", "rows x2", "persist ln:separate"),
    (384, 6, "prefill"): ("t128 ln:separate", "rows", "t128 ln:separate", "rows", "t128 ln:separate", "rows x2", "persist ln:separate"),
    (384, 126, "prefill"): ("t128 ln:separate", "rows", "t128 ln:separate", "rows", "t128 ln:separate", "rows x2", "persist ln:separate"),
    (384, 129, "prefill"): ("t128 ln:separate", "t128", "t128 ln:separate", "t128", "t128 ln:separate", "t128", "persist ln:separate"),
    (384, 390, "prefill"): ("t128 ln:separate", "t128", "t128 ln:separate", "t128", "t128 ln:separate", "t128", "persist ln:separate"),
    (512, 3, "step"): ("rows ln:fused kv:in-kernel", "rows", "rows ln:fused", "rows", "rows ln:fused", "rows x2", "rows ln:fused"),
    (512, 6, "prefill"): ("rows ln:fused", "rows", "rows ln:fused", "rows", "rows ln:fused", "rows x2", "rows ln:fused"),
    (512, 126, "prefill"): ("rows ln:fused", "rows", "rows ln:fused", "rows", "rows ln:fused", "rows x2", "rows ln:fused"),
    (512, 129, "prefill"): ("t128 ln:separate", "t128", "t128 ln:separate", "t128", "t128 ln:separate", "t128 x4", "persist ln:separate"),
    (512, 390, "prefill"): ("t128 ln:separate", "t128", "t128 ln:separate", "t128", "t128 ln:separate", "t128 x4", "persist ln:separate"),
    (768, 3, "step"): ("rows ln:fused kv:in-kernel", "rows", "rows ln:fused", "rows", "rows ln:fused", "rows x3", "rows ln:fused"),
    (768, 6, "prefill"): ("rows ln:fused", "rows", "rows ln:fused", "rows", "rows ln:fused", "rows x3", "rows ln:fused"),
    (768, 126, "prefill"): ("rows ln:fused", "rows", "rows ln:fused", "rows", "rows ln:fused", "rows x3", "rows ln:fused"),
    (768, 129, "prefill"): ("t128 ln:separate", "t128", "t128 ln:separate", "t128", "t128 ln:separate", "t128 x4", "persist ln:separate"),
    (768, 390, "prefill"): ("t128 ln:separate", "t128", "t128 ln:separate", "t128", "t128 ln:separate", "t128 x4", "persist ln:separate"),
    (1024, 3, "step"): ("rows ln:fused kv:in-kernel", "rows", "rows ln:fused", "rows", "rows ln:fused", "rows x4", "rows ln:fused"),
    (1024, 6, "prefill"): ("rows ln:fused", "rows", "rows ln:fused", "rows", "rows ln:fused", "rows x4", "rows ln:fused"),
    (1024, 126, "prefill"): ("rows ln:fused", "rows", "rows ln:fused", "rows", "rows ln:fused", "rows x4", "rows ln:fused"),
    (1024, 129, "prefill"): ("t128 ln:separate", "t128", "t128 ln:separate", "t128", "t128 ln:separate", "t128 x4", "persist ln:separate"),
    (1024, 390, "prefill"): ("t128 ln:separate", "t128", "t128 ln:separate", "t128", "t128 ln:separate", "t128 x4", "persist ln:separate"),
    (1280, 3, "step"): ("t128 ln:separate kv:launch", "rows x2", "t128 ln:separate", "rows x2", "t128 ln:separate", "rows x5", "persist ln:separate"),
    (1280, 6, "prefill"): ("t128 ln:separate", "rows x2", "t128 ln:separate", "rows x2", "t128 ln:separate", "rows x5", "persist ln:separate"),
    (1280, 126, "prefill"): ("t128 ln:separate", "rows x2", "t128 ln:separate", "rows x2", "t128 ln:separate", "rows x5", "persist ln:separate"),
    (1280, 129, "prefill"): ("t128 ln:separate", "t128", "t128 ln:separate", "t128", "t128 ln:separate", "t128 x4", "persist ln:separate"),
    (1280, 390, "prefill"): ("t128 ln:separate", "t128", "t128 ln:separate", "t128", "t128 ln:separate", "t128 x4", "persist ln:separate"),
}


def test_routes_cover_every_branch(lib):
    """The census of the launches a decode step and a prefill are made of at every new width (the plan functions of csrc/gemm_plan.cpp through their
    test entry points, no GPU) equals the literal table above, and the table holds every branch the 256-wide scene never takes."""
    assert {n * R.B for n in R.PREFILL_LENGTHS} == {126, 129, 390}
    sites = list(R.ROUTE_SITES)
    got = {}
    for width in R.NEW_WIDTHS:
        for M, step in ((3, True), (2 * R.B, False), (126, False), (129, False), (390, False)):
            r = R.routes(width, M, step, lib)
            got[(width, M, "step" if step else "prefill")] = tuple(R.format_route(r[s]) for s in sites)
    for key in sorted(got):
        print(key, "  ".join("%s %s" % kv for kv in zip(sites, got[key])))
    assert got == ROUTES
    at = lambda w, M, mode, site: ROUTES[(w, M, mode)][sites.index(site)]
    ln_fed = ("qkv", "cross_q", "fc1", "logits")
    # the fused LayerNorm prologue at NV = K / 256 = 2, 3, 4, in a step and on the two row blocks of the 126-row prefill
    for w in (512, 768, 1024):
        assert all(at(w, 3, "step", s).startswith("rows ln:fused") and at(w, 126, "prefill", s).startswith("rows ln:fused") for s in ln_fed if s != "logits")
        assert at(w, 3, "step", "logits") == at(w, 6, "prefill", "logits") == "rows ln:fused"
        assert at(w, 3, "step", "qkv") == "rows ln:fused kv:in-kernel"
    # 384 and 1280: every LayerNorm-fed site leaves the few-row kernel, and qkv appends with launch_kv_append
    for w in (384, 1280):
        assert all("ln:separate" in at(w, 3, "step", s) and not at(w, 3, "step", s).startswith("rows") for s in ln_fed)
        assert at(w, 3, "step", "qkv").endswith("kv:launch")
    # every split of the few-row kernel, in a step and in the 126-row prefill; the K = d products split at 1280 only
    assert [at(w, 3, "step", "fc2") for w in R.NEW_WIDTHS] == ["rows x%d" % R.FC2_SPLITK[w] for w in R.NEW_WIDTHS]
    assert [at(w, 126, "prefill", "fc2") for w in R.NEW_WIDTHS] == ["rows x%d" % R.FC2_SPLITK[w] for w in R.NEW_WIDTHS]
    assert set(R.FC2_SPLITK.values()) == {2, 3, 4, 5}
    assert all(at(1280, M, mode, s) == "rows x2" for M, mode in ((3, "step"), (126, "prefill")) for s in ("out", "cross_out"))
    assert all(at(w, 3, "step", s) == "rows" for w in (384, 512, 768, 1024) for s in ("out", "cross_out"))
    # past DEC_ROWS_MAX = 128 rows nothing is left on the few-row kernel
    assert all(not e.startswith("rows") for (w, M, _), r in ROUTES.items() if M > 128 for e in r)


def test_reference_margin_decides_the_sampled_choices(width):
    """The GPU cases compare a sampled token only where the float64 top-2 margin of the filtered logits exceeds the logits bound: at least 90 % of
    the (row, step) choices of a width's cases must be of that kind (a condition on the token seed, TOKEN_SEED)."""
    m, bound = R.sampled_margins(width), R.bounds(width)["tol"]["logits"]
    decided = int((m > bound).sum())
    print("width %d: %d of %d sampled choices decided by the reference margin (bound %.3e; margins min %.3e median %.3e)"
          % (width, decided, m.numel(), bound, float(m.min()), float(m.median())))
    assert m.numel() == R.B * (len(R.STEPWISE_WIDTHS) + len(R.PREFILL_LENGTHS) * R.PREFILL_STEPS) + len(R.ROWS_N_INITIAL) * R.ROWS_STEPS
    assert decided >= 0.9 * m.numel()
