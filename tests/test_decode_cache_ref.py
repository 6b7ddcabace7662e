"""CPU: nothing hides behind the bounds of tests/test_decode_cache_gpu.py. The planted attention of tests/decode_cache_ref.py is one-hot at every fed
position, every index fault of the decode loop's cache moves a quantity the GPU tests assert by at least 10 times its bound, the rows of a batch differ by
as much, and the float64 reference is the model that oracle/whisper_ref.py states in fp32."""
import importlib

import pytest
import torch

import decode_cache_ref as R

FACTOR = 10.0   # every fault must move an asserted quantity by this many GPU bounds


@pytest.fixture(scope="module")
def sc():
    return R.scene()


def test_targets_cover_every_kind_at_every_boundary():
    for lo in (1, 63, 127, 255):
        kinds = {R.kind(n - 1) for n in R.LENGTHS if lo <= n <= lo + 3}
        assert kinds == {0, 1, 2}, (lo, kinds)
    assert {R.kind(n - 1) for n in (446, 447, 448)} == {0, 1, 2}
    for p in range(R.DIMS[6]):
        assert 0 <= R.tgt(p) <= p
    # past the first tile the interior targets are the keys next to a tile boundary
    assert [R.tgt(n - 1) for n in (66, 129, 258, 447)] == [63, 64, 255, 384]


def test_planted_attention_is_one_hot(sc):
    pt = sc["p_target"]
    print("p_target: min over layers, rows, heads and the 448 positions %.9f" % float(pt.min()))
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


def test_every_fault_moves_an_asserted_quantity(sc):
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
    print("%-34s %-11s %10s %10s %8s" % ("fault", "quantity", "shift", "GPU bound", "ratio"))
    for name, q, shift in rows:
        print("%-34s %-11s %10.3e %10.3e %8.1f" % (name, q, shift, R.TOL[q], shift / R.TOL[q]))
    # a-d move a cache element, d-g a last-position logit, the rows differ in the layer-1 planes and in the logits: every line of the table holds
    for name, q, shift in rows:
        assert shift >= FACTOR * R.TOL[q], (name, q, shift, R.TOL[q])
