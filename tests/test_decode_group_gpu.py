"""The grouped decode (C ABI wca_decode_group through the one loop decode_run: the prefill-to-group broadcast, G decoder rows on one audio's
cross-K/V, the beam step, the cache reorder between the two halves of dec_cache) on the MI355X against float64, on the position-coded checkpoint of
tests/decode_cache_ref.py. tests/decode_group_ref.py rebuilds every row's history from the engine's own trace (wca_test_beam_trace) and states
what the loop must leave (wca_test_decode_state): every cache slot [0, fed_r) of every layer, plane and row and the last forward's logits are
compared element by element; the engine's choices, its sum_logprob and its returned rows are checked against the reference scored along the
engine's live beams. tests/test_decode_group_ref.py shows on the CPU that a skipped reorder, a group-relative source, a short n_keep, a plane left
out, a stale source half, a broadcast by r % B, another audio's cross-K/V or a reordered audio past its budget moves an asserted cache element by
at least 10 bounds."""
import importlib

import numpy as np
import pytest
import torch

import decode_cache_ref as R
import decode_group_ref as GR

pytestmark = pytest.mark.gpu

MAX_ROWS = {"f16": 144, "reference": 15}


@pytest.fixture(scope="module")
def sc():
    return GR.group_scene()


@pytest.fixture(scope="module")
def tok():
    return importlib.import_module("whisper-char-alignment_amd.tokenizer").get_tokenizer(True, language="en", task="transcribe")


@pytest.fixture(scope="module")
def engines(sc):
    pkg = importlib.import_module("whisper-char-alignment_amd")
    made = {}

    def get(precision):
        if precision not in made:
            made[precision] = pkg.WhisperAMD(sc["D"], device="cuda:0", max_batch=MAX_ROWS[precision], precision=precision).load_state_dict(sc["sd"])
        return made[precision]

    return get


@pytest.fixture(scope="module")
def mel_dev(sc):
    return sc["mel5"].cuda()


def _check_state(tag, cache, logits, want_planes, fed, want_logits, logits_rows):
    """cache [L][2][R][T][d] f16 and logits [R][V] f32 of the GPU against the float64 planes (row r: slots [0, fed[r])) and the logits of the rows
    `logits_rows` (a row past its budget computes what is never read): prints the three maxima and where the largest is, then asserts them."""
    cache = torch.from_numpy(cache.astype(np.float64))
    d0 = dd = 0.0
    where = None
    for r, n in enumerate(fed):
        diff = (cache[:, :, r, :n] - want_planes[:, :, r, :n]).abs()
        d0 = max(d0, float(diff[0].max()))
        if float(diff[1:].max()) > dd:
            dd = float(diff[1:].max())
            where = (r, int(diff[1:].amax(dim=(0, 1, 3)).argmax()))
    got = torch.from_numpy(logits.astype(np.float64))[logits_rows]
    dl = float((got - want_logits[logits_rows]).abs().max())
    print("decode-group measure %s: plane0 %.3e plane_deep %.3e (row %d slot %d) logits %.3e (|logits| max %.2f)"
          % (tag, d0, dd, where[0], where[1], dl, float(want_logits.abs().max())))
    assert np.isfinite(logits[logits_rows]).all()
    assert d0 <= R.TOL["plane0"], (tag, "layer-0 planes", d0, R.TOL["plane0"])
    assert dd <= R.TOL["plane_deep"], (tag, "deeper planes", dd, R.TOL["plane_deep"])
    assert dl <= R.TOL["logits"], (tag, "logits", dl, R.TOL["logits"])


def _decode(m, sc, mel_dev, tok, name, fused, mode, **extra):
    audios, ni, budgets, G, _ = GR.SCENES[name]
    initial = GR.initial_tokens(name)
    B, T_max = len(audios), max(n + s for n, s in zip(ni, budgets))
    m.set_decode_mode(fused, 1)
    try:
        out = m.decode_group(mel_dev[list(audios)].contiguous(), None, None, initial, [0] * B, list(budgets), R.text_suppress_mask(), None,
                             eot=tok.eot, timestamp_begin=tok.timestamp_begin, apply_timestamp_rules=False, n_group=G, mode=mode, **extra)
        trace = m.beam_trace() if mode == 0 else None
        assert m.last_decode_positions() == (max(ni), max(budgets) - 1)
        logits, cache = m.decode_state(B * G, T_max)
    finally:
        m.set_decode_mode(True, 1)
    return initial, T_max, out, trace, logits, cache


BEAM = [(name, p, f) for name, p in (("b1g2", "f16"), ("b3g5", "f16"), ("b3g5", "reference"), ("budget", "f16"), ("r65", "f16"), ("r144", "f16"))
        for f in (True, False)]


@pytest.mark.parametrize("name,precision,fused", BEAM, ids=["%s-%s-%s" % (n, p, "fused" if f else "separate") for n, p, f in BEAM])
def test_beam_search_cache_logits_and_choices(sc, engines, mel_dev, tok, name, precision, fused):
    """Beam search: b1g2 one audio; b3g5 three audios of 3 / 60 / 126 initial tokens; budget: one audio passes its budget while the other goes on;
    r65: 5 x 13 rows, row 64 alone in the second block of 64 rows of the few-row GEMM's per-row KV append; r144: 9 x 16 rows, past the few-row
    GEMM. Every choice sequence crosses a tile of 64 keys in at least one audio."""
    audios, ni, budgets, G, _ = GR.SCENES[name]
    B, S = len(audios), max(budgets)
    initial, T_max, (toks, n_tok, lp, n_out), trace, logits, cache = _decode(engines(precision), sc, mel_dev, tok, name, fused, 0)
    tag = "%s %s %s" % (name, precision, "fused" if fused else "separate")
    assert trace.shape == (S, B * G, 2)
    moved, twice, twice_later = GR.coverage(trace, G)
    assert moved >= 3 and twice >= 1 and (B == 1 or twice_later >= 1), (tag, moved, twice, twice_later)
    fw = GR.Forwards(sc["ref"], GR.scene_ckv(sc, name))
    hists, sums, n_decided = GR.check_choices(tag, fw, initial, trace, G, R.TOL["logits"])
    assert n_decided >= 1, tag
    planes, want_logits, fed = GR.final_state(fw.ref, fw.ckv, hists, T_max, fw)
    assert fed == [ni[r // G] + budgets[r // G] - 1 for r in range(B * G)]
    live = [r for r in range(B * G) if budgets[r // G] == S]
    _check_state(tag, cache, logits, planes, fed, want_logits, live)
    # nothing finished (EOT is suppressed): the results are the live beams, best first, as the trace rebuilt them
    assert list(n_out) == [G] * B
    err = 0.0
    for r, row in enumerate(hists[-1]):
        b, g = divmod(r, G)
        assert n_tok[b, g] == len(row) and toks[b, g, :len(row)].tolist() == row, (tag, b, g)
        err = max(err, abs(float(lp[b, g]) - sums[r]) / (budgets[b] * 2 * R.TOL["logits"] + 1e-4))
    print("decode-group choices %s: max |d sum_logprob| over its bound (steps * 2 * %.2e + 1e-4) %.3f" % (tag, R.TOL["logits"], err))
    assert err <= 1.0, (tag, err)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
def test_best_of_rows_hold_their_own_tokens(sc, engines, mel_dev, tok, fused):
    """mode 1, three samples per audio: nothing is reordered; every row holds the K / V of ITS returned tokens on its audio's cross-K/V, and its last
    logits are its own last position's."""
    name = "best_of"
    audios, ni, budgets, G, _ = GR.SCENES[name]
    B = len(audios)
    initial, T_max, (toks, n_tok, lp, n_out), _, logits, cache = _decode(engines("f16"), sc, mel_dev, tok, name, fused, 1, temperature=[0.8, 1.0],
                                                                         seed=[7, 8])
    assert list(n_out) == [G] * B
    rows = []
    for r in range(B * G):
        b, g = divmod(r, G)
        assert n_tok[b, g] == ni[b] + budgets[b] and toks[b, g, :ni[b]].tolist() == initial[b]
        rows.append(toks[b, g, :n_tok[b, g]].tolist())
        assert max(rows[-1]) < R.N_TEXT
    assert all(len({tuple(row) for row in rows[b * G:(b + 1) * G]}) == G for b in range(B)), "the samples of an audio are not different sequences"
    fw = GR.Forwards(sc["ref"], GR.scene_ckv(sc, name))
    planes, want_logits, fed = GR.group_state(fw.ref, fw.ckv, rows, T_max, fw)
    _check_state("best_of %s" % ("fused" if fused else "separate"), cache, logits, planes, fed, want_logits, list(range(B * G)))
