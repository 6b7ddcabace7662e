"""One beam step on the MI355X (csrc/beam.hip: beam_topk + beam_merge through wca_test_beam_step) on supplied logits and histories against
the float64 restatement of upstream's BeamSearchDecoder.update (tests/beam_ref.py), with the logit filters applied by the CPU oracle
(oracle/decoding_ref.py, the filters tests/test_decode_gpu.py pins decode_select against).

Tokens, sources, trace, finished lists and completion counts must be IDENTICAL; scores agree to the rtol = atol = 1e-4 that
tests/test_decode_gpu.py allows sum_logprob (fp32 log-sum-exp order). Identity is a fair demand only where no decision hangs on less than
the fp32 noise of a score (~1e-6 of a log-probability near 10): every case draws its logits from a seed chosen on the CPU so that the
reference's smallest selection margin is at least 1e-3, and asserts that. The planted exact ties are the exception by construction: equal
fp32 inputs give equal scores on both sides, and the stated order (lower source beam, then lower token) decides."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import beam_ref

pytestmark = pytest.mark.gpu

dref = importlib.import_module("oracle.decoding_ref")

CASES = ["first", "text", "after_single_ts", "after_ts_pair", "ts_mass_wins", "finished_row", "no_ts_rules"]
T_MAX = 40
MIN_GAP = 1e-3


@pytest.fixture(scope="module")
def engine():
    pkg = importlib.import_module("whisper-char-alignment_amd")
    return pkg.WhisperAMD(pkg.ModelDimensions(80, 1500, 128, 2, 1, 97, 448, 128, 2, 1), device="cuda:0", max_batch=1, precision="f16")


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _vocab(V):
    """(eot, timestamp_begin, no_timestamps, sot sequence, suppressed ids, blank ids, max_initial_timestamp_index, two text tokens)."""
    if V == 97:   # a vocabulary small enough to read: text [0, 50), eot 50, specials, <|notimestamps|> 59, timestamps [60, 97)
        return 50, 60, 59, [51, 52, 53], [3, 54, 55, 56, 57, 58], [7], 20, (10, 20)
    decoding = importlib.import_module("whisper-char-alignment_amd.decoding")
    tokmod = importlib.import_module("whisper-char-alignment_amd.tokenizer")
    tok = tokmod.get_tokenizer(True, language="en", task="transcribe")
    sup, _ = decoding.filter_masks(tok, decoding.DecodingOptions(language="en"), V)
    return (tok.eot, tok.timestamp_begin, tok.no_timestamps, list(tok.sot_sequence), [int(i) for i in np.nonzero(sup)[0] if i != tok.no_timestamps],
            list(tok.encode(" ")), 50, (400, 500))


def _case(V, G, B, case, seed, tie=None):
    """The inputs of one step and the reference's outcome."""
    eot, tsb, no_ts, sot, suppress, blank, max_init, (ta, tb) = _vocab(V)
    R = B * G
    rules = case != "no_ts_rules"
    initial = sot + ([] if rules else [no_ts])
    n_init = len(initial)
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((R, V)) * 3.0).astype(np.float32)
    # beam g carries its own text token, so that the beams of an audio are distinct sequences
    hist = {"first": lambda g: [], "no_ts_rules": lambda g: [ta + g], "text": lambda g: [tsb + 3, ta + g, tb],
            "after_single_ts": lambda g: [tsb + 3, ta + g, tb, tsb + 10], "after_ts_pair": lambda g: [tsb + 3, ta + g, tsb + 10, tsb + 10],
            "ts_mass_wins": lambda g: [tsb + 3, ta + g, tb], "finished_row": lambda g: [tsb + 3, ta + g, tb]}[case]
    tokens = [initial + hist(r % G) for r in range(R)]
    cur_len = len(tokens[0])
    if case == "ts_mass_wins":
        logits[:, tsb:] += 4.0
    if case in ("text", "finished_row", "after_ts_pair", "no_ts_rules"):
        logits[::2, eot] += 9.0    # every other beam would rather end: finished sequences, and lists that fill
    if case == "first":
        logits[0, min(tsb + max_init + 5, V - 1)] = 50.0   # beyond max_initial_timestamp: must not be offered
        logits[0, ta] = 50.0                               # text at the first position: must not be offered
    sums = -3.0 * rng.random(R)
    if case == "first":
        sums[:] = 0.0
    if tie == "within_row":      # the two best live tokens of every row are exactly equal
        for r in range(R):
            logits[r, ta + 1] = logits[r, ta + 3] = 40.0
    if tie == "between_beams":   # beams 0 and 1 of every audio: identical logits and equal sums, different histories
        for b in range(B):
            logits[b * G + 1] = logits[b * G]
            sums[b * G + 1] = sums[b * G]
    sums = sums.astype(np.float32)
    frozen = (B - 1,) if case == "finished_row" else ()
    cap = np.full(R, 100, np.int32)
    for b in frozen:
        cap[b * G:(b + 1) * G] = cur_len - n_init
    patience = [0.5, None, 2.0][CASES.index(case) % 3]
    bs = beam_ref.BeamSearch(B, G, eot, patience)
    MC = bs.max_candidates
    fin_before = []
    for b in range(B):   # audio 0 starts with one sequence in its list
        if b == 0 and case != "first":
            bs.finished[b].append((tuple(initial + [tsb + 1, ta, tsb + 2, eot]), -1.25))
        fin_before.append(list(bs.finished[b]))
    filters = dref.make_filters(n_init, eot, tsb, no_ts, suppress, blank, apply_timestamp_rules=rules, max_initial_timestamp_index=max_init)
    filtered = torch.from_numpy(logits).clone()
    for f in filters:
        f.apply(filtered, torch.tensor(tokens, dtype=torch.long))
    ref = bs.update(tokens, filtered.double().numpy(), sums.astype(np.float64), first=(case == "first"), frozen=frozen)
    inputs = dict(eot=eot, tsb=tsb, rules=rules, max_init=max_init, suppress=suppress + [no_ts] if rules else suppress, blank=blank + [eot],
                  n_init=n_init, cur_len=cur_len, logits=logits, tokens=tokens, sums=sums, cap=cap, MC=MC, fin_before=fin_before, frozen=frozen)
    return inputs, bs, ref


def _pick_seed(V, G, B, case, tie=None):
    """The first seed whose reference margins are all at least MIN_GAP (chosen on the CPU: nothing of the GPU's result enters)."""
    for seed in range(400):
        inputs, bs, ref = _case(V, G, B, case, 1000 * CASES.index(case) + seed, tie)
        if ref[4] >= MIN_GAP:
            return inputs, bs, ref
    raise AssertionError("no seed in 400 gives margins of %g" % MIN_GAP)


def _run(engine, V, G, B, first, x):
    _lib = importlib.import_module("whisper-char-alignment_amd._lib")
    R, K, MC = B * G, G + 1, x["MC"]
    tok_in = np.full((R, T_MAX), x["eot"], np.int32)
    for r, row in enumerate(x["tokens"]):
        tok_in[r, :len(row)] = row
    sup = np.zeros(V, np.uint8)
    sup[x["suppress"]] = 1
    blank = np.zeros(V, np.uint8)
    blank[x["blank"]] = 1
    fin_n = np.zeros(B, np.int32)
    fin_len = np.zeros((B, MC), np.int32)
    fin_sum = np.zeros((B, MC), np.float32)
    fin_tok = np.full((B, MC, T_MAX), -9, np.int32)
    for b, fin in enumerate(x["fin_before"]):
        fin_n[b] = len(fin)
        for q, (seq, score) in enumerate(fin):
            fin_len[b, q], fin_sum[b, q] = len(seq) - 1, score
            fin_tok[b, q] = x["eot"]
            fin_tok[b, q, :len(seq)] = seq
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t = dict(logits=dev(x["logits"]), tok_in=dev(tok_in), tok_out=dev(np.full((R, T_MAX), x["eot"], np.int32)),
             cur_len=dev(np.full(R, x["cur_len"], np.int32)), n_init=dev(np.full(R, x["n_init"], np.int32)), cap=dev(x["cap"]), sup=dev(sup),
             blank=dev(blank), sums=dev(x["sums"]), src=dev(np.full(R, -1, np.int32)), cand_tok=dev(np.full((R, K), -5, np.int32)),
             cand_lp=dev(np.zeros((R, K), np.float32)), fin_n=dev(fin_n), fin_len=dev(fin_len), fin_sum=dev(fin_sum), fin_tok=dev(fin_tok),
             trace=dev(np.full((R, 2), -7, np.int32)), n_done=dev(np.zeros(1, np.int32)))
    o = _lib.DecodeOpts(224, x["eot"], x["tsb"], 1 if x["rules"] else 0, x["max_init"], -1)
    d = _lib.BeamDesc(logits_dev=_vp(t["logits"]), tokens_in_dev=_vp(t["tok_in"]), tokens_out_dev=_vp(t["tok_out"]), cur_len_dev=_vp(t["cur_len"]),
                      n_initial_dev=_vp(t["n_init"]), cap_dev=_vp(t["cap"]), suppress_mask_dev=_vp(t["sup"]), blank_mask_dev=_vp(t["blank"]),
                      opts=C.pointer(o), sum_logprob_dev=_vp(t["sums"]), src_dev=_vp(t["src"]), cand_tok_dev=_vp(t["cand_tok"]),
                      cand_lp_dev=_vp(t["cand_lp"]), fin_n_dev=_vp(t["fin_n"]), fin_len_dev=_vp(t["fin_len"]), fin_sum_dev=_vp(t["fin_sum"]),
                      fin_tok_dev=_vp(t["fin_tok"]), trace_dev=_vp(t["trace"]), n_done_dev=_vp(t["n_done"]), batch=B, n_group=G, n_vocab=V,
                      T_max=T_MAX, first=1 if first else 0, max_candidates=MC)
    engine._bind_stream()
    _lib.check(engine._lib.wca_test_beam_step(engine._h, C.byref(d)))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in t.items()}


def _compare(x, bs, ref, got, G, B):
    nxt, src, sums, completed, gap, ties = ref
    n = x["cur_len"]
    for r in range(B * G):
        if r // G in x["frozen"]:   # past its budget: copied through
            assert list(got["tok_out"][r]) == list(got["tok_in"][r]) and got["src"][r] == r and list(got["trace"][r]) == [r, -1]
            continue
        assert list(got["tok_out"][r, :n + 1]) == nxt[r], (r, got["tok_out"][r, :n + 1], nxt[r])
        assert (got["tok_out"][r, n + 1:] == x["eot"]).all()
        assert got["src"][r] == src[r] and list(got["trace"][r]) == [src[r], nxt[r][-1]], (r, got["src"][r], src[r])
    np.testing.assert_allclose(got["sums"], sums, rtol=1e-4, atol=1e-4)
    for b in range(B):
        fin = bs.finished[b]
        assert got["fin_n"][b] == len(fin), (b, got["fin_n"][b], fin)
        for q, (seq, score) in enumerate(fin):
            assert got["fin_len"][b, q] == len(seq) - 1 and list(got["fin_tok"][b, q, :len(seq)]) == list(seq), (b, q)
            assert (got["fin_tok"][b, q, len(seq):] == x["eot"]).all()
            np.testing.assert_allclose(got["fin_sum"][b, q], score, rtol=1e-4, atol=1e-4)
    assert int(got["n_done"][0]) == bs.n_done(x["frozen"])


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("G", [1, 2, 5, 8])
@pytest.mark.parametrize("V", [97, 51865])
def test_beam_step_matches_the_reference(engine, V, G, B, case):
    x, bs, ref = _pick_seed(V, G, B, case)
    assert ref[4] >= MIN_GAP and ref[5] == 0, (ref[4], ref[5])   # no decision of this case hangs on fp32 noise, and nothing is tied
    got = _run(engine, V, G, B, case == "first", x)
    _compare(x, bs, ref, got, G, B)
    # the candidates themselves: G + 1 per offering row, none of them a token the filters removed
    offering = [r for r in range(B * G) if r // G not in x["frozen"]]
    assert (got["cand_tok"][offering] >= 0).all() and np.isfinite(got["cand_lp"][offering]).all()
    assert (np.diff(got["cand_lp"][offering], axis=1) <= 0).all()
    for b in x["frozen"]:
        assert (got["cand_tok"][b * G:(b + 1) * G] == -1).all()
    if case == "first":
        assert (got["cand_tok"][offering] >= x["tsb"]).all() and (got["cand_tok"][offering] <= x["tsb"] + x["max_init"]).all()


@pytest.mark.parametrize("tie", ["within_row", "between_beams"])
@pytest.mark.parametrize("V, G, B", [(97, 2, 1), (51865, 5, 3)])
def test_planted_exact_ties_follow_the_stated_order(engine, V, G, B, tie):
    x, bs, ref = _pick_seed(V, G, B, "text", tie)
    assert ref[5] > 0 and ref[4] >= MIN_GAP, (ref[4], ref[5])   # ties were met, and every other margin is wide
    got = _run(engine, V, G, B, False, x)
    _compare(x, bs, ref, got, G, B)
    if tie == "within_row":   # the lower of the two equal tokens comes first in every row's candidates
        ta = _vocab(V)[7][0]
        assert (got["cand_tok"][:, 0] == ta + 1).all() and (got["cand_tok"][:, 1] == ta + 3).all()
        assert np.array_equal(got["cand_lp"][:, 0], got["cand_lp"][:, 1])
