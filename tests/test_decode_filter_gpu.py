"""The logit filters of csrc/decode_filter.h on the MI355X, through every kernel that uses them, on the probe rows of
tests/decode_filter_probes.py: rows whose answer is the last forbidden or the first allowed token of one rule (tests/test_decode_gpu.py,
test_decode_rows_gpu.py, test_decode_sample_gpu.py and test_beam_step_gpu.py compare the choice on random logits, where an argmax lands
within one token of a given boundary about once in 25 000 draws).

  * decode_select_kernel<false>        wca_test_decode_select        one launch per (history, rules, initial form)
  * decode_select_kernel<true>         wca_test_decode_select_rows   every history and both initial forms mixed in each launch
  * decode_select_kernel<true, true>   wca_test_decode_sample_rows   at temperature 0 (the greedy tokens) and at T = 1 on the plant rows
  * beam_topk_kernel                   wca_test_beam_step            G in {1, 5, 16}

Tokens are IDENTICAL to the CPU oracle's (oracle/decoding_ref.select_step; the drawn ones to tests/decode_sample_ref.sample_step, the
candidates to tests/beam_ref.top_candidates on the oracle-filtered row), without exclusions: every margin of a probe is 0.9e-3 or more.
sum_logprob and the candidates' log-probabilities are within rtol = atol = 1e-4 of the float64 log-softmax of the oracle-filtered row
(the tolerance of test_select_kernel_bit_exact; on a 1e-3 ladder one wrong live token near the top moves it by 1e-3). A count row holds
-log(n_live): |sum_logprob + log(n_live)| must be below a quarter of log(n_live + 1) - log(n_live), in float64 from the oracle's own
count -- 5e-6 at 50 000 live tokens. Measured on the MI355X (profiles/decode_filter_tests.txt): 1.9e-7 at 50 333 live tokens, 0.04 of
the bound, and at most 3.7e-7 anywhere; the text-region counts stay in.

The test hooks take their own buffers and no engine state, so max_batch bounds nothing here; the rows go in launches of at most CHUNK."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import decode_filter_probes as P

pytestmark = pytest.mark.gpu

T_MAX = 40
CHUNK = 64
CAND_TOL = 1e-4


@pytest.fixture(scope="module")
def engines():
    pkg = importlib.import_module("whisper-char-alignment_amd")
    dims = {97: pkg.ModelDimensions(80, 1500, 128, 2, 1, 97, 448, 128, 2, 1),            # tests/test_beam_step_gpu.py's
            51865: pkg.ModelDimensions(80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)}      # the `small` fixture's
    return {V: pkg.WhisperAMD(d, device="cuda:0", max_batch=1 if V == 97 else 4, precision="f16") for V, d in dims.items()}


def _lib():
    return importlib.import_module("whisper-char-alignment_amd._lib")


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


_DEVICE = {}


def _device(V):
    """The probes of one vocabulary on the GPU, uploaded once: logits [N, V], the token rows [N, T_MAX], and the masks per rules."""
    if V not in _DEVICE:
        v, ps = P.vocab(V), P.probes(V)
        tokens = np.full((len(ps), T_MAX), v.eot, np.int32)
        for i, p in enumerate(ps):
            tokens[i, :len(p.tokens)] = p.tokens
        rows = {}   # the forms of one (history, rules) share one logits array: upload it once
        logits = torch.empty((len(ps), V), dtype=torch.float32, device="cuda")
        for i, p in enumerate(ps):
            if id(p.logits) not in rows:
                rows[id(p.logits)] = i
                logits[i] = torch.from_numpy(p.logits).cuda()
            else:
                logits[i] = logits[rows[id(p.logits)]]
        masks = {r: tuple(torch.from_numpy(m).cuda() for m in P.kernel_masks(V, r)) for r in (0, 1)}
        _DEVICE[V] = dict(logits=logits, tokens=torch.from_numpy(tokens), cur_len=np.array([len(p.tokens) for p in ps], np.int32),
                          n_init=np.array([p.n_init for p in ps], np.int32), masks=masks)
    return _DEVICE[V]


def _opts(V, rules):
    v = P.vocab(V)
    return _lib().DecodeOpts(224, v.eot, v.tsb, rules, v.max_init, -1)


def _check_written(V, tokens_before, got, cur_len):
    """Nothing but the new token was written."""
    eot = P.vocab(V).eot
    for r in range(len(cur_len)):
        assert torch.equal(got[r, :cur_len[r]], tokens_before[r, :cur_len[r]]) and (got[r, cur_len[r] + 1:] == eot).all(), r


def _check_select(V, idx, tok, lp, what):
    """The chosen tokens and sum_logprob (from 0) of the probes idx against the oracle."""
    ps, refs = P.probes(V), P.references(V)
    worst = 0.0
    for i, t, s in zip(idx, tok, lp):
        p, r = ps[i], refs[i]
        where = (what, V, p.hist, p.rules, p.form, p.label)
        assert not r.dead[t], where + (t, r.token)
        assert t == r.token, where + (t, r.token)
        np.testing.assert_allclose(s, r.logprob, rtol=1e-4, atol=1e-4, err_msg=str(where))
        if p.kind == "count":
            n = r.n_flat
            err, bound = abs(float(s) + np.log(n)), 0.25 * (np.log(n + 1) - np.log(n))
            worst = max(worst, err / bound)
            print("%s V=%d %s rules %d %s %s: n_live %d, |sum_logprob + log n| %.3e, bound %.3e" % (what, V, p.hist, p.rules, p.form, p.label, n, err, bound))
            assert err < bound, where + (n, err, bound)
    return worst


def _rows_order(idx):
    """The probes idx dealt out so that every launch of CHUNK rows mixes the histories and the initial forms."""
    n_launch = -(-len(idx) // CHUNK)
    return [i for s in range(n_launch) for i in idx[s::n_launch]]


def _launch_rows(m, V, idx, rules, temps=None, seeds=None):
    """wca_test_decode_select_rows (or, with temperatures, wca_test_decode_sample_rows) over the probes idx -> (tokens, sum_logprob)."""
    lib, D = _lib(), _device(V)
    eot = P.vocab(V).eot
    sup, blank = D["masks"][rules]
    o = _opts(V, rules)
    toks, lps = [], []
    m._bind_stream()
    for a in range(0, len(idx), CHUNK):
        sel = list(idx[a:a + CHUNK])
        B = len(sel)
        logits = D["logits"][torch.tensor(sel, device="cuda")].contiguous()
        before = D["tokens"][sel].clone()
        cur_len, n_init = D["cur_len"][sel], D["n_init"][sel]
        td, lpd = before.cuda(), torch.zeros(B, device="cuda")
        nd = torch.zeros(8, dtype=torch.int32, device="cuda")
        dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (cur_len, n_init, np.full(B, 100, np.int32))]
        if temps is None:
            lib.check(m._lib.wca_test_decode_select_rows(m._h, _vp(logits), B, V, _vp(td), T_MAX, _vp(dev[0]), _vp(dev[1]), _vp(dev[2]), 5, 8,
                                                         _vp(sup), _vp(blank), C.byref(o), _vp(lpd), _vp(nd)))
        else:
            tdev = torch.tensor(temps[a:a + B], dtype=torch.float32).cuda()
            sdev = torch.from_numpy(np.array(seeds[a:a + B], dtype=np.uint64).view(np.int64)).cuda()
            lib.check(m._lib.wca_test_decode_sample_rows(m._h, _vp(logits), B, V, _vp(td), T_MAX, _vp(dev[0]), _vp(dev[1]), _vp(dev[2]), 5, 8,
                                                         _vp(sup), _vp(blank), C.byref(o), _vp(lpd), _vp(nd), _vp(tdev), _vp(sdev)))
        torch.cuda.synchronize()
        got = td.cpu()
        new = [int(got[r, cur_len[r]]) for r in range(B)]
        assert nd.cpu().tolist() == [0, 0, 0, 0, 0, sum(t == eot for t in new), 0, 0]
        _check_written(V, before, got, cur_len)
        toks += new
        lps += lpd.cpu().tolist()
    return toks, lps


def _by_rules(V, kinds=None):
    ps = P.probes(V)
    return {r: [i for i, p in enumerate(ps) if p.rules == r and (kinds is None or p.kind in kinds)] for r in (1, 0)}


@pytest.mark.parametrize("V", P.VOCABS)
def test_uniform_select_at_every_boundary(engines, V):
    m, lib, D = engines[V], _lib(), _device(V)
    eot = P.vocab(V).eot
    m._bind_stream()
    worst = 0.0
    for hist, rules, form, a, b in P.groups(V):
        B, cur_len, n_init = b - a, int(D["cur_len"][a]), int(D["n_init"][a])
        assert (D["cur_len"][a:b] == cur_len).all() and (D["n_init"][a:b] == n_init).all()
        sup, blank = D["masks"][rules]
        o = _opts(V, rules)
        before = D["tokens"][a:b].clone()
        td, lpd = before.cuda(), torch.zeros(B, device="cuda")
        nd = torch.zeros(T_MAX, dtype=torch.int32, device="cuda")
        lib.check(m._lib.wca_test_decode_select(m._h, _vp(D["logits"][a:b]), B, V, _vp(td), T_MAX, cur_len, n_init, _vp(sup), _vp(blank), C.byref(o),
                                                _vp(lpd), _vp(nd)))
        torch.cuda.synchronize()
        got = td.cpu()
        new = got[:, cur_len].tolist()
        want_done = [0] * T_MAX
        want_done[cur_len] = sum(t == eot for t in new)
        assert nd.cpu().tolist() == want_done, (hist, rules, form)
        _check_written(V, before, got, [cur_len] * B)
        worst = max(worst, _check_select(V, range(a, b), new, lpd.cpu().tolist(), "uniform"))
    print("uniform V=%d: worst count-row error / bound %.3f" % (V, worst))


@pytest.mark.parametrize("V", P.VOCABS)
def test_select_rows_at_every_boundary(engines, V):
    for rules, idx in _by_rules(V).items():
        order = _rows_order(idx)
        D = _device(V)
        if rules:   # cur_len and n_initial differ from row to row within a launch
            assert len(set(D["cur_len"][order[:CHUNK]])) > 4 and len(set(D["n_init"][order[:CHUNK]])) == 2
        tok, lp = _launch_rows(engines[V], V, order, rules)
        worst = _check_select(V, order, tok, lp, "rows")
        print("rows V=%d rules %d: %d rows, worst count-row error / bound %.3f" % (V, rules, len(order), worst))


@pytest.mark.parametrize("V", P.VOCABS)
def test_sample_rows_at_temperature_0_choose_the_greedy_tokens(engines, V):
    for rules, idx in _by_rules(V).items():
        order = _rows_order(idx)
        tok, lp = _launch_rows(engines[V], V, order, rules, temps=[0.0] * len(order), seeds=[11 + i for i in range(len(order))])
        _check_select(V, order, tok, lp, "sample T=0")
        greedy_tok, greedy_lp = _launch_rows(engines[V], V, order, rules)
        assert tok == greedy_tok and np.array_equal(np.array(lp, np.float32).view(np.int32), np.array(greedy_lp, np.float32).view(np.int32))


@pytest.mark.parametrize("V", P.VOCABS)
def test_sample_rows_draw_a_live_plant_and_never_a_dead_one(engines, V):
    """T = 1 on the plant rows: the plant stands 50 above every other logit, the Gumbel noise spans about 19.5 (csrc/decode.hip). Token for
    token what the float64 sampler draws, with seeds whose two best perturbed scores the reference finds further apart than the fp32 margin."""
    ps, refs = P.probes(V), P.references(V)
    n_dead = 0
    for rules, idx in _by_rules(V, ("plant",)).items():
        order = _rows_order(idx)
        want = [P.sample_reference(V, ps[i], 1000 + 53 * n) for n, i in enumerate(order)]
        tok, lp = _launch_rows(engines[V], V, order, rules, temps=[1.0] * len(order), seeds=[w[0] for w in want])
        for i, t, s, (seed, w_tok, w_lp) in zip(order, tok, lp, want):
            p, r = ps[i], refs[i]
            where = (V, p.hist, p.rules, p.form, p.label, seed)
            assert not r.dead[t], where + (t,)
            assert (w_tok == p.expect) == (not r.dead[p.expect]), where   # the reference itself: a live plant is drawn, a dead one is not
            assert t == w_tok, where + (t, w_tok)
            np.testing.assert_allclose(s, w_lp, rtol=1e-4, atol=1e-4, err_msg=str(where))
            n_dead += bool(r.dead[p.expect])
    assert n_dead > 20


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("G", [1, 5, 16])
@pytest.mark.parametrize("V", P.VOCABS)
def test_beam_candidates_at_every_boundary(engines, V, G, first):
    """The G + 1 candidates of every probe row. The beams of an audio are G neighbouring probes of one (history, rules, initial form),
    the last one repeated where the group does not fill an audio. `first` only tells beam_merge that an audio's beams are still
    identical; the candidates of a row do not depend on it."""
    m, lib, D = engines[V], _lib(), _device(V)
    v, refs = P.vocab(V), P.references(V)
    K = G + 1
    audios = {1: [], 0: []}   # rules -> [G probe indices]
    for hist, rules, form, a, b in P.groups(V):
        rows = list(range(a, b)) + [b - 1] * (-(b - a) % G)
        audios[rules] += [rows[j:j + G] for j in range(0, len(rows), G)]
    m._bind_stream()
    n_short = 0
    for rules, groups in audios.items():
        sup, blank = D["masks"][rules]
        o = _opts(V, rules)
        per = max(1, CHUNK // G)
        for a in range(0, len(groups), per):
            sel = [i for g in groups[a:a + per] for i in g]
            B, R = len(sel) // G, len(sel)
            dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
            t = dict(logits=D["logits"][torch.tensor(sel, device="cuda")].contiguous(), tok_in=D["tokens"][sel].cuda(),
                     tok_out=dev(np.full((R, T_MAX), v.eot, np.int32)), cur_len=dev(D["cur_len"][sel]), n_init=dev(D["n_init"][sel]),
                     cap=dev(np.full(R, 100, np.int32)), sums=dev(np.zeros(R, np.float32)), src=dev(np.full(R, -1, np.int32)),
                     cand_tok=dev(np.full((R, K), -5, np.int32)), cand_lp=dev(np.zeros((R, K), np.float32)), fin_n=dev(np.zeros(B, np.int32)),
                     fin_len=dev(np.zeros((B, G), np.int32)), fin_sum=dev(np.zeros((B, G), np.float32)),
                     fin_tok=dev(np.full((B, G, T_MAX), -9, np.int32)), trace=dev(np.full((R, 2), -7, np.int32)), n_done=dev(np.zeros(1, np.int32)))
            d = lib.BeamDesc(logits_dev=_vp(t["logits"]), tokens_in_dev=_vp(t["tok_in"]), tokens_out_dev=_vp(t["tok_out"]), cur_len_dev=_vp(t["cur_len"]),
                             n_initial_dev=_vp(t["n_init"]), cap_dev=_vp(t["cap"]), suppress_mask_dev=_vp(sup), blank_mask_dev=_vp(blank),
                             opts=C.pointer(o), sum_logprob_dev=_vp(t["sums"]), src_dev=_vp(t["src"]), cand_tok_dev=_vp(t["cand_tok"]),
                             cand_lp_dev=_vp(t["cand_lp"]), fin_n_dev=_vp(t["fin_n"]), fin_len_dev=_vp(t["fin_len"]), fin_sum_dev=_vp(t["fin_sum"]),
                             fin_tok_dev=_vp(t["fin_tok"]), trace_dev=_vp(t["trace"]), n_done_dev=_vp(t["n_done"]), batch=B, n_group=G, n_vocab=V,
                             T_max=T_MAX, first=first, max_candidates=G)
            lib.check(m._lib.wca_test_beam_step(m._h, C.byref(d)))
            torch.cuda.synchronize()
            cand_tok, cand_lp = t["cand_tok"].cpu().numpy(), t["cand_lp"].cpu().numpy()
            assert torch.equal(t["tok_in"].cpu(), D["tokens"][sel])
            for r, i in enumerate(sel):
                p, want = P.probes(V)[i], refs[i].cands[:K]
                where = (V, G, p.hist, p.rules, p.form, p.label)
                n = len(want)
                n_short += n < K
                assert cand_tok[r].tolist() == [tk for _, tk in want] + [-1] * (K - n), where + (cand_tok[r].tolist(), want)
                np.testing.assert_allclose(cand_lp[r, :n], [lp for lp, _ in want], rtol=CAND_TOL, atol=CAND_TOL, err_msg=str(where))
                assert np.isneginf(cand_lp[r, n:]).all(), where
    if V == 97 and G == 16:   # after a closing timestamp only eot, the sot tokens and the last timestamps are live: fewer than 17
        assert n_short > 0
