"""The KV-cached greedy decode loop on the MI355X against float64 at every cache length (tests/decode_cache_ref.py: the position-coded checkpoint, the
reference, the lengths): what the loop leaves in the self-attention cache [L][2][B][T_max][d] and in the logits of its last forward (wca_test_decode_state)
is compared element by element, for the three producers of the cache -- the few-row GEMM's append, launch_kv_append (set_decode_mode(False, 1)) and the
prefill's scatter -- and for the per-row form. tests/test_decode_cache_ref.py shows on the CPU that a wrong slot, stride, plane, positional row, key
count or batch row moves one of these quantities by at least 10 bounds."""
import importlib

import numpy as np
import pytest
import torch

import decode_cache_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    return R.scene()


@pytest.fixture(scope="module")
def tok():
    return importlib.import_module("whisper-char-alignment_amd.tokenizer").get_tokenizer(True, language="en", task="transcribe")


@pytest.fixture(scope="module")
def engines(sc):
    pkg = importlib.import_module("whisper-char-alignment_amd")
    made = {}

    def get(precision):
        if precision not in made:
            made[precision] = pkg.WhisperAMD(sc["D"], device="cuda:0", max_batch=len(R.AUDIO), precision=precision).load_state_dict(sc["sd"])
        return made[precision]

    return get


@pytest.fixture(scope="module")
def mel_dev(sc):
    return sc["mel"].cuda()


_check_state, _check_choices = R.check_state, R.check_choices      # shared with tests/test_decode_widths_gpu.py; here on the 256-wide TOL


# f16 at every length; the reference-precision engine (the loop computes in f16 there too, on the hi halves of the pair-format cross-K/V) at the tile boundaries
STEPWISE = [(p, f, n) for p, lengths in (("f16", R.LENGTHS), ("reference", R.LENGTHS_REFERENCE)) for f in (True, False) for n in lengths]


@pytest.mark.parametrize("precision,fused,n", STEPWISE, ids=["%s-%s-%d" % (p, "fused" if f else "separate", n) for p, f, n in STEPWISE])
def test_stepwise_cache_and_logits(sc, engines, mel_dev, tok, precision, fused, n):
    """Every position through run_decode_step: n initial tokens, no prefill, one choice. Teacher-forced by construction."""
    m = engines(precision)
    m.set_decode_mode(fused, 1)
    try:
        toks, n_tok, lp = m.greedy_decode(mel_dev[:R.B], None, None, sc["tokens"][:n].tolist(), R.text_suppress_mask(), None, sample_len=1, eot=tok.eot,
                                          timestamp_begin=tok.timestamp_begin, apply_timestamp_rules=False)
        assert m.last_decode_positions() == (0, n)
        logits, cache = m.decode_state(R.B, n + 1)
    finally:
        m.set_decode_mode(True, 1)
    tag = "step %s %s n=%d" % (precision, "fused" if fused else "separate", n)
    want_logits = sc["ref"].logits(sc["x"][:, n - 1])
    _check_state(tag, cache, logits, R.planes_of(sc["K"][:, :, :n], sc["V"][:, :, :n], n + 1), [n] * R.B, want_logits)
    assert (toks[:, :n] == sc["tokens"][:n].numpy()).all() and (n_tok == n + 1).all()
    _check_choices(tag, want_logits[:, None], toks[:, n:n + 1], lp, R.TOL["logits"])


@pytest.mark.parametrize("n", R.PREFILL_LENGTHS)
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
@pytest.mark.parametrize("precision", ["f16", "reference"])
def test_prefill_then_steps(sc, engines, mel_dev, tok, precision, fused, n):
    """The batched prefill over n initial tokens (the scatter fills slots [0, n)), then PREFILL_STEPS sampled steps; the reference is teacher-forced on the
    tokens the GPU returned. The <|sot|> rows of the prefill stay behind the last step's logits."""
    m = engines(precision)
    S, sot = R.PREFILL_STEPS, 2
    m.set_decode_mode(fused, 1)
    try:
        toks, n_tok, lp = m.greedy_decode(mel_dev[:R.B], None, None, sc["tokens"][:n].tolist(), R.text_suppress_mask(), None, sample_len=S, eot=tok.eot,
                                          timestamp_begin=tok.timestamp_begin, apply_timestamp_rules=False, no_speech=tok.no_speech, sot_index=sot,
                                          prefill=1)
        nsp = m.last_no_speech_prob.copy()
        assert m.last_decode_positions() == (n, S - 1)
        logits, cache = m.decode_state(R.B, n + S, 2 * R.B)
    finally:
        m.set_decode_mode(True, 1)
    tag = "prefill %s %s n=%d" % (precision, "fused" if fused else "separate", n)
    assert (toks[:, :n] == sc["tokens"][:n].numpy()).all() and (n_tok == n + S).all()
    fed = n + S - 1                                   # the last sampled token is never fed
    K, V, x, _ = sc["ref"].forward(torch.from_numpy(toks[:, :fed].astype(np.int64)), sc["ckv"])
    want_logits = torch.cat([sc["ref"].logits(x[:, fed - 1]), sc["ref"].logits(x[:, sot])])
    _check_state(tag, cache, logits, R.planes_of(K, V, n + S), [fed] * R.B, want_logits)
    _check_choices(tag, sc["ref"].logits(x[:, n - 1:fed]), toks[:, n:], lp, R.TOL["logits"])
    want_nsp = want_logits[R.B:].softmax(-1)[:, tok.no_speech].numpy()
    assert np.allclose(nsp, want_nsp, rtol=float(np.expm1(2 * R.TOL["logits"])) + 1e-5, atol=0), (nsp, want_nsp)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
def test_ragged_rows_hold_their_own_positions(sc, engines, mel_dev, tok, fused):
    """wca_decode with per_row 1: rows of 3 / 64 / 65 / 226 initial tokens of their own, padded to 226 in the prefill, then ROWS_STEPS steps at per-row
    positions. Row b's slots [0, n_initial[b] + steps - 1) hold ITS positions -- the pad left-overs of the short rows are overwritten where the
    steps went --, its last logits are its own last position's, and the <|sot|> rows are read at each row's own index."""
    m = engines("f16")
    ni, S = R.ROWS_N_INITIAL, R.ROWS_STEPS
    Bc = len(ni)
    initial = [R.token_row(n, row=b + 1).tolist() for b, n in enumerate(ni)]
    sot = [0, 5, 64, 100]
    m.set_decode_mode(fused, 1)
    try:
        toks, n_tok, lp = m.greedy_decode_rows(mel_dev[:Bc], None, None, initial, sot, [S] * Bc, R.text_suppress_mask(), None, eot=tok.eot,
                                               timestamp_begin=tok.timestamp_begin, apply_timestamp_rules=False, no_speech=tok.no_speech)
        assert m.last_decode_positions() == (max(ni), S - 1)
        T_max = max(ni) + S
        logits, cache = m.decode_state(Bc, T_max, 2 * Bc)
    finally:
        m.set_decode_mode(True, 1)
    tag = "rows %s" % ("fused" if fused else "separate")
    ref = sc["ref"]
    d = sc["D"].n_text_state
    planes = torch.zeros(sc["D"].n_text_layer, 2, Bc, T_max, d, dtype=torch.float64)
    last, at_sot, steps = [], [], []
    for b in range(Bc):
        fed = ni[b] + S - 1
        assert toks[b, :ni[b]].tolist() == initial[b] and n_tok[b] == ni[b] + S
        ckv_b = [(k[b:b + 1], v[b:b + 1]) for k, v in sc["ckv4"]]
        K, V, x, _ = ref.forward(torch.from_numpy(toks[b:b + 1, :fed].astype(np.int64)), ckv_b)
        planes[:, 0, b, :fed] = K[:, 0]
        planes[:, 1, b, :fed] = V[:, 0]
        last.append(ref.logits(x[:, fed - 1]))
        at_sot.append(ref.logits(x[:, sot[b]]))
        steps.append(ref.logits(x[:, ni[b] - 1:fed]))
    _check_state(tag, cache, logits, planes, [n + S - 1 for n in ni], torch.cat(last + at_sot))
    chosen = np.stack([toks[b, ni[b]:ni[b] + S] for b in range(Bc)])
    _check_choices(tag, torch.cat(steps), chosen, lp, R.TOL["logits"])


def test_accessor_refuses_what_the_buffers_do_not_hold(sc, engines, mel_dev, tok):
    m = engines("f16")
    _lib = importlib.import_module("whisper-char-alignment_amd._lib")
    m.greedy_decode(mel_dev[:2], None, None, sc["tokens"][:3].tolist(), R.text_suppress_mask(), None, sample_len=2, eot=tok.eot,
                    timestamp_begin=tok.timestamp_begin, apply_timestamp_rules=False)
    logits, cache = m.decode_state(2, 5)
    assert logits.shape == (2, R.DIMS[5]) and cache.shape == (2, 2, 2, 5, 256)
    for args in ((3, 5), (2, 6), (2, 4), (0, 5), (2, 5, 4), (2, 5, 0)):   # another batch, another T_max, the <|sot|> rows no prefill left
        with pytest.raises(_lib.WcaError):
            m.decode_state(*args)
