"""The KV-cached greedy decode loop on the MI355X against float64 at every Whisper width (384, 512, 768, 1024, 1280; the 256-wide scene is
tests/test_decode_cache_gpu.py). tests/decode_cache_ref.py gives the scene of a width -- the position-coded checkpoint with heads = width / 64, the
float64 reference, the bounds -- and tests/test_decode_cache_ref.py pins on the CPU which launches a step and a prefill are made of at each width
(ROUTES: the fused LayerNorm prologue at K / 256 = 2, 3, 4; the separate LayerNorm + tile GEMM + launch_kv_append route of 384 and 1280; the few-row
kernel's split-K by 2, 3, 4, 5 at fc2 and by 2 at the 1280-wide out-projections) and that every wiring fault moves an asserted quantity by 10 bounds.

Per width, one engine pair (f16 and reference precision, built when first asked) runs
  step     n initial tokens through run_decode_step, one choice: n = 1, 64, 65, 129, 448 in the f16 engine, 65 and 448 in the reference-precision one
           (the loop computes in f16 there too, on the hi halves of the pair-format cross-K/V, whose rows are 2 L 2 d wide);
  prefill  the batched prefill over n = 42, 43, 130 tokens (B n = 126: two row blocks of the few-row kernel; 129 and 390: the tile route), then
           PREFILL_STEPS sampled steps, in both engines;
  rows     the per-row form: rows of 3 / 64 / 65 / 226 tokens of their own, then ROWS_STEPS steps;
each with set_decode_mode(True, 1) and (False, 1). Compared element by element with float64: the cache planes [L][2][B][T][d] over each row's fed
slots, layer 0 and the deeper layers, the logits of the last forward, and the choices and sum_logprob (decode_cache_ref.check_choices).

Bounds, none from the engine (decode_cache_ref.bounds): per quantity max(4 x the distance of the float64 reference with f16-rounded operands and f16-stored
activations from float64 on the width's scene, one f16 spacing of the largest reference entry). Every case prints its distances and their share of
the bounds; profiles/decode_width_tests.txt and DESIGN.md hold the per-width maxima."""
import importlib

import numpy as np
import pytest
import torch

import decode_cache_ref as R

pytestmark = pytest.mark.gpu

CASES = []
for _w in R.NEW_WIDTHS:
    CASES += [(_w, "step", p, f, n) for p, lengths in (("f16", R.STEPWISE_WIDTHS), ("reference", R.STEPWISE_WIDTHS_REFERENCE)) for f in (True, False)
              for n in lengths]
    CASES += [(_w, "prefill", p, f, n) for p in ("f16", "reference") for f in (True, False) for n in R.PREFILL_LENGTHS]
    CASES += [(_w, "rows", "f16", f, max(R.ROWS_N_INITIAL)) for f in (True, False)]

_WORLD = {}
_MAXIMA = {}     # width -> quantity -> the largest share of its bound over the cases run


@pytest.fixture(scope="module", autouse=True)
def _drop_the_last_world():
    yield
    _WORLD.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def tok():
    return importlib.import_module("whisper-char-alignment_amd.tokenizer").get_tokenizer(True, language="en", task="transcribe")


@pytest.fixture
def world(wca):
    """The width's scene, bounds, log-mels on the device and engines, built when the first case of a width asks and dropped when another width
    does (the cases are ordered by width). Nothing in it is changed by a test."""
    def get(width):
        if width not in _WORLD:
            _WORLD.clear()
            torch.cuda.empty_cache()
            sc = R.scene(width)
            made = {}

            def engine(precision):
                if precision not in made:
                    made[precision] = wca.WhisperAMD(sc["D"], device="cuda:0", max_batch=len(R.AUDIO), precision=precision).load_state_dict(sc["sd"])
                return made[precision]

            _WORLD[width] = {"sc": sc, "tol": R.bounds(width)["tol"], "mel": sc["mel"].cuda(), "engine": engine}
        return _WORLD[width]
    return get


def _note(width, dist, tol):
    best = _MAXIMA.setdefault(width, {})
    for q, v in dist.items():
        best[q] = max(best.get(q, 0.0), v / tol[q])


def _step(w, tok, m, tag, n):
    """Every position through run_decode_step: n initial tokens, no prefill, one choice. Teacher-forced by construction."""
    sc, tol = w["sc"], w["tol"]
    toks, n_tok, lp = m.greedy_decode(w["mel"][:R.B], None, None, sc["tokens"][:n].tolist(), R.text_suppress_mask(), None, sample_len=1, eot=tok.eot,
                                      timestamp_begin=tok.timestamp_begin, apply_timestamp_rules=False)
    assert m.last_decode_positions() == (0, n)
    logits, cache = m.decode_state(R.B, n + 1)
    want_logits = sc["ref"].logits(sc["x"][:, n - 1])
    dist = R.check_state(tag, cache, logits, R.planes_of(sc["K"][:, :, :n], sc["V"][:, :, :n], n + 1), [n] * R.B, want_logits, tol)
    assert (toks[:, :n] == sc["tokens"][:n].numpy()).all() and (n_tok == n + 1).all()
    R.check_choices(tag, want_logits[:, None], toks[:, n:n + 1], lp, tol["logits"])
    return dist


def _prefill(w, tok, m, tag, n):
    """The batched prefill over n initial tokens (the scatter fills slots [0, n)), then PREFILL_STEPS sampled steps; the reference is teacher-forced on
    the tokens the GPU returned. The <|sot|> rows of the prefill stay behind the last step's logits."""
    sc, tol = w["sc"], w["tol"]
    S, sot = R.PREFILL_STEPS, 2
    toks, n_tok, lp = m.greedy_decode(w["mel"][:R.B], None, None, sc["tokens"][:n].tolist(), R.text_suppress_mask(), None, sample_len=S, eot=tok.eot,
                                      timestamp_begin=tok.timestamp_begin, apply_timestamp_rules=False, no_speech=tok.no_speech, sot_index=sot,
                                      prefill=1)
    nsp = m.last_no_speech_prob.copy()
    assert m.last_decode_positions() == (n, S - 1)
    logits, cache = m.decode_state(R.B, n + S, 2 * R.B)
    assert (toks[:, :n] == sc["tokens"][:n].numpy()).all() and (n_tok == n + S).all()
    fed = n + S - 1                                   # the last sampled token is never fed
    K, V, x, _ = sc["ref"].forward(torch.from_numpy(toks[:, :fed].astype(np.int64)), sc["ckv"])
    want_logits = torch.cat([sc["ref"].logits(x[:, fed - 1]), sc["ref"].logits(x[:, sot])])
    dist = R.check_state(tag, cache, logits, R.planes_of(K, V, n + S), [fed] * R.B, want_logits, tol)
    R.check_choices(tag, sc["ref"].logits(x[:, n - 1:fed]), toks[:, n:], lp, tol["logits"])
    want_nsp = want_logits[R.B:].softmax(-1)[:, tok.no_speech].numpy()
    assert np.allclose(nsp, want_nsp, rtol=float(np.expm1(2 * tol["logits"])) + 1e-5, atol=0), (nsp, want_nsp)
    return dist


def _rows(w, tok, m, tag):
    """wca_decode with per_row 1: rows of 3 / 64 / 65 / 226 initial tokens of their own, padded to 226 in the prefill, then ROWS_STEPS steps at per-row
    positions. Row b's slots [0, n_initial[b] + steps - 1) hold ITS positions, its last logits are its own last position's, and the <|sot|> rows are
    read at each row's own index."""
    sc, tol = w["sc"], w["tol"]
    ni, S = R.ROWS_N_INITIAL, R.ROWS_STEPS
    Bc = len(ni)
    initial = [R.token_row(n, row=b + 1, width=sc["width"]).tolist() for b, n in enumerate(ni)]
    sot = [0, 5, 64, 100]
    toks, n_tok, lp = m.greedy_decode_rows(w["mel"][:Bc], None, None, initial, sot, [S] * Bc, R.text_suppress_mask(), None, eot=tok.eot,
                                           timestamp_begin=tok.timestamp_begin, apply_timestamp_rules=False, no_speech=tok.no_speech)
    assert m.last_decode_positions() == (max(ni), S - 1)
    T_max = max(ni) + S
    logits, cache = m.decode_state(Bc, T_max, 2 * Bc)
    ref = sc["ref"]
    planes = torch.zeros(sc["D"].n_text_layer, 2, Bc, T_max, sc["D"].n_text_state, dtype=torch.float64)
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
    dist = R.check_state(tag, cache, logits, planes, [n + S - 1 for n in ni], torch.cat(last + at_sot), tol)
    chosen = np.stack([toks[b, ni[b]:ni[b] + S] for b in range(Bc)])
    R.check_choices(tag, torch.cat(steps), chosen, lp, tol["logits"])
    return dist


@pytest.mark.parametrize("width,kind,precision,fused,n", CASES,
                         ids=["%d-%s-%s-%s-n%d" % (w, k, p, "fused" if f else "separate", n) for w, k, p, f, n in CASES])
def test_decode_against_float64(world, tok, width, kind, precision, fused, n):
    w = world(width)
    m = w["engine"](precision)
    tag = "width %d %s %s %s n=%d" % (width, kind, precision, "fused" if fused else "separate", n)
    m.set_decode_mode(fused, 1)
    try:
        dist = _step(w, tok, m, tag, n) if kind == "step" else _prefill(w, tok, m, tag, n) if kind == "prefill" else _rows(w, tok, m, tag)
    finally:
        m.set_decode_mode(True, 1)
    _note(width, dist, w["tol"])


def test_print_the_maxima():
    """The largest share of its bound each quantity reached at each width, over the cases this process ran (nothing is asserted here: every case asserts
    its own)."""
    for width in sorted(_MAXIMA):
        b = R.bounds(width)
        print("decode-width maxima %d: %s" % (width, "  ".join("%s %.2f of %.3e (yardstick %.3e, x %.2f)" % (
            q, r, b["tol"][q], b["yard"][q], r * b["tol"][q] / b["yard"][q]) for q, r in _MAXIMA[width].items())))
