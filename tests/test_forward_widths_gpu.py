"""The whole forward at every Whisper width on both sides of each GEMM plan switch (run on the MI355X with `-m gpu`): per width one engine
(2 + 2 layers, 80 mels, heads d / 64) and one float64 reference forward (tests/forward_ref.py, torch float64 on the device) of the width's
largest batch, whose rows serve every smaller batch -- a row's reference does not depend on the batch. The batches are
forward_ref.case_batches: S - 1 and S for every batch S <= 20 at which the plan of some site changes (tests/test_forward_ref.py prints the
census and pins it against the hand-derived switches), cut only by the ceilings 17 at 384 / 512 wide and 7 at 1280 wide: 17, 17, 15, 11, 7.
Each batch runs in the contract mode and in the f16 mode with separate and with fused LayerNorms, with 6 and with 40 tokens per row (M = B n
on both sides of the few-row kernel's 128 rows in every width).

Observables: model.encode -> ln_post output [B,1500,d]; model.get_attentions(medfilt_width=1) -> softmaxed maps [B,L,H,n,1500] and logits
[B,n,V]. Every row of every batch is compared (the maxima and means run over all of them).

Bounds, none taken from the engine (forward_ref.py): the contract mode within max(8 x the fp32 oracle's own distance from float64 on this
width's first two utterances, the project's floors 1e-5 / 2e-6 / 1e-5 rel); the f16 mode within 4 x the distance of the float64 forward with
f16-rounded operands and f16-stored outputs on the same rows and tokens, maximum and mean. profiles/forward_width_tests.txt holds the
figures of every case. Measured on the MI355X: the contract mode at most 0.48 of its bound (the fp32 checkpoint; 0.46 on f16-exact
weights); the f16 mode at most 1.65 x its yardstick (maps, 768 wide), the encoder output 1.10 x, every mean 0.97 .. 1.03 x; the
fused-LayerNorm runs the same as the separate ones. (Before the statement rounded the encoder's ln_post output, which the f16 mode keeps in
an f16 buffer, the encoder output stood at 2.59 x, and 2.06 x in the mean at 384 wide: that one rounding of order-1 values.)

Once per width the first three utterances also go through the batched route (_batched_route: scores, log-probabilities, selection, jump
frames); the 768-wide engine also runs an fp32 checkpoint that f16 does not hold."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import forward_ref as fr
import postproc_ref as pr

pytestmark = pytest.mark.gpu

MODES = ("contract", "f16", "f16_fused")
SOT, EOT, N_LONG = fr.SOT, fr.EOT, fr.N_LONG
try:        # the cases are the census', so collecting them needs the library; without it one test fails and says why
    _LIB = importlib.import_module("whisper-char-alignment_amd")._lib.load()
    CASES = [c for d in fr.WIDTHS for c in [(d, mode, B) for mode in MODES for B in fr.case_batches(_LIB, d)] + [(d, "batched", fr.BATCHED_B)]]
    _COLLECT_ERROR = None
except Exception as e:      # noqa: BLE001
    _LIB, CASES, _COLLECT_ERROR = None, [], e


def test_cases_come_from_the_census():
    assert _COLLECT_ERROR is None, "the plan census could not be taken: %r" % (_COLLECT_ERROR,)
    assert {d for d, _, _ in CASES} == set(fr.WIDTHS)


def _build(wca, d, B, inexact=False):
    from oracle import whisper_ref
    dims = fr.model_dims(wca, d)
    sd = fr.model_state_dict(dims, seed=fr.MODEL_SEED[d], inexact=inexact)
    mel, tokens, lengths = fr.inputs(d, B)
    out = fr.ForwardRef(sd, dims, device="cuda").forward(mel, tokens)
    ref = fr.observables(out)
    ref["qk"] = torch.stack(out["qk"], dim=1)      # [B, L, H, n, 1500]: what the batched route's head statistics start from
    w = whisper_ref.WhisperRef(sd, dims)
    enc32 = w.encoder(mel[:2])
    logits32, qk32 = w.decoder(tokens[:2], enc32)
    obs32 = fr.observables({"enc": enc32, "qk": qk32, "logits": logits32})
    obs32["qk"] = torch.stack(qk32, dim=1)
    model = wca.WhisperAMD(dims, device="cuda:0", max_batch=B, precision="reference").load_state_dict(sd)
    return {"d": d, "dims": dims, "sd": sd, "mel": mel.cuda(), "tokens": tokens.cuda(), "lengths": lengths, "ref": ref, "obs32": obs32,
            "obs16": None, "model": model, "B": B}


def _cut(obs, B, n, rows=None):
    """rows [0, B) (or `rows` of them) and the first n tokens: under the causal mask a token's maps and logits do not depend on later tokens"""
    r = slice(0, B) if rows is None else rows
    return {"enc": obs["enc"][r], "maps": obs["maps"][r][:, :, :, :n], "logits": obs["logits"][r][:, :n]}


_WORLD = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_the_last_world():
    yield
    _WORLD.clear()
    torch.cuda.empty_cache()


@pytest.fixture
def world(wca):
    """The width's engine, inputs and references, built when the first case of a width asks and dropped when another width does (the cases
    are ordered by width). Nothing in it is changed by a test."""
    def get(d, inexact=False):
        key = (d, inexact)
        if key not in _WORLD:
            _WORLD.clear()
            torch.cuda.empty_cache()
            _WORLD[key] = _build(wca, d, 4 if inexact else fr.b_max(_LIB, d), inexact)
        return _WORLD[key]
    return get


def _observe(w, B, n):
    m = w["model"]
    enc = m.encode(w["mel"][:B])
    maps, logits = m.get_attentions(w["mel"][:B], w["tokens"][:B, :n], [fr.N_CTX] * B, medfilt_width=1)
    return {"enc": enc, "maps": maps, "logits": logits}


def _fmt(dist):
    return "  ".join("%s %.3g (mean %.3g)" % (k, v[0], v[1]) for k, v in dist.items())


def _logprobs64(logits, tokens):
    """log_softmax(logits[sot_len + i, :eot])[tokens[sot_len + 1 + i]] for the n - sot_len - 2 text tokens of one row"""
    n_text = len(tokens) - len(SOT) - 2
    rows = logits[len(SOT):len(SOT) + n_text, :EOT]
    lse = rows.max(axis=-1) + np.log(np.exp(rows - rows.max(axis=-1, keepdims=True)).sum(axis=-1))
    return rows[np.arange(n_text), tokens[len(SOT) + 1:len(SOT) + 1 + n_text]] - lse


def _batched_route(w):
    """The first fr.BATCHED_B utterances (100, 668 and 1237 frames) through encode_batch + align_batch (phase 1 into a cross-K/V slot, the
    decoder behind it on its own stream, the head statistics on the captured logits, the chunked vocabulary projection of the
    log-probabilities, the ragged DTW), in the contract mode. Against float64 (fr.alignment_reference on the reference's logits):
      scores     (wca_test_last_scores) within max(8 x the fp32 oracle's relative distance, the project's 2e-5) of max(1, |s|)
      log-probs  within max(8 x the fp32 oracle's distance, 2 x 1e-5 of the largest |logit|): a log-softmax moves by at most twice what its
                 logits move, and 1e-5 of the largest is the logits' floor
      selection  the reference's two best heads wherever those stand GAP_FACTOR score bounds clear of the third (the postproc tests' rule)
      jump frames  EQUAL to the oracle DTW's on the float64 matrix at every row that is decided: whose frame no matrix within the project's
                 bound of the aggregated matrix (rtol 2e-5, atol 1e-7) and no fp32 rounding of the DTW's cost table can move
                 (fr.jump_decisions). At most 2 % of the rows may be undecided, a condition on the seeds that tests/test_forward_ref.py
                 checks from the reference alone; measured: none is."""
    m, B, n, d = w["model"], fr.BATCHED_B, N_LONG, w["d"]
    LH = w["dims"].n_text_layer * w["dims"].n_text_head
    frames = [L // 320 for L in w["lengths"][:B]]
    m.set_precision("reference")
    opts = m.make_opts(aggregation="topk", topk=fr.TOPK, sot_len=len(SOT), medfilt_width=fr.MEDFILT_WIDTH)
    m.encode_batch(mel=w["mel"][:B])
    jump, sel, lp = m.align_batch(None, None, w["tokens"][:B], [n] * B, frames, opts, token_logprobs_vocab_end=EOT)
    scores = np.zeros((B, LH), np.float32)
    wca_lib = importlib.import_module("whisper-char-alignment_amd")._lib
    wca_lib.check(_LIB.wca_test_last_scores(m._h, B, scores.ctypes.data_as(C.POINTER(C.c_float))))
    tokens = w["tokens"][:B].cpu().numpy()
    qk64, qk32 = w["ref"]["qk"][:B].cpu().numpy().reshape(B, LH, n, -1), w["obs32"]["qk"].double().numpy().reshape(2, LH, n, -1)
    lg64, lg32 = w["ref"]["logits"][:B].cpu().numpy(), w["obs32"]["logits"].double().numpy()
    s32 = np.stack([r["scores"] for r in fr.alignment_reference(qk32, frames[:2], pr.SCORE_RTOL, pr.MATRIX_RTOL, pr.MATRIX_ATOL, pr.GAP_FACTOR)])
    s64 = np.stack([r["scores"] for r in fr.alignment_reference(qk64, frames, pr.SCORE_RTOL, pr.MATRIX_RTOL, pr.MATRIX_ATOL, pr.GAP_FACTOR)])
    lp64 = np.stack([_logprobs64(lg64[b], tokens[b]) for b in range(B)])
    scale = np.maximum(1.0, np.abs(s64))
    yard_s = float(np.max(np.abs(s32 - s64[:2]) / scale[:2]))
    yard_lp = max(float(np.max(np.abs(_logprobs64(lg32[b], tokens[b]) - lp64[b]))) for b in range(2))
    bound_s = max(fr.CONTRACT_FACTOR * yard_s, pr.SCORE_RTOL)
    bound_lp = max(fr.CONTRACT_FACTOR * yard_lp, 2 * fr.FLOOR["logits"] * float(np.abs(lg64).max()))
    got_s = float(np.max(np.abs(scores - s64) / scale))
    n_text = lp64.shape[1]
    got_lp = float(np.max(np.abs(lp[:, :n_text] - lp64)))
    ref = fr.alignment_reference(qk64, frames, bound_s, pr.MATRIX_RTOL, pr.MATRIX_ATOL, pr.GAP_FACTOR)
    N = n - len(SOT) - 1
    undecided = sum(int((~r["decided"]).sum()) for r in ref)
    wrong = [(b, i, int(jump[b][i]), int(r["jump"][i])) for b, r in enumerate(ref) for i in range(N) if r["decided"][i] and jump[b][i] != r["jump"][i]]
    agree = sum(int(np.sum(np.asarray(jump[b][:N]) == r["jump"])) for b, r in enumerate(ref))
    print("\nwidth %d B %d batched route, contract mode, frames %s: scores %.3g of max(1, |s|) (fp32 ref %.3g, bound %.3g)  log-probs %.3g "
          "(fp32 ref %.3g, bound %.3g)  selections decided %s  jump frames: %d of %d rows undecided, %d equal the oracle DTW's on the float64 matrix"
          % (d, B, frames, got_s, yard_s, bound_s, got_lp, yard_lp, bound_lp, [r["selection_decided"] for r in ref], undecided, B * N, agree))
    assert undecided * 50 <= B * N      # a condition on the inputs (the reference alone): at most 2 % of the rows are left out
    assert got_s <= bound_s and got_lp <= bound_lp
    for b, r in enumerate(ref):
        if r["selection_decided"]:
            assert sorted(int(h) for h in sel[b][:fr.TOPK]) == r["heads"], (b, "selected heads")
        assert not np.asarray(jump[b][N:]).any(), (b, "jump row past the DTW rows")
    assert not wrong, ("(utterance, row, engine's frame, oracle's frame)", wrong)
    assert not lp[:, n_text:].any() and jump.shape == (B, n)


@pytest.mark.parametrize("d,mode,B", CASES, ids=["%d-%s-B%d" % c for c in CASES])
def test_forward_against_float64(world, d, mode, B):
    w = world(d)
    m = w["model"]
    if mode == "batched":
        return _batched_route(w)
    m.set_precision("reference" if mode == "contract" else "f16")
    m.set_fuse_ln(mode == "f16_fused")
    try:
        if mode != "contract" and w["obs16"] is None:
            w["obs16"] = fr.observables(fr.ForwardRef(w["sd"], w["dims"], f16_operands=True, device="cuda").forward(w["mel"], w["tokens"]))
        failures = []
        for n in fr.TOKEN_COUNTS:
            ref = _cut(w["ref"], B, n)
            got = fr.distance(_observe(w, B, n), ref)
            plans = fr.site_plans(_LIB, d, B, n, mode == "contract")
            print("\nwidth %d B %d n %d %s: %s" % (d, B, n, mode, fr.format_plans(plans)))
            if mode == "contract":
                yard = fr.distance(_cut(w["obs32"], 2, n), _cut(w["ref"], 2, n))
                bound = fr.contract_bounds(yard)
                print("   engine    %s\n   fp32 ref  %s\n   bound     %s" % (_fmt(got), _fmt(yard), "  ".join("%s %.3g" % kv for kv in bound.items())))
                failures += [(n, k, got[k][0], bound[k]) for k in bound if not got[k][0] <= bound[k]]
            else:
                yard = fr.distance(_cut(w["obs16"], B, n), ref)
                bound = fr.f16_bounds(yard)
                print("   engine    %s\n   f16 ref   %s\n   ratio     %s" % (_fmt(got), _fmt(yard), "  ".join(
                    "%s %.2f (mean %.2f)" % (k, got[k][0] / yard[k][0], got[k][1] / yard[k][1]) for k in bound)))
                failures += [(n, k, got[k], bound[k]) for k in bound if not (got[k][0] <= bound[k][0] and got[k][1] <= bound[k][1])]
        assert not failures, failures
    finally:
        m.set_fuse_ln(False)


@pytest.mark.parametrize("B", [3, 4])
def test_inexact_checkpoint_in_the_contract_mode(world, B):
    """The 768-wide model with fp32 weights that f16 does not hold, on both sides of its QKV switch (B = 4): every pair product gets the
    A_hi W_lo^T term -- an accumulating launch for the residual products, an fp32 addend before the activation for the others, which takes
    the K-doubled call on the two-barrier kernel instead of the pair kernel. Against the float64 forward on the fp32 weights."""
    w = world(768, inexact=True)
    m = w["model"]
    assert m.weights_inexact[0] > 0
    m.set_precision("reference")
    failures = []
    for n in fr.TOKEN_COUNTS:
        got = fr.distance(_observe(w, B, n), _cut(w["ref"], B, n))
        yard = fr.distance(_cut(w["obs32"], 2, n), _cut(w["ref"], 2, n))
        bound = fr.contract_bounds(yard)
        print("\nwidth 768 inexact B %d n %d contract: %s" % (B, n, fr.format_plans(fr.site_plans(_LIB, 768, B, n, True, inexact=True))))
        print("   engine    %s\n   fp32 ref  %s\n   bound     %s" % (_fmt(got), _fmt(yard), "  ".join("%s %.3g" % kv for kv in bound.items())))
        failures += [(n, k, got[k][0], bound[k]) for k in bound if not got[k][0] <= bound[k]]
    assert not failures, failures
