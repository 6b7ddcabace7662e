"""Teacher-token log-probabilities on the MI355X (`-m gpu`): openai-whisper's word `probability` (timing.py:146-150 and 181-184 of
the reference: softmax of logits[len(sot_sequence):, :eot] at the teacher token, averaged per word), computed in the batched pipeline
(wca_align_desc.vocab_end / wca_align_result.token_logprob_host) and by wca_token_logprobs on given logits:
  * the log-sum-exp kernel against float64 log_softmax;
  * the batched path against the fp32 CPU oracle (contract mode) and against the same engine's materialised logits (both modes);
  * with log-probs on, the alignment (jump frames, selected heads) is bit-identical to the path without them;
  * two batches in flight, one with and one without; the error paths; the CLI's --word_confidence records."""
import ctypes as C
import glob
import importlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _m(n):
    return importlib.import_module("whisper-char-alignment_amd." + n)


def _vp(t):
    return C.c_void_p(t.data_ptr())


def _utt(tok, uid, n_samples, n_chars):
    syn, rt = _m("synthetic"), _m("retokenize")
    pcm = syn.synth_audio(uid, n_samples)
    tt = rt.encode(syn.synth_text(uid, n_chars), tok, "char")
    return pcm, tt, [*tok.sot_sequence, tok.no_timestamps, *tt, tok.eot]


def _batch(utts):
    """[(pcm, tt, tokens)] -> (pcm [B, smax] cuda, n_samples, tokens [B, n_max] cuda (eot padded), n_tok, max_frames)"""
    eot = utts[0][2][-1]
    n_max, smax = max(len(u[2]) for u in utts), max(len(u[0]) for u in utts)
    pb = np.zeros((len(utts), smax), dtype=np.float32)
    tarr = np.full((len(utts), n_max), eot, dtype=np.int64)
    for i, (p, _tt, toks) in enumerate(utts):
        pb[i, :len(p)] = p
        tarr[i, :len(toks)] = toks
    return (torch.from_numpy(pb).cuda(), [len(u[0]) for u in utts], torch.from_numpy(tarr).cuda(), [len(u[2]) for u in utts],
            [len(u[0]) // 320 for u in utts])


def _logp64(logits, tokens, sot_len, eot):
    """timing.py:146-149 in float64 log space: logits (n, V) of one utterance -> n_text values."""
    n_text = len(tokens) - sot_len - 2
    lg = torch.as_tensor(logits).double()[sot_len:sot_len + n_text, :eot]
    tg = torch.as_tensor(tokens[sot_len + 1:sot_len + 1 + n_text], dtype=torch.int64)
    return torch.log_softmax(lg, dim=-1).gather(1, tg[:, None])[:, 0].numpy()


def _oracle_logp(ref, pcm, tokens, sot_len, eot):
    from oracle import whisper_ref
    mel = whisper_ref.log_mel_spectrogram(whisper_ref.pad_or_trim(torch.from_numpy(pcm)), _m("audio").mel_filters(ref.dims.n_mels))
    logits, _ = ref.forward(mel[None], torch.tensor(tokens)[None])
    return _logp64(logits[0], tokens, sot_len, eot)


SMALL_SPECS = [(31, 48000, 25), (32, 80000, 40), (33, 32000, 12)]


@pytest.fixture(scope="module")
def small(wca):
    """The 256-wide 3 + 3-layer model of test_split_gpu.py, ragged batch of 3, contract mode."""
    from oracle import whisper_ref
    dims = wca.ModelDimensions(80, 1500, 256, 4, 3, 51865, 448, 256, 4, 3)
    sd = _m("synthetic").random_state_dict(dims, seed=5, cross_qk_std=0.08)
    model = wca.WhisperAMD(dims, device="cuda:0", max_batch=3, precision="reference").load_state_dict(sd)
    tok = _m("tokenizer").get_tokenizer(True, language="English")
    utts = [_utt(tok, u, n, c) for u, n, c in SMALL_SPECS]
    opts = model.make_opts(aggregation="topk", topk=4, sot_len=len(tok.sot_sequence), medfilt_width=3)
    yield dict(model=model, ref=whisper_ref.WhisperRef(sd, dims), tok=tok, utts=utts, batch=_batch(utts), opts=opts)
    model.set_precision("reference")


# ------------------------------------------------------------------------------- 1. the kernel alone
def test_token_logprob_kernel_vs_float64(small, lib, wca):
    model = small["model"]
    model._bind_stream()
    g = torch.Generator().manual_seed(3)
    V = 50257
    for ld, scale in ((V, 80.0), (50304, 80.0), (50261, 5.0), (V + 1, 0.01)):
        rows = 6
        x = (torch.rand(rows, ld, generator=g, dtype=torch.float64) * 2 - 1) * scale
        x[3, :V] = torch.randn(V, generator=g, dtype=torch.float64) * 3       # a peaked row
        x[3, 777] = 60.0
        x = x.float()
        lg = x.cuda()
        am = int(x[2, :V].argmax())
        tg = torch.tensor([0, V - 1, am, 777, 12345, V // 2], dtype=torch.int64)
        out = torch.full((rows,), float("nan"), device="cuda")
        wca._lib.check(lib.wca_token_logprobs(model._h, _vp(lg), rows, ld, V, _vp(tg.cuda()), _vp(out)))
        ref = torch.log_softmax(x[:, :V].double(), dim=-1).gather(1, tg[:, None])[:, 0]
        err = (out.cpu().double() - ref).abs().max().item()
        assert err < 1e-5, (ld, scale, err)
        # a row that does not start on a 16-byte boundary (the scalar head of the float4 loop)
        out1 = torch.full((1,), float("nan"), device="cuda")
        wca._lib.check(lib.wca_token_logprobs(model._h, _vp(lg.view(-1)[1:]), 1, ld, V - 1, _vp(tg[:1].cuda()), _vp(out1)))
        ref1 = torch.log_softmax(x.view(-1)[1:V].double(), dim=0)[0].item()
        assert abs(out1.item() - ref1) < 1e-5
    # a row of length 1: log p = 0
    one = torch.tensor([[37.5, 99.0]], device="cuda")
    out = torch.full((1,), float("nan"), device="cuda")
    wca._lib.check(lib.wca_token_logprobs(model._h, _vp(one), 1, 2, 1, _vp(torch.zeros(1, dtype=torch.int64, device="cuda")), _vp(out)))
    assert out.item() == 0.0
    # a target >= vocab_end has no value: NaN and WCA_ERR_INVALID; argument errors are errors
    tbad = torch.tensor([5, 2], dtype=torch.int64, device="cuda")
    two = torch.zeros(2, 8, device="cuda")
    out2 = torch.zeros(2, device="cuda")
    assert lib.wca_token_logprobs(model._h, _vp(two), 2, 8, 4, _vp(tbad), _vp(out2)) == -1
    assert b"vocab_end" in lib.wca_last_error()
    assert torch.isnan(out2[0]).item() and out2[1].item() == pytest.approx(-np.log(4.0), abs=1e-6)
    assert lib.wca_token_logprobs(model._h, _vp(two), 2, 8, 0, _vp(tbad), _vp(out2)) == -1
    assert lib.wca_token_logprobs(model._h, _vp(two), 2, 8, 51866, _vp(tbad), _vp(out2)) == -1
    assert lib.wca_token_logprobs(model._h, _vp(two), 2, 3, 4, _vp(tbad), _vp(out2)) == -1
    assert lib.wca_token_logprobs(model._h, None, 2, 8, 4, _vp(tbad), _vp(out2)) == -1
    assert lib.wca_token_logprobs(None, _vp(two), 2, 8, 4, _vp(tbad), _vp(out2)) == -1


# ------------------------------------------------------------------------------- 2. contract mode vs the fp32 oracle
def test_batched_logprobs_vs_oracle_small_dims(small):
    model, tok, utts = small["model"], small["tok"], small["utts"]
    model.set_precision("reference")
    sot = len(tok.sot_sequence)
    jump, sel, lp = model.align_batch(*small["batch"], small["opts"], token_logprobs_vocab_end=tok.eot)
    assert lp.shape == jump.shape and lp.dtype == np.float32
    worst = 0.0
    for i, (pcm, tt, toks) in enumerate(utts):
        ref = _oracle_logp(small["ref"], pcm, toks, sot, tok.eot)
        assert len(ref) == len(tt)
        err = np.abs(lp[i, :len(tt)].astype(np.float64) - ref).max()
        worst = max(worst, err)
        assert err < 5e-5, (i, err)
        assert np.all(lp[i, len(tt):] == 0)
    print("contract-mode token log-probs vs fp32 oracle: max |d logp| = %.2e" % worst)


# ------------------------------------------------------------------------------- 3. both modes vs the engine's own logits
@pytest.mark.parametrize("mode", ["f16", "reference"])
def test_batched_logprobs_vs_materialised_logits(small, mode):
    model, tok, utts = small["model"], small["tok"], small["utts"]
    tm = _m("timing")
    model.set_precision(mode)
    pcm, ns, tarr, n_tok, frames = small["batch"]
    sot = len(tok.sot_sequence)
    _j, _s, lp = model.align_batch(pcm, ns, tarr, n_tok, frames, small["opts"], token_logprobs_vocab_end=tok.eot)
    mel = model.log_mel(pcm, ns)
    _w, logits = model.get_attentions(mel, tarr, frames, medfilt_width=3, n_tok=n_tok, want_logits=True)
    for i, (_p, tt, toks) in enumerate(utts):
        ref = _logp64(logits[i].cpu(), toks, sot, tok.eot)
        assert np.abs(lp[i, :len(tt)] - ref).max() < 1e-4, (mode, i)
        # the single-utterance entry (wca_token_logprobs) on the same logits
        one = tm.token_logprobs(logits[i, :n_tok[i]], toks, tok).cpu().numpy()
        assert one.shape == (len(tt),) and np.abs(one - ref).max() < 1e-5, (mode, i)
        wp = tm.word_probabilities(lp[i], tt, tok, "char")
        _words, st, en = tm.words_from_jump_frames(_j[i], tt, tok, "char")
        assert len(wp) == len(en) and all(0.0 < p <= 1.0 for p in wp)


# ------------------------------------------------------------------------------- 4. the alignment is untouched
@pytest.mark.parametrize("mode", ["f16", "reference"])
def test_logprobs_leave_the_alignment_alone(small, mode):
    model, tok = small["model"], small["tok"]
    model.set_precision(mode)
    pcm, ns, tarr, n_tok, frames = small["batch"]
    opts = small["opts"]
    j0, s0 = model.align_batch(pcm, ns, tarr, n_tok, frames, opts)
    j1, s1, lp1 = model.align_batch(pcm, ns, tarr, n_tok, frames, opts, token_logprobs_vocab_end=tok.eot)
    assert np.array_equal(j0, j1) and np.array_equal(s0, s1)
    # pcm_dev = NULL: the encoder state of encode_batch
    model.encode_batch(pcm=pcm, n_samples=ns)
    j2, s2 = model.align_batch(None, None, tarr, n_tok, frames, opts)
    model.encode_batch(pcm=pcm, n_samples=ns)
    j3, s3, lp3 = model.align_batch(None, None, tarr, n_tok, frames, opts, token_logprobs_vocab_end=tok.eot)
    assert np.array_equal(j2, j3) and np.array_equal(s2, s3)
    np.testing.assert_allclose(lp3, lp1, rtol=0, atol=1e-6)


# ------------------------------------------------------------------------------- 5. two batches in flight, error paths
def test_two_batches_in_flight_and_errors(small, wca):
    model, tok, utts = small["model"], small["tok"], small["utts"]
    model.set_precision("reference")
    opts = small["opts"]
    a = small["batch"]
    b = _batch(utts[1:])
    ja, sa, lpa = model.align_batch(*a, opts, token_logprobs_vocab_end=tok.eot)
    jb, sb = model.align_batch(*b, opts)
    model.align_batch(*a, opts, enqueue_only=True, token_logprobs_vocab_end=tok.eot)
    model.align_batch(*b, opts, enqueue_only=True)
    ja2, sa2, lpa2 = model.fetch(3, a[2].shape[1], opts, with_token_logprobs=True)
    assert np.array_equal(ja2, ja) and np.array_equal(sa2, sa) and np.array_equal(lpa2, lpa)
    with pytest.raises(wca._lib.WcaError) as ei:
        model.fetch(2, b[2].shape[1], opts, with_token_logprobs=True)
    assert ei.value.code == -4
    jb2, sb2 = model.fetch(2, b[2].shape[1], opts)   # nothing was consumed by the refused fetch
    assert np.array_equal(jb2, jb) and np.array_equal(sb2, sb)
    # vocab_end outside (0, n_vocab]
    for bad in (-1, model.dims.n_vocab + 1):
        with pytest.raises(wca._lib.WcaError) as ei:
            model.align_batch(*a, opts, token_logprobs_vocab_end=bad)
        assert ei.value.code == -1
    # a teacher token >= vocab_end: the batch's error flag -> WCA_ERR_INVALID at the fetch (the letters are ids >= 64)
    with pytest.raises(wca._lib.WcaError) as ei:
        model.align_batch(*a, opts, token_logprobs_vocab_end=40)
    assert ei.value.code == -1 and "vocab_end" in str(ei.value)
    j4, s4 = model.align_batch(*a, opts)   # the engine is fine afterwards
    assert np.array_equal(j4, ja)


# ------------------------------------------------------------------------------- 6. medium dimensions
def test_medium_dims_contract_mode_vs_oracle(wca):
    """B = 8 ragged (the tile GEMMs) and B = 1 beside it (a different GEMM route) against the fp32 oracle on two utterances."""
    from oracle import whisper_ref
    dims = wca.dims_for("medium")
    sd = _m("synthetic").random_state_dict(dims, seed=0, cross_qk_std=0.08)
    model = wca.WhisperAMD(dims, device="cuda:0", max_batch=8, precision="reference").load_state_dict(sd)
    tok = _m("tokenizer").get_tokenizer(True, language="English")
    utts = [_utt(tok, 200 + u, 160000 - 12000 * u, 64 - 5 * u) for u in range(8)]
    opts = model.make_opts(aggregation="topk", topk=10, sot_len=3, medfilt_width=3)
    _j, _s, lp8 = model.align_batch(*_batch(utts), opts, token_logprobs_vocab_end=tok.eot)
    _j, _s, lp1 = model.align_batch(*_batch(utts[5:6]), opts, token_logprobs_vocab_end=tok.eot)
    del model
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    ref = whisper_ref.WhisperRef(sd, dims)
    worst = 0.0
    for i, got in ((0, lp8[0]), (5, lp8[5]), (5, lp1[0])):
        pcm, tt, toks = utts[i]
        r = _oracle_logp(ref, pcm, toks, 3, tok.eot)
        err = np.abs(got[:len(tt)].astype(np.float64) - r).max()
        worst = max(worst, err)
        assert err < 5e-5, (i, err)
    print("medium dims, contract mode: max |d logp| vs oracle = %.2e" % worst)


# ------------------------------------------------------------------------------- 7. the CLI
def test_cli_word_confidence(tmp_path, wca):
    root = tmp_path
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    pcm = np.load(os.path.join(gold, "sample_pcm_int16.npy"))
    words = "the quick brown fox jumps over the lazy dog".split()
    lines = []
    for u in range(3):
        x = np.roll(pcm, 1000 * u)[: len(pcm) - 2000 * u]
        head = ("NIST_1A\n   1024\nsample_count -i %d\nsample_rate -i 16000\nchannel_count -i 1\nsample_n_bytes -i 2\n"
                "sample_byte_format -s2 01\nsample_coding -s3 pcm\nend_head\n" % len(x)).encode()
        wav = root / ("utt%d.wav" % u)
        wav.write_bytes(head + b" " * (1024 - len(head)) + x.astype("<i2").tobytes())
        w = words[: 9 - 2 * u]
        step = len(x) // (len(w) + 1)
        (root / ("utt%d.wrd" % u)).write_text("".join("%d %d %s\n" % (i * step, (i + 1) * step, t) for i, t in enumerate(w)))
        lines.append("utt%d %s\n" % (u, wav))
    scp = root / "test.scp"
    scp.write_text("".join(lines))
    infer, syn, tm = _m("infer_ali"), _m("synthetic"), _m("timing")
    dims = wca.dims_for("tiny")
    model = wca.WhisperAMD(dims, device="cuda:0", max_batch=1).load_state_dict(syn.random_state_dict(dims, seed=0))
    model.use_official_alignment_heads("tiny")
    argv = ["--model", "tiny", "--random_init", "--dataset", "TIMIT", "--scp", str(scp), "--aggr", "topk", "--topk", "5",
            "--aligned_unit_type", "char", "--medfilt_width", "3", "--batch_size", "1", "--save_prediction", "--teacher", "text"]
    import joblib
    recs = {}
    for flag in (False, True):
        out = root / ("out%d" % flag)
        infer.infer_dataset(infer.parse_args(argv + ["--output_dir", str(out)] + (["--word_confidence"] if flag else [])), model=model)
        res = json.load(open(glob.glob(str(out / "*.json"))[0]))
        recs[flag] = joblib.load(glob.glob(str(out / "*-predictions.pkl"))[0])
        assert ("mean_word_prob" in res) == flag and ("word_confidence" in res) == flag
    base = {"starts", "ends", "texts", "starts_hat", "ends_hat", "predwords", "fids"}
    tok = _m("tokenizer").get_tokenizer(True, language="English")
    opts = model.make_opts(aggregation="topk", topk=5, sot_len=3, medfilt_width=3)
    ds = infer.DATASET["TIMIT"](str(scp), n_mels=80, device="cuda:0", model=model, compute_mel=False)
    all_probs = []
    for n, p in recs[True].items():
        assert set(recs[False][n]) == base and set(p) == base | {"word_probs_hat", "text_logprob"}
        assert np.array_equal(p["ends_hat"], recs[False][n]["ends_hat"])
        assert len(p["word_probs_hat"]) == len(p["ends_hat"]) > 0
        assert all(0.0 < v <= 1.0 for v in p["word_probs_hat"])
        all_probs += list(p["word_probs_hat"])
        # the engine's log-probs of this utterance, batch 1 as in the run
        x, duration, _texts, _s, _e, _f = ds.read(n)
        tt = _m("retokenize").encode(" ".join(p["texts"]), tok, "char")
        toks = [*tok.sot_sequence, tok.no_timestamps, *tt, tok.eot]
        xb = torch.from_numpy(np.asarray(x, dtype=np.float32)[None]).cuda()
        _j, _s2, lp = model.align_batch(xb, [xb.shape[1]], torch.tensor([toks]).cuda(), [len(toks)], [duration // 320], opts,
                                        token_logprobs_vocab_end=tok.eot)
        assert p["text_logprob"] == pytest.approx(float(np.sum(lp[0, :len(tt)], dtype=np.float64)), abs=1e-4)
        np.testing.assert_allclose(p["word_probs_hat"], tm.word_probabilities(lp[0], tt, tok, "char"), rtol=1e-5)
    assert res["mean_word_prob"] == pytest.approx(float(np.mean(all_probs)), rel=1e-9)
