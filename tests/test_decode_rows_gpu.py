"""Greedy decode with per-row prompts on the MI355X (wca_decode with per_row 1): the rows of one batch sit at different decoder
positions. The per-row kernel forms against the uniform kernels they were derived from (bit for bit), the whole loop against
wca_decode (equal lengths: bit for bit; ragged: every row against the same utterance decoded alone), per-row sample
budgets and the refusals. Small dims, like the `small` fixture of test_decode_gpu.py."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _m(n):
    return importlib.import_module("whisper-char-alignment_amd." + n)


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("whisper-char-alignment_amd")


@pytest.fixture(scope="module")
def tok():
    return _m("tokenizer").get_tokenizer(True, language="en", task="transcribe")


@pytest.fixture(scope="module")
def small(pkg):
    dims = pkg.ModelDimensions(80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)
    m = pkg.WhisperAMD(dims, device="cuda:0", max_batch=4, precision="f16")
    m.load_state_dict(_m("synthetic").random_state_dict(dims, seed=5))
    return m, dims


def _mels(m, seeds, n_samples=48000):
    syn, audio = _m("synthetic"), _m("audio")
    return torch.stack([audio.log_mel_spectrogram(audio.pad_or_trim(torch.from_numpy(syn.synth_audio(s, n_samples=n_samples))), 80, model=m)
                        for s in seeds]).cuda()


@pytest.fixture(scope="module")
def mel4(small):
    return _mels(small[0], [3, 4, 8, 9])


def _masks(tok, dims):
    decoding = _m("decoding")
    return decoding.filter_masks(tok, decoding.DecodingOptions(language="en"), dims.n_vocab)


def _initial(tok, n):
    """n initial tokens: the bare sot sequence (n = 3, <|sot|> at 0) or [sot_prev, n - 4 prompt tokens, *sot_sequence] (<|sot|> at n - 3)."""
    sot = list(tok.sot_sequence)
    if n == len(sot):
        return sot, 0
    prompt = [(37 * i) % 5000 + 200 for i in range(n - len(sot) - 1)]
    return [tok.sot_prev] + prompt + sot, 1 + len(prompt)


def _rows(m, tok, dims, mel, lengths, sample_len, batch=None):
    sup, blank = _masks(tok, dims)
    plans = [_initial(tok, n) for n in lengths]
    sl = list(sample_len) if isinstance(sample_len, (list, tuple)) else [sample_len] * len(lengths)
    out = m.greedy_decode_rows(mel, None, None, [p[0] for p in plans], [p[1] for p in plans], sl, sup, blank, eot=tok.eot,
                               timestamp_begin=tok.timestamp_begin, apply_timestamp_rules=True, max_initial_timestamp_index=50, batch=batch,
                               no_speech=tok.no_speech)
    return out + (m.last_no_speech_prob.copy(),)


def _alone(m, tok, dims, mel, n, sample_len):
    sup, blank = _masks(tok, dims)
    initial, sot_index = _initial(tok, n)
    out = m.greedy_decode(mel, None, None, initial, sup, blank, sample_len=sample_len, eot=tok.eot, timestamp_begin=tok.timestamp_begin,
                          apply_timestamp_rules=True, max_initial_timestamp_index=50, no_speech=tok.no_speech, sot_index=sot_index, prefill=1)
    return out + (m.last_no_speech_prob.copy(),)


def _same_or_near_tie(m, mel_b, n_init, row_a, n_a, row_b, n_b, what):
    """The rule of test_decode_modes_agree: True when the two token rows are identical; a differing pair is excused ONLY by a
    teacher-forced logit gap below 1e-3 between the two choices at the first divergent position (then False is returned)."""
    width = min(len(row_a), len(row_b))
    if np.array_equal(row_a[:width], row_b[:width]) and n_a == n_b:
        return True
    p_ = int(np.nonzero(row_a[:width] != row_b[:width])[0][0])
    assert p_ >= n_init, (what, p_)   # the initial tokens are given
    _w, logits = m.get_attentions(mel_b, torch.from_numpy(row_a[:p_].astype(np.int64))[None].cuda(), [100], 3, 1.0)
    row = logits[0, p_ - 1].float().cpu().numpy()
    gap = abs(float(row[row_a[p_]]) - float(row[row_b[p_]]))
    print("%s: rows diverge at position %d: tokens %d / %d, teacher-forced logit gap %.3e" % (what, p_, row_a[p_], row_b[p_], gap))
    assert gap < 1e-3, (what, p_, gap)
    return False


def test_select_rows_kernel_matches_single_row_calls(small, tok):
    """Six rows in six different cases at once, with different n_initial and cur_len: tokens and sum_logprob bit-identical to six
    single-row calls of the uniform kernel on the same logits. The row at its sample cap is a finished row by definition, so its
    single-row twin is the same row with <|eot|> as its last token (the uniform kernel's finished-row case)."""
    m, dims = small
    _lib = _m("_lib")
    sup, blank = _masks(tok, dims)
    V, T_max = dims.n_vocab, 40
    tsb, eot = tok.timestamp_begin, tok.eot
    sot = list(tok.sot_sequence)
    prm = [tok.sot_prev, 400, 401]
    rows = [(sot, []),                                             # first sampled position
            (prm + sot, [tsb + 3, 400, 500]),                      # text
            (sot, [tsb + 3, 400, 500, tsb + 10]),                  # after a single timestamp
            (prm[:2] + sot, [tsb + 3, 400, tsb + 10, tsb + 10]),   # after a timestamp pair
            (sot, [tsb + 3, 400, eot]),                            # finished row
            (prm + sot, [tsb + 3, 400, 500])]                      # at its sample cap
    caps = [100, 100, 100, 100, 100, 3]
    B = len(rows)
    n_init = [len(i) for i, _ in rows]
    cur_len = [len(i) + len(h) for i, h in rows]
    assert len(set(n_init)) > 1 and len(set(cur_len)) > 1
    logits = (torch.randn(B, V, generator=torch.Generator().manual_seed(7)) * 3.0).cuda()
    logits[0, 300] = 50.0   # text at a first position: must not be chosen
    tokens = torch.full((B, T_max), eot, dtype=torch.int32)
    for b, (i, h) in enumerate(rows):
        tokens[b, :cur_len[b]] = torch.tensor(i + h, dtype=torch.int32)
    supd, blankd = torch.from_numpy(sup).cuda(), torch.from_numpy(blank).cuda()
    lp0 = torch.tensor([-1.5 * b for b in range(B)])
    o = _lib.DecodeOpts(224, eot, tsb, 1, 50)
    m._bind_stream()
    # ---- six single-row calls of the uniform kernel
    want_tok, want_lp = [], []
    for b in range(B):
        td = tokens[b:b + 1].clone()
        if b == 5:
            td[0, cur_len[b] - 1] = eot
        td = td.cuda()
        lpd = lp0[b:b + 1].clone().cuda()
        nd = torch.zeros(T_max, dtype=torch.int32, device="cuda")
        _lib.check(m._lib.wca_test_decode_select(m._h, _vp(logits[b:b + 1]), 1, V, _vp(td), T_max, cur_len[b], n_init[b], _vp(supd), _vp(blankd),
                                                 C.byref(o), _vp(lpd), _vp(nd)))
        torch.cuda.synchronize()
        want_tok.append(int(td.cpu()[0, cur_len[b]]))
        want_lp.append(lpd.cpu()[0].item())
    # ---- one per-row call
    td, lpd = tokens.clone().cuda(), lp0.clone().cuda()
    nd = torch.zeros(8, dtype=torch.int32, device="cuda")
    dev = [torch.tensor(v, dtype=torch.int32).cuda() for v in (cur_len, n_init, caps)]
    _lib.check(m._lib.wca_test_decode_select_rows(m._h, _vp(logits), B, V, _vp(td), T_max, _vp(dev[0]), _vp(dev[1]), _vp(dev[2]), 5, 8, _vp(supd),
                                                  _vp(blankd), C.byref(o), _vp(lpd), _vp(nd)))
    torch.cuda.synchronize()
    got = td.cpu()
    got_tok = [int(got[b, cur_len[b]]) for b in range(B)]
    assert got_tok == want_tok, (got_tok, want_tok)
    assert np.array_equal(lpd.cpu().numpy().view(np.int32), np.array(want_lp, np.float32).view(np.int32))
    assert tsb <= got_tok[0] <= tsb + 50 and got_tok[4] == eot and got_tok[5] == eot
    assert lpd.cpu()[4].item() == lp0[4].item() and lpd.cpu()[5].item() == lp0[5].item()
    assert nd.cpu().tolist() == [0, 0, 0, 0, 0, sum(t == eot for t in got_tok), 0, 0]
    for b in range(B):   # nothing but the new token was written
        assert torch.equal(got[b, :cur_len[b]], tokens[b, :cur_len[b]]) and (got[b, cur_len[b] + 1:] == eot).all()


def test_attention_rows_matches_single_row_calls(small):
    m, dims = small
    _lib = _m("_lib")
    H, d = 4, 256
    nk_rows = [1, 2, 63, 64, 65, 230]
    B, nk = len(nk_rows), max(nk_rows)
    g = torch.Generator().manual_seed(11)
    q = torch.randn(B, 1, d, generator=g).half().cuda()
    k = torch.randn(B, nk, d, generator=g).half().cuda()
    v = torch.randn(B, nk, d, generator=g).half().cuda()
    o = torch.zeros(B, 1, d, dtype=torch.float16, device="cuda")
    nkd = torch.tensor(nk_rows, dtype=torch.int32).cuda()
    m._bind_stream()
    _lib.check(m._lib.wca_test_attention_rows(m._h, _vp(q), _vp(k), _vp(v), _vp(o), B, H, 1, nk, _vp(nkd), 0))
    torch.cuda.synchronize()
    for b, n in enumerate(nk_rows):
        kb, vb = k[b, :n].contiguous(), v[b, :n].contiguous()
        ob = torch.zeros(1, 1, d, dtype=torch.float16, device="cuda")
        _lib.check(m._lib.wca_test_attention(m._h, _vp(q[b:b + 1].contiguous()), _vp(kb), _vp(vb), _vp(ob), None, 0, 0, 1, H, 1, n, 0))
        torch.cuda.synchronize()
        assert torch.equal(o[b].view(torch.int16), ob[0].view(torch.int16)), (b, n)
        ref = torch.softmax((q[b, 0].float().view(H, 1, 64) @ kb.float().view(n, H, 64).permute(1, 2, 0)) * 0.125, -1) @ vb.float().view(n, H, 64).permute(1, 0, 2)
        assert (o[b, 0].float() - ref.reshape(d)).abs().max().item() < 5e-3
    # per-row key counts exist for the one-query kernel only
    q2 = torch.randn(B, 2, d, generator=g).half().cuda()
    o2 = torch.zeros(B, 2, d, dtype=torch.float16, device="cuda")
    with pytest.raises(_lib.WcaError):
        _lib.check(m._lib.wca_test_attention_rows(m._h, _vp(q2), _vp(k), _vp(v), _vp(o2), B, H, 2, nk, _vp(nkd), 0))
    with pytest.raises(_lib.WcaError):
        _lib.check(m._lib.wca_test_attention_rows(m._h, _vp(q), _vp(k), _vp(v), _vp(o), B, H, 1, nk, _vp(nkd), 1))


def _equal_lengths(m, tok, dims, mel4):
    n = 1 + 20 + 3
    rows = _rows(m, tok, dims, mel4, [n] * 4, 8)
    pos = m.last_decode_positions()
    sup, blank = _masks(tok, dims)
    initial, sot_index = _initial(tok, n)
    ex = m.greedy_decode(mel4, None, None, initial, sup, blank, sample_len=8, eot=tok.eot, timestamp_begin=tok.timestamp_begin,
                         apply_timestamp_rules=True, max_initial_timestamp_index=50, no_speech=tok.no_speech, sot_index=sot_index, prefill=1)
    ex = ex + (m.last_no_speech_prob.copy(),)
    assert rows[0].shape == ex[0].shape == (4, n + 8)
    for a, b in zip(rows, ex):
        assert np.array_equal(a, b), (a, b)
    assert np.isfinite(rows[2]).all() and np.isfinite(rows[3]).all()
    assert pos == m.last_decode_positions() and pos[0] == n


def test_equal_lengths_give_the_uniform_result(small, tok, mel4):
    """Four rows that share one prompt of 20 tokens: bit for bit what greedy_decode(prefill=1) gives for the batch."""
    m, dims = small
    _equal_lengths(m, tok, dims, mel4)


def test_equal_lengths_give_the_uniform_result_unfused(small, tok, mel4):
    """The same with set_decode_mode(False, 1): the LayerNorm, the tile GEMM and the K/V append are separate launches, and the
    per-row loop appends through kv_append_rows where the uniform loop uses kv_append. Still bit for bit."""
    m, dims = small
    try:
        m.set_decode_mode(False, 1)
        _equal_lengths(m, tok, dims, mel4)
    finally:
        m.set_decode_mode(True, 1)


@pytest.mark.parametrize("lengths", [(3, 5, 9, 17), (3, 4, 37, 226)], ids=["few-row-prefill", "large-gemm-prefill"])
def test_ragged_rows_against_each_row_alone(small, tok, mel4, lengths):
    """Rows with different numbers of initial tokens in one batch against the same utterance decoded alone through
    greedy_decode(prefill=1). The GEMM path (and the fp32 summation order) depends on the row count, so: no_speech_prob
    at rtol 1e-4, identical rows' sum_logprob at rtol = atol = 1e-4, a differing row excused only by a teacher-forced logit gap
    below 1e-3 at its first divergent position, at least three of the four rows identical."""
    m, dims = small
    _ragged(m, dims, tok, mel4, lengths)


def test_ragged_rows_on_a_contract_mode_engine(pkg, tok):
    """The same on an engine in the reference-precision mode, the CLI's default: the encoder and the cross-K/V run on (hi, lo) pairs and
    the decode reads the hi halves of rows that are twice as long."""
    dims = pkg.ModelDimensions(80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)
    m = pkg.WhisperAMD(dims, device="cuda:0", max_batch=4, precision="reference")
    m.load_state_dict(_m("synthetic").random_state_dict(dims, seed=5))
    _ragged(m, dims, tok, _mels(m, [3, 4, 8, 9]), (3, 5, 9, 17))


def _ragged(m, dims, tok, mel4, lengths):
    sample_len = 8
    toks, n_tok, lp, nsp = _rows(m, tok, dims, mel4, lengths, sample_len)
    assert m.last_decode_positions()[0] == max(lengths)
    assert toks.shape == (4, max(lengths) + sample_len)
    same = []
    for b, n in enumerate(lengths):
        t1, n1, lp1, nsp1 = _alone(m, tok, dims, mel4[b:b + 1], n, sample_len)
        assert (toks[b, :n] == t1[0, :n]).all() and n <= n_tok[b] <= n + sample_len
        assert (toks[b, n + sample_len:] == tok.eot).all()   # nothing beyond the row's own budget
        print("ragged %s row %d: no_speech %.6e / alone %.6e, sum_logprob %.6f / alone %.6f" % (lengths, b, nsp[b], nsp1[0], lp[b], lp1[0]))
        np.testing.assert_allclose(nsp[b], nsp1[0], rtol=1e-4)
        same.append(_same_or_near_tie(m, mel4[b:b + 1], n, toks[b, :n + sample_len], n_tok[b], t1[0], n1[0], "ragged %s row %d" % (lengths, b)))
        if same[-1]:
            np.testing.assert_allclose(lp[b], lp1[0], rtol=1e-4, atol=1e-4)
    assert sum(same) >= 3, same


def test_per_row_sample_caps(small, tok, mel4):
    m, dims = small
    lengths, caps = (9, 3), (2, 8)
    toks, n_tok, lp, nsp = _rows(m, tok, dims, mel4[:2], lengths, caps)
    assert toks.shape == (2, 11)
    assert n_tok[0] - lengths[0] <= 2 and (toks[0, lengths[0] + 2:] == tok.eot).all()
    t1, n1, lp1, _ = _alone(m, tok, dims, mel4[:1], lengths[0], 2)
    print("caps: row 0 sum_logprob %.6f, alone with sample_len 2 %.6f" % (lp[0], lp1[0]))
    if _same_or_near_tie(m, mel4[:1], lengths[0], toks[0, :lengths[0] + 2], n_tok[0], t1[0], n1[0], "caps row 0"):
        np.testing.assert_allclose(lp[0], lp1[0], rtol=1e-4, atol=1e-4)
    t2, n2, lp2, _ = _alone(m, tok, dims, mel4[1:2], lengths[1], 8)
    if _same_or_near_tie(m, mel4[1:2], lengths[1], toks[1], n_tok[1], t2[0], n2[0], "caps row 1"):
        np.testing.assert_allclose(lp[1], lp2[0], rtol=1e-4, atol=1e-4)


def test_refusals_leave_the_engine_usable(small, tok, mel4):
    m, dims = small
    _lib = _m("_lib")
    sup, blank = _masks(tok, dims)
    sot = list(tok.sot_sequence)
    kw = dict(eot=tok.eot, timestamp_begin=tok.timestamp_begin, apply_timestamp_rules=True, max_initial_timestamp_index=50, no_speech=tok.no_speech)

    def call(initials, sot_index, sample_len, mel=mel4):
        return m.greedy_decode_rows(mel, None, None, initials, sot_index, sample_len, sup, blank, **kw)

    with pytest.raises(_lib.TooLongError):
        call([sot, [], sot, sot], [0] * 4, [8] * 4)                                     # n_initial = 0
    with pytest.raises(_lib.TooLongError):
        call([sot] * 4, [0] * 4, [8, dims.n_text_ctx + 2 - len(sot), 8, 8])             # n_initial + sample_len = n_text_ctx + 2
    with pytest.raises(_lib.WcaError):
        call([sot] * 4, [0, len(sot), 0, 0], [8] * 4)                                   # sot_index >= n_initial
    with pytest.raises(_lib.WcaError):
        call([sot, sot[:2] + [dims.n_vocab], sot, sot], [0] * 4, [8] * 4)               # a token outside the vocabulary
    with pytest.raises(_lib.WcaError):
        call([sot] * 5, [0] * 5, [8] * 5, mel=torch.cat([mel4, mel4[:1]]))              # batch > max_batch
    # the combinations of descriptor fields that no decode runs: WCA_ERR_INVALID, through the engine's one descriptor call
    opts = _lib.DecodeOpts(8, tok.eot, tok.timestamp_begin, 1, 50, tok.no_speech)
    temps, seeds = np.zeros(4, np.float32), np.arange(4, dtype=np.uint64)
    uniform = (_lib.i32_array(sot), [len(sot)], [0], [8], opts, sup, blank, 0)
    rows = (np.array([sot] * 4, np.int32), [len(sot)] * 4, [0] * 4, [8] * 4, opts, sup, blank, 1)
    for args in ((mel4, None, None, None) + uniform + (0, temps, seeds),               # per_row 0 with a temperature and a seed
                 (None, None, None, 4) + uniform + (0, None, None, True),              # per_row 0 with redecode
                 (mel4, None, None, None) + rows + (0,),                               # per_row 1 with prefill 0
                 (mel4, None, None, None) + rows + (1, temps, None),                   # a temperature without a seed
                 (mel4, None, None, None) + rows + (1, None, seeds),                   # a seed without a temperature
                 (mel4, None, None, None) + rows + (1, temps, seeds, True)):           # redecode together with an input
        with pytest.raises(_lib.WcaError) as err:
            m._decode(*args)
        assert err.value.code == -1, err.value                                          # WCA_ERR_INVALID
    _equal_lengths(m, tok, dims, mel4)
