"""CPU tests of prompt / prefix conditioning in decode (DecodingOptions(prompt=..., prefix=...), upstream
DecodingTask._get_initial_tokens, restated): the initial-token construction, the sample_len cap, sot_index, which engine
call decode() makes, and the C ABI mirror of wca_decode_opts and of the descriptor's prompt fields. The decode itself runs on the GPU
(tests/test_decode_prompt_gpu.py)."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CTX = 448


@pytest.fixture(scope="module")
def decoding():
    return importlib.import_module("whisper-char-alignment_amd.decoding")


@pytest.fixture(scope="module")
def tok():
    return importlib.import_module("whisper-char-alignment_amd.tokenizer").get_tokenizer(True, language="en", task="transcribe")


def _opts(decoding, **kw):
    return decoding.DecodingOptions(language="en", **kw)


def test_plain_start_is_unchanged(decoding, tok):
    sot = list(tok.sot_sequence)
    assert sot == [tok.sot, tok.special_tokens["<|en|>"], tok.transcribe]
    assert decoding.decode_plan(tok, _opts(decoding), N_CTX) == (sot, 224, 0)
    assert decoding.decode_plan(tok, _opts(decoding, without_timestamps=True), N_CTX) == (sot + [tok.no_timestamps], 224, 0)
    # empty prompt / prefix are falsy upstream: nothing is added
    assert decoding.decode_plan(tok, _opts(decoding, prompt=[], prefix=""), N_CTX) == (sot, 224, 0)


def test_list_prompt_and_prefix(decoding, tok):
    sot = list(tok.sot_sequence)
    prompt, prefix = [11, 22, 33, 44], [7, 8]
    assert decoding.initial_tokens(tok, _opts(decoding, prompt=prompt), N_CTX, 224) == [tok.sot_prev, 11, 22, 33, 44] + sot
    assert decoding.initial_tokens(tok, _opts(decoding, prefix=prefix), N_CTX, 224) == sot + [7, 8]
    both = decoding.initial_tokens(tok, _opts(decoding, prompt=prompt, prefix=prefix), N_CTX, 224)
    assert both == [tok.sot_prev, 11, 22, 33, 44] + sot + [7, 8]
    init, sample_len, sot_index = decoding.decode_plan(tok, _opts(decoding, prompt=prompt, prefix=prefix), N_CTX)
    assert init == both and sample_len == 224 and sot_index == 5 and init[sot_index] == tok.sot
    # without_timestamps: <|notimestamps|> sits between the sot sequence and the prefix
    nt = decoding.initial_tokens(tok, _opts(decoding, prompt=prompt, prefix=prefix, without_timestamps=True), N_CTX, 224)
    assert nt == [tok.sot_prev, 11, 22, 33, 44] + sot + [tok.no_timestamps, 7, 8]


def test_str_prompt_and_prefix_use_the_bpe_vocabulary(decoding, fake_vocab):
    tk = importlib.import_module("whisper-char-alignment_amd.tokenizer").get_tokenizer(True, language="en", task="transcribe",
                                                                                         vocab_path=fake_vocab)
    o = _opts(decoding, prompt="  Cholmondeley and Featherstonehaugh ", prefix="abcd efgh", vocab_path=fake_vocab)
    want_prompt = tk.encode(" Cholmondeley and Featherstonehaugh")   # " " + prompt.strip()
    want_prefix = tk.encode(" abcd efgh")
    assert len(want_prompt) > 3 and want_prompt != tk.encode("Cholmondeley and Featherstonehaugh")
    init = decoding.initial_tokens(tk, o, N_CTX, 224)
    assert init == [tk.sot_prev] + want_prompt + list(tk.sot_sequence) + want_prefix


def test_str_prompt_without_vocabulary_is_a_clear_error(decoding, tok):
    for kw in ({"prompt": "hello world"}, {"prefix": "hello"}):
        with pytest.raises(ValueError, match="vocab"):
            decoding.decode_plan(tok, _opts(decoding, **kw), N_CTX)


def test_prompt_keeps_its_last_223_tokens(decoding, tok):
    prompt = list(range(1000, 1300))
    init = decoding.initial_tokens(tok, _opts(decoding, prompt=prompt), N_CTX, 224)
    assert init[0] == tok.sot_prev and init[1:224] == list(range(1077, 1300)) and init[224:] == list(tok.sot_sequence)
    assert len(init) == 1 + 223 + 3


@pytest.mark.parametrize("sample_len,kept", [(224, 150), (100, 124), (300, 74)])
def test_prefix_slicing_quirks(decoding, tok, sample_len, kept):
    """prefix_tokens[-(n_ctx // 2 - sample_len):]: 224 -> [-0:] keeps all, 100 -> the last 124, 300 -> [76:] drops the front."""
    prefix = list(range(2000, 2150))
    init = decoding.initial_tokens(tok, _opts(decoding, prefix=prefix), N_CTX, sample_len)
    assert init[:3] == list(tok.sot_sequence)
    assert init[3:] == prefix[len(prefix) - kept:]


def test_sample_len_cap_and_context_limit(decoding, tok):
    # 1 + 223 + 3 = 227 initial tokens: at most 448 + 1 - 227 = 222 tokens can be sampled
    init, sample_len, sot_index = decoding.decode_plan(tok, _opts(decoding, prompt=list(range(1000, 1300))), N_CTX)
    assert len(init) == 227 and sample_len == 222 and sot_index == 224
    # a long prefix at sample_len 224 is kept whole (the [-0:] quirk): 3 + 300 = 303 -> 146 samples
    init, sample_len, _ = decoding.decode_plan(tok, _opts(decoding, prefix=list(range(300))), N_CTX)
    assert len(init) == 303 and sample_len == 146
    # an explicit small sample_len is not raised
    assert decoding.decode_plan(tok, _opts(decoding, prompt=[5] * 10, sample_len=8), N_CTX)[1] == 8
    # exactly n_ctx initial tokens: one token can still be sampled (it is never embedded)
    init, sample_len, _ = decoding.decode_plan(tok, _opts(decoding, prefix=list(range(445))), N_CTX)
    assert len(init) == 448 and sample_len == 1
    with pytest.raises(ValueError, match="n_text_ctx"):
        decoding.decode_plan(tok, _opts(decoding, prefix=list(range(446))), N_CTX)


def test_other_options_stay_refused(decoding):
    for kw in ({"beam_size": 5}, {"temperature": 0.5}, {"best_of": 2}, {"language": None}):
        with pytest.raises(NotImplementedError):
            decoding._check_supported(decoding.DecodingOptions(**{"language": "en", **kw}))
    decoding._check_supported(decoding.DecodingOptions(language="en", prompt=[1], prefix=[2]))


class _StubModel:
    """Records the greedy_decode call decode() makes and returns EOT-padded rows with two sampled tokens."""

    def __init__(self, dims):
        self.dims = dims
        self.is_multilingual = True
        self.calls = []

    def greedy_decode(self, mel, pcm, n_samples, initial, sup, blank, sample_len, eot, timestamp_begin, apply_timestamp_rules,
                      max_initial_timestamp_index, batch, no_speech, sot_index=0, prefill=0):
        self.calls.append(dict(initial=list(initial), sample_len=sample_len, sot_index=sot_index, prefill=prefill, batch=batch))
        T = len(initial) + sample_len
        toks = np.full((batch, T), eot, np.int32)
        toks[:, :len(initial)] = initial
        toks[:, len(initial):len(initial) + 2] = [timestamp_begin, timestamp_begin + 5]
        self.last_no_speech_prob = np.full(batch, 0.25, np.float32)
        return toks, np.full(batch, len(initial) + 2, np.int32), np.full(batch, -1.5, np.float32)


def test_decode_passes_the_plan_to_the_engine(decoding, tok, wca):
    dims = wca.ModelDimensions(80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)
    m = _StubModel(dims)
    res = decoding.decode(m, None, _opts(decoding), encoded_batch=2)
    assert m.calls[-1] == dict(initial=list(tok.sot_sequence), sample_len=224, sot_index=0, prefill=0, batch=2)
    prompt = list(range(1000, 1300))
    res = decoding.decode(m, None, _opts(decoding, prompt=prompt, prefix=[9, 10]), encoded_batch=2)
    call = m.calls[-1]
    assert call["prefill"] == 1 and call["sot_index"] == 224 and call["sample_len"] == 448 + 1 - 229
    assert call["initial"] == [tok.sot_prev] + prompt[-223:] + list(tok.sot_sequence) + [9, 10]
    # the result holds the sampled tokens only: neither the prompt nor the prefix
    assert [r.tokens for r in res] == [[tok.timestamp_begin, tok.timestamp_begin + 5]] * 2
    assert res[0].avg_logprob == pytest.approx(-1.5 / 3) and res[0].no_speech_prob == 0.25
    decoding.decode(m, None, _opts(decoding, prefix=[9]), encoded_batch=1)
    assert m.calls[-1]["prefill"] == 1 and m.calls[-1]["sot_index"] == 0


def test_decode_opts_and_desc_mirror_the_header(wca):
    src = open(os.path.join(ROOT, "include", "wca.h")).read()

    def fields(name):
        body = re.search(r"typedef struct \{([^{}]*)\} %s;" % name, src, flags=re.S).group(1)
        return re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))

    assert fields("wca_decode_opts") == [f[0] for f in wca._lib.DecodeOpts._fields_] and ctypes.sizeof(wca._lib.DecodeOpts) == 6 * 4
    # what a prompted decode needs sits in the descriptor: <|sot|>'s position per row, and the batched prefill
    desc = fields("wca_decode_desc")
    assert desc == [f[0] for f in wca._lib.DecodeDesc._fields_]
    assert "sot_index_host" in desc and desc[-4:] == ["batch", "per_row", "prefill", "redecode"]
    lib = wca._lib.load()
    assert lib.wca_version() >= 8
    a, b = ctypes.c_int32(0), ctypes.c_int32(0)
    assert lib.wca_last_decode_positions(None, ctypes.byref(a), ctypes.byref(b)) < 0
    assert lib.wca_decode(None, ctypes.byref(wca._lib.DecodeDesc())) < 0


def test_cli_accepts_initial_prompt():
    infer = importlib.import_module("whisper-char-alignment_amd.infer_ali")
    base = ["--model", "tiny", "--random_init", "--output_dir", "out"]
    assert infer.parse_args(base).initial_prompt is None
    assert infer.parse_args(base + ["--initial_prompt", "Cholmondeley"]).initial_prompt == "Cholmondeley"
