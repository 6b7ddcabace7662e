"""CPU tests of the pieces the long-form drivers are made of (whisper-char-alignment_amd: longform.py, and transcribe.py's grouping,
planning and merge), each on its own against a stub model; what they do together is pinned by tests/test_longform_trace.py."""
import importlib

import numpy as np
import pytest
import torch

import quiet_cuts_ref


@pytest.fixture(scope="module")
def lf():
    return importlib.import_module("whisper-char-alignment_amd.longform")


@pytest.fixture(scope="module")
def tr():
    return importlib.import_module("whisper-char-alignment_amd.transcribe")


class _Model:
    max_batch = 4

    def __init__(self):
        self.calls = []

    def log_mel_long(self, pcm):
        self.calls.append(("log_mel_long", pcm.shape[0] // 16000))
        return torch.zeros(80, (pcm.shape[0] + 480000) // 160)

    def quiet_cuts(self, mel_long, n_pieces, radius=500, half_width=12, content_frames=None):
        self.calls.append(("quiet_cuts", mel_long.shape[1], n_pieces, radius))
        return quiet_cuts_ref.quiet_cuts(mel_long.numpy(), n_pieces, radius, half_width, content_frames)

    def mel_window(self, mel_long, seek, size):
        self.calls.append(("mel_window", mel_long.shape[1], seek, size))
        many = isinstance(seek, list)
        out = torch.zeros(len(seek) if many else 1, 80, 3000)
        out[:, 0, 0] = torch.tensor(seek if many else [seek], dtype=torch.float32)
        return out if many else out[0]


def test_the_constants_are_shared_and_the_token_limit_is_the_engines(lf, tr, wca):
    al = importlib.import_module("whisper-char-alignment_amd.align_long")
    engine = importlib.import_module("whisper-char-alignment_amd.engine")
    assert tr.MAX_LENGTH is al.MAX_LENGTH is lf.MAX_LENGTH is engine.MAX_LENGTH == 448
    assert (tr.INPUT_STRIDE, tr.FRAME_SECONDS, tr.TIME_PRECISION, tr.FRAMES_PER_SECOND) == (2, 0.01, 0.02, 100)
    assert (al.INPUT_STRIDE, al.FRAME_SECONDS) == (lf.INPUT_STRIDE, lf.FRAME_SECONDS) == (2, 0.01)
    assert tr.load_model is al.load_model is lf.load_model


def test_sample_rates_and_groups(lf):
    assert lf.sample_rates(8000, 3) == [8000] * 3 and lf.sample_rates((8000, 16000.0), 2) == [8000, 16000] and lf.sample_rates(16000, 0) == []
    with pytest.raises(ValueError, match="2 rates for 3"):
        lf.sample_rates([8000, 8000], 3)
    assert lf.groups_of([1, 2, 3, 4, 5], 2) == [[1, 2], [3, 4], [5]] and lf.groups_of([], 3) == []


def test_pad_token_rows(lf):
    toks = lf.pad_token_rows([[1, 2, 3], [4], [5, 6]], 9)
    assert toks.dtype == torch.int64 and toks.tolist() == [[1, 2, 3], [4, 9, 9], [5, 6, 9]]
    assert lf.pad_token_rows([[7, 8]], 9).tolist() == [[7, 8]]


def test_cut_windows_makes_one_call_per_recording(lf):
    model, mels = _Model(), {3: torch.zeros(80, 9000), 5: torch.zeros(80, 12000)}
    one = lf.cut_windows(model, mels, [(5, 100, 3000)])
    assert one.shape == (1, 80, 3000) and model.calls == [("mel_window", 12000, 100, 3000)]   # the plain call
    model.calls.clear()
    got = lf.cut_windows(model, mels, [(3, 0, 3000), (5, 10, 3000), (5, 20, 500), (5, 30, 3000)])
    assert model.calls == [("mel_window", 9000, 0, 3000), ("mel_window", 12000, [10, 20, 30], [3000, 500, 3000])]
    assert got.shape == (4, 80, 3000) and got[:, 0, 0].tolist() == [0.0, 10.0, 20.0, 30.0]   # rows in request order


def test_aligner_options_clamp_topk_to_the_heads(lf, wca):
    class _M:
        dims = wca.ModelDimensions(80, 1500, 256, 4, 2, 51865, 448, 256, 4, 2)

        def make_opts(self, **kw):
            return kw

    tok = importlib.import_module("whisper-char-alignment_amd.tokenizer").get_tokenizer(True, language="en", task="transcribe")
    opts = lf.aligner_options(_M(), tok, topk=50, medfilt_width=5)
    assert opts == dict(aggregation="topk", topk=8, w_colnorm=1.0, w_rownorm=1.0, w_coverage=0.0, sot_len=3, medfilt_width=5, qk_scale=1.0)
    assert lf.aligner_options(_M(), tok, aggr="mean", topk=50)["topk"] == 50
    with pytest.raises(TypeError):
        lf.aligner_options(_M(), tok, top_k=3)


def test_plan_recording(tr):
    model, mel = _Model(), torch.zeros(80, 15000 + 3000)
    assert tr.plan_recording(mel, None, None, 4, model) == ([None], None)
    assert tr.plan_recording(mel, "10,20,30", None, 4, model) == ([[(1000, 2000), (3000, 15000)]], None) and model.calls == []
    clips, pieces = tr.plan_recording(mel, None, 2, 4, model)
    assert clips == [[(0, 7500)], [(7500, 15000)]] and model.calls == [("quiet_cuts", 18000, 2, 500)]
    assert pieces == [{"start_frame": 0, "stop_frame": 7500, "level": None}, {"start_frame": 7500, "stop_frame": 15000, "level": 0}]
    short = tr.plan_recording(torch.zeros(80, 3007), None, 2, 4, model)   # too short to cut: the plain loop, and the one piece
    assert short == ([None], [{"start_frame": 0, "stop_frame": 7, "level": None}]) and len(model.calls) == 1


@pytest.mark.parametrize("pieces,seconds,want_groups,computed_at_yield", [
    (None, [40, 50, 60, 70, 80], [[0, 1, 2, 3], [4]], [4, 5]),        # max_batch recordings, each computed as it joins its group
    (2, [40, 50, 60, 70, 80], [[0, 1], [2, 3], [4]], [2, 4, 5]),      # max_batch // 2, whatever their length
    ("auto", [150, 150, 70, 150, 70], [[0, 1], [2, 3, 4]], [3, 5]),   # 150 s takes two rows, 70 s one; recording 2 is computed one ahead
])
def test_form_groups_fill_max_batch_rows_and_drop_a_group_when_the_next_is_asked_for(tr, pieces, seconds, want_groups, computed_at_yield):
    model = _Model()
    audios = [np.zeros(16000 * s, np.float32) for s in seconds]
    groups, computed, before = [], [], None
    for group, mels, plans in tr.form_groups(model, audios, [16000] * 5, None, pieces, 4):
        assert before is None or (before[0] is mels and not set(before[1]) & set(mels))   # the last group's log-mels are gone
        assert list(mels) == list(plans) == group and all(mels[i].shape[1] == 100 * seconds[i] + 3000 for i in group)
        groups.append(list(group))
        computed.append(sum(c[0] == "log_mel_long" for c in model.calls))
        before = (mels, list(mels))
    assert groups == want_groups and computed == computed_at_yield
    assert [c[1] for c in model.calls if c[0] == "log_mel_long"] == seconds   # each once, in input order
    assert list(tr.form_groups(model, [], [], None, pieces, 4)) == []


def test_merge_pieces(tr):
    def out(seek, tokens):
        return {"segments": [{"id": 0, "seek": seek, "tokens": tokens}], "tokens": [7, 8, *tokens], "windows": [{"seek": seek}], "windows_without_words": 1}

    class _Tok:
        def decode(self, tokens):
            return "+".join(map(str, tokens))

    pieces = [{"start_frame": 0, "stop_frame": 10, "level": None}, {"start_frame": 10, "stop_frame": 20, "level": 3}]
    res = tr.merge_pieces([out(0, [1, 2]), out(10, [3])], pieces, tokenizer=_Tok(), language="de", extra={"language_probability": 0.5}, n_prompt=2)
    assert list(res) == ["text", "segments", "language", "language_probability", "windows", "windows_without_words", "pieces"]
    assert res["text"] == "1+2+3" and [s["id"] for s in res["segments"]] == [0, 1] and res["windows"] == [{"seek": 0, "piece": 0}, {"seek": 10, "piece": 1}]
    assert res["windows_without_words"] == 2 and res["pieces"] is pieces and res["language"] == "de"
    plain = tr.merge_pieces([out(0, [1, 2])], None, tokenizer=None, language="en", extra={}, n_prompt=2)
    assert list(plain) == ["text", "segments", "language", "windows", "windows_without_words"] and plain["text"] == "" and plain["windows"] == [{"seek": 0}]
