"""CPU tests of transcribe(pieces=...) and transcribe(clip_timestamps=...) (whisper-char-alignment_amd/transcribe.py) against a stub
model and a scripted decoder, as tests/test_transcribe_batch.py does for the lock-step loop: the plan (plan_pieces), the clip loop of
SeekState against a restatement of upstream's seek_clips loop, the rounds a recording's pieces are decoded in, the merge, and what must
not have changed. The stub's quiet_cuts is the numpy restatement (tests/quiet_cuts_ref.py); the GPU side is
tests/test_transcribe_pieces_gpu.py and tests/test_quiet_cuts_gpu.py."""
import importlib

import numpy as np
import pytest
import torch

import quiet_cuts_ref


@pytest.fixture(scope="module")
def tr():
    return importlib.import_module("whisper-char-alignment_amd.transcribe")


@pytest.fixture(scope="module")
def decoding():
    return importlib.import_module("whisper-char-alignment_amd.decoding")


@pytest.fixture(scope="module")
def tok():
    return importlib.import_module("whisper-char-alignment_amd.tokenizer").get_tokenizer(True, language="en", task="transcribe")


def _result(decoding, tokens, avg_logprob=-0.3, no_speech_prob=0.1):
    return decoding.DecodingResult(language="en", tokens=list(tokens), text="", avg_logprob=avg_logprob, no_speech_prob=no_speech_prob,
                                   temperature=0.0, compression_ratio=1.0)


class _Model:
    """The engine as transcribe sees it without words. The long mel is silence with the recording's id in its first element, a window
    carries (id, seek, size), and every call is written down."""
    is_multilingual = True

    def __init__(self, max_batch):
        self.max_batch, self.calls = max_batch, []

    def log_mel_long(self, pcm):
        mel = torch.zeros(80, (pcm.shape[0] + 480000) // 160)
        mel[0, 0] = float(pcm[0])
        return mel

    def quiet_cuts(self, mel_long, n_pieces, radius=500, half_width=12, content_frames=None):
        self.calls.append(("quiet_cuts", int(mel_long[0, 0]), n_pieces, radius))
        return quiet_cuts_ref.quiet_cuts(mel_long.numpy(), n_pieces, radius, half_width, content_frames)

    def mel_window(self, mel_long, seek, size):
        self.calls.append(("mel_window", int(mel_long[0, 0]), seek, size))
        many = isinstance(seek, (list, tuple))
        out = torch.zeros(len(seek) if many else 1, 80, 3000)
        for b, (s, z) in enumerate(zip(seek, size) if many else [(seek, size)]):
            out[b, 0, :3] = torch.tensor([float(mel_long[0, 0]), float(s), float(z)])
        return out if many else out[0]


def _recording(rec_id, seconds):
    pcm = np.zeros(16000 * seconds, np.float32)
    pcm[0] = rec_id
    return pcm


class _Decoder:
    """A window decodes to <|0.00|> a <|size / 2|> (the loop advances by the window) unless `special[(recording, seek)]` says otherwise;
    every call is recorded as a list of (recording, seek, size, prompt)."""

    def __init__(self, tok, decoding, special=None):
        self.tok, self.decoding, self.special, self.calls = tok, decoding, special or {}, []

    def decode_windows(self, windows, prompts):
        assert windows.shape[0] == len(prompts) and windows.shape[1:] == (80, 3000)
        rows, out = [], []
        for w, p in zip(windows, prompts):
            rec, seek, size = (int(round(float(v))) for v in w[0, :3])
            rows.append((rec, seek, size, list(p)))
            plain = [self.tok.timestamp_begin, self.tok.encode("a")[0], self.tok.timestamp_begin + size // 2]
            out.append(self.special.get((rec, seek), _result(self.decoding, plain)))
        self.calls.append(rows)
        return out


def _one(tr, model, audio, **kw):
    """transcribe() of one recording with a BATCH decoder in place of the engine's (transcribe() itself takes the one-window form)."""
    return tr.transcribe_batch(model, [audio], **kw)[0]


# ------------------------------------------------------------------------------------------------ plan_pieces
def test_plan_pieces_by_hand(tr):
    assert tr.plan_pieces(15000, 3, 4) == (3, 500)        # 5000 frames a piece: the radius is the 5 s cap
    assert tr.plan_pieces(3000, 3, 4) == (3, 499)         # 1000 frames a piece: 1000 // 2 - 1
    assert tr.plan_pieces(10, 4, 4) == (2, 1)             # capped to 10 // 4 = 2 pieces of 5 frames: 5 // 2 - 1
    assert tr.plan_pieces(8, 2, 4) == (2, 1)              # the least the kernel takes: 8 // 2 = 4 = 2 x 1 + 2
    assert tr.plan_pieces(7, 4, 4) == (1, 0)              # 7 // 4 = 1 piece: no split
    assert tr.plan_pieces(15000, 1, 4) == (1, 0)
    assert tr.plan_pieces(0, 3, 4) == (1, 0)
    assert tr.plan_pieces(15000, "auto", 16) == (2, 500)  # 150 s: two pieces of at least two windows
    assert tr.plan_pieces(60000, "auto", 4) == (4, 500)   # 10 min: as many as the batch has rows
    assert tr.plan_pieces(60000, "auto", 16) == (10, 500)
    assert tr.plan_pieces(11999, "auto", 8) == (1, 0)
    assert tr.plan_pieces(60000, "auto", 1) == (1, 0)
    assert tr.plan_pieces(4001, 4, 4) == (4, 499)         # 1000 // 2 - 1
    for cf, pieces, mb in [(15000, 3, 4), (3000, 3, 4), (10, 4, 4), (8, 2, 4), (60000, "auto", 16), (4001, 4, 4), (24001, 16, 16)]:
        n, radius = tr.plan_pieces(cf, pieces, mb)
        assert quiet_cuts_ref.valid(cf, cf, n, radius, 12), (cf, pieces, mb)   # every plan is one wca_quiet_cuts takes
    with pytest.raises(ValueError):
        tr.plan_pieces(15000, 5, 4)
    with pytest.raises(ValueError):
        tr.plan_pieces(15000, 0, 4)
    with pytest.raises(ValueError):
        tr.plan_pieces(15000, "many", 4)


# ------------------------------------------------------------------------------------------------ clips
def _upstream_windows(content_frames, clip_timestamps, advance_of):
    """The window sequence of upstream whisper.transcribe's loop (its seek_points / seek_clips bookkeeping, restated line by line), with
    the decode replaced by advance_of(seek, segment_size) -> frames; a stop beyond the recording is clamped, as SeekState documents."""
    seek_points = [round(ts * 100) for ts in clip_timestamps]
    if len(seek_points) == 0:
        seek_points.append(0)
    if len(seek_points) % 2 == 1:
        seek_points.append(content_frames)
    seek_clips = [(a, min(b, content_frames)) for a, b in zip(seek_points[::2], seek_points[1::2])]
    windows = []
    clip_idx = 0
    seek = seek_clips[clip_idx][0]
    while clip_idx < len(seek_clips):
        seek_clip_start, seek_clip_end = seek_clips[clip_idx]
        if seek < seek_clip_start:
            seek = seek_clip_start
        if seek >= seek_clip_end:
            clip_idx += 1
            if clip_idx < len(seek_clips):
                seek = seek_clips[clip_idx][0]
            continue
        segment_size = min(3000, content_frames - seek, seek_clip_end - seek)
        windows.append((seek, segment_size))
        seek += advance_of(seek, segment_size)
    return windows


CLIP_CASES = {
    "whole": [],
    "odd count runs to the end": [12.0],
    "one pair": [10.0, 75.5],
    "past the end": [80.0, 500.0],
    "starts past the end": [10.0, 20.0, 300.0, 400.0],
    "adjacent": [0.0, 31.0, 31.0, 62.0, 62.0, 63.0],
    "shorter than a window": [5.0, 7.5, 40.0, 40.02],
    "three and a half": [1.0, 2.0, 50.0, 90.0, 20.0, 30.0, 95.0],   # (upstream takes them in the order given)
    "empty clip": [10.0, 10.0, 20.0, 15.0, 30.0, 31.0],
}


@pytest.mark.parametrize("name", list(CLIP_CASES))
@pytest.mark.parametrize("inside_speech", [False, True], ids=["by-window", "inside-speech"])
def test_seek_state_clips_restate_upstreams_loop(tr, tok, decoding, name, inside_speech):
    content = 10050   # 100.5 s
    ts, a = tok.timestamp_begin, tok.encode("a")[0]

    def advance_of(seek, size):   # every third window ends inside speech, 3 s before its end (where it is long enough)
        return size - 300 if inside_speech and size > 400 and (seek // 7) % 3 == 0 else size

    want = _upstream_windows(content, CLIP_CASES[name], advance_of)
    st = tr.SeekState(content + 3000, tok, clips=tr.clip_frames(CLIP_CASES[name], content))
    got = []
    while not st.done:
        seek, size, _ = st.request()
        got.append((seek, size))
        adv = advance_of(seek, size)
        tokens = [ts, a, ts + size // 2] if adv == size else [ts, a, ts + adv // 2, ts + adv // 2, a]
        st.commit() if st.receive(_result(decoding, tokens)) is not None else None
        assert len(got) < 100
    assert got == want
    assert [(w["seek"], w["size"]) for w in st.result()["windows"]] == want
    if name == "whole":
        plain = tr.SeekState(content + 3000, tok)
        assert plain.clips == st.clips == [(0, content)]


def test_clip_frames(tr):
    assert tr.clip_frames("0", 500) == [(0, 500)] and tr.clip_frames("", 500) == [(0, 500)] and tr.clip_frames([], 500) == [(0, 500)]
    assert tr.clip_frames("1.5,2.25, 3", 500) == [(150, 225), (300, 500)]
    assert tr.clip_frames([13.32, 26.66], 4001) == [(1332, 2666)] and tr.clip_frames(1.0, 500) == [(100, 500)]
    assert tr.clip_frames([0.125, 0.135], 500) == [(12, 14)]   # Python's round, as upstream: 12.5 -> 12, 13.5 -> 14
    with pytest.raises(ValueError):
        tr.SeekState(3500, None, clips=[(-1, 100)], decode_text=lambda t: "")


def test_clip_timestamps_give_the_windows_the_clips_dictate(tr, tok, decoding):
    audio = _recording(1, 100)
    dec = _Decoder(tok, decoding)
    res = _one(tr, _Model(1), audio, language="en", clip_timestamps="10,45.5,70,72,90", decode_windows=dec.decode_windows)
    want = [(1000, 3000), (4000, 550), (7000, 200), (9000, 1000)]
    assert [(w["seek"], w["size"]) for w in res["windows"]] == want
    assert [[(r[1], r[2]) for r in call] for call in dec.calls] == [[w] for w in want]
    assert "pieces" not in res and all("piece" not in w for w in res["windows"])
    assert [s["start"] for s in res["segments"]] == [10.0, 40.0, 70.0, 90.0] and [s["id"] for s in res["segments"]] == [0, 1, 2, 3]
    # the previous text crosses from one clip into the next, as upstream's all_tokens does
    assert dec.calls[2][0][3] == res["segments"][0]["tokens"] + res["segments"][1]["tokens"]
    both = tr.transcribe_batch(_Model(2), [audio, _recording(2, 50)], language="en", clip_timestamps=[10, 45.5, 70, 72, 90],
                               decode_windows=_Decoder(tok, decoding).decode_windows)
    assert both[0] == res and [(w["seek"], w["size"]) for w in both[1]["windows"]] == [(1000, 3000), (4000, 550)]


# ------------------------------------------------------------------------------------------------ pieces
def _inside(tok, decoding):
    ts, a = tok.timestamp_begin, tok.encode("a")[0]
    return _result(decoding, [ts, a, ts + 200, ts + 200, a, a])   # ends inside speech: advances to the pair, 400 frames


def test_three_pieces_are_decoded_side_by_side(tr, tok, decoding):
    """200 s of silence in three pieces: the cuts fall on the even frames nearest 6666 and 13333. The middle piece's first window ends
    inside speech, so that piece needs a fourth round, which it decodes alone."""
    model, dec = _Model(4), _Decoder(tok, decoding, {(1, 6666): _inside(tok, decoding)})
    res = _one(tr, model, _recording(1, 200), language="en", initial_prompt=[7, 8], pieces=3, decode_windows=dec.decode_windows)
    assert [(p["start_frame"], p["stop_frame"]) for p in res["pieces"]] == [(0, 6666), (6666, 13332), (13332, 20000)]
    assert [p["level"] for p in res["pieces"]] == [None, 0, 0]
    assert ("quiet_cuts", 1, 3, 500) in model.calls
    # round r decodes the r-th window of every unfinished piece in ONE call, and the batch shrinks
    assert [[(r[1], r[2]) for r in call] for call in dec.calls] == [
        [(0, 3000), (6666, 3000), (13332, 3000)], [(3000, 3000), (7066, 3000), (16332, 3000)], [(6000, 666), (10066, 3000), (19332, 668)],
        [(13066, 266)]]
    # ... with one window cut per recording and round: a list call while several pieces are live, the plain call for the last one
    cuts = [c for c in model.calls if c[0] == "mel_window"]
    assert len(cuts) == len(dec.calls) == 4
    assert cuts[0] == ("mel_window", 1, [0, 6666, 13332], [3000, 3000, 3000]) and cuts[3] == ("mel_window", 1, 13066, 266)
    # every piece starts from the initial prompt only and conditions on its own previous text
    prompts = {r[1]: r[3] for call in dec.calls for r in call}
    by_seek = {}
    for s in res["segments"]:
        by_seek.setdefault(s["seek"], []).extend(s["tokens"])
    assert prompts[0] == prompts[6666] == prompts[13332] == [7, 8]
    assert prompts[3000] == [7, 8] + by_seek[0] and prompts[6000] == [7, 8] + by_seek[0] + by_seek[3000]
    assert prompts[7066] == [7, 8] + by_seek[6666] and prompts[13066] == [7, 8] + by_seek[6666] + by_seek[7066] + by_seek[10066]
    assert prompts[16332] == [7, 8] + by_seek[13332]
    # merged in piece order: consecutive ids, non-decreasing starts, the windows of piece 0, then 1, then 2
    assert [s["id"] for s in res["segments"]] == list(range(len(res["segments"]))) and len(res["segments"]) == 10
    starts = [s["start"] for s in res["segments"]]
    assert starts == sorted(starts) and starts[0] == 0.0 and starts[3] == 66.66
    assert [w["piece"] for w in res["windows"]] == [0, 0, 0, 1, 1, 1, 1, 2, 2, 2]
    assert [w["seek"] for w in res["windows"]] == [0, 3000, 6000, 6666, 7066, 10066, 13066, 13332, 16332, 19332]
    # every window lies inside its piece, and the pieces tile [0, content_frames)
    for w in res["windows"]:
        p = res["pieces"][w["piece"]]
        assert p["start_frame"] <= w["seek"] and w["seek"] + w["size"] <= p["stop_frame"]
    assert res["pieces"][0]["start_frame"] == 0 and res["pieces"][-1]["stop_frame"] == 20000
    assert all(a["stop_frame"] == b["start_frame"] for a, b in zip(res["pieces"], res["pieces"][1:]))
    assert res["windows_without_words"] == 0 and res["language"] == "en"


def test_pieces_equal_the_same_ranges_as_clips(tr, tok, decoding):
    """What the GPU test asks of the engine, here of the host loop: pieces=3 is the three clip runs merged."""
    special = {(1, 6666): _inside(tok, decoding), (1, 16332): _result(decoding, [tok.timestamp_begin], avg_logprob=-2.0, no_speech_prob=0.9)}
    audio = _recording(1, 200)
    res = _one(tr, _Model(4), audio, language="en", pieces=3, decode_windows=_Decoder(tok, decoding, special).decode_windows)
    assert [w["skipped"] for w in res["windows"]].count(True) == 1
    segments, windows = [], []
    for k, p in enumerate(res["pieces"]):
        part = _one(tr, _Model(1), audio, language="en", clip_timestamps=[p["start_frame"] / 100, p["stop_frame"] / 100],
                             decode_windows=_Decoder(tok, decoding, special).decode_windows)
        segments += [{**s, "id": len(segments) + j} for j, s in enumerate(part["segments"])]
        windows += [{**w, "piece": k} for w in part["windows"]]
    assert res["segments"] == segments and res["windows"] == windows


def test_batch_groups_hold_as_many_recordings_as_their_pieces_fit(tr, tok, decoding):
    audios = [_recording(1, 150), _recording(2, 70), _recording(3, 150)]
    model, dec = _Model(4), _Decoder(tok, decoding)
    got = tr.transcribe_batch(model, audios, language="en", pieces=2, decode_windows=dec.decode_windows)
    # max_batch // 2 = two recordings a group; the first round of the first group has their four pieces as its rows
    assert [[r[0] for r in call] for call in dec.calls][0] == [1, 1, 2, 2] and max(len(call) for call in dec.calls) == 4
    assert [sorted({r[0] for r in call}) for call in dec.calls] == [[1, 2], [1, 2], [1], [3], [3], [3]]
    assert [[(p["start_frame"], p["stop_frame"]) for p in r["pieces"]] for r in got] == [[(0, 7500), (7500, 15000)], [(0, 3500), (3500, 7000)],
                                                                                           [(0, 7500), (7500, 15000)]]
    # one window cut per recording and round
    assert [c[1] for c in model.calls if c[0] == "mel_window"] == [1, 2, 1, 2, 1, 3, 3, 3]
    alone = [_one(tr, _Model(4), a, language="en", pieces=2, decode_windows=_Decoder(tok, decoding).decode_windows) for a in audios]
    assert got == alone
    # "auto": 150 s gives two pieces, 70 s none (it keeps its one row): all four rows of max_batch in one group, then the last recording
    model, dec = _Model(4), _Decoder(tok, decoding)
    got = tr.transcribe_batch(model, audios, language="en", pieces="auto", decode_windows=dec.decode_windows)
    assert [[r[0] for r in call] for call in dec.calls][0] == [1, 1, 2] and dec.calls[3][0][0] == 3
    assert [len(r["pieces"]) for r in got] == [2, 1, 2] and got[1]["pieces"] == [{"start_frame": 0, "stop_frame": 7000, "level": None}]
    assert [w["piece"] for w in got[1]["windows"]] == [0, 0, 0]
    assert not any(c[0] == "quiet_cuts" and c[1] == 2 for c in model.calls)


def test_detected_language_goes_to_every_piece(tr, tok, decoding):
    seen = []

    def detect(windows):
        seen.append([tuple(int(round(float(v))) for v in w[0, :3]) for w in windows])
        return ["de"] * len(windows), [0.75] * len(windows)

    dec = _Decoder(tok, decoding)
    res = _one(tr, _Model(4), _recording(1, 150), language="auto", pieces=2, detect_languages=detect, decode_windows=dec.decode_windows)
    assert seen == [[(1, 0, 3000)]]   # detected once, on the recording's first window
    assert res["language"] == "de" and res["language_probability"] == 0.75 and len(res["pieces"]) == 2
    assert [len(call) for call in dec.calls] == [2, 2, 2]


def test_without_pieces_and_clips_the_result_is_todays(tr, tok, decoding):
    special = {(1, 0): _inside(tok, decoding), (1, 3400): _result(decoding, [tok.timestamp_begin], avg_logprob=-2.0, no_speech_prob=0.9)}
    audio = _recording(1, 94)
    model = _Model(4)
    res = _one(tr, model, audio, language="en", initial_prompt=[7, 8], decode_windows=_Decoder(tok, decoding, special).decode_windows)
    assert list(res) == ["text", "segments", "language", "windows", "windows_without_words"]
    assert all(list(w) == ["seek", "size", "advance", "skipped", "max_frames", "aligned"] for w in res["windows"])
    assert all(list(s) == ["id", "seek", "start", "end", "text", "tokens", "temperature", "avg_logprob", "compression_ratio", "no_speech_prob",
                           "words"] for s in res["segments"])
    assert [(w["seek"], w["size"], w["advance"], w["skipped"]) for w in res["windows"]] == [(0, 3000, 400, False), (400, 3000, 3000, False),
                                                                                           (3400, 3000, 3000, True), (6400, 3000, 3000, False)]
    # every window was cut with the plain call
    assert [c for c in model.calls if c[0] == "mel_window"] == [("mel_window", 1, 0, 3000), ("mel_window", 1, 400, 3000),
                                                                ("mel_window", 1, 3400, 3000), ("mel_window", 1, 6400, 3000)]
    # the same windows and segments as the loop over one recording (seek_loop), which has no clips and no pieces
    dec = _Decoder(tok, decoding, special)
    mel = model.log_mel_long(torch.from_numpy(audio))
    loop = tr.seek_loop(mel.shape[1], lambda seek, size: model.mel_window(mel, seek, size), lambda w, p: dec.decode_windows(w[None], [p])[0], tok,
                        initial_prompt_tokens=[7, 8], decode_text=lambda toks: None)
    assert loop["segments"] == res["segments"] and loop["windows"] == res["windows"]
    # pieces=1 and a recording too short to cut: the same, plus the one piece
    one = _one(tr, _Model(4), audio, language="en", initial_prompt=[7, 8], pieces=1, decode_windows=_Decoder(tok, decoding, special).decode_windows)
    assert one.pop("pieces") == [{"start_frame": 0, "stop_frame": 9400, "level": None}]
    assert [w.pop("piece") for w in one["windows"]] == [0, 0, 0, 0] and one == res


def test_refusals(tr, tok, decoding):
    audio = _recording(1, 150)
    dec = _Decoder(tok, decoding)
    with pytest.raises(ValueError, match="clip_timestamps"):
        _one(tr, _Model(4), audio, language="en", pieces=2, clip_timestamps="0,10", decode_windows=dec.decode_windows)
    with pytest.raises(ValueError, match="max_batch"):
        _one(tr, _Model(4), audio, language="en", pieces=5, decode_windows=dec.decode_windows)
    with pytest.raises(ValueError, match="max_batch"):
        tr.transcribe_batch(_Model(2), [audio], language="en", pieces=3, decode_windows=dec.decode_windows)
    with pytest.raises(ValueError):
        _one(tr, _Model(4), audio, language="en", pieces="some", decode_windows=dec.decode_windows)
    assert dec.calls == []
    # what tests/test_transcribe.py pins still holds with the new keywords
    for kw in (dict(pieces=2), dict(clip_timestamps="0,10")):
        with pytest.raises(NotImplementedError):
            tr.transcribe(None, audio, language="en", temperature=(0.0, 0.2, 0.4), **kw)
        with pytest.raises(NotImplementedError):
            tr.transcribe(None, audio, language="en", temperature=0.2, **kw)
        with pytest.raises(NotImplementedError):
            tr.transcribe(None, audio, language=None, **kw)
        with pytest.raises(ValueError, match="vocab"):
            tr.transcribe(None, audio, language="en", word_timestamps=True, **kw)
        with pytest.raises(ValueError):
            tr.transcribe(None, audio, language="en", word_confidence=True, **kw)


def test_cli_flags(tr):
    base = ["--audio", "x.wav", "--output_dir", "out", "--random_init"]
    args = tr.parse_args(base)
    assert args.pieces is None and args.clip_timestamps is None
    assert tr.parse_args(base + ["--pieces", "auto"]).pieces == "auto" and tr.parse_args(base + ["--pieces", "4", "--batch", "4"]).pieces == 4
    assert tr.parse_args(base + ["--clip_timestamps", "0,12.5,30"]).clip_timestamps == "0,12.5,30"
    with pytest.raises(SystemExit):
        tr.parse_args(base + ["--pieces", "several"])
    for bad in (["--pieces", "4"], ["--pieces", "4", "--batch", "3"], ["--pieces", "0"], ["--pieces", "2", "--batch", "2", "--clip_timestamps", "0,5"]):
        with pytest.raises(SystemExit):   # (refused before the model is looked at)
            tr.main(tr.parse_args(base + bad), model=object())


def test_abi_mirror_of_quiet_cuts(wca):
    lib = wca._lib.load()
    assert lib.wca_version() >= 15
    assert lib.wca_quiet_cuts(None, None, 0, 0, 0, 0, 0, None, None) < 0 and b"null" in lib.wca_last_error()
