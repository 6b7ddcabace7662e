#!/usr/bin/env python3
"""Generates tests/golden/longform_trace.json: what the long-form host layer (transcribe.py, align_long.py) asks of the engine and what it
returns, against a stub model that writes every engine call down as (name, argument shapes, int lists, scalar options).

It pins the host Python of the long-form paths so that it can be restructured without moving behaviour: the fixture is generated once,
on the commit before such a change, and tests/test_longform_trace.py replays the same cases and compares the serialised call lists and
result dicts for equality (key order included). Recordings are 20 to 130 s of zeros; where pieces are involved the stub's quiet_cuts is the
numpy restatement tests/quiet_cuts_ref.py.

Cases (`run_all`):
  * transcribe / transcribe_batch over {one recording through transcribe(), three of 20 / 70 / 94 s with max_batch 2, so a second group
    forms} x {plain, clip_timestamps="5,25,40", pieces=2, pieces="auto" with a 130 s recording} x {language "en", "auto" with a scripted
    detect_languages: all one language, two languages} x {word_timestamps off, on with word_confidence};
  * language="auto" through the ENGINE's detection (model.detect_language), which leaves encoded state behind for the first round: one
    language (used), two languages, clips, a recording without a first window (dropped), and an English-only model;
  * transcribe(decode_window=...) with pieces (wrapped row by row), and a call without a vocabulary;
  * the refusals, in their order, each with the stub's (empty) call list;
  * force_align_long_batch over 70 s and 20 s with a 12-word transcript each (open and closed windows), and an over-long word;
  * transcribe.main and align_long.main over a two-line --scp: the paths written, each JSON's key order and content.
Run from the repo root:  python tests/golden/make_longform_trace.py
"""
import base64
import contextlib
import importlib
import io
import json
import os
import struct
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for _p in (ROOT, TESTS):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import quiet_cuts_ref  # noqa: E402

OUT = os.path.join(HERE, "longform_trace.json")
TEXT = " ab cd"
LANGUAGE_BY_SECONDS = {"one": {}, "two": {70: "de", 130: "de"}}   # scripted detection: a recording's language by its length ("fr" otherwise)


def _m(name):
    return importlib.import_module("whisper-char-alignment_amd." + name)


def write_vocab(path):
    """A tiktoken-format vocabulary of the right size (the 256 bytes + synthetic 4-letter tokens), as tests/conftest.py's fake_vocab."""
    ranks = dict(_m("tokenizer")._byte_ranks())
    i = 0
    while len(ranks) < 50257:
        w = bytes([97 + (i % 26), 97 + (i // 26) % 26, 97 + (i // 676) % 26, 97 + (i // 17576) % 26])
        i += 1
        if w not in ranks:
            ranks[w] = len(ranks)
    with open(path, "wb") as f:
        for tokb, r in sorted(ranks.items(), key=lambda kv: kv[1]):
            f.write(base64.b64encode(tokb) + b" " + str(r).encode() + b"\n")
    return str(path)


def describe(v):
    """An engine-call argument as JSON: a float tensor / array by its shape, an integer tensor by shape and values, the rest as it is."""
    if isinstance(v, torch.Tensor):
        return {"shape": list(v.shape)} if v.is_floating_point() else {"shape": list(v.shape), "ints": v.tolist()}
    if isinstance(v, np.ndarray):
        return {"shape": list(v.shape), "sum": float(v.sum())}
    if isinstance(v, (list, tuple)):
        return [describe(x) for x in v]
    if isinstance(v, dict):
        return {k: describe(x) for k, x in v.items()}
    if isinstance(v, np.generic):
        return v.item()
    return v


class TraceModel:
    """The engine as the long-form host layer sees it. A window carries (seek, size, frames of its recording's log-mel) in its first
    elements, so the scripted decoder and detection know what they look at; a decode or alignment without a mel looks at the windows of
    the call that encoded last, as the engine's state does."""

    _silence = {}

    def __init__(self, max_batch, multilingual=True, languages=None, jump_step=1):
        self.dims = _m("engine").ModelDimensions(80, 1500, 256, 4, 2, 51865 if multilingual else 51864, 448, 256, 4, 2)
        self.is_multilingual, self.max_batch, self.device = multilingual, max_batch, torch.device("cpu")
        self.languages, self.jump_step = languages or {}, jump_step
        self.calls, self.state = [], None
        tok = _m("tokenizer").get_tokenizer(multilingual, language="en", task="transcribe")
        self.ts, self.text = tok.timestamp_begin, None

    def _say(self, name, *args, **kw):
        self.calls.append([name, describe(list(args)), describe(kw)])

    # ---- front end
    def resample(self, pcm, sr_in):
        self._say("resample", pcm, sr_in)
        return torch.zeros(pcm.shape[-1] * 16000 // sr_in)

    def log_mel_long(self, pcm):
        self._say("log_mel_long", pcm)
        frames = (pcm.shape[0] + 480000) // 160
        if frames not in self._silence:   # (never written to: one tensor per length serves every case)
            self._silence[frames] = torch.zeros(self.dims.n_mels, frames)
        return self._silence[frames]

    def quiet_cuts(self, mel_long, n_pieces, radius=500, half_width=12, content_frames=None):
        self._say("quiet_cuts", mel_long, n_pieces, radius=radius)
        return quiet_cuts_ref.quiet_cuts(mel_long.numpy(), n_pieces, radius, half_width, content_frames)

    def mel_window(self, mel_long, seek, size):
        self._say("mel_window", mel_long, seek, size)
        many = isinstance(seek, (list, tuple))
        out = torch.zeros(len(seek) if many else 1, self.dims.n_mels, 3000)
        for b, (s, z) in enumerate(zip(seek, size) if many else [(seek, size)]):
            out[b, 0, :3] = torch.tensor([float(s), float(z), float(mel_long.shape[1])])
        return out if many else out[0]

    @staticmethod
    def _rows(mel):
        return [tuple(int(round(float(v))) for v in w[0, :3]) for w in mel]

    # ---- detection and decode
    def detect_language(self, mel=None, tokenizer=None, *, pcm=None, n_samples=None, batch=None, sot=None, lang_begin=None, n_lang=None):
        self._say("detect_language", mel, pcm=pcm, n_samples=n_samples, sot=sot, lang_begin=lang_begin, n_lang=n_lang)
        self.state = mel
        codes = list(_m("tokenizer").LANGUAGES)
        picks = [codes.index(self.languages.get((frames - 3000) // 100, "fr")) for _s, _z, frames in self._rows(mel)]
        probs = np.full((len(picks), n_lang), 0.25 / (n_lang - 1), np.float32)
        probs[np.arange(len(picks)), picks] = 0.75
        return np.array([lang_begin + j for j in picks], np.int32), probs

    def _script(self, seek, size):
        """(sampled tokens, sum_logprob, no_speech_prob) of the window at `seek`: by (seek // 200) % 4 it ends inside speech (seek advances
        to the timestamp pair, 400 frames), is plain, is skipped as no speech, or is plain again."""
        kind = (seek // 200) % 4
        if kind == 0:
            return [self.ts, *self.text, self.ts + 200, self.ts + 200, *self.text], -1.0, 0.05
        if kind == 2:
            return [self.ts, *self.text, self.ts + 100], -100.0, 0.9
        return [self.ts, *self.text, self.ts + min(100, size // 2)], -1.0, 0.05

    def _decoded(self, mel, initials, T, eot):
        if mel is not None:
            self.state = mel
        rows = self._rows(self.state)
        assert len(rows) == len(initials)
        toks, n_tokens, sums, nsp = np.full((len(rows), T), eot, np.int32), [], [], []
        for b, ((seek, size, _f), init) in enumerate(zip(rows, initials)):
            out, sum_logprob, no_speech_prob = self._script(seek, size)
            toks[b, :len(init)] = init
            toks[b, len(init):len(init) + len(out)] = out
            n_tokens.append(len(init) + len(out)), sums.append(sum_logprob), nsp.append(no_speech_prob)
        self.last_no_speech_prob = np.array(nsp, np.float32)
        return toks, np.array(n_tokens, np.int32), np.array(sums, np.float32)

    def greedy_decode(self, mel, pcm, n_samples, initial, sup, blank, sample_len, eot, timestamp_begin, apply_timestamp_rules,
                      max_initial_timestamp_index, batch, no_speech, sot_index=0, prefill=0):
        self._say("greedy_decode", mel, pcm, n_samples, list(initial), sup, blank, sample_len=sample_len, eot=eot, timestamp_begin=timestamp_begin,
                  apply_timestamp_rules=apply_timestamp_rules, max_initial_timestamp_index=max_initial_timestamp_index, batch=batch,
                  no_speech=no_speech, sot_index=sot_index, prefill=prefill)
        return self._decoded(mel, [list(initial)] * batch, len(initial) + sample_len, eot)

    def greedy_decode_rows(self, mel, pcm, n_samples, initial_tokens, sot_index, sample_len, sup, blank, eot, timestamp_begin,
                           apply_timestamp_rules, max_initial_timestamp_index, batch, no_speech):
        self._say("greedy_decode_rows", mel, pcm, n_samples, initial_tokens, sot_index, sample_len, sup, blank, eot=eot,
                  timestamp_begin=timestamp_begin, apply_timestamp_rules=apply_timestamp_rules,
                  max_initial_timestamp_index=max_initial_timestamp_index, batch=batch, no_speech=no_speech)
        return self._decoded(mel, initial_tokens, max(len(i) + s for i, s in zip(initial_tokens, sample_len)), eot)

    # ---- alignment
    def make_opts(self, **kw):
        self._say("make_opts", **kw)
        return kw

    def encode_batch(self, mel=None, pcm=None, n_samples=None):
        self._say("encode_batch", mel=mel, pcm=pcm, n_samples=n_samples)
        self.state = mel
        return mel.shape[0]

    def align_batch(self, pcm, n_samples, tokens, n_tok, max_frames, opts, enqueue_only=False, token_logprobs_vocab_end=None, open_end=None):
        self._say("align_batch", pcm, n_samples, tokens, list(n_tok), list(max_frames), opts, enqueue_only=enqueue_only,
                  token_logprobs_vocab_end=token_logprobs_vocab_end, open_end=open_end)
        assert tokens.shape[0] == len(self.state)
        B, n = tokens.shape
        out = [np.tile(np.arange(n, dtype=np.int32) * self.jump_step, (B, 1)), None]
        if token_logprobs_vocab_end is not None:
            out.append(np.full((B, n), np.log(0.5), np.float32))
        if open_end is not None:   # the path of an open row ends half way through its units: an interior window commits about half its words
            sot_len = opts["sot_len"]
            out += [np.array([(k - sot_len - 2) // 2 for k in n_tok], np.int32), np.full(B, -1.0, np.float32)]
        return tuple(out)


def _audio(seconds):
    return np.zeros(16000 * seconds, np.float32)


def _outcome(model, call):
    """One case's record: the result (or the exception) and every engine call the stub saw."""
    try:
        result = call()
    except (ValueError, TypeError, NotImplementedError) as e:
        return {"raises": type(e).__name__, "message": str(e), "calls": model.calls}
    return {"result": result, "calls": model.calls}


def _model(vocab, **kw):
    model = TraceModel(**kw)
    tok = _m("tokenizer").get_tokenizer(model.is_multilingual, language="en", task="transcribe", vocab_path=vocab)
    model.text = tok.encode(TEXT) if vocab is not None else [tok.encode(ch)[0] for ch in TEXT]   # (without the merge table: byte by byte)
    return model


def transcribe_cases(vocab):
    tr = _m("transcribe")
    cases = {}
    modes = {"plain": {}, "clips": {"clip_timestamps": "5,25,40"}, "pieces2": {"pieces": 2}, "auto": {"pieces": "auto"}}
    for n_rec in (1, 3):
        for mode, mode_kw in modes.items():
            seconds = {1: [130 if mode == "auto" else 94], 3: [20, 130 if mode == "auto" else 70, 94]}[n_rec]
            for lang in ("en", "one", "two"):
                for words in (False, True):
                    model = _model(vocab, max_batch=2)
                    kw = dict(language="en", vocab_path=vocab, initial_prompt="abcd", word_timestamps=words, word_confidence=words, **mode_kw)
                    if lang != "en":
                        def detect(mel_windows, model=model, lang=lang):
                            model._say("detect_languages", mel_windows)
                            rows = model._rows(mel_windows)
                            return [LANGUAGE_BY_SECONDS[lang].get((f - 3000) // 100, "fr") for _s, _z, f in rows], [0.75] * len(rows)
                        kw.update(language="auto", detect_languages=detect)
                    audios = [_audio(s) for s in seconds]
                    call = (lambda: tr.transcribe(model, audios[0], **kw)) if n_rec == 1 else (lambda: tr.transcribe_batch(model, audios, **kw))
                    cases["%d-%s-%s-%s" % (n_rec, mode, lang, "words" if words else "segments")] = _outcome(model, call)
    # language="auto" through the engine's own detection: the state it leaves behind is decoded by the first round, or dropped
    engine_auto = {
        "one-language": ([20, 70, 94], {}, {}),
        "two-languages": ([20, 70, 94], {70: "de"}, {}),
        "clips": ([20, 70], {}, {"clip_timestamps": "5,25,40"}),
        "pieces2": ([130], {}, {"pieces": 2}),
        "no-first-window": ([0, 20], {}, {}),
        "words": ([70, 20], {}, {"word_timestamps": True, "word_confidence": True}),
    }
    for name, (seconds, languages, extra) in engine_auto.items():
        model = _model(vocab, max_batch=2, languages=languages)
        audios = [_audio(s) for s in seconds]
        cases["engine-auto-" + name] = _outcome(model, lambda: tr.transcribe_batch(model, audios, language="auto", vocab_path=vocab, **extra))
    model = _model(vocab, max_batch=1)
    cases["engine-auto-transcribe"] = _outcome(model, lambda: tr.transcribe(model, _audio(70), language="auto", vocab_path=vocab))
    model = _model(None, max_batch=2, multilingual=False)   # (the vocabulary file is the multilingual one)
    cases["engine-auto-english-only"] = _outcome(model, lambda: tr.transcribe_batch(model, [_audio(20), _audio(40)], language="auto"))
    model = _model(vocab, max_batch=2)
    cases["no-vocabulary"] = _outcome(model, lambda: tr.transcribe_batch(model, [_audio(40), _audio(20)], language="en", initial_prompt=[7, 8],
                                                                        condition_on_previous_text=False, sample_rate=[16000, 8000]))
    # transcribe(decode_window=...) is wrapped row by row, also where the rows are the pieces of one recording
    model = _model(vocab, max_batch=2)
    decoding = _m("decoding")

    def decode_window(window, prompt):
        (seek, size, _f), = model._rows(window[None])
        model._say("decode_window", window, list(prompt))
        out, sum_logprob, no_speech_prob = model._script(seek, size)
        return decoding.DecodingResult(language="en", tokens=out, text="", avg_logprob=sum_logprob / (len(out) + 1), no_speech_prob=no_speech_prob,
                                       temperature=0.0, compression_ratio=1.0)
    cases["decode-window-pieces2"] = _outcome(model, lambda: tr.transcribe(model, _audio(130), language="en", vocab_path=vocab, pieces=2,
                                                                           decode_window=decode_window))
    return cases


def refusal_cases(vocab):
    """Every refusal fires before any audio is read (the stub sees no call); where a call earns several, the first in the documented order."""
    tr = _m("transcribe")
    ok = dict(language="en", vocab_path=vocab)
    calls = {
        "temperature": dict(ok, temperature=(0.0, 0.2), pieces=2, clip_timestamps="0,5", word_confidence=True),
        "language-none": dict(ok, language=None, pieces=2, clip_timestamps="0,5"),
        "pieces-and-clips": dict(ok, pieces=2, clip_timestamps="0,5", word_confidence=True),
        "confidence-without-words": dict(ok, word_confidence=True, vocab_path=None, pieces=3),
        "words-without-vocabulary": dict(ok, word_timestamps=True, vocab_path=None, pieces=3),
        "pieces-above-max-batch": dict(ok, pieces=3),
        "pieces-zero": dict(ok, pieces=0),
        "pieces-word": dict(ok, pieces="some"),
        "sample-rates": dict(ok, sample_rate=[16000]),
    }
    cases = {}
    for name, kw in calls.items():
        model = _model(vocab, max_batch=2)
        cases["batch-" + name] = _outcome(model, lambda: tr.transcribe_batch(model, [_audio(20), _audio(20)], **kw))
        if name != "sample-rates":
            model = _model(vocab, max_batch=2)
            cases["one-" + name] = _outcome(model, lambda: tr.transcribe(model, _audio(20), **kw))
    model = _model(vocab, max_batch=0)
    cases["max-batch-zero"] = _outcome(model, lambda: tr.transcribe_batch(model, [_audio(20)], **ok))
    model = _model(vocab, max_batch=1)
    cases["language-missing"] = _outcome(model, lambda: tr.transcribe(model, _audio(20), vocab_path=vocab))
    assert all("raises" in c and c["calls"] == [] for c in cases.values()), [n for n, c in cases.items() if "raises" not in c or c["calls"]]
    return cases


TRANSCRIPTS = ["the quick brown fox jumps over the lazy dog near river bank", "pack my box with five dozen liquor jugs and then go home"]


def align_cases(vocab):
    al = _m("align_long")
    cases = {}
    for name, seconds, max_batch in (("two-recordings", [70, 20], 2), ("groups-of-one", [70, 20], 1)):
        model = _model(vocab, max_batch=max_batch, jump_step=20)
        audios = [_audio(s) for s in seconds]
        cases[name] = _outcome(model, lambda: al.force_align_long_batch(model, audios, TRANSCRIPTS, language="en", vocab_path=vocab))
    model = _model(vocab, max_batch=1, jump_step=20)
    cases["one-recording-mean-subword"] = _outcome(model, lambda: al.force_align_long(model, _audio(40), TRANSCRIPTS[0], language="en", vocab_path=vocab,
                                                                                      aggr="mean", aligned_unit_type="subword", sample_rate=8000))
    refused = {"over-long-word": dict(audios=[_audio(20), _audio(20)], texts=[TRANSCRIPTS[0], "a" * 500 + " b"], vocab_path=vocab),
               "no-vocabulary": dict(audios=[_audio(20)], texts=[TRANSCRIPTS[0]], vocab_path=None),
               "texts-and-recordings": dict(audios=[_audio(20)], texts=TRANSCRIPTS, vocab_path=vocab),
               "sample-rates": dict(audios=[_audio(20)], texts=[TRANSCRIPTS[0]], vocab_path=vocab, sample_rate=[8000, 8000])}
    for name, kw in refused.items():
        model = _model(vocab, max_batch=2)
        audios, texts = kw.pop("audios"), kw.pop("texts")
        cases["refused-" + name] = _outcome(model, lambda: al.force_align_long_batch(model, audios, texts, language="en", **kw))
        assert "raises" in cases["refused-" + name] and all(c[0] == "make_opts" for c in model.calls), name   # (no audio read, no GPU work)
    return cases


def _write_wav(path, n):
    data = np.zeros(n, dtype="<i2").tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, 16000, 32000, 2, 16))
        f.write(b"data" + struct.pack("<I", len(data)) + data)


def _written(paths, work):
    """The files a command line wrote: name, key order, and content with the working directory taken out of the paths it holds."""
    out = []
    for p in paths:
        with open(p) as f:
            content = json.load(f)
        for key in ("audio", "text"):
            if isinstance(content.get(key), str) and content[key].startswith(work):   # (transcribe's "text" is the transcript, not a path)
                content[key] = os.path.relpath(content[key], work)
        out.append({"path": os.path.relpath(p, work), "keys": list(content), "content": content})
    return out


def cli_cases(vocab, work):
    tr, al = _m("transcribe"), _m("align_long")
    np.save(os.path.join(work, "rec_a.npy"), _audio(40))
    _write_wav(os.path.join(work, "rec_b.wav"), 16000 * 20)
    scp = os.path.join(work, "list.scp")
    with open(scp, "w") as f:
        f.write("first %s\n%s\n" % (os.path.join(work, "rec_a.npy"), os.path.join(work, "rec_b.wav")))
    cases = {}
    runs = {"transcribe-batch2-words": ["--batch", "2", "--word_timestamps", "--word_confidence"],
            "transcribe-batch1": [],
            "transcribe-batch2-auto-pieces": ["--batch", "2", "--language", "auto", "--pieces", "2"],
            "transcribe-batch1-clips": ["--clip_timestamps", "6,25"]}
    for name, flags in runs.items():
        model = _model(vocab, max_batch=2)
        args = tr.parse_args(["--scp", scp, "--output_dir", os.path.join(work, name), "--random_init", "--vocab", vocab] + flags)
        cases[name] = {"written": _written(tr.main(args, model=model), work), "calls": model.calls}
    for k, text in enumerate(TRANSCRIPTS):
        with open(os.path.join(work, "text_%d.txt" % k), "w", encoding="utf-8") as f:
            f.write(text)
    scp = os.path.join(work, "align.scp")
    with open(scp, "w") as f:
        f.write("%s\t%s\n%s\t%s\n" % (os.path.join(work, "rec_a.npy"), os.path.join(work, "text_0.txt"),
                                      os.path.join(work, "rec_b.wav"), os.path.join(work, "text_1.txt")))
    for name, flags in {"align-batch2": ["--batch", "2"], "align-batch1": []}.items():
        model = _model(vocab, max_batch=2, jump_step=20)
        args = al.parse_args(["--scp", scp, "--output_dir", os.path.join(work, name), "--random_init", "--vocab", vocab] + flags)
        cases[name] = {"written": _written(al.main(args, model=model), work), "calls": model.calls}
    cases["defaults"] = {"transcribe": dict(sorted(vars(tr.parse_args(["--audio", "x.wav", "--output_dir", "out"])).items())),   # (by name: the
                         "align_long": dict(sorted(vars(al.parse_args(["--audio", "x.wav", "--text", "x.txt", "--output_dir", "out",   # order in
                                                                       "--vocab", "v"])).items()))}                                  # --help is free)
    return cases


@contextlib.contextmanager
def one_tokenizer_per_argument_list():
    """Reading the 50257-rank vocabulary takes longer than everything else a case does, and decode builds its tokenizer anew in every
    call: while the cases run, get_tokenizer hands out one (stateless) tokenizer per distinct argument list."""
    holders = [m for m in map(_m, ("tokenizer", "decoding", "transcribe", "align_long")) if hasattr(m, "get_tokenizer")]
    real, made = _m("tokenizer").get_tokenizer, {}

    def get_tokenizer(*args, **kw):
        key = (args, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = real(*args, **kw)
        return made[key]

    for m in holders:
        m.get_tokenizer = get_tokenizer
    try:
        yield
    finally:
        for m in holders:
            m.get_tokenizer = real


def run_all(work):
    """Every case, as the JSON-ready dict the fixture holds. work: an empty directory for the vocabulary and the command lines' files."""
    vocab = write_vocab(os.path.join(work, "fake.tiktoken"))
    with one_tokenizer_per_argument_list(), contextlib.redirect_stdout(io.StringIO()):   # (the command lines print a line per file)
        sections = {"transcribe": transcribe_cases(vocab), "refusals": refusal_cases(vocab), "align_long": align_cases(vocab),
                    "cli": cli_cases(vocab, work)}
    text = json.dumps(describe(sections), separators=(",", ":"))
    assert work not in text, "a case's record depends on the working directory"
    return json.loads(text)


def serialise(record):
    """The string two records are compared by: key order counts, and a NaN equals a NaN."""
    return json.dumps(record, separators=(",", ":"))


PACKED = ("calls", "segments", "windows", "words")   # lists whose entries repeat from case to case


def pack(sections):
    """The fixture's form: every entry of a PACKED list is kept once, in "table", and the lists hold its index there."""
    table, index = [], {}

    def walk(v):
        if isinstance(v, dict):
            return {k: [keep(walk(x)) for x in x_list] if k in PACKED and isinstance(x_list, list) else walk(x_list) for k, x_list in v.items()}
        return [walk(x) for x in v] if isinstance(v, list) else v

    def keep(entry):
        key = serialise(entry)
        if key not in index:
            index[key] = len(table)
            table.append(entry)
        return index[key]

    return {"sections": walk(sections), "table": table}


def unpack(packed):
    table = packed["table"]

    def walk(v):
        if isinstance(v, dict):
            return {k: [walk(table[x]) for x in x_list] if k in PACKED and isinstance(x_list, list) else walk(x_list) for k, x_list in v.items()}
        return [walk(x) for x in v] if isinstance(v, list) else v

    return walk(packed["sections"])


def main():
    with tempfile.TemporaryDirectory() as work:
        sections = run_all(work)
    assert serialise(unpack(pack(sections))) == serialise(sections)
    with open(OUT, "w") as f:
        f.write(serialise(pack(sections)) + "\n")
    print("wrote %s: %d bytes, %s" % (OUT, os.path.getsize(OUT), ", ".join("%d %s cases" % (len(v), k) for k, v in sections.items())))


if __name__ == "__main__":
    main()
