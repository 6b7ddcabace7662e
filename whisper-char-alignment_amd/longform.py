"""What the two long-form drivers share (transcribe.py: long-form transcription, align_long.py: long-form forced alignment), each thing
once: the frame constants, a recording's way to 16 kHz mono, one round's window cut, the padded token matrix, the aligner's options, and
the pieces of the two command lines that are the same. Host Python only: what runs on the GPU is in the drivers' docstrings."""
import os
import re

import numpy as np
import torch

from .audio import HOP_LENGTH, SAMPLE_RATE, load_audio
from .engine import MAX_LENGTH, WhisperAMD, dims_for  # noqa: F401  (MAX_LENGTH: framed tokens per window; the drivers take it from here)

INPUT_STRIDE = 2                                         # mel frames per encoder frame (N_FRAMES // n_audio_ctx)
TIME_PRECISION = INPUT_STRIDE * HOP_LENGTH / SAMPLE_RATE  # 0.02 s per timestamp token step / encoder frame
FRAME_SECONDS = HOP_LENGTH / SAMPLE_RATE                  # 0.01 s per mel frame
FRAMES_PER_SECOND = SAMPLE_RATE // HOP_LENGTH             # 100
ALIGNER_KEYWORDS = ("aligned_unit_type", "aggr", "topk", "medfilt_width", "w_colnorm", "w_rownorm", "w_coverage")   # add_aligner_options' names


def as_pcm(audio, model, sample_rate=SAMPLE_RATE):
    """One recording as 16 kHz mono f32 [n]: a path is read with its own rate and channels (audio.load_audio), an array or tensor
    ([n], or [channels, n]) is taken at `sample_rate`. Anything not at 16 kHz goes through model.resample with its channels (the kernel
    averages them); 16 kHz audio stays on the host and is averaged there."""
    if isinstance(audio, (str, os.PathLike)):
        audio, sample_rate = load_audio(audio)
    if not isinstance(audio, torch.Tensor):
        audio = torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32))
    audio = audio.to(torch.float32)
    if int(sample_rate) != SAMPLE_RATE:
        if audio.dim() not in (1, 2):
            raise ValueError("audio must be one recording [n] or [channels, n]; got shape %s" % (tuple(audio.shape),))
        return model.resample(audio, int(sample_rate))
    if audio.dim() == 2:
        audio = audio.mean(dim=0)
    if audio.dim() != 1:
        raise ValueError("audio must be one mono recording [n]; got shape %s" % (tuple(audio.shape),))
    return audio


def sample_rates(sample_rate, n_recordings):
    """One rate per recording: `sample_rate` is one int for every array / tensor input, or one per recording."""
    rates = [int(r) for r in sample_rate] if isinstance(sample_rate, (list, tuple)) else [int(sample_rate)] * n_recordings
    if len(rates) != n_recordings:
        raise ValueError("sample_rate lists %d rates for %d recordings" % (len(rates), n_recordings))
    return rates


def groups_of(items, n):   # `items` in consecutive groups of at most n
    return [items[g0:g0 + n] for g0 in range(0, len(items), n)]


def cut_windows(model, mels, requests):
    """One round's windows as one batch [B, n_mels, 3000]. requests: (recording, seek, size) per row, a recording's rows side by side;
    mels[recording] is its long log-mel. One mel_window call per recording: its rows are windows of the same long mel. A recording with
    one row is cut with the plain call (a view, no copy), and only several recordings are concatenated."""
    windows = []
    for rec in dict.fromkeys(rec for rec, _, _ in requests):
        mine = [(seek, size) for r, seek, size in requests if r == rec]
        windows.append(model.mel_window(mels[rec], *mine[0])[None] if len(mine) == 1 else
                       model.mel_window(mels[rec], [seek for seek, _ in mine], [size for _, size in mine]))
    return torch.cat(windows) if len(windows) > 1 else windows[0]


def pad_token_rows(rows, eot):
    """Token rows of different lengths as one int64 matrix [len(rows), longest], filled up with `eot` (on the host)."""
    toks = torch.full((len(rows), max(len(r) for r in rows)), eot, dtype=torch.int64)
    for b, r in enumerate(rows):
        toks[b, :len(r)] = torch.tensor(r, dtype=torch.int64)
    return toks


_CUE_TIME = r"(?:(\d+):)?(\d{1,2}):(\d{2})[.,](\d{1,3})"   # [hours:]minutes:seconds, then `,` (SRT) or `.` (WebVTT) and the fraction
_CUE_TIMING = re.compile(r"^\s*" + _CUE_TIME + r"\s*-->\s*" + _CUE_TIME)
_CUE_TAG = re.compile(r"<[^>]*>|\{\\[^}]*\}")   # <i>, </b>, <c.colour>, <00:01.000> (WebVTT); {\an8} (SubStation overrides inside SRT)


def _cue_seconds(h, m, s, frac):
    return int(h or 0) * 3600 + int(m) * 60 + int(s) + int(frac.ljust(3, "0")) / 1000.0


def parse_cues(text):
    """The cues of an SRT or WebVTT file's text as [(start_s, end_s, text)], in file order. A cue is a block of lines (blocks are
    separated by blank lines) with a timing line `start --> end`, `[hh:]mm:ss,mmm` or `[hh:]mm:ss.mmm`; whatever follows the end time on
    that line (WebVTT cue settings) is ignored, as are lines before it (the SRT counter, a WebVTT cue identifier). The lines after it are
    the cue's text: joined with one space, tags like <i> or <c.yellow> and override blocks like {\\an8} removed, white space collapsed.
    Blocks without a timing line -- the WEBVTT header, NOTE, STYLE and REGION blocks -- are skipped; a cue without text is kept (it
    carries no words). No ordering is checked here: force_align_cues does that."""
    cues = []
    for block in re.split(r"\n[ \t]*\n", text.lstrip("\ufeff").replace("\r\n", "\n").replace("\r", "\n")):
        lines = block.strip("\n").split("\n")
        if lines[0].startswith(("WEBVTT", "NOTE", "STYLE", "REGION")):
            continue
        for k, line in enumerate(lines[:2]):   # (the timing line is the first line, or the second after a counter / identifier)
            m = _CUE_TIMING.match(line)
            if m:
                body = " ".join(_CUE_TAG.sub("", ln) for ln in lines[k + 1:])
                cues.append((_cue_seconds(*m.groups()[:4]), _cue_seconds(*m.groups()[4:]), " ".join(body.split())))
                break
    return cues


def read_cues(path):
    """parse_cues of a UTF-8 .srt / .vtt file."""
    with open(path, encoding="utf-8") as f:
        return parse_cues(f.read())


def aligner_options(model, tokenizer, *, aggr="topk", topk=10, medfilt_width=3, w_colnorm=1.0, w_rownorm=1.0, w_coverage=0.0):
    """The engine's options for the paper's aligner on a window whose token row starts with tokenizer.sot_sequence."""
    if aggr == "topk":
        topk = min(int(topk), model.dims.n_text_layer * model.dims.n_text_head)   # filter_attention keeps at most every head (timing.py:13-43)
    return model.make_opts(aggregation=aggr, topk=topk, w_colnorm=w_colnorm, w_rownorm=w_rownorm, w_coverage=w_coverage,
                           sot_len=len(tokenizer.sot_sequence), medfilt_width=medfilt_width, qk_scale=1.0)


# ------------------------------------------------------------------------------------------------ command line
def add_model_options(p):
    p.add_argument("--model", type=str, default="medium")
    p.add_argument("--weights", type=str, default=None, help="local openai-whisper checkpoint (.pt)")
    p.add_argument("--random_init", action="store_true", help="seeded random weights (dry run without a checkpoint)")
    p.add_argument("--forward_precision", type=str, default="reference", choices=["reference", "split", "f16"])
    p.add_argument("--batch", type=int, default=1, help="recordings processed in lock-step (the engine's max_batch)")
    p.add_argument("--sample_rate", type=int, default=SAMPLE_RATE, help="rate of raw .npy arrays ([n] or [channels, n]); audio files carry their own")


def add_aligner_options(p):
    p.add_argument("--medfilt_width", type=int, default=3)
    p.add_argument("--aggr", type=str, default="topk", choices=["mean", "topk"])
    p.add_argument("--topk", type=int, default=10)
    p.add_argument("--aligned_unit_type", type=str, default="char", choices=["subword", "char"])
    p.add_argument("--w_colnorm", type=float, default=1.0)
    p.add_argument("--w_rownorm", type=float, default=1.0)
    p.add_argument("--w_coverage", type=float, default=0.0)


def source(path):
    """A raw array is taken at --sample_rate; a file is read, with its own rate, by as_pcm."""
    return np.load(path) if path.endswith(".npy") else path


def load_model(args, device="cuda:0"):
    if args.weights:
        return WhisperAMD.from_checkpoint(args.weights, device=device, max_batch=max(1, args.batch), name=args.model,
                                          precision=args.forward_precision)
    if args.random_init:
        from .synthetic import random_state_dict
        dims = dims_for(args.model)
        return WhisperAMD(dims, device=device, max_batch=max(1, args.batch),
                          precision=args.forward_precision).load_state_dict(random_state_dict(dims, seed=0))
    raise SystemExit("no weights: pass --weights /local/path/%s.pt (openai-whisper checkpoint; nothing is downloaded by name) "
                     "or --random_init for a dry run" % args.model)
