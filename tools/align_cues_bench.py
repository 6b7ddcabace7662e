"""Cue-anchored forced alignment beside the sequential window loop, in one process:
  1. the windowed DTW kernel (wca_dtw_batch_dev_windows, a diagonal band of +-50 frames) beside the closed one (wca_dtw_batch_dev) at
     N = 443 with M = 1500, P = 1 and P = 16, alternating the two forms in every round, device events around the whole entry point
     with its copies (the windowed call also checks its windows on the host and uploads them);
  2. seconds of audio aligned per second (wall clock around the whole call, log-mel included) of force_align_long and of
     force_align_cues on ONE synthetic recording of --minutes, on the alignment-like planted checkpoint of tools/align_long_bench.py
     (synthetic.aligned_state_dict at whisper-medium's size, max_batch 16). The cues are cut from the sequential result: runs of
     --words-per-cue words, from the first word's start to the last word's end. The two forms alternate for --rounds rounds.

    python tools/align_cues_bench.py [--minutes 10] [--rounds 5] [--model medium] [--precision reference] [--cue-slack 1.0] [--out FILE]

The checkpoint is synthetic: the figures say what the two schedules cost, nothing about quality on speech."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.align_long_bench import byte_vocab, timed  # noqa: E402


def _m(n):
    return importlib.import_module("whisper-char-alignment_amd." + n)


def kernel_leg(eng, rounds, lines, record):
    _lib = _m("_lib")
    pi = C.POINTER(C.c_int32)
    rng = np.random.default_rng(0)
    N, M = 443, 1500
    centre = np.round(np.arange(N) * ((M - 1) / (N - 1))).astype(np.int64)
    lo, hi = np.clip(centre - 50, 0, M - 1).astype(np.int32), np.clip(centre + 50, 0, M - 1).astype(np.int32)
    lo[0], hi[-1] = 0, M - 1
    record["kernel"] = []
    for P in (1, 16):
        md = torch.from_numpy(rng.random((P, N, M), dtype=np.float32)).cuda()
        jf = np.zeros((P, N), np.int32)
        los, his = np.ascontiguousarray(np.tile(lo, (P, 1))), np.ascontiguousarray(np.tile(hi, (P, 1)))

        def closed():
            _lib.check(eng._lib.wca_dtw_batch_dev(eng._h, C.c_void_p(md.data_ptr()), P, N, M, jf.ctypes.data_as(pi)))

        def windowed():
            _lib.check(eng._lib.wca_dtw_batch_dev_windows(eng._h, C.c_void_p(md.data_ptr()), P, N, M, None, None, los.ctypes.data_as(pi),
                                                          his.ctypes.data_as(pi), jf.ctypes.data_as(pi)))

        closed(), windowed()
        torch.cuda.synchronize()
        tc, tw = [], []
        for _ in range(rounds):
            tc.append(timed(closed))
            tw.append(timed(windowed))
        mc, mw = float(np.median(tc)), float(np.median(tw))
        record["kernel"].append({"N": N, "M": M, "P": P, "closed_ms": mc, "windowed_ms": mw, "closed_ms_all": tc, "windowed_ms_all": tw})
        lines.append("DTW N=%d M=%d P=%-2d: closed %7.3f ms | windowed %7.3f ms (x%.2f; rounds closed %s | windowed %s)"
                     % (N, M, P, mc, mw, mw / mc, " ".join("%.3f" % t for t in tc), " ".join("%.3f" % t for t in tw)))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def loop_leg(args, lines, record):
    pkg, syn, al = importlib.import_module("whisper-char-alignment_amd"), _m("synthetic"), _m("align_long")
    dims = _m("engine").dims_for(args.model)
    model = pkg.WhisperAMD(dims, device="cuda:0", max_batch=16, precision=args.precision)
    model.load_state_dict(syn.aligned_state_dict(dims, seed=0, frames_per_token=args.frames_per_unit))
    vocab = args.vocab or byte_vocab(os.path.join(tempfile.mkdtemp(), "bytes.tiktoken"))
    seconds = args.minutes * 60.0
    text = syn.synth_text(100, int(seconds * 50 / args.frames_per_unit * 0.97))   # the text ends a little before the audio
    audio = syn.synth_audio(100, int(seconds * 16000))
    kw = dict(language="en", vocab_path=vocab, topk=10, medfilt_width=3)
    al.force_align_long(model, audio[:16000 * 40], text[:400], **kw)   # warm-up of every kernel shape
    seq = al.force_align_long(model, audio, text, **kw)
    words = [w for w in seq["words"] if w["start"] is not None]
    n = args.words_per_cue
    cues = [(g[0]["start"], g[-1]["end"], "".join(w["word"] for w in g).strip()) for g in (words[k:k + n] for k in range(0, len(words), n))]
    al.force_align_cues(model, audio, cues, cue_slack=args.cue_slack, **kw)   # warm-up of the batched shapes
    ts, tc, out = [], [], None
    for _ in range(args.rounds):
        ts.append(wall(lambda: al.force_align_long(model, audio, text, **kw))[0])
        dt, out = wall(lambda: al.force_align_cues(model, audio, cues, cue_slack=args.cue_slack, **kw))
        tc.append(dt)
    ms, mc = float(np.median(ts)), float(np.median(tc))
    moved = [abs(a["start"] - b["start"]) for a, b in zip(out["words"], words) if a["start"] is not None]
    rec = {"minutes": args.minutes, "cues": len(cues), "words": len(words), "cue_slack": args.cue_slack,
           "sequential": {"seconds": ms, "audio_seconds_per_second": seconds / ms, "windows": len(seq["windows"]), "rounds": len(seq["windows"]),
                          "unaligned_words": seq["unaligned_words"], "seconds_all": ts},
           "cues_form": {"seconds": mc, "audio_seconds_per_second": seconds / mc, "windows": len(out["windows"]),
                         "rounds": -(-len(out["windows"]) // 16), "unaligned_words": out["unaligned_words"], "seconds_all": tc},
           "speedup": ms / mc, "word_start_moved_max_s": max(moved), "word_start_moved_median_s": float(np.median(moved))}
    record["loop"] = rec
    lines.append("%s %s, one %.1f min recording, %d words in %d cues of %d words, slack %.1f s" % (args.model, args.precision, args.minutes, len(words),
                                                                                                 len(cues), n, args.cue_slack))
    lines.append("  force_align_long: %7.3f s wall -> %8.1f s of audio per second (%d windows = %d rounds at batch 1, %d unaligned; rounds %s)"
                 % (ms, seconds / ms, len(seq["windows"]), len(seq["windows"]), seq["unaligned_words"], " ".join("%.3f" % t for t in ts)))
    lines.append("  force_align_cues: %7.3f s wall -> %8.1f s of audio per second (%d windows in %d rounds of up to 16 rows, %d unaligned; rounds %s)"
                 % (mc, seconds / mc, len(out["windows"]), rec["cues_form"]["rounds"], out["unaligned_words"], " ".join("%.3f" % t for t in tc)))
    lines.append("  cues / sequential: x%.2f; word starts moved by at most %.2f s (median %.2f s) against the sequential result"
                 % (ms / mc, rec["word_start_moved_max_s"], rec["word_start_moved_median_s"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--model", type=str, default="medium")
    ap.add_argument("--precision", type=str, default="reference", choices=["reference", "f16"])
    ap.add_argument("--frames-per-unit", type=float, default=5.0)
    ap.add_argument("--words-per-cue", type=int, default=8)
    ap.add_argument("--cue-slack", type=float, default=1.0)
    ap.add_argument("--vocab", type=str, default=None)
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    lines, record = [], {"minutes": args.minutes, "rounds": args.rounds, "model": args.model, "precision": args.precision}
    eng = _m("engine").default_engine(0)
    eng._bind_stream()
    kernel_leg(eng, args.rounds, lines, record)
    if not args.skip_loop:
        loop_leg(args, lines, record)
    lines.append(json.dumps(record))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
