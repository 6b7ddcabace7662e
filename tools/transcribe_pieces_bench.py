#!/usr/bin/env python3
"""Long-form transcription of ONE recording, window after window against cut into pieces that are decoded side by side
(transcribe.transcribe(pieces=N): cuts at quiet frames, wca_quiet_cuts; one decode batch of up to N rows per round).

Seeded random weights at whisper-medium dimensions, one synthetic recording of --minutes, condition_on_previous_text=True. The same
recording is transcribed with every --pieces value on one engine of max_batch = the largest value; pieces=1 is the plain call without the
keyword, the path every recording took before. Every setting is warmed once untimed, then timed over --rounds passes whose order rotates,
with a device synchronise inside the timed region; the median is reported as seconds of audio per second of wall clock, with the decoded
windows and the windows per round (decode call). With random weights the decoder emits noise, so the number of windows is whatever the seek
rules make of it, and it differs a little between settings (every piece ends in a short window of its own).
--parent-transcribe PATH times the transcribe() of another revision of transcribe.py (loaded beside this package's, on the same engine)
in the same rotation: the parent commit's host loop against this one's pieces=1, with the spread of the repeated pieces=1 runs beside it.
  usage: transcribe_pieces_bench.py [--pieces 1,4,8,16] [--minutes 10] [--sample-len 64] [--rounds 5] [--out profiles/transcribe_pieces_bench.txt]"""
import argparse
import importlib
import importlib.util
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
wca = importlib.import_module("whisper-char-alignment_amd")
syn = importlib.import_module("whisper-char-alignment_amd.synthetic")
tr = importlib.import_module("whisper-char-alignment_amd.transcribe")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--pieces", type=str, default="1,4,8,16")
    p.add_argument("--minutes", type=float, default=10.0)
    p.add_argument("--sample-len", type=int, default=64)
    p.add_argument("--rounds", type=int, default=5, help="timed passes over all settings (order rotated); the median is reported")
    p.add_argument("--model", type=str, default="medium")
    p.add_argument("--precision", type=str, default="f16", choices=["f16", "reference"])
    p.add_argument("--parent-transcribe", type=str, default=None, help="another revision's transcribe.py, timed in the same rotation")
    p.add_argument("--out", type=str, default=None, help="also write the report to this file")
    args = p.parse_args()
    settings = [int(v) for v in args.pieces.split(",")]
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dims = wca.dims_for(args.model)
    model = wca.WhisperAMD(dims, max_batch=max(settings), precision=args.precision)
    model.load_state_dict(syn.random_state_dict(dims, seed=0, cross_qk_std=0.08))
    seconds = int(60 * args.minutes)
    audio = torch.from_numpy(syn.synth_audio(700, 16000 * seconds))
    kw = dict(language="en", condition_on_previous_text=True, sample_len=args.sample_len)
    say("%s dims, %s forward, one recording of %d s, sample_len %d, max_batch %d, %d timed rounds" % (
        args.model, model.precision, seconds, args.sample_len, model.max_batch, args.rounds))

    runs = {}
    for n in settings:
        runs["pieces=%d" % n] = (lambda n=n: tr.transcribe(model, audio, **kw) if n == 1 else tr.transcribe(model, audio, pieces=n, **kw))
    if args.parent_transcribe:
        spec = importlib.util.spec_from_file_location(wca.__name__ + "._parent_transcribe", args.parent_transcribe)
        parent = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = parent
        spec.loader.exec_module(parent)
        runs["parent"] = lambda: parent.transcribe(model, audio, **kw)
    names = list(runs)

    # warm-up, untimed: every setting once on the whole recording with a prompt of the maximum length, so that the engine's grow-only
    # buffers (KV cache, logits, per-row tables) reach their final size for that row count before anything is timed
    long_prompt = [300 + (7 * i) % 4000 for i in range(dims.n_text_ctx // 2 - 1)]
    for n in settings:
        tr.transcribe(model, audio, initial_prompt=long_prompt, **({"pieces": n} if n > 1 else {}), **kw)
    torch.cuda.synchronize()
    times, shape = {name: [] for name in names}, {}
    for rnd in range(args.rounds):
        order = names[rnd % len(names):] + names[:rnd % len(names)]
        for name in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = runs[name]()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            times[name].append(dt)
            per_piece = {}
            for w in res["windows"]:
                per_piece[w.get("piece", 0)] = per_piece.get(w.get("piece", 0), 0) + 1
            shape[name] = (len(res["windows"]), max(per_piece.values()), len(res.get("pieces", [0])))
            say("  round %d %-10s %7.3f s (%d windows in %d rounds)" % (rnd, name + ":", dt, shape[name][0], shape[name][1]))
    base = float(np.median(times[names[0]]))
    for name in names:
        dt = float(np.median(times[name]))
        windows, rounds, n = shape[name]
        say("%-10s median %7.3f s of %d (min %.3f, max %.3f)  %8.1f s of audio per second  %d windows in %d rounds = %.2f windows per round, "
            "%d piece(s)  (%.2fx %s)" % (name + ":", dt, len(times[name]), min(times[name]), max(times[name]), seconds / dt, windows, rounds,
                                         windows / rounds, n, base / dt, names[0]))
    if "parent" in times and "pieces=1" in times:
        a, b = times["pieces=1"], times["parent"]
        say("pieces=1 against the parent's transcribe(): medians %.3f / %.3f s, gap %+.3f s; spread of the repeated pieces=1 runs %.3f s "
            "(parent's %.3f s)" % (np.median(a), np.median(b), np.median(a) - np.median(b), max(a) - min(a), max(b) - min(b)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
