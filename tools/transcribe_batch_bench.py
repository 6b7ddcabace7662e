#!/usr/bin/env python3
"""Long-form transcription throughput, one recording at a time against several in lock-step (transcribe.transcribe_batch).

Seeded random weights at whisper-medium dimensions, synthetic recordings of 2-5 minutes, condition_on_previous_text=True (every
window is decoded with the recording's own previous text as its prompt, so the rows of a batch sit at different decoder positions:
wca_decode with per_row 1). For every --batch value the same recordings are transcribed; batch 1 is N sequential transcribe() calls,
the path a `--scp` list took before transcribe_batch existed. Every batch size is warmed once untimed, then timed over --rounds
passes whose order rotates; the median is reported as recordings/s and decoded windows/s per batch size.
With random weights the decoder emits noise, so the number of windows per recording is whatever the seek rules make of it; it is
printed, and it is the same work for every batch size up to argmax near-ties.
  usage: transcribe_batch_bench.py [--batch 1,4,8,16] [--recordings 16] [--minutes 2,5] [--sample-len 64] [--rounds 3] [--model medium]"""
import argparse
import importlib
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
    p.add_argument("--batch", type=str, default="1,4,8,16")
    p.add_argument("--recordings", type=int, default=16)
    p.add_argument("--minutes", type=str, default="2,5", help="shortest,longest recording")
    p.add_argument("--sample-len", type=int, default=64)
    p.add_argument("--rounds", type=int, default=3, help="timed passes over all batch sizes (order rotated); the median is reported")
    p.add_argument("--budget-seconds", type=float, default=1e9, help="start no further round once this much time has been spent timing")
    p.add_argument("--model", type=str, default="medium")
    p.add_argument("--precision", type=str, default="f16", choices=["f16", "reference"])
    args = p.parse_args()
    batches = [int(b) for b in args.batch.split(",")]
    lo, hi = (float(v) for v in args.minutes.split(","))
    dims = wca.dims_for(args.model)
    model = wca.WhisperAMD(dims, max_batch=max(batches), precision=args.precision)
    model.load_state_dict(syn.random_state_dict(dims, seed=0, cross_qk_std=0.08))
    rng = np.random.default_rng(0)
    seconds = [int(60 * (lo + (hi - lo) * rng.random())) for _ in range(args.recordings)]
    audios = [torch.from_numpy(syn.synth_audio(500 + i, 16000 * s)) for i, s in enumerate(seconds)]
    kw = dict(language="en", condition_on_previous_text=True, sample_len=args.sample_len)
    print("%s dims, %s forward, %d recordings of %d-%d s (%.1f min of audio), sample_len %d" % (
        args.model, model.precision, len(audios), min(seconds), max(seconds), sum(seconds) / 60.0, args.sample_len), flush=True)

    def run(B):
        if B == 1:
            return [tr.transcribe(model, a, **kw) for a in audios]
        out = []
        for g0 in range(0, len(audios), B):   # groups of B recordings, as transcribe_batch forms them on an engine with max_batch = B
            out += tr.transcribe_batch(model, audios[g0:g0 + B], **kw)
        return out

    # warm-up, untimed: every batch size once on 40 s clips with a prompt of the maximum length, so that the engine's grow-only
    # buffers (KV cache, logits, per-row tables, encoder scratch) reach their final size for that batch size before anything is timed
    clips = [a[:16000 * 40] for a in audios]
    long_prompt = [300 + (7 * i) % 4000 for i in range(dims.n_text_ctx // 2 - 1)]
    for B in batches:
        if B == 1:
            tr.transcribe(model, clips[0], initial_prompt=long_prompt, **kw)
        else:
            tr.transcribe_batch(model, clips[:B], initial_prompt=long_prompt, **kw)
    torch.cuda.synchronize()
    # timed: `rounds` passes over all batch sizes, the order rotated every round so that no size always runs first (clock / thermal drift)
    times = {B: [] for B in batches}
    windows = {}
    t_start = time.perf_counter()
    for rnd in range(args.rounds):
        if rnd > 0 and time.perf_counter() - t_start > args.budget_seconds:
            print("stopping after %d round(s): the time budget of %.0f s is used" % (rnd, args.budget_seconds), flush=True)
            break
        order = batches[rnd % len(batches):] + batches[:rnd % len(batches)]
        for B in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            results = run(B)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            times[B].append(dt)
            windows[B] = sum(len(r["windows"]) for r in results)
            print("  round %d batch %2d: %7.2f s (%d windows)" % (rnd, B, dt, windows[B]), flush=True)
    base = float(np.median(times[batches[0]]))
    for B in batches:
        dt = float(np.median(times[B]))
        print("batch %2d: median %7.2f s of %d (min %.2f, max %.2f)  %6.3f recordings/s  %7.2f windows/s  (%d windows, %.2fx batch %d)" % (
            B, dt, len(times[B]), min(times[B]), max(times[B]), len(audios) / dt, windows[B] / dt, windows[B], base / dt, batches[0]), flush=True)


if __name__ == "__main__":
    main()
