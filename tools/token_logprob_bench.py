#!/usr/bin/env python3
"""Cost of the teacher-token log-probabilities (wca_align_batch_enqueue, vocab_end = eot) on the fused batch path: the bench
workload (whisper-medium dims, seeded random weights, contract mode, B = 64 utterances of 10 s with 64 characters, top-10,
medfilt 3 -- BASELINE.json configs[1]) in ONE process, with and without log-probs in alternating rounds, each round a two-deep
enqueue / fetch pipeline like bench.py's. Prints one JSON line: utt/s of each variant (median over rounds) and the relative cost.
  python tools/token_logprob_bench.py [--rounds 6] [--steps 8] [--batch 64] [--precision reference]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
wca = importlib.import_module("whisper-char-alignment_amd")
syn = importlib.import_module("whisper-char-alignment_amd.synthetic")
tk = importlib.import_module("whisper-char-alignment_amd.tokenizer")
rt = importlib.import_module("whisper-char-alignment_amd.retokenize")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=6)
    p.add_argument("--steps", type=int, default=8, help="batches per timed round")
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--seconds", type=float, default=10.0)
    p.add_argument("--chars", type=int, default=64)
    p.add_argument("--precision", default="reference", choices=["reference", "f16"])
    args = p.parse_args()
    dims = wca.dims_for("medium")
    model = wca.WhisperAMD(dims, device="cuda:0", max_batch=args.batch).load_state_dict(syn.random_state_dict(dims, seed=0, cross_qk_std=0.08))
    model.set_precision(args.precision)
    tok = tk.get_tokenizer(True, language="English")
    n_samples = int(args.seconds * 16000)
    batches = []
    for bi in range(2):
        ids = range(bi * args.batch, (bi + 1) * args.batch)
        pcm = np.stack([syn.synth_audio(u, n_samples) for u in ids])
        toks = [[*tok.sot_sequence, tok.no_timestamps, *rt.encode(syn.synth_text(u, args.chars), tok, "char"), tok.eot] for u in ids]
        n_max = max(len(t) for t in toks)
        tarr = np.full((args.batch, n_max), tok.eot, dtype=np.int64)
        for j, t in enumerate(toks):
            tarr[j, :len(t)] = t
        batches.append((torch.from_numpy(pcm).cuda(), [n_samples] * args.batch, torch.from_numpy(tarr).cuda(), [len(t) for t in toks],
                        [n_samples // 320] * args.batch))
    opts = model.make_opts(aggregation="topk", topk=10, sot_len=len(tok.sot_sequence), medfilt_width=3)

    def run(steps, lp):
        ve = tok.eot if lp else None
        for i in range(steps):
            model.align_batch(*batches[i % 2], opts, enqueue_only=True, token_logprobs_vocab_end=ve)
            if i > 0:
                model.fetch(args.batch, batches[(i - 1) % 2][2].shape[1], opts, with_token_logprobs=lp)
        model.fetch(args.batch, batches[(steps - 1) % 2][2].shape[1], opts, with_token_logprobs=lp)

    for lp in (False, True):   # warm-up: allocations, code objects
        run(2, lp)
    torch.cuda.synchronize()
    rates = {False: [], True: []}
    for r in range(args.rounds):
        for lp in ((False, True) if r % 2 == 0 else (True, False)):
            t0 = time.perf_counter()
            run(args.steps, lp)
            torch.cuda.synchronize()
            rates[lp].append(args.steps * args.batch / (time.perf_counter() - t0))
    off, on = statistics.median(rates[False]), statistics.median(rates[True])
    print(json.dumps({"workload": "medium dims, %s mode, B=%d, %.0f s, %d chars, top-10, medfilt 3" % (args.precision, args.batch, args.seconds, args.chars),
                      "rounds": args.rounds, "steps_per_round": args.steps, "utt_per_s_without": round(off, 2), "utt_per_s_with": round(on, 2),
                      "cost_pct": round(100.0 * (off - on) / off, 2), "rounds_without": [round(x, 2) for x in rates[False]],
                      "rounds_with": [round(x, 2) for x in rates[True]], "gpu": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
