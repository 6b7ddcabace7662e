#!/usr/bin/env python3
"""Cost of one round of align_batch on the character route and on the alignment-heads route, in ONE process: whisper-medium dims, seeded
random weights, B = 16 windows of 30 s (max_frames 1500), each route with the row length it would have in transcribe -- about 300
character tokens against about 60 sub-word tokens (the ids are byte-level stand-ins: only the row length costs) -- in alternating rounds,
median wall time per round (enqueue + fetch, phase 1 included: transcribe aligns on an encoded state, so the difference of the two is
what the route changes). Then the stages of phase 2 between the engine's own device events (wca_set_profiling / wca_last_stage_ms), in
further rounds of the same calls: on the heads route the three passes of csrc/align_heads.hip are what lies between the events of the
head-statistics stage. Beside them, between device events too, a device-to-device copy of the bytes the passes read once (S heads x n_tok
x 1500 frames x 4 B per window). No cache is cleared between repeats. Records a cost; claims no speed-up. Prints one JSON line.
  python tools/align_heads_bench.py [--rounds 7] [--batch 16] [--precision reference]"""
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
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--chars", type=int, default=296, help="text tokens per row on the character route")
    p.add_argument("--subwords", type=int, default=58, help="text tokens per row on the alignment-heads route")
    p.add_argument("--precision", default="reference", choices=["reference", "f16"])
    p.add_argument("--stage_reps", type=int, default=15, help="profiled rounds per route for the stage times")
    args = p.parse_args()
    B = args.batch
    dims = wca.dims_for("medium")
    model = wca.WhisperAMD(dims, device="cuda:0", max_batch=B).load_state_dict(syn.random_state_dict(dims, seed=0, cross_qk_std=0.08))
    model.set_precision(args.precision)
    model.use_official_alignment_heads("medium")
    tok = tk.get_tokenizer(True, language="English")
    n_samples, frames = 480000, 1500
    pcm = torch.from_numpy(np.stack([syn.synth_audio(u, n_samples) for u in range(B)])).cuda()

    def rows(n_text):
        toks = [[*tok.sot_sequence, tok.no_timestamps, *rt.encode(syn.synth_text(u, n_text), tok, "char"), tok.eot] for u in range(B)]
        arr = np.full((B, max(len(t) for t in toks)), tok.eot, dtype=np.int64)
        for j, t in enumerate(toks):
            arr[j, :len(t)] = t
        return torch.from_numpy(arr).cuda(), [len(t) for t in toks]

    sot_len = len(tok.sot_sequence)
    routes = {"char": (rows(args.chars), model.make_opts(aggregation="topk", topk=10, sot_len=sot_len, medfilt_width=3), {}),
              "heads": (rows(args.subwords), model.make_opts(sot_len=sot_len, medfilt_width=7), {"alignment_heads": True})}

    def one_round(name):
        (tokens, n_tok), opts, kw = routes[name]
        return model.align_batch(pcm, [n_samples] * B, tokens, n_tok, [frames] * B, opts, **kw)

    for name in routes:   # warm-up: allocations, code objects
        one_round(name)
        one_round(name)
    torch.cuda.synchronize()
    ms = {name: [] for name in routes}
    for r in range(args.rounds):
        for name in (("char", "heads") if r % 2 == 0 else ("heads", "char")):
            t0 = time.perf_counter()
            one_round(name)
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0))

    # the three passes alone: the engine's own device events around the stages of phase 2 (wca_set_profiling / wca_last_stage_ms), in
    # the fused path itself. On the heads route the three launches sit between the events of the head-statistics stage and nothing
    # between those of the aggregation stage; the DTW stage is the same kernel on both routes, on each route's own rows
    names = {3: "decoder_with_capture", 4: "head_stats_or_three_passes", 5: "topk_and_aggregate", 6: "dtw"}
    model.set_profiling(True)
    stages = {}
    for name in routes:
        runs = []
        for _ in range(args.stage_reps):
            one_round(name)
            runs.append(model.last_stage_ms())
        stages[name] = {label: round(1e3 * statistics.median(r[i] for r in runs), 1) for i, label in names.items()}
    model.set_profiling(False)
    # a device-to-device copy of the bytes the passes read once, between device events as well
    heads = model.flat_heads(model.alignment_heads)
    S, n = len(heads), max(routes["heads"][0][1])
    read = torch.empty(B, S, n, frames, device="cuda", dtype=torch.float32)
    dst = torch.empty_like(read)
    copies = []
    for i in range(5 + args.stage_reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        dst.copy_(read)
        t1.record()
        torch.cuda.synchronize()
        if i >= 5:
            copies.append(1e3 * t0.elapsed_time(t1))
    print(json.dumps({"workload": "medium dims, %s mode, B=%d windows of 30 s, max_frames 1500" % (args.precision, B), "rounds": args.rounds,
                      "char_route": {"text_tokens": args.chars, "top-k": 10, "medfilt": 3, "round_ms_median": round(statistics.median(ms["char"]), 2),
                                     "rounds_ms": [round(x, 2) for x in ms["char"]], "stage_us_median": stages["char"]},
                      "heads_route": {"text_tokens": args.subwords, "heads": S, "medfilt": 7, "round_ms_median": round(statistics.median(ms["heads"]), 2),
                                      "rounds_ms": [round(x, 2) for x in ms["heads"]], "stage_us_median": stages["heads"]},
                      "stage_reps": args.stage_reps, "passes_shape": [B, S, n, frames], "bytes_read_once": int(read.numel() * 4),
                      "three_passes_us": stages["heads"]["head_stats_or_three_passes"],
                      "d2d_copy_of_bytes_read_us": round(statistics.median(copies), 1), "gpu": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
