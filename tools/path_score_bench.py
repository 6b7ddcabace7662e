#!/usr/bin/env python3
"""Cost of the per-row path scores (wca_align_desc.path_scores) on the fused batch path: the bench workload (whisper-medium dims, seeded
random weights, contract mode, B = 64 utterances of 10 s with 64 characters, top-10, medfilt 3 -- BASELINE.json configs[1]) in ONE
process, with and without path scores in alternating rounds, each round a two-deep enqueue / fetch pipeline like bench.py's. Then the
kernel alone beside the DTW: the synchronous step calls wca_dtw_batch_dev_open and wca_dtw_path_scores (the same DTW launch, plus the score
kernel, one memset and two more copies to the host) on B problems of the workload's shape, median wall time per call.
Prints one JSON line.
  python tools/path_score_bench.py [--rounds 6] [--steps 8] [--batch 64] [--precision reference]"""
import argparse
import ctypes as C
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
    p.add_argument("--kernel_reps", type=int, default=200)
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

    def run(steps, ps):
        for i in range(steps):
            model.align_batch(*batches[i % 2], opts, enqueue_only=True, path_scores=ps)
            if i > 0:
                model.fetch(args.batch, batches[(i - 1) % 2][2].shape[1], opts, with_path_scores=ps)
        return model.fetch(args.batch, batches[(steps - 1) % 2][2].shape[1], opts, with_path_scores=ps)

    for ps in (False, True):   # warm-up: allocations, code objects
        last = run(2, ps)
    torch.cuda.synchronize()
    mean_score = float(np.sum(last[2] * last[3], dtype=np.float64) / max(int(last[3].sum()), 1))
    rates = {False: [], True: []}
    for r in range(args.rounds):
        for ps in ((False, True) if r % 2 == 0 else (True, False)):
            t0 = time.perf_counter()
            run(args.steps, ps)
            torch.cuda.synchronize()
            rates[ps].append(args.steps * args.batch / (time.perf_counter() - t0))
    off, on = statistics.median(rates[False]), statistics.median(rates[True])

    # the kernel alone: the workload's DTW shape (text rows x encoder frames), B problems, column-normalised like the aggregated maps
    N, M = max(batches[0][3]) - len(tok.sot_sequence) - 1, n_samples // 320
    m = np.random.default_rng(0).random((args.batch, N, M), dtype=np.float32)
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    md = torch.from_numpy(m).cuda()
    flags = wca._lib.i32_array([0] * args.batch)
    pi, pf = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    jump, end = np.zeros((args.batch, N), np.int32), np.zeros(args.batch, np.int32)
    mean, cells = np.zeros((args.batch, N), np.float32), np.zeros((args.batch, N), np.int32)
    model._bind_stream()
    lib, h, ptr = model._lib, model._h, C.c_void_p(md.data_ptr())

    def dtw_only():
        wca._lib.check(lib.wca_dtw_batch_dev_open(h, ptr, args.batch, N, M, None, None, flags, jump.ctypes.data_as(pi), end.ctypes.data_as(pi), None))

    def dtw_scores():
        wca._lib.check(lib.wca_dtw_path_scores(h, ptr, args.batch, N, M, None, None, flags, jump.ctypes.data_as(pi), end.ctypes.data_as(pi),
                                               mean.ctypes.data_as(pf), cells.ctypes.data_as(pi)))

    times = {}
    for name, fn in (("dtw", dtw_only), ("dtw_and_scores", dtw_scores)):
        for _ in range(5):
            fn()
        ts = []
        for _ in range(args.kernel_reps):
            t0 = time.perf_counter()
            fn()
            ts.append(1e6 * (time.perf_counter() - t0))
        times[name] = statistics.median(ts)
    print(json.dumps({"workload": "medium dims, %s mode, B=%d, %.0f s, %d chars, top-10, medfilt 3" % (args.precision, args.batch, args.seconds, args.chars),
                      "rounds": args.rounds, "steps_per_round": args.steps, "utt_per_s_without": round(off, 2), "utt_per_s_with": round(on, 2),
                      "cost_pct": round(100.0 * (off - on) / off, 2), "rounds_without": [round(x, 2) for x in rates[False]],
                      "rounds_with": [round(x, 2) for x in rates[True]], "mean_cell_score_random_weights": round(mean_score, 4),
                      "step_call_shape": [args.batch, N, M], "step_call_dtw_us": round(times["dtw"], 1),
                      "step_call_dtw_and_scores_us": round(times["dtw_and_scores"], 1),
                      "score_kernel_memset_and_copies_us": round(times["dtw_and_scores"] - times["dtw"], 1), "gpu": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
