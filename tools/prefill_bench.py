#!/usr/bin/env python3
"""Prompted greedy decode (wca_decode) at the bench's model / batch: time from the start of the decode to the first
sampled token, initial tokens fed one position at a time (prefill 0) against the batched prefill (prefill 1), for several
initial-token counts, in both precision modes; then a full prompted decode both ways. The encoder state is queued and
finished before each timed call (wca_encode_batch), so only the decoder is timed.
usage: prefill_bench.py [B] [rounds]      (WCA_MODEL=medium by default; prints one JSON line at the end)"""
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
wca = importlib.import_module("whisper-char-alignment_amd")
syn = importlib.import_module("whisper-char-alignment_amd.synthetic")
tok_mod = importlib.import_module("whisper-char-alignment_amd.tokenizer")

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
N_INITIAL = (3, 4, 35, 131, 227)
FULL_N, FULL_SAMPLE = 131, 64
model_name = os.environ.get("WCA_MODEL", "medium")
dims = wca.dims_for(model_name)
m = wca.WhisperAMD(dims, max_batch=B, precision="f16")
m.load_state_dict(syn.random_state_dict(dims, seed=0, cross_qk_std=0.08))
tok = tok_mod.get_tokenizer(True, language="en")
sup = np.zeros(dims.n_vocab, np.uint8)
sup[tok.eot] = 1  # never finish early: a full decode runs exactly sample_len steps
sup[tok.no_timestamps] = 1
pcm = torch.from_numpy(np.stack([syn.synth_audio(b, 160000) for b in range(B)])).cuda()
ns = np.full(B, 160000, np.int32)
kw = dict(eot=tok.eot, timestamp_begin=tok.timestamp_begin, apply_timestamp_rules=True, max_initial_timestamp_index=50,
          no_speech=tok.no_speech)


def initial_tokens(n):
    """n = 3: the plain start; 4: sot sequence + <|notimestamps|>; more: [sot_prev] + (n - 4) prompt tokens + sot sequence."""
    if n == 3:
        return list(tok.sot_sequence), 0
    if n == 4:
        return list(tok.sot_sequence) + [tok.no_timestamps], 0
    prompt = [(97 * i) % 20000 + 300 for i in range(n - 4)]
    return [tok.sot_prev] + prompt + list(tok.sot_sequence), n - 3


def timed(initial, sot_index, prefill, sample_len):
    ms = []
    for r in range(rounds + 1):
        m.encode_batch(pcm=pcm, n_samples=ns)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m.greedy_decode(None, None, None, initial, sup, None, batch=B, sample_len=sample_len, sot_index=sot_index, prefill=prefill, **kw)
        torch.cuda.synchronize()
        if r > 0:  # round 0 warms up (buffer growth, first launches)
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), out


results = {"model": model_name, "batch": B, "rounds": rounds}
for precision in ("f16", "reference"):
    m.set_precision(precision)
    rows = {}
    for n in N_INITIAL:
        initial, sot_index = initial_tokens(n)
        step_ms, a = timed(initial, sot_index, 0, 1)
        pre_ms, b = timed(initial, sot_index, 1, 1)
        same = float(np.mean(a[0][:, n] == b[0][:, n]))
        rows[n] = {"stepwise_ms": round(step_ms, 2), "prefill_ms": round(pre_ms, 2), "speedup": round(step_ms / pre_ms, 2),
                   "first_token_agree": same}
        print("%-9s n_initial %3d: first token after %8.2f ms stepwise, %7.2f ms prefill (x%.1f); first tokens agree in %.0f %% of rows"
              % (precision, n, step_ms, pre_ms, step_ms / pre_ms, 100 * same), flush=True)
    initial, sot_index = initial_tokens(FULL_N)
    step_ms, a = timed(initial, sot_index, 0, FULL_SAMPLE)
    pre_ms, b = timed(initial, sot_index, 1, FULL_SAMPLE)
    rows["full"] = {"n_initial": FULL_N, "sample_len": FULL_SAMPLE, "stepwise_ms": round(step_ms, 2), "prefill_ms": round(pre_ms, 2),
                    "speedup": round(step_ms / pre_ms, 2)}
    print("%-9s full decode, n_initial %d + %d sampled: %8.2f ms stepwise, %8.2f ms prefill (x%.2f)"
          % (precision, FULL_N, FULL_SAMPLE, step_ms, pre_ms, step_ms / pre_ms), flush=True)
    results[precision] = rows
print(json.dumps(results))
