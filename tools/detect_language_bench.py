#!/usr/bin/env python3
"""Language identification (wca_detect_language) at whisper-medium dimensions with synthetic weights: ms per detection at batch 1, 8
and max_batch, beside encode_batch alone on the same inputs (so what the one decoder position and the language head add is
visible), and detection followed by a decode of the state it left against that decode alone (the pair costs ONE encoder pass).
usage: detect_language_bench.py [max_batch] [rounds]      (WCA_MODEL=medium by default; prints one JSON line at the end)"""
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
decoding = importlib.import_module("whisper-char-alignment_amd.decoding")
tok_mod = importlib.import_module("whisper-char-alignment_amd.tokenizer")

max_batch = int(sys.argv[1]) if len(sys.argv) > 1 else 32
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
SAMPLE_LEN = 16
model_name = os.environ.get("WCA_MODEL", "medium")
dims = wca.dims_for(model_name)
m = wca.WhisperAMD(dims, max_batch=max_batch, precision="f16")
m.load_state_dict(syn.random_state_dict(dims, seed=0))
tok = tok_mod.get_tokenizer(True, num_languages=m.num_languages)
opts = decoding.DecodingOptions(language="en", sample_len=SAMPLE_LEN, suppress_tokens="")
pcm = torch.from_numpy(np.stack([syn.synth_audio(b, 160000) for b in range(max_batch)])).cuda()
mel_all = m.log_mel(pcm)
lang = dict(sot=tok.sot, lang_begin=tok.all_language_tokens[0], n_lang=len(tok.all_language_tokens))


def timed(fn):
    ms = []
    for r in range(rounds + 1):
        torch.cuda.synchronize()
        m.synchronize()
        t0 = time.perf_counter()
        fn()
        m.synchronize()
        torch.cuda.synchronize()
        if r > 0:  # round 0 warms up (buffer growth, first launches)
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


results = {"model": model_name, "rounds": rounds, "sample_len": SAMPLE_LEN, "batches": {}}
for B in sorted({1, min(8, max_batch), max_batch}):
    mel = mel_all[:B].contiguous()

    def encode_alone():   # the encoder pass alone; the state is then drained outside the clock
        m.encode_batch(mel=mel)

    enc_ms = []
    for r in range(rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        encode_alone()
        m.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        decoding.decode(m, None, opts, encoded_batch=B, want_text=False)
        if r > 0:
            enc_ms.append(dt)
    enc = float(np.median(enc_ms))

    det_ms = []
    for r in range(rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.detect_language(mel, **lang)
        dt = (time.perf_counter() - t0) * 1e3
        decoding.decode(m, None, opts, encoded_batch=B, want_text=False)
        if r > 0:
            det_ms.append(dt)
    det = float(np.median(det_ms))

    pair = timed(lambda: (m.detect_language(mel, **lang), decoding.decode(m, None, opts, encoded_batch=B, want_text=False)))
    alone = timed(lambda: decoding.decode(m, mel, opts, want_text=False))
    twice = timed(lambda: (m.detect_language(mel, **lang), decoding.decode(m, mel, opts, want_text=False)))
    row = {"encode_ms": round(enc, 3), "detect_ms": round(det, 3), "step_and_head_ms": round(det - enc, 3), "decode_alone_ms": round(alone, 3),
           "detect_then_decode_ms": round(pair, 3), "detect_then_reencode_decode_ms": round(twice, 3)}
    results["batches"][B] = row
    print("B %3d: encode_batch %8.3f ms | detect_language %8.3f ms (+%.3f for the step and the head) | decode alone %8.3f ms, detect + decode of "
          "its state %8.3f ms (+%.3f), detect + decode with a second encoder pass %8.3f ms" %
          (B, enc, det, det - enc, alone, pair, pair - alone, twice), flush=True)
print(json.dumps(results))
