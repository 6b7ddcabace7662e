#!/usr/bin/env python3
"""Beam search (wca_decode_group) beside the greedy decode at whisper-medium dimensions: ms per decoded position with the encoder state
already queued (wca_encode_batch), so that only the prefill and the KV-cached loop are timed -- tools/decode_bench.py's method: a host
clock around a synchronous call, one warm-up round, then `rounds` timed ones.
usage: beam_bench.py [sample_len] [rounds]
For B in {1, 4} audios: the greedy per-row decode (the form the beam is built on: one batched prefill, then the table kernels) and beam
sizes 2 and 5 on B x G decoder rows. EOT is suppressed, so every run makes exactly sample_len choices and no list ever fills.
The cache reorder (kv_reorder) is timed on its own through wca_test_kv_reorder at the loop's shapes and mean key count, with device events
over `reps` back-to-back launches, beside a device-to-device copy of the same bytes (torch's copy_ of an equally large f16 buffer):
achieved bytes/s counts every kept element once read and once written, and the reorder's share of a decoded position is its launch time over
the loop's ms per position (the first choice only broadcasts, so sample_len - 1 of sample_len positions reorder).
Reading each audio's cross-K/V G times per step (the grouped one-query attention) is part of the beam's ms per position, not separated."""
import ctypes as C
import importlib
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
wca = importlib.import_module("whisper-char-alignment_amd")
syn = importlib.import_module("whisper-char-alignment_amd.synthetic")
tok_mod = importlib.import_module("whisper-char-alignment_amd.tokenizer")
_lib = importlib.import_module("whisper-char-alignment_amd._lib")

sample_len = int(sys.argv[1]) if len(sys.argv) > 1 else 64
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
BATCHES, BEAMS, REPS = (1, 4), (2, 5), 50
model_name = os.environ.get("WCA_MODEL", "medium")
dims = wca.dims_for(model_name)
m = wca.WhisperAMD(dims, max_batch=max(BATCHES) * max(BEAMS), precision="f16")
m.load_state_dict(syn.random_state_dict(dims, seed=0, cross_qk_std=0.08))
tok = tok_mod.get_tokenizer(True, language="en")
initial = list(tok.sot_sequence)
sup = np.zeros(dims.n_vocab, np.uint8)
sup[tok.eot] = 1  # never finish early: every round makes exactly sample_len choices
sup[tok.no_timestamps] = 1
kw = dict(eot=tok.eot, timestamp_begin=tok.timestamp_begin, apply_timestamp_rules=True, max_initial_timestamp_index=50)
T_max = len(initial) + sample_len
L, d = dims.n_text_layer, dims.n_text_state


def vp(t):
    return C.c_void_p(t.data_ptr())


def time_decode(B, G):
    pcm = torch.from_numpy(np.stack([syn.synth_audio(b, 160000) for b in range(B)])).cuda()
    ns = np.full(B, 160000, np.int32)
    best = []
    for r in range(rounds + 1):
        m.encode_batch(pcm=pcm, n_samples=ns)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if G == 0:
            m.greedy_decode_rows(None, None, None, [initial] * B, [0] * B, [sample_len] * B, sup, None, batch=B, **kw)
        else:
            m.decode_group(None, None, None, [initial] * B, [0] * B, [sample_len] * B, sup, None, batch=B, n_group=G, mode=0, **kw)
        torch.cuda.synchronize()
        if r:   # round 0 warms up
            best.append((time.perf_counter() - t0) * 1e3 / sample_len)
    return best


def time_reorder(R):
    """(ms per kv_reorder launch, ms per device-to-device copy of the same bytes, bytes moved per launch) at the loop's mean key count."""
    n_keep = len(initial) + sample_len // 2
    src = torch.zeros((2 * L, R, T_max, d), dtype=torch.float16, device="cuda")
    dst = torch.zeros_like(src)
    idx = torch.tensor([(r // 2) * 2 for r in range(R)], dtype=torch.int32, device="cuda")   # half the rows continue a neighbour's beam
    keep = torch.full((R,), n_keep, dtype=torch.int32, device="cuda")
    flat_src = torch.zeros(2 * L * R * n_keep * d, dtype=torch.float16, device="cuda")
    flat_dst = torch.zeros_like(flat_src)
    m._bind_stream()
    out = []
    for fn in (lambda: _lib.check(m._lib.wca_test_kv_reorder(m._h, vp(src), vp(dst), 2 * L, R, R, T_max, d, vp(idx), 1, vp(keep))),
               lambda: flat_dst.copy_(flat_src)):
        for _ in range(5):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / REPS)
    return out[0], out[1], 2 * flat_src.numel() * 2


print("beam_bench: %s, sample_len %d (T_max %d), %d timed rounds after one warm-up; ms per decoded position = call time / sample_len"
      % (model_name, sample_len, T_max, rounds), flush=True)
for B in BATCHES:
    greedy = time_decode(B, 0)
    print("B=%d greedy (per-row form, %d rows):      %s  median %.3f ms per position" % (B, B, " ".join("%.3f" % v for v in greedy), float(np.median(greedy))),
          flush=True)
    for G in BEAMS:
        beam = time_decode(B, G)
        reorder_ms, copy_ms, nbytes = time_reorder(B * G)
        med = float(np.median(beam))
        print("B=%d beam_size=%d (%d rows):                %s  median %.3f ms per position (%.2fx greedy)"
              % (B, G, B * G, " ".join("%.3f" % v for v in beam), med, med / float(np.median(greedy))), flush=True)
        print("    kv_reorder at %d keys: %.4f ms per launch = %.1f %% of a position; %.0f GB/s (read + write of %.1f MB) beside %.4f ms = %.0f GB/s for "
              "a device-to-device copy of the same bytes"
              % (len(initial) + sample_len // 2, reorder_ms, 100.0 * reorder_ms * (sample_len - 1) / sample_len / med, nbytes / reorder_ms / 1e6,
                 nbytes / 1e6, copy_ms, nbytes / copy_ms / 1e6), flush=True)
