#!/usr/bin/env python3
"""Greedy ASR pre-pass (wca_decode) at the bench's model / batch: ms per autoregressive step with the encoder state
already queued (wca_encode_batch), so that only the KV-cached loop is timed.
usage: decode_bench.py [B] [sample_len] [rounds] [--temperature T] [--seed S]
--temperature T (with --seed S, default 0): the same rows through wca_decode with temperature_host / seed_host at temperature T, row b with seed S + b. That is the
per-row form (the prompt goes through one batched prefill, not position by position), so its base line is --temperature 0, which runs the
same per-row form greedily; without --temperature the loop is the uniform form (per_row 0) as before.
Environment: WCA_DEC_MODES=0,1 (default): separate launches, then the fused few-row GEMMs (wca_set_decode_mode)."""
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

argv, named = [], {"--temperature": None, "--seed": 0}
for a in sys.argv[1:]:
    if argv and argv[-1] in named:
        named[argv.pop()] = float(a)
    else:
        argv.append(a)
temperature, seed = named["--temperature"], int(named["--seed"])
B = int(argv[0]) if len(argv) > 0 else 64
sample_len = int(argv[1]) if len(argv) > 1 else 64
rounds = int(argv[2]) if len(argv) > 2 else 3
model_name = os.environ.get("WCA_MODEL", "medium")
dims = wca.dims_for(model_name)
m = wca.WhisperAMD(dims, max_batch=B, precision="f16")
m.load_state_dict(syn.random_state_dict(dims, seed=0, cross_qk_std=0.08))
tok = tok_mod.get_tokenizer(True, language="en")
initial = list(tok.sot_sequence)
sup = np.zeros(dims.n_vocab, np.uint8)
sup[tok.eot] = 1  # never finish early: every round runs exactly sample_len steps
sup[tok.no_timestamps] = 1
pcm = torch.from_numpy(np.stack([syn.synth_audio(b, 160000) for b in range(B)])).cuda()
ns = np.full(B, 160000, np.int32)
kw = dict(sample_len=sample_len, eot=tok.eot, timestamp_begin=tok.timestamp_begin, apply_timestamp_rules=True,
          max_initial_timestamp_index=50)
for fused in [bool(int(x)) for x in os.environ.get("WCA_DEC_MODES", "0,1").split(",")]:   # fused few-row GEMMs (1) / separate launches (0)
  m.set_decode_mode(fused)
  print("decode mode: fused=%s" % fused, flush=True)
  for r in range(rounds + 1):
    m.encode_batch(pcm=pcm, n_samples=ns)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if temperature is None:
      toks, n_tok, lp = m.greedy_decode(None, None, None, initial, sup, None, batch=B, **kw)
    else:
      toks, n_tok, lp = m.decode_rows_sampled(None, None, None, [initial] * B, [0] * B, [sample_len] * B, sup, None, batch=B,
                                              temperature=[temperature] * B, seed=[seed + b for b in range(B)],
                                              **{k: v for k, v in kw.items() if k != "sample_len"})
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    steps = len(initial) - 1 + sample_len  # the prompt is fed position by position through the same step
    if temperature is not None:
      steps = sample_len                   # one prefill forward over the prompt, then sample_len - 1 steps
    print("  round %d: B=%d %s%s  %.1f ms for %d sampled tokens (+%d prompt positions)  -> %.3f ms per position, %.0f utt/s decode-only"
          % (r, B, model_name, "" if temperature is None else " T=%g (rows form)" % temperature, dt * 1e3, sample_len, len(initial), dt * 1e3 / steps, B / dt), flush=True)
  print("  tokens[0][:12] =", toks[0][:12].tolist(), " n_tok[0] =", int(n_tok[0]))
