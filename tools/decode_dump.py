#!/usr/bin/env python3
"""Every result of the greedy decode path on seeded small engines, one file per result, for byte-for-byte comparison (cmp) of two builds
of this tree: a refactor of the decode path runs this in the tree before and in the tree after.

  * uniform decode (greedy_decode: wca_decode with per_row 0): the plain start, and a 12-token prompt with prefill 0 and 1
  * ragged per-row decode (wca_decode with per_row 1) with per-row budgets, in both precision modes
    each fused and unfused, B = 20 at 512-wide dims:
    tokens, n_tokens, sum_logprob, no_speech_prob
  * the same ragged rows with a temperature (0 / 0.4 / 1.0 cycling) and a seed (100 + b) per row, from the input and again with
    redecode=True on the state that decode left
  * grouped decodes (decode_group: wca_decode_group) of the first four of those rows, beside each of the above: beam search with 1, 3 and 5
    beams (20 rows, the engine's limit) and with 3 beams and max_candidates 6; 1 and 4 independent samples per audio, and the 4 again
    with redecode=True; a beam decode of three audios and the align_batch(pcm=None) that takes the state it left. Per case the results,
    n_out, the beam trace, and from decode_state the logits rows and the cache slots the call defines
  * align_batch of a ragged batch of 3 in both precision modes: plain, with teacher-token log-probs, and with open-end rows
    (True, False, True) plus log-probs; each in one call and as enqueue_only=True then fetch
  * get_attentions weights and logits of a ragged batch of 3 in both precision modes (the teacher-forced decoder)
  * transcribe of two synthetic recordings (45 s and 70 s) alone and as a transcribe_batch, word_timestamps=True, on a synthetic vocabulary

usage: decode_dump.py OUTDIR [one-stream]     one-stream: set_overlap(0), for an ordered kernel trace"""
import base64
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
wca = importlib.import_module("whisper-char-alignment_amd")
syn, audio, decoding, tokenizer, tr = (importlib.import_module("whisper-char-alignment_amd." + n)
                                       for n in ("synthetic", "audio", "decoding", "tokenizer", "transcribe"))
out_dir, one_stream = sys.argv[1], len(sys.argv) > 2
os.makedirs(out_dir, exist_ok=True)
tok = tokenizer.get_tokenizer(True, language="en", task="transcribe")


def save(name, arrays, keys=("tokens", "n_tokens", "sum_logprob", "no_speech_prob")):
    for key, a in zip(keys, arrays):
        np.save(os.path.join(out_dir, "%s.%s.npy" % (name, key)), a.cpu().numpy() if isinstance(a, torch.Tensor) else a)


def save_group(name, out, rows, G, beam=False):
    """The results of a decode_group, the beam's trace, and what it left on the device: the logits rows and, of the cache, the slots the call
    defines. Row (b, g) has fed its n_initial tokens and one position per choice after the first, so slots [0, n_initial + choices - 1),
    clamped where a row past its budget stays at slot T_max - 2; the rest of the cache is uninitialised memory."""
    save(name, out + (m.last_no_speech_prob,), keys=("tokens", "n_tokens", "sum_logprob", "n_out", "no_speech_prob"))
    if beam:
        save(name, (m.beam_trace(),), keys=("trace",))
    n_init, T_max, steps = [len(r) for r in rows[0]], out[0].shape[2], m.last_decode_positions()[1] + 1
    logits, cache = m.decode_state(len(n_init) * G, T_max)
    for r in range(len(n_init) * G):
        cache[:, :, r, min(n_init[r // G] + steps - 1, T_max - 1):] = 0
    save(name, (logits, cache), keys=("logits", "cache"))


def initial(n):
    """n initial tokens: the bare sot sequence (n = 3) or [sot_prev, n - 4 prompt tokens, *sot_sequence]; and the position of <|sot|>."""
    sot = list(tok.sot_sequence)
    if n == len(sot):
        return sot, 0
    prompt = [(37 * i) % 5000 + 200 for i in range(n - len(sot) - 1)]
    return [tok.sot_prev] + prompt + sot, 1 + len(prompt)


def fake_vocab(path):
    """A tiktoken-format vocabulary of the right size: the 256 bytes and synthetic 4-letter tokens."""
    ranks, i = dict(tokenizer._byte_ranks()), 0
    while len(ranks) < 50257:
        w = bytes([97 + (i % 26), 97 + (i // 26) % 26, 97 + (i // 676) % 26, 97 + (i // 17576) % 26])
        i += 1
        ranks.setdefault(w, len(ranks))
    with open(path, "wb") as f:
        for tokb, r in sorted(ranks.items(), key=lambda kv: kv[1]):
            f.write(base64.b64encode(tokb) + b" " + str(r).encode() + b"\n")
    return path


B = 20
dims = wca.ModelDimensions(80, 1500, 512, 8, 2, 51865, 448, 512, 8, 2)
m = wca.WhisperAMD(dims, device="cuda:0", max_batch=B, precision="f16")
m.load_state_dict(syn.random_state_dict(dims, seed=11))
if one_stream:
    m.set_overlap(0)
mel = torch.stack([audio.log_mel_spectrogram(audio.pad_or_trim(torch.from_numpy(syn.synth_audio(s, n_samples=32000))), 80, model=m)
                   for s in range(40, 40 + B)]).cuda()
sup, blank = decoding.filter_masks(tok, decoding.DecodingOptions(language="en"), dims.n_vocab)
kw = dict(eot=tok.eot, timestamp_begin=tok.timestamp_begin, apply_timestamp_rules=True, max_initial_timestamp_index=50, no_speech=tok.no_speech)
plans = [initial(3 if p == 0 else 4 + p) for p in [(0, 7, 30, 101)[b % 4] for b in range(B)]]
budgets = [10 - b % 4 for b in range(B)]
att_rows = [[*tok.sot_sequence, tok.no_timestamps, *[300 + 7 * i for i in range(n)], tok.eot] for n in (9, 4, 6)]
att_tokens = torch.full((3, max(len(r) for r in att_rows)), tok.eot, dtype=torch.int64)
for b, r in enumerate(att_rows):
    att_tokens[b, :len(r)] = torch.tensor(r)
align_pcm = torch.from_numpy(np.stack([syn.synth_audio(s, n_samples=32000) for s in range(40, 43)])).cuda()
align_ns = [32000, 25600, 19200]
align_opts = m.make_opts("topk", topk=4, sot_len=len(tok.sot_sequence), medfilt_width=3)

for precision in ("f16", "reference"):
    m.set_precision(precision)
    for fused in (True, False):
        m.set_decode_mode(fused)
        tag = "%s.%s" % (precision, "fused" if fused else "unfused")
        for name, n, prefill in (("plain", 3, 0), ("prompt.prefill0", 12, 0), ("prompt.prefill1", 12, 1)) if precision == "f16" else ():
            init, sot_index = initial(n)
            out = m.greedy_decode(mel, None, None, init, sup, blank, sample_len=10, sot_index=sot_index, prefill=prefill, **kw)
            save("uniform.%s.%s" % (name, tag), out + (m.last_no_speech_prob,))
        out = m.greedy_decode_rows(mel, None, None, [p[0] for p in plans], [p[1] for p in plans], budgets, sup, blank, **kw)
        save("rows.%s" % tag, out + (m.last_no_speech_prob,))
        # temperature sampling on the same ragged rows, then once more on the state that decode left (no encoder pass)
        skw = dict(temperature=[(0.0, 0.4, 1.0)[b % 3] for b in range(B)], seed=[100 + b for b in range(B)], **kw)
        out = m.decode_rows_sampled(mel, None, None, [p[0] for p in plans], [p[1] for p in plans], budgets, sup, blank, **skw)
        save("sampled.%s" % tag, out + (m.last_no_speech_prob,))
        out = m.decode_rows_sampled(None, None, None, [p[0] for p in plans], [p[1] for p in plans], budgets, sup, blank, batch=B, redecode=True,
                                    **skw)
        save("sampled.redecode.%s" % tag, out + (m.last_no_speech_prob,))
        # grouped decodes of the first four audios (3, 11, 34 and 105 initial tokens, budgets 10, 9, 8, 7: the stop test runs at choices 4, 8)
        grows = ([p[0] for p in plans[:4]], [p[1] for p in plans[:4]], budgets[:4], sup, blank)
        for G, MC in ((1, None), (3, None), (5, None), (3, 6)):
            out = m.decode_group(mel[:4], None, None, *grows, n_group=G, mode=0, max_candidates=MC, **kw)
            save_group("beam.g%d%s.%s" % (G, ".mc%d" % MC if MC else "", tag), out, grows, G, beam=True)
        gkw = dict(mode=1, temperature=[0.0, 0.4, 1.0, 0.4], seed=[100 + b for b in range(4)], **kw)
        for G in (1, 4):
            save_group("samples.g%d.%s" % (G, tag), m.decode_group(mel[:4], None, None, *grows, n_group=G, **gkw), grows, G)
        out = m.decode_group(None, None, None, *grows, n_group=4, batch=4, redecode=True, **gkw)
        save_group("samples.g4.redecode.%s" % tag, out, grows, 4)
        # the state a beam decode leaves is the one the alignment takes (transcribe)
        arows = ([p[0] for p in plans[:3]], [p[1] for p in plans[:3]], budgets[:3], sup, blank)
        save_group("beam.b3.%s" % tag, m.decode_group(mel[:3], None, None, *arows, n_group=3, mode=0, **kw), arows, 3, beam=True)
        save("beam.b3.align.%s" % tag, m.align_batch(None, None, att_tokens.cuda(), [len(r) for r in att_rows], [100, 80, 60], align_opts),
             keys=("jump", "sel"))
    m.set_decode_mode(True)
    # the fused alignment at B = 3: plain, with teacher-token log-probs, with open-end rows; each in one call and as enqueue then fetch
    for name, akw, fkw in (("plain", {}, {}), ("logprobs", dict(token_logprobs_vocab_end=tok.eot), dict(with_token_logprobs=True)),
                           ("open", dict(token_logprobs_vocab_end=tok.eot, open_end=[True, False, True]),
                            dict(with_token_logprobs=True, with_end_rows=True))):
        keys = ("jump", "sel") + (("token_logprobs",) if "with_token_logprobs" in fkw else ()) + (("end_rows", "scores") if "open_end" in akw else ())
        args = (align_pcm, align_ns, att_tokens.cuda(), [len(r) for r in att_rows], [100, 80, 60], align_opts)
        save("align.%s.%s" % (name, precision), m.align_batch(*args, **akw), keys=keys)
        m.align_batch(*args, enqueue_only=True, **akw)
        save("align.%s.fetch.%s" % (name, precision), m.fetch(3, att_tokens.shape[1], align_opts, **fkw), keys=keys)
    save("attentions.%s" % precision, m.get_attentions(mel[:3], att_tokens, [100, 80, 60], 3, 1.0, n_tok=[len(r) for r in att_rows]),
         keys=("weights", "logits"))

m.set_precision("f16")
vocab = fake_vocab(os.path.join(out_dir, "fake.tiktoken"))
recordings = [syn.synth_audio(30 + i, 16000 * s + 40 * i) for i, s in enumerate((45, 70))]
tkw = dict(language="en", vocab_path=vocab, word_timestamps=True)
results = {"alone%d" % i: tr.transcribe(m, a, **tkw) for i, a in enumerate(recordings)}
results.update(("batch%d" % i, r) for i, r in enumerate(tr.transcribe_batch(m, recordings, **tkw)))
for name, res in results.items():
    with open(os.path.join(out_dir, "transcribe.%s.json" % name), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
torch.cuda.synchronize()
print("decode_dump: %d files in %s" % (len(os.listdir(out_dir)), out_dir))
