"""Long-form forced alignment, measured with device events:
  1. the open-end DTW kernel (wca_dtw_batch_dev_open, every problem open) beside the closed one (wca_dtw_batch_dev) at the same shapes,
     N = 443 with M = 1500 and N = 200 with M = 750, P = 1 and P = 64, alternating the two forms in every round. Both calls copy their
     results to the host; the open one also uploads its flags and brings back end rows and scores.
  2. seconds of audio aligned per second (wall clock around force_align_long / force_align_long_batch, log-mel included) for one synthetic
     recording of --minutes, and for lock-step batches of 4 and 16 such recordings, on the alignment-like planted checkpoint
     (synthetic.aligned_state_dict: a ridge at --frames-per-unit encoder frames per text unit in every window, so an interior window holds
     about 1500 / frames-per-unit units of the run it is offered and the loop advances by almost a whole window).

    python tools/align_long_bench.py [--minutes 10] [--rounds 7] [--model medium] [--precision reference] [--vocab FILE] [--out FILE]

Without --vocab a byte-level vocabulary of the right size is written to a temporary file (the transcript is lower-case ASCII)."""
import argparse
import base64
import ctypes as C
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _m(n):
    return importlib.import_module("whisper-char-alignment_amd." + n)


def byte_vocab(path):
    ranks = dict(_m("tokenizer")._byte_ranks())
    i = 0
    while len(ranks) < 50257:
        w = bytes([97 + (i % 26), 97 + (i // 26) % 26, 97 + (i // 676) % 26, 97 + (i // 17576) % 26])
        i += 1
        if w not in ranks:
            ranks[w] = len(ranks)
    with open(path, "wb") as f:
        for tokb, r in sorted(ranks.items(), key=lambda kv: kv[1]):
            f.write(base64.b64encode(tokb) + b" " + str(r).encode() + b"\n")
    return path


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def kernel_leg(eng, rounds, lines, record):
    _lib = _m("_lib")
    pi = C.POINTER(C.c_int32)
    rng = np.random.default_rng(0)
    record["kernel"] = []
    for N, M in ((443, 1500), (200, 750)):
        for P in (1, 64):
            md = torch.from_numpy(rng.random((P, N, M), dtype=np.float32)).cuda()
            jf, er, sc = np.zeros((P, N), np.int32), np.zeros(P, np.int32), np.zeros(P, np.float32)
            flags = _lib.i32_array([1] * P)

            def closed():
                _lib.check(eng._lib.wca_dtw_batch_dev(eng._h, C.c_void_p(md.data_ptr()), P, N, M, jf.ctypes.data_as(pi)))

            def opened():
                _lib.check(eng._lib.wca_dtw_batch_dev_open(eng._h, C.c_void_p(md.data_ptr()), P, N, M, None, None, flags, jf.ctypes.data_as(pi),
                                                           er.ctypes.data_as(pi), sc.ctypes.data_as(C.POINTER(C.c_float))))

            closed(), opened()
            torch.cuda.synchronize()
            tc, to = [], []
            for _ in range(rounds):
                tc.append(timed(closed))
                to.append(timed(opened))
            mc, mo = float(np.median(tc)), float(np.median(to))
            record["kernel"].append({"N": N, "M": M, "P": P, "closed_ms": mc, "open_ms": mo, "closed_ms_all": tc, "open_ms_all": to})
            lines.append("DTW N=%d M=%d P=%-2d: closed %7.3f ms | open-end %7.3f ms (x%.2f; rounds closed %s | open %s)"
                         % (N, M, P, mc, mo, mo / mc, " ".join("%.3f" % t for t in tc), " ".join("%.3f" % t for t in to)))


def loop_leg(args, lines, record):
    pkg, syn, al = importlib.import_module("whisper-char-alignment_amd"), _m("synthetic"), _m("align_long")
    dims = _m("engine").dims_for(args.model)
    model = pkg.WhisperAMD(dims, device="cuda:0", max_batch=16, precision=args.precision)
    model.load_state_dict(syn.aligned_state_dict(dims, seed=0, frames_per_token=args.frames_per_unit))
    vocab = args.vocab or byte_vocab(os.path.join(tempfile.mkdtemp(), "bytes.tiktoken"))
    seconds = args.minutes * 60.0
    n_units = int(seconds * 50 / args.frames_per_unit * 0.97)   # the text ends a little before the audio
    texts = [syn.synth_text(100 + i, n_units) for i in range(16)]
    audios = [syn.synth_audio(100 + i, int(seconds * 16000)) for i in range(16)]
    kw = dict(language="en", vocab_path=vocab, topk=10, medfilt_width=3)
    al.force_align_long(model, audios[0][:16000 * 40], texts[0][:400], **kw)   # warm-up of every kernel shape
    record["loop"] = []
    for B in (1, 4, 16):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = al.force_align_long_batch(model, audios[:B], texts[:B], **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        windows = sum(len(o["windows"]) for o in out)
        unaligned = sum(o["unaligned_words"] for o in out)
        words = sum(len(o["words"]) for o in out)
        rec = {"batch": B, "minutes_each": args.minutes, "seconds": dt, "audio_seconds_per_second": B * seconds / dt, "windows": windows,
               "words": words, "unaligned_words": unaligned, "windows_without_words": sum(o["windows_without_words"] for o in out)}
        record["loop"].append(rec)
        lines.append("loop %s %s, %2d x %.1f min: %7.2f s wall -> %8.1f s of audio per second (%d windows, %d words, %d unaligned, %d windows "
                     "without words)" % (args.model, args.precision, B, args.minutes, dt, rec["audio_seconds_per_second"], windows, words, unaligned,
                                         rec["windows_without_words"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--model", type=str, default="medium")
    ap.add_argument("--precision", type=str, default="reference", choices=["reference", "f16"])
    ap.add_argument("--frames-per-unit", type=float, default=5.0)
    ap.add_argument("--vocab", type=str, default=None)
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    lines, record = [], {"minutes": args.minutes, "rounds": args.rounds, "model": args.model, "precision": args.precision}
    eng = _m("engine").default_engine(0)
    eng._bind_stream()
    kernel_leg(eng, args.rounds, lines, record)
    if not args.skip_loop:
        loop_leg(args, lines, record)
    lines.append(json.dumps(record))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
