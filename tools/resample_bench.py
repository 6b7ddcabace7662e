"""The resampler to 16 kHz (wca_resample_16k) on one hour of audio at 48 kHz mono, 44.1 kHz mono and 44.1 kHz stereo, next to a
device-to-device copy (torch.Tensor.copy_) that moves the same number of bytes: device-event times, alternating the two in every round.

    python tools/resample_bench.py [--minutes 60] [--rounds 7] [--out FILE]

Bytes are what the algorithm needs: 4 (C n_in + n_out), every input sample read once and every output written once. The copy reads half
of that and writes half of it. What the kernel pays on top of the copy is the halo of every tile (n_taps samples per 2048 outputs), the
trip through LDS and n_taps multiply-adds per output."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    pkg = importlib.import_module("whisper-char-alignment_amd")
    audio = importlib.import_module("whisper-char-alignment_amd.audio")
    eng = pkg.WhisperAMD(pkg.ModelDimensions(80, 1500, 128, 2, 1, 51865, 448, 128, 2, 1), device="cuda:0", max_batch=1, precision="f16")
    lines, record = [], {"minutes": args.minutes, "rounds": args.rounds, "settings": []}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for sr_in, channels in ((48000, 1), (44100, 1), (44100, 2)):
        n_in = int(args.minutes * 60 * sr_in)
        L, M, W, n_taps = audio.resample_plan(sr_in)
        n_out = -(-n_in * L // M)
        gen = torch.Generator(device="cuda").manual_seed(sr_in + channels)
        pcm = torch.rand(channels, n_in, device="cuda", generator=gen) * 2 - 1
        nbytes = 4 * (channels * n_in + n_out)
        src = torch.empty(nbytes // 8, device="cuda", dtype=torch.float32).normal_()   # read nbytes / 2, write nbytes / 2
        dst = torch.empty_like(src)

        def resample():
            return eng.resample(pcm, sr_in)

        def copy():
            return dst.copy_(src)

        out = resample()
        copy()   # warm-up of both
        torch.cuda.synchronize()
        assert out.shape == (n_out,) and bool(torch.isfinite(out).all())
        t_rs, t_cp = [], []
        for _ in range(args.rounds):
            t_rs.append(timed(resample))   # (includes the allocation of the output tensor from torch's caching allocator)
            t_cp.append(timed(copy))
        mr, mc = float(np.median(t_rs)), float(np.median(t_cp))
        gr, gc = nbytes / mr * 1e-6, nbytes / mc * 1e-6
        record["settings"].append({"sr_in": sr_in, "channels": channels, "n_in": n_in, "n_out": n_out, "bytes": nbytes, "resample_ms": mr,
                                   "resample_ms_all": t_rs, "resample_GBps": gr, "copy_ms": mc, "copy_ms_all": t_cp, "copy_GBps": gc,
                                   "fraction_of_copy": gr / gc})
        lines.append("%6d Hz x %d, %.1f min (%d -> %d samples, %.1f MB): wca_resample_16k %7.3f ms = %7.1f GB/s (rounds %s) | copy_ of the same "
                     "bytes %7.3f ms = %7.1f GB/s (rounds %s) | %.2f of the copy" % (
                         sr_in, channels, args.minutes, n_in, n_out, nbytes * 1e-6, mr, gr, " ".join("%.3f" % t for t in t_rs), mc, gc,
                         " ".join("%.3f" % t for t in t_cp), gr / gc))
        del pcm, src, dst, out
    lines.append(json.dumps(record))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
