"""Whole-recording log-mel (wca_log_mel_long, one call) next to the 30 s entry point called once per 30 s piece (wca_log_mel, batch 1)
on the same samples: device-event times, alternating the two forms in every round, both precision modes.

    python tools/logmel_long_bench.py [--minutes 60] [--rounds 5] [--out FILE]

The two do not compute the same thing (one floor over the recording against one per piece; zero padding after the recording against
reflection at every 30 s cut): this measures the cost of the front end, not a replacement of one by the other."""
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    pkg = importlib.import_module("whisper-char-alignment_amd")
    syn = importlib.import_module("whisper-char-alignment_amd.synthetic")
    n = int(args.minutes * 60 * 16000)
    pieces = (n + 479999) // 480000
    pcm = torch.from_numpy(syn.synth_audio(0, n)).cuda()
    eng = pkg.WhisperAMD(pkg.ModelDimensions(80, 1500, 128, 2, 1, 51865, 448, 128, 2, 1), device="cuda:0", max_batch=1, precision="f16")
    lines, record = [], {"minutes": args.minutes, "samples": n, "pieces": pieces, "rounds": args.rounds}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def long_form():
        return eng.log_mel_long(pcm)

    def piecewise():
        return [eng.log_mel(pcm[i * 480000:(i + 1) * 480000]) for i in range(pieces)]

    for mode in ("f16", "reference"):
        eng.set_precision(mode)
        long_form(), piecewise()   # warm-up of both shapes
        torch.cuda.synchronize()
        t_long, t_piece = [], []
        for _ in range(args.rounds):
            t_long.append(timed(long_form))
            t_piece.append(timed(piecewise))
        frames_long, frames_piece = (n + 480000) // 160, pieces * 3000
        ml, mp = float(np.median(t_long)), float(np.median(t_piece))
        record[mode] = {"long_ms": ml, "long_ms_all": t_long, "piecewise_ms": mp, "piecewise_ms_all": t_piece,
                        "long_us_per_frame": 1e3 * ml / frames_long, "piecewise_us_per_frame": 1e3 * mp / frames_piece}
        lines.append("%-9s %.1f min: wca_log_mel_long %8.2f ms (%d frames, %.3f us/frame; rounds %s) | %d x wca_log_mel %8.2f ms (%d frames, "
                     "%.3f us/frame; rounds %s)" % (mode, args.minutes, ml, frames_long, 1e3 * ml / frames_long,
                                                    " ".join("%.1f" % t for t in t_long), pieces, mp, frames_piece, 1e3 * mp / frames_piece,
                                                    " ".join("%.1f" % t for t in t_piece)))
    lines.append(json.dumps(record))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
