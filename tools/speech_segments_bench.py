"""Speech segments of a long recording (wca_speech_segments, one call: its kernels, the copy of the result and the synchronise) next to two
reference points in the same process: the whole-recording log-mel it reads (wca_log_mel_long) and a device-to-device copy of the mel's
content bytes (the least any pass over the mel costs). Host-clock times around a device synchronise, the three alternating in every round.

    python tools/speech_segments_bench.py [--minutes 60] [--rounds 7] [--out profiles/speech_segments_bench.txt]

The recording is synthetic: gated noise (synthetic.synth_audio) with a stretch of digital silence in every minute, so that the detector
has segments to find. The expectation to hold the result against: the call costs less than the log-mel, because it reads once what the
other computes. Which kernel takes the time is a question for a kernel trace of this script (rocprofv3 --kernel-trace --stats)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--n-mels", type=int, default=80, choices=[80, 128])
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    pkg = importlib.import_module("whisper-char-alignment_amd")
    syn = importlib.import_module("whisper-char-alignment_amd.synthetic")
    n = int(args.minutes * 60 * 16000)
    x = syn.synth_audio(0, n)
    for start in range(20 * 16000, n, 60 * 16000):   # 15 s of digital silence in every minute
        x[start:start + 15 * 16000] = 0.0
    pcm = torch.from_numpy(x).cuda()
    n_vocab = 51866 if args.n_mels == 128 else 51865
    eng = pkg.WhisperAMD(pkg.ModelDimensions(args.n_mels, 1500, 128, 2, 1, n_vocab, 448, 128, 2, 1), device="cuda:0", max_batch=1, precision="f16")
    mel = eng.log_mel_long(pcm)
    cf = mel.shape[1] - 3000
    content = mel[:, :cf]
    spare = torch.empty_like(content)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t)

    runs = {"wca_speech_segments": lambda: eng.speech_segments(mel), "wca_log_mel_long": lambda: eng.log_mel_long(pcm),
            "device copy of the content": lambda: spare.copy_(content)}
    for fn in runs.values():   # warm-up of every shape
        fn()
    times = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            times[k].append(timed(fn))
    segs, stats = eng.speech_segments(mel)
    med = {k: float(np.median(v)) for k, v in times.items()}
    lines = ["%.1f min, %d mel rows, %d content frames (%.1f MB of mel), %d segments, stats %s; %d rounds, median ms (all rounds)" % (
        args.minutes, args.n_mels, cf, 4e-6 * args.n_mels * cf, len(segs), stats, args.rounds)]
    for k in runs:
        lines.append("%-28s %9.3f ms   (%s)" % (k, med[k], " ".join("%.3f" % t for t in times[k])))
    ratio = med["wca_speech_segments"] / med["wca_log_mel_long"]
    lines.append("speech segments / log-mel = %.3f: the call costs %s than the log-mel it reads" % (ratio, "less" if ratio < 1 else "MORE"))
    lines.append(json.dumps({"minutes": args.minutes, "n_mels": args.n_mels, "content_frames": cf, "n_segments": len(segs), "stats": stats,
                             "median_ms": med, "all_ms": times}))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
