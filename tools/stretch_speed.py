#!/usr/bin/env python
"""Speed of the bundle builder's device work (csrc/stretch.hip and what follows it): every version of ONE 5-minute 44.1 kHz
track that `python -m beat_this_amd.preprocess` makes with its defaults (--pitch_shift -5:6 --time_stretch 20:4: the track, 11
pitch shifts, 10 tempo changes), from the mono 44.1 kHz signal in host memory (its upload included) to the float16
spectrograms on the device.
Timed with device events around the whole set, median of 7 runs after one warm-up; the pitch shifts, the tempo changes and the
bare stretch kernels are also timed on their own.  Prints one JSON line.  There is no gate: the numbers go into DESIGN.md.

    python tools/stretch_speed.py [--seconds 300] [--runs 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from beat_this_amd import preprocess as PP  # noqa: E402
from beat_this_amd.dataset.augment import precomputed_augmentation_filenames  # noqa: E402
from beat_this_amd.preprocessing import stretch_length  # noqa: E402


def timed(fn, runs):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()
    sr = PP.AUG_SR
    n = int(args.seconds * sr)
    rng = np.random.default_rng(0)
    t = np.arange(n) / sr
    x = sum(a * np.sin(2 * np.pi * f * t) for f, a in ((220.3, 0.3), (1333.1, 0.2), (5120.7, 0.1))) + 0.01 * rng.standard_normal(n)
    x[::22050] += 0.3
    pre = PP.Preprocessor.__new__(PP.Preprocessor)           # (the device part only: no data directory)
    pre.device = torch.device("cuda:0")
    pre.logmel = PP.LogMelSpect(device=pre.device)
    names = precomputed_augmentation_filenames(PP.augmentations_of((-5, 6), (20, 4)))
    pitch = [m for m in names if PP.variant_of(m)[0] == "pitch"]
    tempo = [m for m in names if PP.variant_of(m)[0] == "tempo"]
    sig = x.astype(np.float32)
    d = torch.from_numpy(sig).to(pre.device)
    res = {"seconds": args.seconds, "versions": len(names), "runs": args.runs,
           "all_ms": timed(lambda: pre.spectrograms(sig, sr, names), args.runs),
           "pitch_ms": timed(lambda: pre.spectrograms(sig, sr, pitch), args.runs),
           "tempo_ms": timed(lambda: pre.spectrograms(sig, sr, tempo), args.runs),
           "stretch_L1.25_ms": timed(lambda: stretch_length(d, 1.25), args.runs),
           "stretch_L0.8333_ms": timed(lambda: stretch_length(d, 1 / 1.2), args.runs)}
    res["audio_seconds_per_second"] = args.seconds * len(names) / (res["all_ms"] * 1e-3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
