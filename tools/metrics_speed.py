#!/usr/bin/env python
"""Timing of the beat-tracking metrics (beat_this_amd/metrics.py, csrc/metrics.hip) on two workloads:

  gtzan: 1000 tracks of 30 s, about 60 beats and 15 downbeats each (truth with jitter, predictions with jitter, dropouts and
         insertions), scored as the evaluator does: beats and downbeats, trimmed at 5 s;
  long:  100 tracks of 300 s (about 600 beats each).

    python tools/metrics_speed.py [--reps 10] [--oracle-tracks 50] [--extended] [--json out.json]

Prints one JSON line: per workload, the device call (one bt_beat_metrics on inputs already on the device, beats and downbeats
each, CUDA events, median of --reps), beat_metrics_many end to end (upload, call, copy back), bt_beat_metrics_host on one
thread, and the numpy oracle (tests/metrics_reference.py, which has mir_eval's loops) timed on --oracle-tracks tracks and
scaled to the whole workload.  With --extended the same four legs for the rest of mir_eval.beat (goto, p_score,
information_gain) join them under ext_* keys: one bt_beat_metrics_ext alone, beat_metrics_many(extended=True) end to end (both
device calls), bt_beat_metrics_ext_host on one thread, and tests/metrics_ext_reference.py."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TH = (0.07, 0.04, 0.175, 0.175)
EXT = (0.35, 0.2, 0.2, 0.2, 41)


def workload(n, dur, seed):
    """n tracks of dur seconds -> [(truth beats, pred beats)], [(truth downbeats, pred downbeats)]"""
    rng = np.random.default_rng(seed)
    beats, downs = [], []
    for _ in range(n):
        period = 60 / rng.uniform(80, 160)
        t = np.arange(rng.uniform(0, period), dur, period) + rng.normal(0, 0.01, 1)
        t = np.sort(np.clip(t + rng.normal(0, 0.005, t.size), 0, None))
        p = t + rng.normal(0, 0.02, t.size)
        p = p[rng.random(p.size) > 0.05]
        p = np.sort(np.clip(np.concatenate([p, rng.uniform(0, dur, rng.integers(0, 4))]), 0, None))
        beats.append((t, p))
        downs.append((t[::4].copy(), p[::4].copy()))
    return beats, downs


def csr(pairs, side):
    arrs = [p[side] for p in pairs]
    off = np.zeros(len(arrs) + 1, np.int64)
    off[1:] = np.cumsum([a.size for a in arrs])
    return np.concatenate(arrs + [np.zeros(1)]), off


def time_device(pairs, reps, extended=False):
    from beat_this_amd import _lib

    dev = torch.device("cuda")
    ref, roff = csr(pairs, 0)
    est, eoff = csr(pairs, 1)
    t = {k: torch.from_numpy(v).to(dev) for k, v in dict(ref=ref, roff=roff, est=est, eoff=eoff).items()}
    n = len(pairs)
    L = _lib.lib()
    wsb = (L.bt_beat_metrics_ext_workspace_bytes if extended else L.bt_beat_metrics_workspace_bytes)(
        n, int(roff[-1]), int(eoff[-1]))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    out = torch.empty((n, 12), dtype=torch.float64, device=dev)
    st = _lib.stream_ptr(dev)

    def call():
        fn, args = (L.bt_beat_metrics_ext, EXT) if extended else (L.bt_beat_metrics, TH)
        _lib.check(fn(st, t["ref"].data_ptr(), t["roff"].data_ptr(), t["est"].data_ptr(), t["eoff"].data_ptr(), n, 5.0, *args,
                      ws.data_ptr(), wsb, out.data_ptr()))

    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def time_many(pairs, reps, extended=False):
    from beat_this_amd.metrics import beat_metrics_many

    beat_metrics_many([p[0] for p in pairs], [p[1] for p in pairs], extended=extended)
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        beat_metrics_many([p[0] for p in pairs], [p[1] for p in pairs], extended=extended)
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def time_host(pairs, reps, extended=False):
    from beat_this_amd import _lib

    ref, roff = csr(pairs, 0)
    est, eoff = csr(pairs, 1)
    out = np.zeros((len(pairs), 12))
    ms = []
    for _ in range(max(1, reps // 2)):
        t0 = time.perf_counter()
        fn, args = (_lib.lib().bt_beat_metrics_ext_host, EXT) if extended else (_lib.lib().bt_beat_metrics_host, TH)
        _lib.check(fn(ref.ctypes.data, roff.ctypes.data, est.ctypes.data, eoff.ctypes.data, len(pairs), 5.0, *args,
                      out.ctypes.data))
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def time_oracle(pairs, k, extended=False):
    import metrics_ext_reference as X
    import metrics_reference as R

    row = X.row_ext if extended else R.row
    sub = pairs[:k]
    t0 = time.perf_counter()
    for r, e in sub:
        row(r, e, 5.0)
    return (time.perf_counter() - t0) * 1e3 / len(sub) * len(pairs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--oracle-tracks", type=int, default=50)
    ap.add_argument("--extended", action="store_true", help="also time goto, p_score and information_gain (ext_* keys)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0)}
    for name, n, dur in (("gtzan", 1000, 30.0), ("long", 100, 300.0)):
        beats, downs = workload(n, dur, seed=1 if name == "gtzan" else 2)
        r = {"tracks": n, "beats_per_track": float(np.mean([p[0].size for p in beats]))}
        for target, pairs in (("beat", beats), ("downbeat", downs)):
            med, best = time_device(pairs, args.reps)
            r[f"device_ms_{target}"] = round(med, 4)
            r[f"device_min_ms_{target}"] = round(best, 4)
            r[f"many_ms_{target}"] = round(time_many(pairs, args.reps), 3)
            r[f"host_1thread_ms_{target}"] = round(time_host(pairs, args.reps), 3)
            r[f"oracle_ms_{target}"] = round(time_oracle(pairs, min(args.oracle_tracks, n)), 1)
            if args.extended:
                med, best = time_device(pairs, args.reps, True)
                r[f"ext_device_ms_{target}"] = round(med, 4)
                r[f"ext_device_min_ms_{target}"] = round(best, 4)
                r[f"ext_many_ms_{target}"] = round(time_many(pairs, args.reps, True), 3)
                r[f"ext_host_1thread_ms_{target}"] = round(time_host(pairs, args.reps, True), 3)
                r[f"ext_oracle_ms_{target}"] = round(time_oracle(pairs, min(args.oracle_tracks, n), True), 1)
        res[name] = r
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
