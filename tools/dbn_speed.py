#!/usr/bin/env python
"""Timing of the DBN post-processor (Postprocessor(type="dbn"), csrc/dbn.hip) on the bench's batch: 6 tracks of 300 s
(15000 frames at 50 fps each) of pulse-train logits with noise.

    python tools/dbn_speed.py [--reps 10] [--oracle-tracks 1] [--json out.json]

Prints, as one JSON line: the device decode of all 6 tracks (one bt_dbn_decode = three launches, CUDA events, median),
the same decode end to end through Postprocessor.ragged (including the device-to-host copy), bt_dbn_host for the
6 tracks on a 16-thread pool, and the numpy oracle (tests/dbn_reference.py) per track."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def tracks(n=6, T=15000):
    out = []
    for k in range(n):
        rng = np.random.default_rng(100 + k)
        period = 60 * 50 / (90 + 15 * k)
        beat = rng.normal(size=T) * 1.5 - 4
        down = rng.normal(size=T) * 1.5 - 5
        for i, f in enumerate(np.arange(5, T, period).astype(int)):
            beat[f] += 8
            if i % 4 == 0:
                down[f] += 8
        out.append((torch.from_numpy(beat).float(), torch.from_numpy(down).float()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--oracle-tracks", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import ctypes as C

    from beat_this_amd import _lib
    from beat_this_amd.postprocessor import Postprocessor

    pp = Postprocessor(type="dbn")
    tr = tracks()
    res = dict(tracks=len(tr), frames_per_track=len(tr[0][0]))
    lens = [len(t[0]) for t in tr]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    if torch.cuda.is_available():
        dev = torch.device("cuda:0")
        beat = torch.cat([t[0] for t in tr]).to(dev)
        down = torch.cat([t[1] for t in tr]).to(dev)
        total, n = int(off[-1]), len(tr)
        lib = _lib.lib()
        tab = pp._dbn_tables.ctypes.data
        d_tab = pp._dbn_device_tables(dev)
        logits = torch.cat([beat, down])
        spans = np.stack([off[:-1], total + off[:-1], np.diff(off), off[:-1]], 1).astype(np.int32)
        d_spans = torch.from_numpy(spans).to(dev)
        ws = torch.empty(lib.bt_dbn_workspace_bytes(tab, n, total), dtype=torch.uint8, device=dev)
        buf = torch.empty(n + 2 * total, dtype=torch.int32, device=dev)

        def launch():
            _lib.check(lib.bt_dbn_decode(_lib.stream_ptr(dev), tab, d_tab.data_ptr(), logits.data_ptr(), 0, d_spans.data_ptr(),
                                         n, total, buf.data_ptr(), ws.data_ptr(), ws.numel()))
        launch()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        res["device_decode_ms"] = float(np.median(ts))
        res["device_decode_ms_min"] = float(np.min(ts))
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            got = pp.ragged(beat, down, off)
            ts.append((time.perf_counter() - t0) * 1e3)
        res["ragged_end_to_end_ms"] = float(np.median(ts))
        res["beats_per_track"] = [len(g[0]) for g in got]
    # host decoder, one track per task on a 16-thread pool (ctypes releases the GIL)
    cpu = [(t[0].double().numpy(), t[1].double().numpy()) for t in tr]

    def host(t):
        rows = np.zeros((len(t[0]), 2), np.int32)
        c = C.c_int32()
        _lib.check(_lib.lib().bt_dbn_host(pp._dbn_tables.ctypes.data, t[0].ctypes.data, t[1].ctypes.data, len(t[0]),
                                          rows.ctypes.data, C.byref(c)))
        return rows[: c.value]
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(host, cpu[:1]))
        t0 = time.perf_counter()
        host_rows = list(ex.map(host, cpu))
        res["host_16_threads_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    host(cpu[0])
    res["host_one_track_ms"] = (time.perf_counter() - t0) * 1e3
    if torch.cuda.is_available():
        res["device_equals_host"] = all(np.array_equal(h[:, 0] / 50.0, g[0]) for h, g in zip(host_rows, got))
    import dbn_reference as R

    t0 = time.perf_counter()
    for k in range(a.oracle_tracks):
        R.postp_dbn(*tr[k])
    res["numpy_oracle_ms_per_track"] = (time.perf_counter() - t0) * 1e3 / max(a.oracle_tracks, 1)
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        open(a.json, "w").write(line + "\n")


if __name__ == "__main__":
    main()
