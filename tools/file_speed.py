#!/usr/bin/env python
"""Speed of the FILE path: audio files on disk -> beat times on the host, where every other number of this project starts from
a waveform in memory.  Writes six 5-minute stereo 16-bit 44.1 kHz WAV files (seeded noise plus clicks) into a temporary
directory, reads them once (warm page cache) and times, interleaved, median of 7 with min .. max:

  (a) today's loop: File2Beats()(path) per file -- load_audio, float64 conversion and channel mean on the host
  (b) File2Beats.many(paths): raw bytes into pinned buffers, one bt_pcm_decode_batch launch, the batched stages
  (c) File2Beats(device_decode=True)(path) per file
  (d) Audio2Beats.many on the waveforms already decoded on the host (pinned fp32): the floor the headline measures
  (e) the device time of the bt_pcm_decode_batch launch alone (events), next to bytes moved / 6.3 TB/s
  (r) reading the files' raw bytes into pinned buffers alone (wav.read_raw, the reader threads of (b))
  (a30), (c30): (a) and (c) for ONE 30-second file

The model is a randomly initialised BeatThis of the default size: the times do not depend on the weights.  Prints one JSON
line.  There is no gate: the numbers go into DESIGN.md section 23.

    python tools/file_speed.py [--files 6] [--seconds 300] [--runs 7]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from beat_this_amd import _lib, inference, wav  # noqa: E402
from beat_this_amd.inference import Audio2Beats, File2Beats, _host_mono, load_audio  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def write_wav(path, seconds, seed, sr=44100):
    from scipy.io import wavfile

    rng = np.random.default_rng(seed)
    n = int(seconds * sr)
    x = rng.integers(-1500, 1501, (n, 2), dtype=np.int16)
    period = int(sr * 60.0 / (96 + 7 * seed))
    for k in range(0, n - 400, period):                # clicks: a decaying 1 kHz burst on every beat
        t = np.arange(400)
        x[k: k + 400] += (12000 * np.exp(-t / 80.0) * np.sin(2 * np.pi * 1000.0 * t / sr)).astype(np.int16)[:, None]
    wavfile.write(path, sr, x)


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(min(ms)), 3), "max_ms": round(float(max(ms)), 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--files", type=int, default=6)
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as tmp:
        paths = [os.path.join(tmp, f"t{k}.wav") for k in range(args.files)]
        for k, p in enumerate(paths):
            write_wav(p, args.seconds, k)
        short = os.path.join(tmp, "short.wav")
        write_wav(short, 30.0, 99)
        for p in paths + [short]:
            with open(p, "rb") as f:                    # (warm page cache)
                while f.read(1 << 24):
                    pass
        host = File2Beats(checkpoint_path=None, device=dev)
        ondev = File2Beats(checkpoint_path=None, device=dev, device_decode=True)
        ondev.model = host.model
        decoded = [torch.from_numpy(_host_mono(load_audio(p)[0])).pin_memory() for p in paths]
        infos = [wav.probe(p) for p in paths]
        pinned = [inference._raw_pinned(i.raw_span[1]) for i in infos]

        def leg_e():
            """the decode launch alone, on bytes already on the device"""
            raws = [b[: i.raw_span[1]].to(dev) for b, i in zip(pinned, infos)]
            pay = [i.raw_span[2] for i in infos]
            n_fr = np.array([i.n_frames for i in infos], dtype=np.int64)
            off = np.concatenate([[0], np.cumsum((n_fr + 3) // 4 * 4)])
            out = torch.empty(int(off[-1]), dtype=torch.float32, device=dev)
            table = np.zeros((len(infos), 4), dtype=np.int64)
            table[:, 0] = [r.data_ptr() + p for r, p in zip(raws, pay)]
            table[:, 1], table[:, 2] = n_fr, out.data_ptr() + 4 * off[:-1]
            table[:, 3] = [i.format | (i.channels << 32) for i in infos]
            d_table = torch.from_numpy(table).to(dev)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            _lib.check(_lib.lib().bt_pcm_decode_batch(_lib.stream_ptr(dev), d_table.data_ptr(), len(infos), int(n_fr.max())))
            b.record()
            b.synchronize()
            return a.elapsed_time(b), sum(i.data_bytes for i in infos) + 4 * int(n_fr.sum())

        def leg_r():
            jobs = [inference._read_pool().submit(wav.read_raw, i, p, b) for i, p, b in zip(infos, paths, pinned)]
            for j in jobs:
                j.result()

        legs = {
            "a_loop_file2beats": lambda: [host(p) for p in paths],
            "b_file2beats_many": lambda: host.many(paths),
            "c_loop_device_decode": lambda: [ondev(p) for p in paths],
            "d_audio2beats_many_decoded": lambda: Audio2Beats.many_async(host, decoded, 44100).result(),
            "r_read_raw_pinned": leg_r,
            "a30_file2beats_one_30s": lambda: host(short),
            "c30_device_decode_one_30s": lambda: ondev(short),
        }
        ref = legs["a_loop_file2beats"]()               # warm-up of every leg; (b) and (c) must give (a)'s beats
        for name in ("b_file2beats_many", "c_loop_device_decode"):
            got = legs[name]()
            assert all(np.array_equal(g[0], r[0]) and np.array_equal(g[1], r[1]) for g, r in zip(got, ref)), name
        for name in ("d_audio2beats_many_decoded", "r_read_raw_pinned", "a30_file2beats_one_30s", "c30_device_decode_one_30s"):
            legs[name]()
        leg_e()
        times = {name: [] for name in legs}
        e_ms, e_bytes = [], 0
        for _ in range(args.runs):                      # interleaved: one run of every leg per round
            for name, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append(1e3 * (time.perf_counter() - t0))
            ms, e_bytes = leg_e()
            e_ms.append(ms)
        res = {"files": args.files, "seconds": args.seconds, "runs": args.runs, "audio_seconds": args.files * args.seconds,
               "raw_bytes": sum(i.data_bytes for i in infos)}
        res.update({name: stats(ms) for name, ms in times.items()})
        res["e_pcm_decode_batch_device"] = dict(stats(e_ms), bytes_moved=e_bytes,
                                                floor_ms=round(1e3 * e_bytes / HBM_BYTES_PER_S, 4))
        print(json.dumps(res))


if __name__ == "__main__":
    main()
