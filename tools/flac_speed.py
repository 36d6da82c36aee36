#!/usr/bin/env python
"""Speed of the FLAC file path: FLAC files on disk -> beat times on the host, against the same audio as WAV files.  Writes six
5-minute stereo 16-bit 44.1 kHz tracks (seeded noise plus clicks) as WAV and, with the test encoder (tests/flac_cases.py:
frames of 4096, LPC order 4 and fixed order 2 subframes, all channel assignments), as FLAC; reads them once (warm page cache)
and times, interleaved, median of 7 with min .. max:

  (w)   File2Beats.many(the WAV files): one bt_pcm_decode_batch launch in front of the batched stages
  (f)   File2Beats.many(the FLAC files): one bt_flac_decode_batch call (frame search, Rice, LPC, mix) in front of the same stages
  (h1)  bt_flac_decode_host over the six files on one host thread: what a host library's decode loop costs at best
  (h16) the same on 16 threads
  (e)   the device time of the bt_flac_decode_batch launches alone (events), on bytes already on the device

The encoder is Python: a track's first 20 seconds are encoded and their frame bodies repeated (with their own headers, numbers
and CRC-16s) up to 5 minutes; the WAV files hold the same integers.  The model is a randomly initialised BeatThis of the
default size.  Prints one JSON line.  There is no gate: the numbers go into DESIGN.md section 30.

    python tools/flac_speed.py [--files 6] [--seconds 300] [--runs 7]
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flac_cases as F  # noqa: E402
import wav_cases as W  # noqa: E402
from beat_this_amd import _lib, flac  # noqa: E402
from beat_this_amd.inference import File2Beats  # noqa: E402

BLOCK, UNIT_SECONDS, SR = 4096, 20.0, 44100


def unit_pcm(seed):
    rng = np.random.default_rng(seed)
    n = int(UNIT_SECONDS * SR) // BLOCK * BLOCK
    x = rng.integers(-1500, 1501, (n, 2)).astype(np.int64)
    period = int(SR * 60.0 / (96 + 7 * seed))
    t = np.arange(400)
    burst = (12000 * np.exp(-t / 80.0) * np.sin(2 * np.pi * 1000.0 * t / SR)).astype(np.int64)
    for k in range(0, n - 400, period):                # clicks: a decaying 1 kHz burst on every beat
        x[k: k + 400] += burst[:, None]
    return x


class Crc16:
    """CRC-16 of header + body from the body's own CRC: the register is linear over GF(2), so crc(h + b) = Z(crc(h)) ^ crc(b)
    with Z = "len(b) zero bytes", a 16 x 16 bit matrix raised to a power"""

    def __init__(self):
        self.step = [self._zero_byte(1 << i) for i in range(16)]
        self.cache = {}

    @staticmethod
    def _zero_byte(c):
        return ((c << 8) & 0xFFFF) ^ F._T16[c >> 8]

    @staticmethod
    def _apply(m, c):
        out = 0
        for i in range(16):
            if c >> i & 1:
                out ^= m[i]
        return out

    def zeros(self, n):
        if n not in self.cache:
            result, base = [1 << i for i in range(16)], self.step
            k = n
            while k:
                if k & 1:
                    result = [self._apply(base, v) for v in result]
                base = [self._apply(base, v) for v in base]
                k >>= 1
            self.cache[n] = result
        return self.cache[n]

    def __call__(self, head, body, body_crc):
        return self._apply(self.zeros(len(body)), F.crc16(head)) ^ body_crc


def write_pair(stem, seconds, seed):
    """<stem>.wav and <stem>.flac with the same integers"""
    unit = unit_pcm(seed)
    lpc = dict(type="lpc", coefs=[7800, -3100, 900, -300], precision=14, shift=12, porder=4)
    fixed = dict(type="fixed", order=2, porder=4)
    assigns = (10, 8, 9, 1)
    bodies = []
    for k in range(len(unit) // BLOCK):
        body = F.frame_body(unit[k * BLOCK: (k + 1) * BLOCK], 16, assigns[k % 4], [lpc if k % 2 == 0 else fixed, lpc])
        bodies.append((body, F.crc16(body), assigns[k % 4]))
    n_frames = int(seconds * SR) // BLOCK
    pcm = np.tile(unit, (-(-n_frames // len(bodies)), 1))[: n_frames * BLOCK]
    crc = Crc16()
    shape = np.zeros((BLOCK, 2), dtype=np.int64)
    audio = bytearray()
    for k in range(n_frames):
        body, body_crc, assign = bodies[k % len(bodies)]
        audio += F.write_frame(shape, 16, SR, k, False, assign=assign, body=body, crc=lambda h, b, c=body_crc: crc(h, b, c))
    info = F.streaminfo(BLOCK, BLOCK, SR, 2, 16, len(pcm), F.pcm_md5(pcm, 16))
    with open(stem + ".flac", "wb") as f:
        f.write(b"fLaC" + F.metadata([(0, info), (1, bytes(4096))]) + bytes(audio))
    W.write_wav(stem + ".wav", "s16", pcm, rate=SR)


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(min(ms)), 3), "max_ms": round(float(max(ms)), 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--files", type=int, default=6)
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        stems = [os.path.join(tmp, f"t{k}") for k in range(args.files)]
        for k, s in enumerate(stems):
            write_pair(s, args.seconds, k)
        encode_s = time.perf_counter() - t0
        wavs, flacs = [s + ".wav" for s in stems], [s + ".flac" for s in stems]
        datas = [np.fromfile(p, dtype=np.uint8) for p in flacs]          # (warm page cache, and the host legs' input)
        for p in wavs:
            np.fromfile(p, dtype=np.uint8)
        f2b = File2Beats(checkpoint_path=None, device=dev)
        infos = [flac.probe(p) for p in flacs]
        assert all(i is not None for i in infos)
        c_infos = [i.c_info() for i in infos]
        outs = [np.empty(i.total_samples, dtype=np.float32) for i in infos]

        def host_one(k):
            st = _lib.FlacStatus()
            _lib.check(lib.bt_flac_decode_host(datas[k].ctypes.data, C.byref(c_infos[k]), outs[k].ctypes.data, None, C.byref(st)))
            assert st.code == _lib.FLAC_OK
        pool = ThreadPoolExecutor(max_workers=16)

        # the decode launches alone, on bytes already on the device
        raws = [torch.from_numpy(d).to(dev) for d in datas]
        n = np.array([i.total_samples for i in infos], dtype=np.int64)
        off = np.concatenate([[0], np.cumsum((n + 3) // 4 * 4)])
        ws_n = [lib.bt_flac_workspace_bytes(C.byref(i)) for i in c_infos]
        ws_off = np.concatenate([[0], np.cumsum([(w + 255) // 256 * 256 for w in ws_n])])
        big = torch.empty(int(off[-1]), dtype=torch.float32, device=dev)
        ws = torch.empty(int(ws_off[-1]), dtype=torch.uint8, device=dev)
        status = torch.empty((len(infos), 3), dtype=torch.int64, device=dev)
        spans = (_lib.FlacSpan * len(infos))()
        for t, (d, i) in enumerate(zip(raws, c_infos)):
            spans[t] = _lib.FlacSpan(d.data_ptr(), big.data_ptr() + 4 * int(off[t]), ws.data_ptr() + int(ws_off[t]), int(ws_n[t]),
                                     status.data_ptr() + 24 * t, i)
        d_spans = torch.from_numpy(np.frombuffer(bytes(spans), dtype=np.uint8).copy()).to(dev)

        def leg_e():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            _lib.check(lib.bt_flac_decode_batch(_lib.stream_ptr(dev), spans, d_spans.data_ptr(), len(infos)))
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        legs = {
            "w_many_wav": lambda: f2b.many(wavs),
            "f_many_flac": lambda: f2b.many(flacs),
            "h1_flac_decode_host_1_thread": lambda: [host_one(k) for k in range(len(infos))],
            "h16_flac_decode_host_16_threads": lambda: list(pool.map(host_one, range(len(infos)))),
        }
        ref = legs["w_many_wav"]()                       # warm-up of every leg; the FLAC files must give the WAV files' beats
        got = legs["f_many_flac"]()
        assert all(np.array_equal(g[0], r[0]) and np.array_equal(g[1], r[1]) for g, r in zip(got, ref))
        legs["h1_flac_decode_host_1_thread"]()
        leg_e()
        assert (status.view(torch.int32)[:, 0] == 0).all()
        for k, o in enumerate(outs):                     # the device launches and the host twin agree bit for bit
            assert np.array_equal(big[int(off[k]): int(off[k]) + int(n[k])].cpu().numpy().view(np.uint32), o.view(np.uint32))
        times = {name: [] for name in legs}
        e_ms = []
        for _ in range(args.runs):                       # interleaved: one run of every leg per round
            for name, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append(1e3 * (time.perf_counter() - t0))
            e_ms.append(leg_e())
        res = {"files": args.files, "seconds": args.seconds, "runs": args.runs, "audio_seconds": float(n.sum()) / SR,
               "flac_bytes": int(sum(len(d) for d in datas)), "pcm_bytes": int(4 * n.sum()), "encode_s": round(encode_s, 1),
               "workspace_bytes": int(sum(ws_n))}
        res.update({name: stats(ms) for name, ms in times.items()})
        res["e_flac_decode_batch_device"] = stats(e_ms)
        print(json.dumps(res))


if __name__ == "__main__":
    main()
