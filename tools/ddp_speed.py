#!/usr/bin/env python
"""Timing of the rank-ordered gradient sum of data-parallel training (csrc/reduce.hip) at the size of
final0's trainable set (18 946 658 fp32 gradients, cut into ``world`` segments as ``parallel.GradientExchange`` cuts them): what
one rank does between the two collectives of an optimiser step.  Per world in 2, 4, 8 the legs, interleaved run by run:

  kernel      bt_grad_rank_sum, in place over rank 0's part (the exchange's call)
  variant     the same entry point of another build of the library (--variant LIB; e.g. -DBT_REDUCE_NT: non-temporal loads)
  torch.sum   torch.sum(parts.view(W, -1), 0, out=...): what one writes without the kernel (its association is torch's own)

``queued``: --queue calls enqueued behind matrix products, so the kernels run back to back (device time per call); ``call``: one
call on an idle GPU between device events (launch time counts).  Medians of --reps runs after a warm-up run, with their spread.
Next to them the streaming floor: (W + 1) x 4 bytes per element of a segment at 6.3 TB/s (DESIGN.md section 14's figure).

With two or more GPUs one epoch of the synthetic data folder (tests/dataset_reference.py) is timed under
``python -m beat_this_amd.train --gpus 2`` against ``--gpus 1`` (--train; whole processes, start-up included); on one GPU
that is reported as not measured.

    python tools/ddp_speed.py [--reps 7] [--queue 20] [--variant LIB] [--train]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOTAL = 18_946_658          # final0's trainable parameters (tools/optim_speed.py)
HBM_ACHIEVABLE = 6.3e12     # bytes / s
WORLDS = (2, 4, 8)


def event_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def queued_time(fn, n, blocker):
    """ms per call of ``fn`` when ``n`` calls wait in the stream behind ``blocker``'s work"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    blocker()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def summary(ts):
    return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}


def measure(reps, queue, variant):
    from beat_this_amd import _lib
    from beat_this_amd.parallel import segment_length

    dev = torch.device("cuda:0")
    lib = _lib.lib()
    libs = {"kernel": lib}
    if variant:
        other = C.CDLL(os.path.abspath(variant))
        other.bt_grad_rank_sum.restype, other.bt_grad_rank_sum.argtypes = _lib.EXPORTS["bt_grad_rank_sum"]
        libs["variant"] = other
    big = torch.randn(8192, 8192, device=dev)

    def blocker():
        for _ in range(6):
            torch.mm(big, big)

    out = {}
    for world in WORLDS:
        per = segment_length(TOTAL, world)
        src = torch.randn(world * per, device=dev) * 1e-3
        # consecutive calls take the next of RING copies of the parts (more than 600 MB together): the gradients of a real step
        # arrive from a collective, not from the 256 MB last-level cache that a repeated call on one buffer would be served by
        ring = [src.clone() for _ in range(max(2, -(-600_000_000 // (4 * world * per))))]
        turn = [0]
        dst = torch.empty(per, device=dev)
        stream = _lib.stream_ptr(dev)

        def next_parts():
            turn[0] = (turn[0] + 1) % len(ring)
            return ring[turn[0]]

        def kernel(handle):
            parts = next_parts()
            _lib.check(handle.bt_grad_rank_sum(stream, parts.data_ptr(), per, world, per, parts.data_ptr()))

        legs = {name: (lambda h=handle: kernel(h)) for name, handle in libs.items()}
        legs["torch.sum"] = lambda: torch.sum(next_parts().view(world, per), 0, out=dst)
        # the kernel's legs agree with each other bit for bit before anything is timed
        results = {}
        for name in libs:
            for parts in ring:
                parts.copy_(src)
            legs[name]()
            results[name] = ring[turn[0]][:per].clone()
        assert all(torch.equal(r.view(torch.int32), results["kernel"].view(torch.int32)) for r in results.values())
        call, queued = {k: [] for k in legs}, {k: [] for k in legs}
        for rep in range(reps + 1):   # (run 0 is the warm-up)
            for name, fn in legs.items():
                for parts in ring:
                    parts.copy_(src)
                torch.cuda.synchronize()
                t = event_time(fn)
                torch.cuda.synchronize()
                q = queued_time(fn, queue, blocker)   # (in place: a later call on the same copy adds rank 0's running sum again)
                if rep:
                    call[name].append(t)
                    queued[name].append(q)
        floor = per * (world + 1) * 4 / HBM_ACHIEVABLE * 1e3
        print(f"world {world}: segment of {per} elements, floor {floor:.4f} ms ({(world + 1) * 4} B / element at {HBM_ACHIEVABLE / 1e12:.1f} TB/s)")
        out[f"world{world}"] = {"segment": per, "floor_ms": floor}
        for name in legs:
            c, q = summary(call[name]), summary(queued[name])
            out[f"world{world}"][name] = {"call_ms": c, "queued_ms": q}
            print(f"  {name:10s} queued {q['median']:.4f} ms ({q['min']:.4f} .. {q['max']:.4f}) = {q['median'] / floor:.2f} x floor, "
                  f"call {c['median']:.4f} ms ({c['min']:.4f} .. {c['max']:.4f})")
    return out


def train_epoch_times():
    """one epoch of the synthetic folder under --gpus 1 and --gpus 2, whole processes -> {gpus: seconds}, or None on one GPU"""
    if torch.cuda.device_count() < 2:
        print("data-parallel epoch: not measured (this machine shows one GPU)")
        return None
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from dataset_reference import build_data_folder

    times = {}
    with tempfile.TemporaryDirectory() as tmp:
        root = build_data_folder(os.path.join(tmp, "data"))
        for gpus in (1, 2, 1, 2):
            cmd = [sys.executable, "-m", "beat_this_amd.train", "--data-dir", root, "--output", os.path.join(tmp, f"g{gpus}.ckpt"),
                   "--gpus", str(gpus), "--max-epochs", "1", "--batch-size", "1", "--accumulate-grad-batches", "1", "--train-length", "150",
                   "--n-layers", "2", "--transformer-dim", "64", "--no-tempo-augmentation", "--no-pitch-augmentation",
                   "--no-mask-augmentation", "--val-frequency", "1"]
            t0 = time.monotonic()
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
            if r.returncode:
                raise RuntimeError(f"--gpus {gpus} failed:\n{r.stdout[-2000:]}{r.stderr[-4000:]}")
            times.setdefault(gpus, []).append(time.monotonic() - t0)
    for gpus, ts in times.items():
        print(f"data-parallel epoch, --gpus {gpus}: {min(ts):.2f} s (whole process, best of {len(ts)}; five batches of a D = 64 model)")
    return {str(k): v for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--queue", type=int, default=20)
    ap.add_argument("--variant", type=str, default=None, help="another build of the library whose bt_grad_rank_sum is timed as a third leg")
    ap.add_argument("--train", action="store_true", help="also time one --gpus 2 epoch of the synthetic folder against --gpus 1")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ddp_speed.py measures on a ROCm GPU: none is visible")
    out = measure(args.reps, args.queue, args.variant)
    if args.train:
        out["train_epoch_s"] = train_epoch_times()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
