#!/usr/bin/env python
"""Timing of the optimiser step (csrc/optim.hip, beat_this_amd/optim.py) on the trainable set of final0
(the six main layers, the final RMSNorm and the heads; tensors and parameters counted from ``state_dict_shapes``), two
parameter groups as ``param_groups_for`` builds them:

  A  this package's step (one launch) and the same with max_grad_norm (three launches)
  B  torch.optim.AdamW(fused=True)
  C  torch.optim.AdamW(foreach=True)
  D  torch.nn.utils.clip_grad_norm_ followed by the fused torch step

Two times per leg, both between device events, the median of --reps runs after a warm-up, the legs interleaved run by run in
one session:

  call     one ``step()`` call with the gradients in place and an idle GPU: the call's Python and launch time counts wherever
           it is longer than the kernels (what a loop sees that waits for every step)
  queued   --queue steps enqueued behind matrix products that keep the GPU busy while the host enqueues them, so the kernels
           run back to back: device time per step, what compares with the bandwidth floor

Printed next to them: the bandwidth floor of the step, from the bytes per element
the kernel moves (reads p, g, m, v; writes p, m, v and the cleared g: 32 B; the norm reads g once more: 4 B) and the HBM rate
that streaming kernels reach on an MI355X (6.3 TB/s of the 8 TB/s peak).

    python tools/optim_speed.py [--reps 7] [--queue 10]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from beat_this_amd import optim as OP  # noqa: E402
from beat_this_amd.weights import resolve_hparams, state_dict_shapes  # noqa: E402

HBM_ACHIEVABLE = 6.3e12   # bytes / s
BYTES_STEP, BYTES_NORM = 32, 4


def trainable_shapes(hp="final0"):
    return [s for k, s in state_dict_shapes(resolve_hparams(hp)).items()
            if k.startswith(("transformer_blocks.", "task_heads.")) and not k.endswith("freqs")]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--queue", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    shapes = trainable_shapes()
    n_params = int(sum(np.prod(s) for s in shapes))
    gen = torch.Generator().manual_seed(0)

    def params():
        return [torch.nn.Parameter((torch.randn(*s, generator=gen) * 0.05).to(dev)) for s in shapes]

    def groups(ps):
        return [{"params": [p for p in ps if p.ndim >= 2], "weight_decay": 0.01}, {"params": [p for p in ps if p.ndim <= 1], "weight_decay": 0}]

    def fill(ps):
        for p in ps:
            g = torch.randn(p.shape, device=dev) * 1e-3
            if p.grad is None:
                p.grad = g
            else:
                p.grad.copy_(g)

    legs = {}
    for name, kw in (("A  ours", {}), ("A  ours + clip", dict(max_grad_norm=1.0))):
        ps = params()
        opt = OP.AdamW(groups(ps), lr=8e-4, **kw)
        legs[name] = (ps, opt.step)
    for name, kw in (("B  torch fused", dict(fused=True)), ("C  torch foreach", dict(foreach=True))):
        ps = params()
        opt = torch.optim.AdamW(groups(ps), lr=8e-4, **kw)
        legs[name] = (ps, opt.step)
    ps = params()
    opt_d = torch.optim.AdamW(groups(ps), lr=8e-4, fused=True)

    def clip_then_step(ps=ps):
        torch.nn.utils.clip_grad_norm_(ps, 1.0)
        opt_d.step()
    legs["D  torch clip + fused"] = (ps, clip_then_step)

    big = torch.randn(8192, 8192, device=dev)

    def blocker():   # some tens of milliseconds of GPU work: the host enqueues the steps meanwhile
        for _ in range(6):
            torch.mm(big, big)

    times = {k: [] for k in legs}
    queued = {k: [] for k in legs}
    for rep in range(args.reps + 1):          # (run 0 is the warm-up)
        for name, (ps, step) in legs.items():
            fill(ps)
            torch.cuda.synchronize()
            t = event_time(step)
            fill(ps)
            torch.cuda.synchronize()
            q = queued_time(step, args.queue, blocker)
            if rep:
                times[name].append(t)
                queued[name].append(q)
    floor = n_params * BYTES_STEP / HBM_ACHIEVABLE * 1e3
    floor_clip = n_params * (BYTES_STEP + BYTES_NORM) / HBM_ACHIEVABLE * 1e3
    print(f"final0 trainable set: {len(shapes)} tensors, {n_params} parameters ({n_params * 4 / 2 ** 20:.1f} MiB each of p, g, m, v)")
    print(f"bandwidth floor at {HBM_ACHIEVABLE / 1e12:.1f} TB/s: {floor:.4f} ms per step ({BYTES_STEP} B / element), "
          f"{floor_clip:.4f} ms with the norm ({BYTES_STEP + BYTES_NORM} B / element)")
    out = {"tensors": len(shapes), "parameters": n_params, "floor_ms": floor, "floor_clip_ms": floor_clip}
    print(f"  {'leg':24s} {'call, ms (min .. max)':>34s} {'queued, ms (min .. max)':>34s}")
    for name, ts in times.items():
        med, qs = float(np.median(ts)), queued[name]
        qmed = float(np.median(qs))
        out[name.split("  ", 1)[1]] = {"call_ms": med, "queued_ms": qmed}
        print(f"  {name:24s} {med:14.4f} ({min(ts):.4f} .. {max(ts):.4f}) {qmed:14.4f} ({min(qs):.4f} .. {max(qs):.4f})")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
