#!/usr/bin/env python
"""Timing of weight averaging in the optimiser step (csrc/optim.hip, beat_this_amd/optim.py) on the
trainable set of final0 (tools/optim_speed.py's: 18.9 M parameters, two parameter groups), three legs interleaved run by run:

  1  the plain step                        AdamW(...).step()
  2  the averaging step                    AdamW(..., ema_decay=0.999).step(): the same launch with a fourth stream
  3  the plain step, then the average      step(); torch._foreach_lerp_(averages, parameters, 1 - decay): what one writes
                                           without the fused step -- a second pass over every weight

Two times per leg, as tools/optim_speed.py takes them: ``call`` (one call on an idle GPU, between device events: Python and
launch time count) and ``queued`` (--queue calls enqueued behind matrix products, so the kernels run back to back: device time
per step).  Medians of --reps runs after a warm-up, with their spread.  Next to them the bandwidth floors: the plain step moves
32 B per element, the averaging one 40 B (it reads and writes e), leg 3 44 B (lerp reads e and p and writes e).

``--parent DIR``: the plain step of another checkout of this package (the parent commit, built in DIR) against this one's, each
in a fresh child process, alternating --rounds times in this session: leg 1 must not have moved.

    python tools/ema_speed.py [--reps 7] [--queue 10] [--parent DIR] [--rounds 3]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_ACHIEVABLE = 6.3e12   # bytes / s (tools/optim_speed.py)
BYTES = {"1  plain": 32, "2  averaging": 40, "3  plain + foreach_lerp": 44}
DECAY = 0.999


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


def measure(root, reps, queue, plain_only):
    """``root``: the checkout whose package is imported (this one, or --parent's)"""
    sys.path.insert(0, root)
    from beat_this_amd import optim as OP
    from beat_this_amd.weights import resolve_hparams, state_dict_shapes

    dev = torch.device("cuda:0")
    shapes = [s for k, s in state_dict_shapes(resolve_hparams("final0")).items()
              if k.startswith(("transformer_blocks.", "task_heads.")) and not k.endswith("freqs")]
    gen = torch.Generator().manual_seed(0)

    def params():
        return [torch.nn.Parameter((torch.randn(*s, generator=gen) * 0.05).to(dev)) for s in shapes]

    def groups(ps):
        return [{"params": [p for p in ps if p.ndim >= 2], "weight_decay": 0.01}, {"params": [p for p in ps if p.ndim <= 1], "weight_decay": 0}]

    def fill(ps):
        for p in ps:
            p.grad.copy_(torch.randn(p.shape, device=dev) * 1e-3)

    legs = {}
    ps = params()
    legs["1  plain"] = (ps, OP.AdamW(groups(ps), lr=8e-4).step)
    if not plain_only:
        ps = params()
        legs["2  averaging"] = (ps, OP.AdamW(groups(ps), lr=8e-4, ema_decay=DECAY).step)
        ps = params()
        opt3 = OP.AdamW(groups(ps), lr=8e-4)
        avg = [p.detach().clone() for p in ps]

        @torch.no_grad()
        def step_then_lerp(ps=ps):
            opt3.step()
            torch._foreach_lerp_(avg, ps, 1.0 - DECAY)
        legs["3  plain + foreach_lerp"] = (ps, step_then_lerp)
    big = torch.randn(8192, 8192, device=dev)

    def blocker():
        for _ in range(6):
            torch.mm(big, big)

    call, queued = {k: [] for k in legs}, {k: [] for k in legs}
    for rep in range(reps + 1):          # (run 0 is the warm-up)
        for name, (ps, step) in legs.items():
            fill(ps)
            torch.cuda.synchronize()
            t = event_time(step)
            fill(ps)
            torch.cuda.synchronize()
            q = queued_time(step, queue, blocker)
            if rep:
                call[name].append(t)
                queued[name].append(q)
    return int(sum(np.prod(s) for s in shapes)), call, queued


def summary(ts):
    return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--queue", type=int, default=10)
    ap.add_argument("--parent", type=str, default=None, help="another built checkout whose plain step is timed against this one's")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--plain-of", type=str, default=None, help=argparse.SUPPRESS)   # (the child process of --parent)
    args = ap.parse_args()
    if args.plain_of:
        _, call, queued = measure(args.plain_of, args.reps, args.queue, plain_only=True)
        print(json.dumps({"call": call["1  plain"], "queued": queued["1  plain"]}))
        return
    out = {}
    if args.parent:
        seen = {"parent": {"call": [], "queued": []}, "this": {"call": [], "queued": []}}
        for _ in range(args.rounds):
            for name, root in (("parent", os.path.abspath(args.parent)), ("this", ROOT)):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-of", root, "--reps", str(args.reps), "--queue",
                                    str(args.queue)], capture_output=True, text=True, timeout=300)
                if r.returncode:
                    raise RuntimeError(f"the {name} measurement failed:\n{r.stdout}{r.stderr}")
                got = json.loads(r.stdout.strip().splitlines()[-1])
                for k in seen[name]:
                    seen[name][k] += got[k]
        print(f"the plain step, {args.rounds} processes each, alternating:")
        for name, got in seen.items():
            out[f"plain_{name}"] = {k: summary(v) for k, v in got.items()}
            print(f"  {name:8s} call {summary(got['call'])['median']:.4f} ms ({min(got['call']):.4f} .. {max(got['call']):.4f}), "
                  f"queued {summary(got['queued'])['median']:.4f} ms ({min(got['queued']):.4f} .. {max(got['queued']):.4f})")
    n_params, call, queued = measure(ROOT, args.reps, args.queue, plain_only=False)
    print(f"final0 trainable set: {n_params} parameters; floors at {HBM_ACHIEVABLE / 1e12:.1f} TB/s: "
          + ", ".join(f"{k.split('  ')[1]} {n_params * b / HBM_ACHIEVABLE * 1e3:.4f} ms ({b} B / element)" for k, b in BYTES.items()))
    print(f"  {'leg':26s} {'call, ms (min .. max)':>34s} {'queued, ms (min .. max)':>34s}")
    for name in call:
        c, q = summary(call[name]), summary(queued[name])
        out[name.split("  ", 1)[1]] = {"call_ms": c, "queued_ms": q, "floor_ms": n_params * BYTES[name] / HBM_ACHIEVABLE * 1e3}
        print(f"  {name:26s} {c['median']:14.4f} ({c['min']:.4f} .. {c['max']:.4f}) {q['median']:14.4f} ({q['min']:.4f} .. {q['max']:.4f})")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
