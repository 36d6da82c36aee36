#!/usr/bin/env python
"""Timing of 16-mixed in the differentiable frontend: one whole-model training step, forward + backward,
at final0 widths (D = 512, 6 layers, ff_mult 4), B = 8, T = 1500, four legs interleaved run by run in one session on one card,

  fp32:        fp32 trunk + fp32 frontend
  trunk16:     16-mixed trunk + fp32 frontend (``set_train_precision("16-mixed")`` alone)
  both16:      16-mixed trunk + 16-mixed frontend (``set_frontend_precision("16-mixed")`` on top)
  autocast:    the whole model restated in torch ops (tools/frontend_speed.py) under ``torch.autocast`` fp16

Times are device-event times after a warm-up; per leg the median and the min .. max spread over --reps runs, and the peak of
``torch.cuda.max_memory_allocated`` over one step.

``--units`` times the three conv units alone instead (forward + backward through ``ConvUnitFn`` at the shapes they have inside
that step), fp32 against mixed.

    python tools/front_mixed_speed.py [--units] [--reps 7] [--batch 8] [--frames 1500] [--dim 512] [--layers 6]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from backward_speed import event_time, torch_trunk  # noqa: E402
from frontend_speed import torch_frontend  # noqa: E402
from beat_this_amd import weights as W  # noqa: E402
from beat_this_amd.model import BeatThis  # noqa: E402
from beat_this_amd.model import backward as bw  # noqa: E402


def summary(times):
    return {k: dict(median=round(float(np.median(t)), 2), min=round(min(t), 2), max=round(max(t), 2)) for k, t in times.items()}


def interleaved(legs, reps):
    for fn in legs.values():   # warm-up
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(reps):      # (interleaved: the legs see the same clocks and the same neighbours)
        for k, fn in legs.items():
            times[k].append(event_time(fn))
    return times


def units(model, B, T, reps, dev):
    gen = torch.Generator().manual_seed(2)
    res = {}
    for i, blk in enumerate(model.frontend.blocks):
        F_, C_ = 32 >> i, 32 << i
        x = torch.randn(B, T, F_, C_, generator=gen).to(dev).requires_grad_(True)
        g = (torch.randn(B, T, F_ // 2, 2 * C_, generator=gen) * 2.0 ** -6).to(dev)
        ps = [blk.conv2d.weight, blk.norm.weight, blk.norm.bias]

        def step(mixed, x=x, g=g, blk=blk, ps=ps):
            return torch.autograd.grad([bw.conv_unit(blk, x, False, mixed)], [x] + ps, [g])

        times = interleaved({"fp32": lambda: step(False), "mixed": lambda: step(True)}, reps)
        res[f"conv{i}_ms"] = summary(times)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--units", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=1500)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--layers", type=int, default=6)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    B, T, D, NL = args.batch, args.frames, args.dim, args.layers
    hp = W.resolve_hparams(dict(transformer_dim=D, n_layers=NL))
    sd = W.random_state_dict(hp, seed=3, style="lively")
    model = BeatThis(**{k: hp[k] for k in ("spect_dim", "transformer_dim", "ff_mult", "n_layers", "head_dim", "stem_dim")})
    model.load_state_dict(sd)
    model = model.to(dev)
    model.set_frontend_trainable()
    model.transformer_blocks.requires_grad_(True)
    model.task_heads.requires_grad_(True)
    res = dict(shape=f"B={B} T={T} D={D} L={NL} ff_mult={hp['ff_mult']}", reps=args.reps)
    if args.units:
        res.update(units(model, B, T, args.reps, dev))
        print(json.dumps(res), flush=True)
        return
    gen = torch.Generator().manual_seed(1)
    spect = (torch.rand(B, T, 128, generator=gen) * 3).to(dev)
    g_b, g_d = (torch.randn(B, T, generator=gen) * 2.0 ** -6).to(dev), (torch.randn(B, T, generator=gen) * 2.0 ** -6).to(dev)
    params = dict(model.named_parameters())
    names = [n for n in params if not n.endswith("freqs")]
    tparams = {n: params[n].detach().clone().requires_grad_(True) for n in names}
    stats = {n: b for n, b in model.named_buffers()}
    freqs = sd["transformer_blocks.layers.0.0.rotary_embed.freqs"].float()
    ang = torch.arange(max(T, 32), dtype=torch.float32)[:, None] * freqs[None, :]
    cos, sin = ang.cos().to(dev), ang.sin().to(dev)

    def device_step(trunk, front):
        def step():
            model.set_train_precision(trunk).set_frontend_precision(front)
            out = model(spect)
            return torch.autograd.grad([out["beat"], out["downbeat"]], [params[n] for n in names], [g_b, g_d])
        return step

    def autocast():
        with torch.autocast("cuda", dtype=torch.float16):
            beat, down = torch_trunk(torch_frontend(spect, tparams, stats, cos, sin), tparams, NL, D // 32, cos[:T], sin[:T])
        return torch.autograd.grad([beat.float(), down.float()], [tparams[n] for n in names], [g_b, g_d])

    legs = {"fp32": device_step("32-true", "32-true"), "trunk16": device_step("16-mixed", "32-true"),
            "both16": device_step("16-mixed", "16-mixed"), "autocast": autocast}
    peak = {}
    for fn in legs.values():        # (a first step each: what is allocated once is no part of a step)
        fn()
    for name, fn in legs.items():
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        out = fn()
        torch.cuda.synchronize()
        peak[name] = dict(peak=int(torch.cuda.max_memory_allocated(dev)), above_the_step_start=int(torch.cuda.max_memory_allocated(dev) - base))
        del out
    for k, v in summary(interleaved(legs, args.reps)).items():
        res[k + "_ms"] = v
    res["max_memory_allocated_bytes"] = peak
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
