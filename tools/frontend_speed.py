#!/usr/bin/env python
"""Timing of one whole-model training step: forward + backward at final0 widths (D = 512, 6 layers,
ff_mult 4), B = 8, T = 1500, three legs interleaved run by run in one session on one card,

  whole:  ``set_frontend_trainable()`` -- the frontend (csrc/train_front.hip and the trunk's unit code on its twelve leaves), the
          trunk and the heads on the differentiable route, gradients of every weight
  trunk:  the trunk-only route, ``task_heads(transformer_blocks(h))`` on a given (B, T, D) input (the fp32 leg of
          tools/backward_speed.py and tools/mixed_speed.py)
  torch:  the whole model restated in torch ops under torch-ROCm's autograd, fp32, BatchNorm on its running statistics

Times are device-event times after a warm-up; per leg the median and the min .. max spread over --reps runs, and the peak of
``torch.cuda.max_memory_allocated`` over one step.  Also printed: the whole leg's distance from the torch leg's gradients.

    python tools/frontend_speed.py [--reps 7] [--batch 8] [--frames 1500] [--dim 512] [--layers 6]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from backward_speed import event_time, rmsnorm, rope, torch_trunk  # noqa: E402
from beat_this_amd import weights as W  # noqa: E402
from beat_this_amd.model import BeatThis  # noqa: E402


def torch_pair(x, p, a, f, cos, sin):
    """x + attention, then + feed-forward, on (sequences, tokens, C); a, f: the two key prefixes"""
    b, n, dim = x.shape
    heads = dim // 32
    xn = rmsnorm(x, p[a + "norm.gamma"])
    q, k, v = F.linear(xn, p[a + "to_qkv.weight"]).view(b, n, 3, heads, 32).permute(2, 0, 3, 1, 4)
    o = F.scaled_dot_product_attention(rope(q, cos[:n], sin[:n]), rope(k, cos[:n], sin[:n]), v)
    gates = torch.sigmoid(F.linear(xn, p[a + "to_gates.weight"], p[a + "to_gates.bias"]))
    o = (o * gates.permute(0, 2, 1)[..., None]).permute(0, 2, 1, 3).reshape(b, n, dim)
    x = F.linear(o, p[a + "to_out.0.weight"]) + x
    h = F.gelu(F.linear(rmsnorm(x, p[f + "net.0.gamma"]), p[f + "net.1.weight"], p[f + "net.1.bias"]))
    return F.linear(h, p[f + "net.4.weight"], p[f + "net.4.bias"]) + x


def torch_frontend(x, p, stats, cos, sin):
    """BeatThis.frontend in torch ops (beat_tracker.py:54-80, 290-301); p: trainable tensors, stats: the running statistics"""
    def bn(t, pfx):
        return F.batch_norm(t, stats[pfx + "running_mean"], stats[pfx + "running_var"], p[pfx + "weight"], p[pfx + "bias"], False, 0.0, 1e-5)

    s = "frontend.stem."
    x = bn(x.transpose(1, 2), s + "bn1d.")
    x = F.gelu(bn(F.conv2d(x[:, None], p[s + "conv2d.weight"], stride=(4, 1), padding=(0, 1)), s + "bn2d."))
    for i in range(3):
        q = f"frontend.blocks.{i}."
        if q + "partial.attnF.norm.gamma" in p:
            b, c, f, t = x.shape
            y = x.permute(0, 3, 2, 1).reshape(b * t, f, c)
            y = torch_pair(y, p, q + "partial.attnF.", q + "partial.ffF.", cos, sin)
            y = y.view(b, t, f, c).permute(0, 2, 1, 3).reshape(b * f, t, c)
            y = torch_pair(y, p, q + "partial.attnT.", q + "partial.ffT.", cos, sin)
            x = y.view(b, f, t, c).permute(0, 3, 1, 2)
        x = F.gelu(bn(F.conv2d(x, p[q + "conv2d.weight"], stride=(2, 1), padding=(0, 1)), q + "norm."))
    b, c, f, t = x.shape
    return F.linear(x.permute(0, 3, 1, 2).reshape(b, t, c * f), p["frontend.linear.weight"], p["frontend.linear.bias"])


def main(argv=None):
    ap = argparse.ArgumentParser()
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
    gen = torch.Generator().manual_seed(1)
    spect = (torch.rand(B, T, 128, generator=gen) * 3).to(dev)
    h = torch.randn(B, T, D, generator=gen).to(dev)
    g_b, g_d = torch.randn(B, T, generator=gen).to(dev), torch.randn(B, T, generator=gen).to(dev)
    params = dict(model.named_parameters())
    names = [n for n in params if not n.endswith("freqs")]
    trunk_names = [n for n in names if not n.startswith("frontend.")]
    tparams = {n: params[n].detach().clone().requires_grad_(True) for n in names}
    stats = {n: b for n, b in model.named_buffers()}
    freqs = sd["transformer_blocks.layers.0.0.rotary_embed.freqs"].float()
    ang = torch.arange(max(T, 32), dtype=torch.float32)[:, None] * freqs[None, :]
    cos, sin = ang.cos().to(dev), ang.sin().to(dev)

    def whole():
        out = model(spect)
        return torch.autograd.grad([out["beat"], out["downbeat"]], [params[n] for n in names], [g_b, g_d])

    def trunk():
        out = model.task_heads(model.transformer_blocks(h))
        return torch.autograd.grad([out["beat"], out["downbeat"]], [params[n] for n in trunk_names], [g_b, g_d])

    def restated():
        beat, down = torch_trunk(torch_frontend(spect, tparams, stats, cos, sin), tparams, NL, D // 32, cos[:T], sin[:T])
        return torch.autograd.grad([beat, down], [tparams[n] for n in names], [g_b, g_d])

    legs = {"whole": whole, "trunk": trunk, "torch": restated}
    peak, grads = {}, {}
    for fn in legs.values():        # (a first step each: what is allocated once -- the engine, the rotary table -- is no part of a step)
        fn()
    for name, fn in legs.items():   # one step each: the peak over the step, and the gradients for the comparison
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        out = fn()
        torch.cuda.synchronize()
        peak[name] = dict(peak=int(torch.cuda.max_memory_allocated(dev)), above_the_step_start=int(torch.cuda.max_memory_allocated(dev) - base))
        if name != "trunk":
            grads[name] = [g.detach().float().cpu() for g in out]
        del out
    away = max(float((u - v).double().norm() / v.double().norm()) for u, v in zip(grads["whole"], grads["torch"]))
    del grads
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.reps):   # (interleaved: the legs see the same clocks and the same neighbours)
        for k, fn in legs.items():
            times[k].append(event_time(fn))
    res = dict(shape=f"B={B} T={T} D={D} L={NL} ff_mult={hp['ff_mult']}", reps=args.reps)
    for k, t in times.items():
        res[k + "_ms"] = dict(median=round(float(np.median(t)), 2), min=round(min(t), 2), max=round(max(t), 2))
    res["max_memory_allocated_bytes"] = peak
    res["worst_rel_l2_of_the_whole_leg_from_the_torch_leg"] = away
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
