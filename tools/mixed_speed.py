#!/usr/bin/env python
"""Timing of one training step of the trunk and the heads on the two precisions of the differentiable route (DESIGN.md section
16): forward + backward of ``task_heads(transformer_blocks(x))`` at final0 widths (D = 512, 6 layers, ff_mult 4), B = 8,
T = 1500, three legs interleaved run by run in one session on one card,

  fp32:     the route as it is by default (csrc/train.hip: exact fp32 MFMA GEMMs, vector-unit attention sweeps)
  mixed:    ``set_train_precision("16-mixed")`` (csrc/train_mixed.inc: fp16 MFMA GEMMs and attention sweeps, fp32 accumulation)
  autocast: the same trunk restated in torch ops under ``torch.autocast("cuda", float16)`` with torch-ROCm's autograd -- what the
            reference's 16-mixed trainer runs

Times are device-event times after a warm-up; per leg the median and the min .. max spread over --reps runs.  Also printed: the
library calls alone per unit for both precisions (attention forward / backward, feed-forward forward / backward), each leg's peak
of ``torch.cuda.max_memory_allocated`` over one step, and the mixed leg's distance from the fp32 leg's gradients.

    python tools/mixed_speed.py [--reps 9] [--batch 8] [--frames 1500] [--dim 512] [--layers 6]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from backward_speed import event_time, torch_trunk  # noqa: E402
from beat_this_amd import _lib  # noqa: E402
from beat_this_amd import weights as W  # noqa: E402
from beat_this_amd.model import BeatThis  # noqa: E402


def unit_calls(model, x, reps):
    """the attention's and the feed-forward's library calls alone on preallocated buffers, interleaved between the precisions
    -> {"attention" | "feed-forward": {"fp32" | "mixed": [forward ms, backward ms]}}"""
    L = _lib.lib()
    dev = x.device
    B, T, D = x.shape
    H, hid = D // 32, model.hparams["ff_mult"] * D
    eng = model.engine()
    eng.ensure_positions(T)
    at, ff = model.transformer_blocks.layers[0]
    net4 = ff.net._modules["4"]
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    gy = torch.randn(B, T, D, device=dev)
    st = _lib.stream_ptr(dev)
    spec = {"attention": (_lib.UNIT_ATTN,
                          dict(gamma=at.norm.gamma, w1=at.to_qkv.weight, w2=at.to_gates.weight, b2=at.to_gates.bias, w3=at.to_out[0].weight),
                          dict(y=new(B, T, D), save_o=new(B, T, D), save_lse=new(B, T, H), gx=new(B, T, D), g_gamma=new(D),
                               g_w1=new(3 * D, D), g_w2=new(H, D), g_b2=new(H), g_w3=new(D, D))),
            "feed-forward": (_lib.UNIT_FF,
                             dict(gamma=ff.net[0].gamma, w1=ff.net[1].weight, b1=ff.net[1].bias, w2=net4.weight, b2=net4.bias),
                             dict(y=new(B, T, D), gx=new(B, T, D), g_gamma=new(D), g_w1=new(hid, D), g_b1=new(hid), g_w2=new(D, hid),
                                  g_b2=new(D)))}
    out = {}
    for name, (unit, params, bufs) in spec.items():
        a = _lib.TrainArgs()
        a.B, a.T, a.dim, a.hidden, a.rope_len = B, T, D, hid, eng.packed.desc.rope_len
        a.rope, a.x, a.gy = eng.packed._rope_t.data_ptr(), x.data_ptr(), gy.data_ptr()
        for k, t in list(params.items()) + list(bufs.items()):
            setattr(a, k, t.data_ptr())
        ws = torch.empty(L.bt_train_workspace_bytes(unit, 1, B, T, D, hid), dtype=torch.uint8, device=dev)
        a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
        calls = {"fp32": [lambda: _lib.check(L.bt_train_forward(st, unit, C.byref(a))),
                          lambda: _lib.check(L.bt_train_backward(st, unit, C.byref(a)))],
                 "mixed": [lambda: _lib.check(L.bt_train_forward_mixed(st, unit, C.byref(a), None)),
                           lambda: _lib.check(L.bt_train_backward_mixed(st, unit, C.byref(a), None))]}
        times = {k: [[], []] for k in calls}
        for i in range(2):   # (the forward first: the backward reads what it saved)
            for k in calls:
                calls[k][i]()
            torch.cuda.synchronize()
            for _ in range(reps):
                for k in calls:
                    times[k][i].append(event_time(calls[k][i]))
        out[name] = {k: [round(float(np.median(t)), 3) for t in v] for k, v in times.items()}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
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
    model.transformer_blocks.requires_grad_(True)
    model.task_heads.requires_grad_(True)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(B, T, D, generator=gen).to(dev)
    g_b, g_d = torch.randn(B, T, generator=gen).to(dev), torch.randn(B, T, generator=gen).to(dev)
    names = [n for n, p in model.named_parameters() if n.startswith(("transformer_blocks.", "task_heads.")) and not n.endswith("freqs")]
    params = dict(model.named_parameters())
    tparams = {n: params[n].detach().clone().requires_grad_(True) for n in names}
    freqs = sd["transformer_blocks.layers.0.0.rotary_embed.freqs"].float()
    ang = torch.arange(T, dtype=torch.float32)[:, None] * freqs[None, :]
    cos, sin = ang.cos().to(dev), ang.sin().to(dev)

    def route(precision):
        model.set_train_precision(precision)
        out = model.task_heads(model.transformer_blocks(x))
        return torch.autograd.grad([out["beat"], out["downbeat"]], [params[n] for n in names], [g_b, g_d])

    def autocast():
        with torch.autocast("cuda", dtype=torch.float16):
            beat, down = torch_trunk(x, tparams, NL, D // 32, cos, sin)
        return torch.autograd.grad([beat, down], [tparams[n] for n in names], [g_b.to(beat.dtype), g_d.to(down.dtype)])

    legs = {"fp32": lambda: route("32-true"), "mixed": lambda: route("16-mixed"), "autocast": autocast}
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
        grads[name] = [g.detach().float().cpu() for g in out]
        del out
    away = {k: max(float((u - v).double().norm() / v.double().norm()) for u, v in zip(grads[k], grads["fp32"])) for k in ("mixed", "autocast")}
    del grads
    for _ in range(2):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.reps):   # (interleaved: the legs see the same clocks and the same neighbours)
        for k, fn in legs.items():
            times[k].append(event_time(fn))
    model.set_train_precision("32-true")
    calls = unit_calls(model, x, args.reps)
    res = dict(shape=f"B={B} T={T} D={D} L={NL} ff_mult={hp['ff_mult']}", reps=args.reps)
    for k, t in times.items():
        res[k + "_ms"] = dict(median=round(float(np.median(t)), 2), min=round(min(t), 2), max=round(max(t), 2))
    res["mixed_faster_than_fp32_beyond_the_spread"] = bool(max(times["mixed"]) < min(times["fp32"]))
    res["per_call_ms_forward_backward"] = calls
    res["max_memory_allocated_bytes"] = peak
    res["worst_rel_l2_from_the_fp32_leg"] = away
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
