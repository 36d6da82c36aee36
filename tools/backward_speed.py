#!/usr/bin/env python
"""Timing of one training step of the transformer trunk and the heads on the differentiable route (csrc/train.hip,
beat_this_amd/model/backward.py): forward + backward of ``task_heads(transformer_blocks(x))`` at final0
widths (D = 512, 6 layers, ff_mult 4), B = 8, T = 1500,

  route:   the package's autograd Functions over bt_train_forward / bt_train_backward (what ``loss.backward()`` runs)
  torch:   the same trunk restated in torch ops (fp32, F.scaled_dot_product_attention) with torch-ROCm's autograd, on the same
           card in the same session; the two legs are interleaved run by run
  kernels: the library calls alone, unit by unit with preallocated buffers (no torch glue, no allocation), by device events

Times are device-event times after a warm-up, the median of --reps runs.  The two legs' gradients are compared at the timed
size (relative L2 per tensor, printed).  Also printed: the extra device memory of a step on the route (saved tensors + the
largest workspace).

    python tools/backward_speed.py [--reps 7] [--batch 8] [--frames 1500] [--dim 512] [--layers 6]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from beat_this_amd import _lib  # noqa: E402
from beat_this_amd import weights as W  # noqa: E402
from beat_this_amd.model import BeatThis  # noqa: E402


def rmsnorm(x, gamma):
    return F.normalize(x, dim=-1) * math.sqrt(x.shape[-1]) * gamma


def rope(t, cos, sin):
    te, to = t[..., 0::2], t[..., 1::2]
    return torch.stack((te * cos - to * sin, to * cos + te * sin), dim=-1).flatten(-2)


def torch_trunk(x, p, n_layers, heads, cos, sin):
    """the trunk and the SumHead in torch ops; p: {state dict key: tensor}"""
    b, n, dim = x.shape
    for l in range(n_layers):
        a, f = f"transformer_blocks.layers.{l}.0.", f"transformer_blocks.layers.{l}.1."
        xn = rmsnorm(x, p[a + "norm.gamma"])
        q, k, v = F.linear(xn, p[a + "to_qkv.weight"]).view(b, n, 3, heads, 32).permute(2, 0, 3, 1, 4)
        o = F.scaled_dot_product_attention(rope(q, cos, sin), rope(k, cos, sin), v)
        gates = torch.sigmoid(F.linear(xn, p[a + "to_gates.weight"], p[a + "to_gates.bias"]))
        o = (o * gates.permute(0, 2, 1)[..., None]).permute(0, 2, 1, 3).reshape(b, n, dim)
        x = F.linear(o, p[a + "to_out.0.weight"]) + x
        h = F.gelu(F.linear(rmsnorm(x, p[f + "net.0.gamma"]), p[f + "net.1.weight"], p[f + "net.1.bias"]))
        x = F.linear(h, p[f + "net.4.weight"], p[f + "net.4.bias"]) + x
    x = rmsnorm(x, p["transformer_blocks.norm.gamma"])
    bd = F.linear(x, p["task_heads.beat_downbeat_lin.weight"], p["task_heads.beat_downbeat_lin.bias"])
    return bd[..., 0] + bd[..., 1], bd[..., 1]


def event_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def kernels_alone(model, x, reps):
    """the library calls of one step, unit by unit on preallocated buffers -> {unit: (forward ms, backward ms)} per call"""
    L = _lib.lib()
    dev = x.device
    B, T, D = x.shape
    H, hid = D // 32, model.hparams["ff_mult"] * D
    eng = model.engine()
    eng.ensure_positions(T)
    tb = model.transformer_blocks
    at, ff = tb.layers[0][0], tb.layers[0][1]
    lin = model.task_heads.beat_downbeat_lin
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    gy = torch.randn(B, T, D, device=dev)
    units = {}

    def args(unit, params, outs, grads):
        a = _lib.TrainArgs()
        a.B, a.T, a.dim, a.hidden, a.rope_len, a.sum_head = B, T, D, hid, eng.packed.desc.rope_len, 1
        a.rope, a.x, a.gy = eng.packed._rope_t.data_ptr(), x.data_ptr(), gy.data_ptr()
        keep = []
        for k, t in list(params.items()) + list(outs.items()) + list(grads.items()):
            setattr(a, k, t.data_ptr())
            keep.append(t)
        ws = torch.empty(max(L.bt_train_workspace_bytes(unit, bw, B, T, D, hid) for bw in (0, 1)), dtype=torch.uint8, device=dev)
        a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
        return a, keep + [ws]

    net4 = ff.net._modules["4"]
    units["attention"] = (_lib.UNIT_ATTN, *args(
        _lib.UNIT_ATTN, dict(gamma=at.norm.gamma, w1=at.to_qkv.weight, w2=at.to_gates.weight, b2=at.to_gates.bias, w3=at.to_out[0].weight),
        dict(y=new(B, T, D), save_o=new(B, T, D), save_lse=new(B, T, H)),
        dict(gx=new(B, T, D), g_gamma=new(D), g_w1=new(3 * D, D), g_w2=new(H, D), g_b2=new(H), g_w3=new(D, D))))
    units["feed-forward"] = (_lib.UNIT_FF, *args(
        _lib.UNIT_FF, dict(gamma=ff.net[0].gamma, w1=ff.net[1].weight, b1=ff.net[1].bias, w2=net4.weight, b2=net4.bias),
        dict(y=new(B, T, D)), dict(gx=new(B, T, D), g_gamma=new(D), g_w1=new(hid, D), g_b1=new(hid), g_w2=new(D, hid), g_b2=new(D))))
    units["final norm"] = (_lib.UNIT_NORM, *args(_lib.UNIT_NORM, dict(gamma=tb.norm.gamma), dict(y=new(B, T, D)),
                                                 dict(gx=new(B, T, D), g_gamma=new(D))))
    a, keep = args(_lib.TRAIN_UNIT_HEAD, dict(w1=lin.weight, b1=lin.bias), dict(y=new(B, T), y2=new(B, T)),
                   dict(gx=new(B, T, D), g_w1=new(2, D), g_b1=new(2)))
    a.gy2 = gy.data_ptr()   # ([B T] floats of it)
    units["head"] = (_lib.TRAIN_UNIT_HEAD, a, keep)
    st = _lib.stream_ptr(dev)
    out = {}
    for name, (unit, a, keep) in units.items():
        times = []
        for fn in (L.bt_train_forward, L.bt_train_backward):
            call = lambda: _lib.check(fn(st, unit, C.byref(a)))
            call()
            torch.cuda.synchronize()
            times.append(float(np.median([event_time(call) for _ in range(reps)])))
        out[name] = times
    return out


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

    def route():
        out = model.task_heads(model.transformer_blocks(x))
        return torch.autograd.grad([out["beat"], out["downbeat"]], [params[n] for n in names], [g_b, g_d])

    def restated():
        beat, down = torch_trunk(x, tparams, NL, D // 32, cos, sin)
        return torch.autograd.grad([beat, down], [tparams[n] for n in names], [g_b, g_d])

    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    a = route()
    torch.cuda.synchronize()
    peak_route = torch.cuda.max_memory_allocated(dev) - base
    b = restated()
    worst = max(float((u - v).double().norm() / v.double().norm()) for u, v in zip(a, b))
    del a, b
    for _ in range(2):
        route()
        restated()
    torch.cuda.synchronize()
    t_route, t_torch = [], []
    for _ in range(args.reps):   # (interleaved: both legs see the same clocks and the same neighbours)
        t_route.append(event_time(route))
        t_torch.append(event_time(restated))
    alone = kernels_alone(model, x, args.reps)
    per_step = sum(NL * sum(alone[u]) for u in ("attention", "feed-forward")) + sum(alone["final norm"]) + sum(alone["head"])
    Lb = _lib.lib()
    hid = hp["ff_mult"] * D
    ws = max(Lb.bt_train_workspace_bytes(u, 1, B, T, D, hid) for u in (_lib.UNIT_ATTN, _lib.UNIT_FF, _lib.UNIT_NORM, _lib.TRAIN_UNIT_HEAD))
    saved = NL * (3 * B * T * D + B * T * (D // 32)) * 4 + 2 * B * T * D * 4   # per layer: attention x, O, lse and FF x; norm x, head x
    print(json.dumps(dict(
        shape=f"B={B} T={T} D={D} L={NL} ff_mult={hp['ff_mult']}", route_ms=float(np.median(t_route)), torch_ms=float(np.median(t_torch)),
        route_ms_all=[round(t, 2) for t in t_route], torch_ms_all=[round(t, 2) for t in t_torch],
        kernels_alone_ms=round(per_step, 2), per_call_ms={k: [round(t, 3) for t in v] for k, v in alone.items()},
        worst_rel_l2_between_legs=worst, largest_workspace_bytes=int(ws), saved_bytes=int(saved), peak_extra_bytes_route=int(peak_route))),
        flush=True)


if __name__ == "__main__":
    main()
