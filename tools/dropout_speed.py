#!/usr/bin/env python
"""What dropout costs on the fine-tuning route (csrc/dropout.h, csrc/train.hip): forward + backward of
``task_heads(transformer_blocks(x))`` at final0 widths (D = 512, 6 layers, ff_mult 4), B = 8, T = 1500, four legs interleaved
run by run in one session:

  A:   the route without dropout (the code path of tools/backward_speed.py's ``route`` leg)
  B:   the route with dropout enabled at p (``BeatThis.enable_dropout``, ``train()`` mode): Philox4x32-10 evaluated in the kernels
  C:   the trunk restated in torch ops with ``F.scaled_dot_product_attention(dropout_p=p)`` and ``F.dropout`` at the other three
       sites (torch's own generator and masks: the time is comparable, the numbers are not)
  C0:  the same restatement without dropout, so that C - C0 is what dropout costs torch

Times are device-event times after a warm-up, the median of --reps runs.  Also timed alone, on preallocated buffers: the
attention's and the feed-forward's library calls with and without dropout, which shows where B - A goes.

    python tools/dropout_speed.py [--reps 7] [--batch 8] [--frames 1500] [--dim 512] [--layers 6] [--p 0.2]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from backward_speed import event_time, rmsnorm, rope  # noqa: E402
from beat_this_amd import _lib  # noqa: E402
from beat_this_amd import weights as W  # noqa: E402
from beat_this_amd.model import BeatThis  # noqa: E402


def torch_trunk(x, p, n_layers, heads, cos, sin, rate):
    """tools/backward_speed.py's restatement with the reference's four dropouts per layer (roformer.py)"""
    b, n, dim = x.shape
    drop = (lambda t: F.dropout(t, rate)) if rate > 0 else (lambda t: t)
    for l in range(n_layers):
        a, f = f"transformer_blocks.layers.{l}.0.", f"transformer_blocks.layers.{l}.1."
        xn = rmsnorm(x, p[a + "norm.gamma"])
        q, k, v = F.linear(xn, p[a + "to_qkv.weight"]).view(b, n, 3, heads, 32).permute(2, 0, 3, 1, 4)
        o = F.scaled_dot_product_attention(rope(q, cos, sin), rope(k, cos, sin), v, dropout_p=rate)
        gates = torch.sigmoid(F.linear(xn, p[a + "to_gates.weight"], p[a + "to_gates.bias"]))
        o = (o * gates.permute(0, 2, 1)[..., None]).permute(0, 2, 1, 3).reshape(b, n, dim)
        x = drop(F.linear(o, p[a + "to_out.0.weight"])) + x
        h = drop(F.gelu(F.linear(rmsnorm(x, p[f + "net.0.gamma"]), p[f + "net.1.weight"], p[f + "net.1.bias"])))
        x = drop(F.linear(h, p[f + "net.4.weight"], p[f + "net.4.bias"])) + x
    x = rmsnorm(x, p["transformer_blocks.norm.gamma"])
    bd = F.linear(x, p["task_heads.beat_downbeat_lin.weight"], p["task_heads.beat_downbeat_lin.bias"])
    return bd[..., 0] + bd[..., 1], bd[..., 1]


def units_alone(model, x, reps, rate):
    """the attention's and the feed-forward's library calls on preallocated buffers
    -> {unit: {"plain": [forward ms, backward ms], "dropout": [forward ms, backward ms]}}"""
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
    specs = {
        "attention": (_lib.UNIT_ATTN, dict(gamma=at.norm.gamma, w1=at.to_qkv.weight, w2=at.to_gates.weight, b2=at.to_gates.bias,
                                           w3=at.to_out[0].weight, y=new(B, T, D), save_o=new(B, T, D), save_lse=new(B, T, H),
                                           gx=new(B, T, D), g_gamma=new(D), g_w1=new(3 * D, D), g_w2=new(H, D), g_b2=new(H),
                                           g_w3=new(D, D))),
        "feed-forward": (_lib.UNIT_FF, dict(gamma=ff.net[0].gamma, w1=ff.net[1].weight, b1=ff.net[1].bias, w2=net4.weight,
                                            b2=net4.bias, y=new(B, T, D), gx=new(B, T, D), g_gamma=new(D), g_w1=new(hid, D),
                                            g_b1=new(hid), g_w2=new(D, hid), g_b2=new(D))),
    }
    st = _lib.stream_ptr(dev)
    d = _lib.TrainDropout(p=rate, seed=1, stream=0)
    out = {}
    for name, (unit, fields) in specs.items():
        a = _lib.TrainArgs()
        a.B, a.T, a.dim, a.hidden, a.rope_len = B, T, D, hid, eng.packed.desc.rope_len
        a.rope, a.x, a.gy = eng.packed._rope_t.data_ptr(), x.data_ptr(), gy.data_ptr()
        for k, t in fields.items():
            setattr(a, k, t.data_ptr())
        ws = torch.empty(L.bt_train_workspace_bytes_dropout(unit, 1, B, T, D, hid), dtype=torch.uint8, device=dev)
        a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
        out[name] = {}
        for leg, dp in (("plain", None), ("dropout", C.byref(d))):
            times = []
            for fn in (L.bt_train_forward_dropout, L.bt_train_backward_dropout):
                call = lambda: _lib.check(fn(st, unit, C.byref(a), dp))
                call()
                torch.cuda.synchronize()
                times.append(float(np.median([event_time(call) for _ in range(reps)])))
            out[name][leg] = times
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=1500)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--p", type=float, default=0.2)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    B, T, D, NL, rate = args.batch, args.frames, args.dim, args.layers, args.p
    hp = W.resolve_hparams(dict(transformer_dim=D, n_layers=NL))
    sd = W.random_state_dict(hp, seed=3, style="lively")
    keys = ("spect_dim", "transformer_dim", "ff_mult", "n_layers", "head_dim", "stem_dim")
    model = BeatThis(**{k: hp[k] for k in keys}, dropout={"frontend": 0.1, "transformer": rate})
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

    def route(dropout):
        def step():
            if dropout:
                model.enable_dropout(seed=1).train()
            else:
                model.disable_dropout().eval()
            out = model.task_heads(model.transformer_blocks(x))
            return torch.autograd.grad([out["beat"], out["downbeat"]], [params[n] for n in names], [g_b, g_d])
        return step

    def restated(r):
        def step():
            beat, down = torch_trunk(x, tparams, NL, D // 32, cos, sin, r)
            return torch.autograd.grad([beat, down], [tparams[n] for n in names], [g_b, g_d])
        return step

    legs = {"A": route(False), "B": route(True), "C": restated(rate), "C0": restated(0.0)}
    for _ in range(2):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.reps):   # (interleaved: every leg sees the same clocks and the same neighbours)
        for k, fn in legs.items():
            times[k].append(event_time(fn))
    model.disable_dropout().eval()
    alone = units_alone(model, x, args.reps, rate)
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps(dict(
        shape=f"B={B} T={T} D={D} L={NL} ff_mult={hp['ff_mult']} p={rate}", A_route_ms=med["A"], B_route_dropout_ms=med["B"],
        C_torch_dropout_ms=med["C"], C0_torch_ms=med["C0"], route_increase_ms=med["B"] - med["A"], torch_increase_ms=med["C"] - med["C0"],
        all_ms={k: [round(t, 2) for t in v] for k, v in times.items()},
        per_call_ms={u: {leg: [round(t, 3) for t in v] for leg, v in legs_.items()} for u, legs_ in alone.items()})), flush=True)


if __name__ == "__main__":
    main()
