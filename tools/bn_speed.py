#!/usr/bin/env python
"""What batch-statistics BatchNorm costs a whole-model training step: forward + backward of the model at
final0 widths (D = 512, 6 layers, ff_mult 4), B = 8, T = 1500, on the differentiable route with ``set_frontend_trainable()``,

  frozen:  the frontend's BatchNorms on their running statistics (section 17)
  batch:   ``set_batch_statistics()`` in ``train()`` mode: the statistics of each call's batch, running buffers updated

on two models with the same weights, interleaved run by run in one session.  Times are device-event times after a warm-up: the
median of --reps runs, with min ... max.  ``--units`` also times the five units that differ (the stem, the three conv units,
forward and backward) through the library calls alone, frozen against batch, to show where an excess goes.

    python tools/bn_speed.py [--reps 7] [--batch 8] [--frames 1500] [--units]
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

from beat_this_amd import _lib  # noqa: E402
from beat_this_amd import weights as W  # noqa: E402
from beat_this_amd.model import BeatThis  # noqa: E402


def event_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ts):
    return dict(median=round(float(np.median(ts)), 3), min=round(min(ts), 3), max=round(max(ts), 3))


def units_alone(model, B, T, reps):
    """the stem and the conv units through bt_front_* and bt_front_bn_* on preallocated buffers -> {unit: {leg: [fwd, bwd] ms}}"""
    L = _lib.lib()
    dev = model.device
    st = _lib.stream_ptr(dev)
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    fr = model.frontend
    out = {}
    specs = [("stem", _lib.FRONT_STEM, 128, 32, (B, T, 128), (B, T, 32, 32), fr.stem.conv2d.weight, fr.stem.bn2d, fr.stem.bn1d)]
    for i, blk in enumerate(fr.blocks):
        F_, C_ = 32 >> i, 32 << i
        specs.append((f"conv{i}", _lib.FRONT_CONV, F_, C_, (B, T, F_, C_), (B, T, F_ // 2, 2 * C_), blk.conv2d.weight, blk.norm, None))
    for name, unit, F_, C_, xs, ys, w, bn, bn1 in specs:
        x, gy = torch.rand(xs, device=dev) * 3, torch.randn(ys, device=dev)
        base = [x, gy, new(*ys), new(*ys), new(*xs), new(*w.shape)]
        keep = []
        out[name] = {}
        for leg, Args in (("frozen", _lib.FrontArgs), ("batch", _lib.FrontBnArgs)):
            a = Args(B=B, T=T, F=F_, C=C_)
            a.x, a.gy, a.y, a.save_pre, a.gx, a.g_w, a.w = (t.data_ptr() for t in (*base, w))
            for f, node in (("bn", bn), ("bn1", bn1)):
                if node is None:
                    continue
                n = node.weight.shape[0]
                mean, var = node.running_mean.clone(), node.running_var.clone()   # (the batch leg moves its own copies)
                gw, gb = new(n), new(n)
                keep += [mean, var, gw, gb]
                for k, t in (("_w", node.weight), ("_b", node.bias), ("_mean", mean), ("_var", var)):
                    setattr(a, f + k, t.data_ptr())
                setattr(a, f"g_{f}_w", gw.data_ptr())
                setattr(a, f"g_{f}_b", gb.data_ptr())
                if leg == "batch":
                    sm, sr = new(n), new(n)
                    keep += [sm, sr]
                    s = "save1" if f == "bn1" else "save"
                    setattr(a, s + "_mean", sm.data_ptr())
                    setattr(a, s + "_rstd", sr.data_ptr())
            if leg == "frozen":
                need = max(L.bt_front_workspace_bytes(unit, bw, B, T, F_, C_, 0) for bw in (0, 1))
                fns = (L.bt_front_forward, L.bt_front_backward)
            else:
                need = max(L.bt_front_bn_workspace_bytes(unit, bw, B, T, F_, C_) for bw in (0, 1))
                fns = (L.bt_front_bn_forward, L.bt_front_bn_backward)
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            a.ws, a.ws_bytes = ws.data_ptr(), need
            times = []
            for fn in fns:
                call = lambda: _lib.check(fn(st, unit, C.byref(a)))
                call()
                torch.cuda.synchronize()
                times.append(round(float(np.median([event_time(call) for _ in range(reps)])), 3))
            out[name][leg] = times
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=1500)
    ap.add_argument("--units", action="store_true")
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    B, T = args.batch, args.frames
    hp = W.resolve_hparams({})
    sd = W.random_state_dict(hp, seed=3, style="lively")
    models = {}
    for leg in ("frozen", "batch"):
        m = BeatThis(**{k: hp[k] for k in ("spect_dim", "transformer_dim", "ff_mult", "n_layers", "head_dim", "stem_dim")})
        m.load_state_dict(sd)
        m = m.to(dev).train()
        m.set_frontend_trainable()
        m.transformer_blocks.requires_grad_(True)
        m.task_heads.requires_grad_(True)
        if leg == "batch":
            m.set_batch_statistics()
        models[leg] = m
    gen = torch.Generator().manual_seed(1)
    x = (torch.rand(B, T, 128, generator=gen) * 3).to(dev)
    g_b, g_d = torch.randn(B, T, generator=gen).to(dev), torch.randn(B, T, generator=gen).to(dev)

    def step(m):
        params = [p for n, p in m.named_parameters() if p.requires_grad and not n.endswith("rotary_embed.freqs")]
        out = m(x)
        return torch.autograd.grad([out["beat"], out["downbeat"]], params, [g_b, g_d])

    for _ in range(2):   # warm-up: both legs
        for m in models.values():
            step(m)
    torch.cuda.synchronize()
    times = {leg: [] for leg in models}
    for _ in range(args.reps):   # (interleaved: both legs see the same clocks and the same neighbours)
        for leg, m in models.items():
            times[leg].append(event_time(lambda: step(m)))
    res = dict(shape=f"B={B} T={T} D={hp['transformer_dim']} L={hp['n_layers']}", frozen_ms=summary(times["frozen"]),
               batch_ms=summary(times["batch"]),
               excess_ms=round(float(np.median(times["batch"]) - np.median(times["frozen"])), 3))
    if args.units:
        res["units_alone_ms_fwd_bwd"] = units_alone(models["frozen"], B, T, args.reps)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
