#!/usr/bin/env python
"""Timing of the training losses (csrc/loss.hip) against the reference's formulation written in torch ops
(restated here: max_pool1d, crops, look_at, binary_cross_entropy_with_logits and autograd's backward of each).

  train: ShiftTolerantBCELoss forward + backward at the training shape, B = 8, T = 1500, beat and downbeat
         (pos_weights 1 / 4, a bool padding mask, the downbeat mask of one piece zero)
  eval:  1000 ragged pieces of 1300 - 1700 frames, each scored alone (the reference's test step, batch size 1): the fused path
         is one bt_bce_loss call for all of them; torch runs one loss per piece

Times are device-event times after a warm-up, the median of --reps runs.  At the timed sizes the fused values and gradients
are checked against the torch ones (values 1e-5 relative, gradients 1e-6 of max |grad|).

    python tools/loss_speed.py [--reps 20]
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

from beat_this_amd import _lib  # noqa: E402
from beat_this_amd.loss import SHIFT_TOLERANT, ShiftTolerantBCELoss  # noqa: E402


def torch_shift_tolerant(preds, targets, mask, pos_weight, tol=3):
    """the reference's ShiftTolerantBCELoss.forward in torch ops"""
    spread = F.max_pool1d(preds, 1 + 2 * tol, 1)[..., tol:-tol]
    cropped = targets[..., 2 * tol:-2 * tol]
    look_at = cropped + (1 - F.max_pool1d(targets, 1 + 4 * tol, 1))
    if mask is not None:
        look_at = look_at * mask[..., 2 * tol:-2 * tol]
    return F.binary_cross_entropy_with_logits(spread, cropped, weight=look_at, pos_weight=pos_weight)


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def train_leg(dev, reps):
    g = torch.Generator().manual_seed(1)
    B, T = 8, 1500
    beat = (torch.randn(B, T, generator=g) * 3).to(dev)
    down = (torch.randn(B, T, generator=g) * 3).to(dev)
    tb = torch.zeros(B, T)
    td = torch.zeros(B, T)
    for b in range(B):
        period = 20 + 3 * b
        tb[b, b::period] = 1
        td[b, b::4 * period] = 1
    tb, td = tb.to(dev), td.to(dev)
    pad = torch.ones(B, T, dtype=torch.bool)
    pad[3, 1200:] = False
    pad = pad.to(dev)
    dmask = pad * torch.tensor([1, 1, 1, 1, 1, 0, 1, 1], dtype=torch.bool, device=dev)[:, None]
    pw_b, pw_d = torch.tensor(1.0, device=dev), torch.tensor(4.0, device=dev)
    fb, fd = ShiftTolerantBCELoss(1.0).to(dev), ShiftTolerantBCELoss(4.0).to(dev)

    def run(fused):
        xb = beat.clone().requires_grad_(True)
        xd = down.clone().requires_grad_(True)
        if fused:
            total = fb(xb, tb, pad) + fd(xd, td, dmask)
        else:
            total = torch_shift_tolerant(xb, tb, pad, pw_b) + torch_shift_tolerant(xd, td, dmask.float(), pw_d)
        total.backward()
        return total.detach(), xb.grad, xd.grad

    vf, gbf, gdf = run(True)
    vt, gbt, gdt = run(False)
    assert abs(float(vf) - float(vt)) <= 1e-5 * abs(float(vt)), (float(vf), float(vt))
    for a, b in ((gbf, gbt), (gdf, gdt)):
        assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())
    return dict(leg="train B=8 T=1500 beat+downbeat fwd+bwd", fused_ms=timed(lambda: run(True), reps),
                torch_ms=timed(lambda: run(False), reps), value=float(vf))


def eval_leg(dev, reps, n=1000):
    rng = np.random.default_rng(2)
    lens = rng.integers(1300, 1701, n)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(lens)
    x = torch.from_numpy((rng.normal(0, 3, off[-1])).astype(np.float32)).to(dev)
    y = np.zeros(off[-1], np.float32)
    for i in range(n):
        y[off[i] + int(rng.integers(0, 25)):off[i + 1]:25] = 1
    y = torch.from_numpy(y).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    L = _lib.lib()
    wsb = L.bt_bce_loss_workspace_bytes(n, int(lens.max()))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    rs = torch.empty(n, dtype=torch.float64, device=dev)
    rc = torch.empty(n, dtype=torch.int64, device=dev)
    st = _lib.stream_ptr(dev)

    def fused():
        _lib.check(L.bt_bce_loss(st, SHIFT_TOLERANT, 3, 2.5, None, x.data_ptr(), 0, y.data_ptr(), 0, None, 0, d_off.data_ptr(), n,
                                 int(lens.min()), int(lens.max()), ws.data_ptr(), wsb, rs.data_ptr(), rc.data_ptr(), None, 0,
                                 None, None))

    pw = torch.tensor(2.5, device=dev)
    pieces = [(x[off[i]:off[i + 1]][None], y[off[i]:off[i + 1]][None]) for i in range(n)]
    out = torch.empty(n, device=dev)

    def reference():
        for i, (xi, yi) in enumerate(pieces):
            out[i] = torch_shift_tolerant(xi, yi, None, pw)

    fused()
    reference()
    torch.cuda.synchronize()
    mine = (rs / rc).cpu().numpy()
    ref = out.double().cpu().numpy()
    assert np.abs(mine - ref).max() <= 1e-5 * np.abs(ref).max(), np.abs(mine - ref).max()
    return dict(leg=f"eval {n} pieces of 1300-1700 frames, forward", fused_ms=timed(fused, reps),
                torch_ms=timed(reference, max(3, reps // 4), warmup=2), frames=int(off[-1]))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    args = p.parse_args(argv)
    dev = torch.device("cuda:0")
    for leg in (train_leg(dev, args.reps), eval_leg(dev, args.reps)):
        leg["speedup"] = round(leg["torch_ms"] / leg["fused_ms"], 2)
        print(json.dumps(leg), flush=True)


if __name__ == "__main__":
    main()
