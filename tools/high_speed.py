#!/usr/bin/env python
"""Timing of the "32-high" training precision: one training step, forward + backward, at final0 widths
(D = 512, 6 layers, ff_mult 4), B = 8, T = 1500, the legs interleaved run by run in one session on one card,

  trunk_32true / trunk_32high / trunk_bf16:   the trunk and the heads alone on the frontend's output
  model_32true / model_32high / model_bf16:   the whole model, both parts on the one precision
  trunk_torch / model_torch:                  the same two steps restated in torch ops in fp32 (tools/backward_speed.py,
                                              tools/frontend_speed.py)

"32true" is ``set_train_precision("32-true")``, "32high" ``("32-high")``, "bf16" ``("16-mixed", operand="bf16")`` (and the
frontend's setter with the same arguments in the model legs).  Times are device-event times after a warm-up; per leg the median
and the min .. max spread over --reps runs, and the peak of ``torch.cuda.max_memory_allocated`` above the step's start.

    python tools/high_speed.py [--reps 7] [--batch 8] [--frames 1500] [--dim 512] [--layers 6]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from backward_speed import torch_trunk  # noqa: E402
from front_mixed_speed import interleaved, summary  # noqa: E402
from frontend_speed import torch_frontend  # noqa: E402
from beat_this_amd import weights as W  # noqa: E402
from beat_this_amd.model import BeatThis  # noqa: E402

PRECISIONS = {"32true": ("32-true", None), "32high": ("32-high", None), "bf16": ("16-mixed", "bf16")}


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
    g_b, g_d = (torch.randn(B, T, generator=gen) * 2.0 ** -6).to(dev), (torch.randn(B, T, generator=gen) * 2.0 ** -6).to(dev)
    params = dict(model.named_parameters())
    names = [n for n in params if not n.endswith("freqs")]
    trunk_names = [n for n in names if n.startswith(("transformer_blocks.", "task_heads."))]
    tparams = {n: params[n].detach().clone().requires_grad_(True) for n in names}
    stats = {n: b for n, b in model.named_buffers()}
    freqs = sd["transformer_blocks.layers.0.0.rotary_embed.freqs"].float()
    ang = torch.arange(max(T, 32), dtype=torch.float32)[:, None] * freqs[None, :]
    cos, sin = ang.cos().to(dev), ang.sin().to(dev)

    def trunk_step(precision, operand):
        def step():
            model.set_train_precision(precision, operand)
            out = model.task_heads(model.transformer_blocks(h))
            return torch.autograd.grad([out["beat"], out["downbeat"]], [params[n] for n in trunk_names], [g_b, g_d])
        return step

    def model_step(precision, operand):
        def step():
            model.set_train_precision(precision, operand).set_frontend_precision(precision, operand)
            out = model(spect)
            return torch.autograd.grad([out["beat"], out["downbeat"]], [params[n] for n in names], [g_b, g_d])
        return step

    def trunk_torch():
        beat, down = torch_trunk(h, tparams, NL, D // 32, cos[:T], sin[:T])
        return torch.autograd.grad([beat, down], [tparams[n] for n in trunk_names], [g_b, g_d])

    def model_torch():
        beat, down = torch_trunk(torch_frontend(spect, tparams, stats, cos, sin), tparams, NL, D // 32, cos[:T], sin[:T])
        return torch.autograd.grad([beat, down], [tparams[n] for n in names], [g_b, g_d])

    legs = {}
    for tag, (precision, operand) in PRECISIONS.items():
        legs["trunk_" + tag] = trunk_step(precision, operand)
    legs["trunk_torch"] = trunk_torch
    for tag, (precision, operand) in PRECISIONS.items():
        legs["model_" + tag] = model_step(precision, operand)
    legs["model_torch"] = model_torch
    peak = {}
    for fn in legs.values():        # (a first step each: what is allocated once is no part of a step)
        fn()
    for name, fn in legs.items():
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        out = fn()
        torch.cuda.synchronize()
        peak[name] = int(torch.cuda.max_memory_allocated(dev) - base)
        del out
    res = dict(shape=f"B={B} T={T} D={D} L={NL} ff_mult={hp['ff_mult']}", reps=args.reps)
    times = interleaved(legs, args.reps)
    for k, v in summary(times).items():
        res[k + "_ms"] = v
    for part in ("trunk", "model"):
        res[f"{part}_32high_over_32true"] = round(res[f"{part}_32high_ms"]["median"] / res[f"{part}_32true_ms"]["median"], 4)
        res[f"{part}_32high_over_bf16"] = round(res[f"{part}_32high_ms"]["median"] / res[f"{part}_bf16_ms"]["median"], 4)
        res[f"{part}_32high_faster_than_32true_beyond_the_spread"] = bool(max(times[f"{part}_32high"]) < min(times[f"{part}_32true"]))
    res["peak_bytes_above_the_step_start"] = peak
    model.set_train_precision("32-true").set_frontend_precision("32-true")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
