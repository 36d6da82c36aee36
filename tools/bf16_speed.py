#!/usr/bin/env python
"""Timing of the operand formats of 16-mixed: one whole-model training step, forward + backward, at final0
widths (D = 512, 6 layers, ff_mult 4), B = 8, T = 1500, legs interleaved run by run in one session on one card,

  fp32:   fp32 trunk + fp32 frontend (the frame of reference)
  fp16:   both parts 16-mixed on fp16 operands
  bf16:   both parts 16-mixed on bfloat16 operands (``set_train_precision("16-mixed", operand="bf16")`` and the frontend's)

Times are device-event times after a warm-up; per leg the median and the min .. max spread over --reps runs.  The step is the
one of tools/front_mixed_speed.py; the loss scale is no part of it (a multiplication of the loss and, in the optimiser step, a
4-byte read-back that bfloat16 does without).

    python tools/bf16_speed.py [--reps 9] [--batch 8] [--frames 1500] [--dim 512] [--layers 6]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from front_mixed_speed import interleaved, summary  # noqa: E402
from beat_this_amd import weights as W  # noqa: E402
from beat_this_amd.model import BeatThis  # noqa: E402


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
    model = BeatThis(**{k: hp[k] for k in ("spect_dim", "transformer_dim", "ff_mult", "n_layers", "head_dim", "stem_dim")})
    model.load_state_dict(W.random_state_dict(hp, seed=3, style="lively"))
    model = model.to(dev)
    model.set_frontend_trainable()
    model.transformer_blocks.requires_grad_(True)
    model.task_heads.requires_grad_(True)
    gen = torch.Generator().manual_seed(1)
    spect = (torch.rand(B, T, 128, generator=gen) * 3).to(dev)
    g_b, g_d = (torch.randn(B, T, generator=gen) * 2.0 ** -6).to(dev), (torch.randn(B, T, generator=gen) * 2.0 ** -6).to(dev)
    params = [p for n, p in model.named_parameters() if not n.endswith("freqs")]

    def device_step(precision, operand):
        def step():
            model.set_train_precision(precision, operand).set_frontend_precision(precision, operand)
            out = model(spect)
            return torch.autograd.grad([out["beat"], out["downbeat"]], params, [g_b, g_d])
        return step

    legs = {"fp32": device_step("32-true", None), "fp16": device_step("16-mixed", "fp16"), "bf16": device_step("16-mixed", "bf16")}
    res = dict(shape=f"B={B} T={T} D={D} L={NL} ff_mult={hp['ff_mult']}", reps=args.reps)
    for k, v in summary(interleaved(legs, args.reps)).items():
        res[k + "_ms"] = v
    res["bf16_over_fp16"] = round(res["bf16_ms"]["median"] / res["fp16_ms"]["median"], 4)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
