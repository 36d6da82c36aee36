#!/usr/bin/env python
"""What frontend dropout costs: one whole-model training step, forward + backward, at final0 widths
(D = 512, 6 layers, ff_mult 4), B = 8, T = 1500, the legs interleaved run by run in one session on one card:

  fp32_none / fp32_trunk / fp32_both:     the differentiable route in fp32 without dropout, with the trunk's dropout
                                          (``enable_dropout(seed)``, 0.2) and with the frontend's on top
                                          (``enable_dropout(seed, frontend=True)``, 0.1 in the twelve leaves)
  mixed_none / mixed_trunk / mixed_both:  the same three with both precisions "16-mixed"
  torch_none / torch_drop:                the whole model restated in torch ops (fp32), without dropout and with
                                          ``F.scaled_dot_product_attention(dropout_p=...)`` / ``F.dropout`` at the reference's
                                          sites of the leaves (0.1) and of the trunk (0.2); torch's own generator and masks: the
                                          time is comparable, the numbers are not

Times are device-event times after a warm-up; per leg the median and the min .. max over --reps runs.  Also printed: what the
trunk's dropout adds (trunk - none), what the frontend's adds on top (both - trunk) and the frontend's share of the sum -- the
time-direction leaves hold as many attention probabilities as the trunk, 3 x B x 32 x T^2 against 6 x B x 16 x T^2.

    python tools/front_dropout_speed.py [--reps 7] [--batch 8] [--frames 1500] [--dim 512] [--layers 6]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from backward_speed import rmsnorm, rope  # noqa: E402
from dropout_speed import torch_trunk  # noqa: E402
from front_mixed_speed import interleaved, summary  # noqa: E402
from beat_this_amd import weights as W  # noqa: E402
from beat_this_amd.model import BeatThis  # noqa: E402

P_FRONT, P_TRUNK = 0.1, 0.2


def torch_pair(x, p, a, f, cos, sin, rate):
    """tools/frontend_speed.py's leaf pair with the reference's four dropouts (roformer.py): x + attention, then + feed-forward"""
    b, n, dim = x.shape
    heads = dim // 32
    drop = (lambda t: F.dropout(t, rate)) if rate > 0 else (lambda t: t)
    xn = rmsnorm(x, p[a + "norm.gamma"])
    q, k, v = F.linear(xn, p[a + "to_qkv.weight"]).view(b, n, 3, heads, 32).permute(2, 0, 3, 1, 4)
    o = F.scaled_dot_product_attention(rope(q, cos[:n], sin[:n]), rope(k, cos[:n], sin[:n]), v, dropout_p=rate)
    gates = torch.sigmoid(F.linear(xn, p[a + "to_gates.weight"], p[a + "to_gates.bias"]))
    o = (o * gates.permute(0, 2, 1)[..., None]).permute(0, 2, 1, 3).reshape(b, n, dim)
    x = drop(F.linear(o, p[a + "to_out.0.weight"])) + x
    h = drop(F.gelu(F.linear(rmsnorm(x, p[f + "net.0.gamma"]), p[f + "net.1.weight"], p[f + "net.1.bias"])))
    return drop(F.linear(h, p[f + "net.4.weight"], p[f + "net.4.bias"])) + x


def torch_frontend(x, p, stats, cos, sin, rate):
    """tools/frontend_speed.py's frontend with dropout at ``rate`` in the leaves of the partial transformers"""
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
            y = torch_pair(y, p, q + "partial.attnF.", q + "partial.ffF.", cos, sin, rate)
            y = y.view(b, t, f, c).permute(0, 2, 1, 3).reshape(b * f, t, c)
            y = torch_pair(y, p, q + "partial.attnT.", q + "partial.ffT.", cos, sin, rate)
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
    keys = ("spect_dim", "transformer_dim", "ff_mult", "n_layers", "head_dim", "stem_dim")
    model = BeatThis(**{k: hp[k] for k in keys}, dropout={"frontend": P_FRONT, "transformer": P_TRUNK})
    model.load_state_dict(sd)
    model = model.to(dev)
    model.set_frontend_trainable()
    model.transformer_blocks.requires_grad_(True)
    model.task_heads.requires_grad_(True)
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

    def device_step(precision, dropout):
        def step():
            model.set_train_precision(precision).set_frontend_precision(precision)
            if dropout == "none":
                model.disable_dropout().eval()
            else:
                model.enable_dropout(seed=1, frontend=dropout == "both").train()
            out = model(spect)
            return torch.autograd.grad([out["beat"], out["downbeat"]], [params[n] for n in names], [g_b, g_d])
        return step

    def restated(front, trunk):
        def step():
            h = torch_frontend(spect, tparams, stats, cos, sin, front)
            beat, down = torch_trunk(h, tparams, NL, D // 32, cos[:T], sin[:T], trunk)
            return torch.autograd.grad([beat, down], [tparams[n] for n in names], [g_b, g_d])
        return step

    legs = {f"{name}_{dropout}": device_step(precision, dropout)
            for name, precision in (("fp32", "32-true"), ("mixed", "16-mixed")) for dropout in ("none", "trunk", "both")}
    legs["torch_none"], legs["torch_drop"] = restated(0.0, 0.0), restated(P_FRONT, P_TRUNK)
    res = dict(shape=f"B={B} T={T} D={D} L={NL} ff_mult={hp['ff_mult']} p_frontend={P_FRONT} p_transformer={P_TRUNK}", reps=args.reps)
    times = summary(interleaved(legs, args.reps))
    model.disable_dropout().eval()
    for k, v in times.items():
        res[k + "_ms"] = v
    med = {k: v["median"] for k, v in times.items()}
    for name in ("fp32", "mixed"):
        trunk, front = med[name + "_trunk"] - med[name + "_none"], med[name + "_both"] - med[name + "_trunk"]
        res[name + "_increase_ms"] = dict(trunk=round(trunk, 2), frontend=round(front, 2),
                                          frontend_share=round(front / (trunk + front), 3) if trunk + front > 0 else None)
    res["torch_increase_ms"] = round(med["torch_drop"] - med["torch_none"], 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
