#!/usr/bin/env python
"""Record tests/golden/trunk_grads.npz: gradients of the reference's own transformer trunk and task heads, run on CPU torch.

The reference's ``BeatThis`` (transformer_dim 64, one layer, ff_mult 1, zero dropout, eval(), float32) is loaded with
``random_state_dict(seed=3, style="lively")``; a seeded ``x = randn(2, 40, 64)`` goes through
``task_heads(transformer_blocks(x))`` and ``(beat * g_b).sum() + (downbeat * g_d).sum()`` is backpropagated with seeded
``g_b``, ``g_d``.  Stored: x, g_b, g_d, the gradient of x (``grad.x``) and of every trunk / head parameter that receives one
(``grad.<state dict key>``), all fp32.  No test runs this; tests/test_trunk_grad_reference.py pins the oracle's restatement
(the accuracy yardstick of the GPU backward) to the file.

    python tools/make_trunk_grad_golden.py /path/to/reference/checkout [out.npz]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HPARAMS = dict(transformer_dim=64, n_layers=1, ff_mult=1)
SEED_WEIGHTS, SEED_DATA = 3, 20261017


def main(argv):
    ref_root = os.path.abspath(argv[0])
    out = argv[1] if len(argv) > 1 else os.path.join(ROOT, "tests", "golden", "trunk_grads.npz")
    sys.path[:0] = [os.path.join(ROOT, "oracle", "shims"), ref_root, ROOT]
    from beat_this.model.beat_tracker import BeatThis

    from beat_this_amd.weights import random_state_dict, resolve_hparams

    hp = resolve_hparams(HPARAMS)
    model = BeatThis(spect_dim=hp["spect_dim"], transformer_dim=hp["transformer_dim"], ff_mult=hp["ff_mult"],
                     n_layers=hp["n_layers"], head_dim=hp["head_dim"], stem_dim=hp["stem_dim"],
                     dropout={"frontend": 0.0, "transformer": 0.0}, sum_head=hp["sum_head"],
                     partial_transformers=hp["partial_transformers"]).float().eval()
    model.load_state_dict(random_state_dict(hp, seed=SEED_WEIGHTS, style="lively"))
    gen = torch.Generator().manual_seed(SEED_DATA)
    x = torch.randn(2, 40, 64, generator=gen).requires_grad_(True)
    g_b = torch.randn(2, 40, generator=gen)
    g_d = torch.randn(2, 40, generator=gen)
    model.zero_grad()
    y = model.task_heads(model.transformer_blocks(x))
    ((y["beat"] * g_b).sum() + (y["downbeat"] * g_d).sum()).backward()
    arrays = {"x": x.detach().numpy(), "g_b": g_b.numpy(), "g_d": g_d.numpy(), "grad.x": x.grad.numpy()}
    for name, p in model.named_parameters():
        if name.startswith(("transformer_blocks.", "task_heads.")) and p.grad is not None:
            arrays["grad." + name] = p.grad.to(torch.float32).numpy()
    np.savez_compressed(out, **arrays)
    print(f"{out}: {len(arrays)} arrays, {os.path.getsize(out)} bytes")
    for k, v in arrays.items():
        print(f"  {k:70s} {tuple(v.shape)}  |.| = {float(np.linalg.norm(v)):.4g}")


if __name__ == "__main__":
    main(sys.argv[1:])
