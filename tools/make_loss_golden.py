#!/usr/bin/env python
"""Record tests/golden/loss_reference.npz: the reference's own loss.py (beat_this/model/loss.py) run on CPU torch over seeded
cases -- the three classes, tolerances 0 / 1 / 3 / 5, pos_weight 1 / 2.7, no / bool / float masks, binary and soft targets,
rows of exactly 1 + 4 tolerance frames and of 1500, ties (all-zero and plateau logits), a NaN logit, +-inf logits, fp16
inputs and an (N, C, T) batch.  Stored per case: the inputs, the loss value and the gradient in preds.  No test runs this.

    python tools/make_loss_golden.py /path/to/reference/checkout [out.npz]
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("MaskedBCELoss", "ShiftTolerantBCELoss", "SplittedShiftTolerantBCELoss")


def load_reference_loss(ref_root):
    path = os.path.join(ref_root, "beat_this", "model", "loss.py")
    spec = importlib.util.spec_from_file_location("reference_loss", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_targets(rng, shape, soft):
    y = (rng.random(shape) < 0.08).astype(np.float32)
    if soft:   # label smoothing, and half-height neighbours of some beats
        y = y * 0.9 + 0.05
        nb = np.roll(y, 1, axis=-1) > 0.5
        y = np.where(nb & (rng.random(shape) < 0.5), np.float32(0.5), y).astype(np.float32)
    return y


def main(argv):
    ref_root = argv[0]
    out = argv[1] if len(argv) > 1 else os.path.join(ROOT, "tests", "golden", "loss_reference.npz")
    R = load_reference_loss(ref_root)
    rng = np.random.default_rng(20261016)
    cases = []

    def add(cls, tol, pw, mask_kind, soft, shape, logits=None, dtype="float32", note=""):
        x = rng.normal(0.0, 3.0, shape).astype(np.float32) if logits is None else np.asarray(logits, np.float32).reshape(shape)
        y = make_targets(rng, shape, soft)
        m = None
        if mask_kind == "bool":
            m = rng.random(shape) < 0.85
        elif mask_kind == "float":
            m = (rng.random(shape) < 0.85).astype(np.float32)
        cases.append(dict(cls=cls, tol=tol, pw=pw, mask=mask_kind, soft=soft, dtype=dtype, note=note, x=x, y=y, m=m))

    for cls in CLASSES:
        for tol in ((0,) if cls == "MaskedBCELoss" else (0, 1, 3, 5)):
            for pw in (1.0, 2.7):
                for mask_kind in (("bool", "float") if cls.startswith("Splitted") else ("none", "bool", "float")):
                    for soft in (False, True):
                        T = 1 + 4 * tol + (0 if (len(cases) % 2 == 0 or tol == 0) else int(rng.integers(1, 10)))
                        add(cls, tol, pw, mask_kind, soft, (2, max(T, 3)))
    add("ShiftTolerantBCELoss", 3, 2.7, "bool", False, (1, 1500), note="T1500")
    add("SplittedShiftTolerantBCELoss", 3, 2.7, "float", True, (1, 1500), note="T1500")
    add("ShiftTolerantBCELoss", 3, 1.0, "none", False, (3, 2, 30), note="NCT")
    for cls in CLASSES[1:]:
        mk = "float" if cls.startswith("Splitted") else "none"
        add(cls, 3, 2.7, mk, False, (2, 40), logits=np.zeros(80), note="zeros")
        add(cls, 3, 1.0, mk, False, (2, 40), logits=np.round(rng.normal(0, 1, 80) / 2) * 2, note="plateau")
        nan = rng.normal(0, 3, 80)
        nan[17] = np.nan
        add(cls, 3, 2.7, mk, False, (2, 40), logits=nan, note="nan")
        inf = rng.normal(0, 3, 80)
        inf[[5, 30, 44, 61]] = [np.inf, -np.inf, np.inf, -np.inf]
        add(cls, 1, 2.7, mk, False, (2, 40), logits=inf, note="inf")
    add("MaskedBCELoss", 0, 2.7, "none", False, (2, 40), logits=np.array([np.inf, -np.inf] * 40), note="inf")
    add("ShiftTolerantBCELoss", 3, 2.7, "bool", False, (2, 60), dtype="float16", note="fp16")
    add("MaskedBCELoss", 0, 2.7, "float", True, (2, 60), dtype="float16", note="fp16")

    arrays, meta = {}, []
    for i, c in enumerate(cases):
        dt = getattr(torch, c["dtype"])
        x = torch.from_numpy(c["x"]).to(dt).requires_grad_(True)
        y = torch.from_numpy(c["y"]).to(dt)
        m = None if c["m"] is None else torch.from_numpy(c["m"])
        kw = {} if c["cls"] == "MaskedBCELoss" else dict(tolerance=c["tol"])
        fn = getattr(R, c["cls"])(pos_weight=c["pw"], **kw)
        value = fn(x, y, m) if m is not None or c["cls"].startswith("Splitted") else fn(x, y)
        value.backward()
        arrays[f"c{i}_x"] = x.detach().numpy()
        arrays[f"c{i}_y"] = y.numpy()
        if m is not None:
            arrays[f"c{i}_m"] = m.numpy()
        arrays[f"c{i}_grad"] = x.grad.numpy()
        arrays[f"c{i}_value"] = np.float64(value.detach().double())
        meta.append({k: c[k] for k in ("cls", "tol", "pw", "mask", "soft", "dtype", "note")} | {"value_dtype": str(value.dtype)})
    arrays["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(out, **arrays)
    print(f"{len(cases)} cases -> {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main(sys.argv[1:])
