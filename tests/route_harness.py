"""The device side of the training route's GPU tests (test_gpu_backward, _dropout, _mixed, _frontend_backward, _batch_stats,
_front_mixed, _front_dropout, _train_route, _finetune*, _ema, _optim): random inputs, the bit comparison, the run under both
poison bytes, the model factory, the whole-model backward and the 16-mixed gate.  Where the tests' own copies differed in
strength, this is the strongest of them.  The comparisons work on CPU tensors too (tests/test_route_harness.py)."""
import ctypes as C

import numpy as np
import torch

import route_grads as RG
from gpu_util import POISONS, Guarded, assert_intact, dev

MODEL_KEYS = ("spect_dim", "transformer_dim", "ff_mult", "n_layers", "head_dim", "stem_dim", "sum_head", "partial_transformers")
MIXED_GATE = 2.0
POISON_WORD = int.from_bytes(bytes([POISONS[1]] * 4), "little")
_CACHE = {}


def randn(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def same_bits(a, b):
    """the same shape, the same dtype and the same bytes, whatever the dtype"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().reshape(-1).view(torch.uint8),
                                                                     b.contiguous().reshape(-1).view(torch.uint8))


def _words(t):
    """the payload as 32-bit words (a trailing part of less than a word is left out)"""
    raw = t.contiguous().reshape(-1).view(torch.uint8)
    return raw[:raw.numel() // 4 * 4].view(torch.int32)


def both_poisons(name, run):
    """run(poison) under both poison bytes -> the first result.  A result is a dict of tensors or a tuple of such dicts.  The two
    runs have to be bit-identical; a float tensor has to be finite (0xFF is a NaN in every float format) and free of the 0x7B
    word; an integer tensor is compared exactly and may hold any value."""
    res = [run(p) for p in POISONS]
    parts = [r if isinstance(r, (tuple, list)) else (r,) for r in res]
    assert len(parts[0]) == len(parts[1]), name
    for first, second in zip(*parts):
        assert set(first) == set(second), f"{name}: the two runs return different tensors"
        for k in first:
            a, b = first[k], second[k]
            assert same_bits(a, b), f"{name}: {k} differs between two runs (or depends on the poison)"
            if a.is_floating_point():
                assert torch.isfinite(a).all(), f"{name}: {k} keeps bytes of the 0xFF poison (or is not finite)"
                assert not (_words(b) == POISON_WORD).any(), f"{name}: {k} keeps words of the 0x7B poison"
    return res[0]


# ---- models -----------------------------------------------------------------------------------------------------------------------
def state_dict(hp, seed, style, counters=0):
    """``weights.random_state_dict`` of the resolved ``hp``, one object per configuration; ``counters``: added to every
    num_batches_tracked (an update that overwrites instead of blending shows)"""
    from beat_this_amd import weights as W

    key = ("sd", tuple(sorted(hp.items())), seed, style, counters)
    if key not in _CACHE:
        sd = W.random_state_dict(W.resolve_hparams(hp), seed=seed, style=style)
        for k in sd:
            if counters and k.endswith("num_batches_tracked"):
                sd[k] = sd[k] + counters
        _CACHE[key] = sd
    return _CACHE[key]


def make_model(hp, sd, *, frontend=False, trunk=True, freeze_freqs=False, dropout=None, cache=None):
    """``BeatThis(hp)`` with the weights ``sd`` on the GPU, the trunk and the heads trainable (``trunk``); ``frontend``: the frontend
    too, behind its opt-in; ``freeze_freqs``: the rotary tables stay fixed; ``dropout``: the constructor's rates.  ``cache``: None = a model of
    the caller's own, else a hashable key under which the tests that leave its state as they found it share one model."""
    from beat_this_amd import weights as W
    from beat_this_amd.model import BeatThis

    if cache is not None and ("model", cache) in _CACHE:
        return _CACHE["model", cache]
    hp = W.resolve_hparams(hp)
    m = BeatThis(**{k: hp[k] for k in MODEL_KEYS}, **({} if dropout is None else {"dropout": dropout}))
    m.load_state_dict(sd)
    m = m.to(dev())
    if frontend:
        m.set_frontend_trainable()
    if trunk:
        m.transformer_blocks.requires_grad_(True)
        m.task_heads.requires_grad_(True)
    if freeze_freqs:
        for n, p in m.named_parameters():
            if n.endswith("rotary_embed.freqs"):
                p.requires_grad_(False)
    if cache is not None:
        _CACHE["model", cache] = m
    return m


def make_batch(B, T, seed):
    """the device entries of a ``ds.batch(...)`` result"""
    gen = torch.Generator().manual_seed(seed)
    spect = torch.log1p(torch.rand(B, T, 128, generator=gen) * 30)
    beat = torch.rand(B, T, generator=gen) < 0.06
    down = beat & (torch.rand(B, T, generator=gen) < 0.3)
    mask = torch.ones(B, T, dtype=torch.bool)
    mask[-1, T - 20:] = False
    d = dev()
    return dict(spect=spect.to(d), truth_beat=beat.to(d), truth_downbeat=down.to(d), padding_mask=mask.to(d))


# ---- the whole model's backward ---------------------------------------------------------------------------------------------------
def weighted_backward(m, x, g_b, g_d):
    """gradients of sum(beat g_b) + sum(downbeat g_d) -> (gradients by name and "x", beat, downbeat, the buffers after the call)"""
    m.zero_grad(set_to_none=True)
    xd = x.to(dev()).requires_grad_(True)
    out = m(xd)
    (out["beat"] * g_b.to(dev())).sum().add((out["downbeat"] * g_d.to(dev())).sum()).backward()
    got = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    got["x"] = xd.grad.clone()
    m.zero_grad(set_to_none=True)
    return got, out["beat"].detach(), out["downbeat"].detach(), {n: b.detach().clone() for n, b in m.named_buffers()}


def loss_backward(forward, m, x, beat, down, mask, scale=1.0):
    """gradients of the shift-tolerant loss of ``forward(x on the device)`` = {"beat", "downbeat"}, taken of loss * scale and
    divided by scale -> {<parameter name>, "x", "beat", "downbeat"}"""
    from beat_this_amd.model.loss import ShiftTolerantBCELoss

    m.zero_grad(set_to_none=True)
    xd = x.to(dev()).requires_grad_(True)
    out = forward(xd)
    fn = ShiftTolerantBCELoss().to(dev())
    loss = fn(out["beat"], beat.to(dev()), mask.to(dev()).bool()) + fn(out["downbeat"], down.to(dev()), mask.to(dev()).bool())
    (loss * scale).backward()
    res = {n: p.grad / scale for n, p in m.named_parameters() if p.grad is not None}
    res.update(x=xd.grad / scale, beat=out["beat"].detach(), downbeat=out["downbeat"].detach())
    m.zero_grad(set_to_none=True)
    return res


def model_device(m, x, beat, down, mask, scale=1.0):
    return loss_backward(m, m, x, beat, down, mask, scale)


# ---- one frontend unit through the C ABI ----------------------------------------------------------------------------------------------
def abi_front_unit(sd, unit, dims, B, T, x, gy, poison, mixed=False, batch=False):
    """Forward + backward of one frontend unit through bt_front_* (running statistics) or, with ``batch``, bt_front_bn_* (batch
    statistics), fp32 or 16-mixed.  unit, dims: "stem", None; "conv", (key prefix, F, C); "linear", (F, C, dim); "swap", (F, C).
    Every input, parameter, running buffer, saved tensor, output, gradient and the workspaces are ``Guarded`` buffers filled with
    ``poison``; their bands are checked once, after the backward.
    -> {"y", "save_pre" (conv), "x" (= gx), <state dict key>: gradient}; with ``batch`` a pair of that and {<key>: running
    buffer after the forward} (the backward must leave them alone)."""
    from beat_this_amd import _lib as L

    d, keep, bias = dev(), [], None
    if unit == "stem":
        code, F_, C_, dim, xs, ys = L.FRONT_STEM, 128, 32, 0, (B, T, 128), (B, T, 32, 32)
        wkey, bns = "frontend.stem.conv2d.weight", {"bn1": "frontend.stem.bn1d.", "bn": "frontend.stem.bn2d."}
    elif unit == "conv":
        p, F_, C_ = dims
        code, dim, xs, ys = L.FRONT_CONV, 0, (B, T, F_, C_), (B, T, F_ // 2, 2 * C_)
        wkey, bns = p + "conv2d.weight", {"bn": p + "norm."}
    elif unit == "linear":
        F_, C_, dim = dims
        code, xs, ys = L.FRONT_LINEAR, (B, T, F_, C_), (B, T, dim)
        wkey, bns, bias = "frontend.linear.weight", {}, "frontend.linear.bias"
    else:
        F_, C_ = dims
        code, dim, xs, ys, wkey, bns = L.FRONT_SWAP, 0, (B, T, F_, C_), (B, F_, T, C_), None, {}
    assert not batch or unit in ("stem", "conv")

    def guarded(shape, data=None, dtype=torch.float32):
        g = Guarded(shape, dtype).fill(poison, data=None if data is None else data.to(d))
        keep.append(g)
        return g

    a = L.FrontBnArgs(B=B, T=T, F=F_, C=C_) if batch else L.FrontArgs()
    if not batch:
        a.B, a.T, a.F, a.C, a.dim = B, T, F_, C_, dim
    a.mixed = int(mixed)
    a.x, a.gy = guarded(xs, x).ptr(), guarded(ys, gy).ptr()
    outs = {"y": guarded(ys), "x": guarded(xs)}
    a.y, a.gx = outs["y"].ptr(), outs["x"].ptr()
    if unit == "conv":
        outs["save_pre"] = guarded(ys)
        a.save_pre = outs["save_pre"].ptr()
    for field, key in (("w", wkey), ("b", bias)):
        if key is not None:
            setattr(a, field, guarded(sd[key].shape, sd[key]).ptr())
            outs[key] = guarded(sd[key].shape)
            setattr(a, "g_" + field, outs[key].ptr())
    stats = {}
    for f, p in bns.items():
        n = sd[p + "weight"].shape
        for leaf, field in (("weight", "_w"), ("bias", "_b")):
            setattr(a, f + field, guarded(n, sd[p + leaf]).ptr())
            outs[p + leaf] = guarded(n)
            setattr(a, f"g_{f}{field}", outs[p + leaf].ptr())
        stats[p + "running_mean"], stats[p + "running_var"] = guarded(n, sd[p + "running_mean"]), guarded(n, sd[p + "running_var"])
        setattr(a, f + "_mean", stats[p + "running_mean"].ptr())
        setattr(a, f + "_var", stats[p + "running_var"].ptr())
        if batch:
            stats[p + "num_batches_tracked"] = guarded((1,), sd[p + "num_batches_tracked"].reshape(1), torch.int64)
            setattr(a, f + "_tracked", stats[p + "num_batches_tracked"].ptr())
            save = "save1" if f == "bn1" else "save"
            setattr(a, save + "_mean", guarded(n).ptr())
            setattr(a, save + "_rstd", guarded(n).ptr())
    lib = L.lib()
    if batch:
        size = lambda query, backward: query(code, backward, B, T, F_, C_)
        query, plain = (lib.bt_front_bn_workspace_bytes_mixed if mixed else lib.bt_front_bn_workspace_bytes), None
        calls = (lib.bt_front_bn_forward, lib.bt_front_bn_backward)
    else:
        size = lambda query, backward: query(code, backward, B, T, F_, C_, dim)
        query, plain = (lib.bt_front_workspace_bytes_mixed, lib.bt_front_workspace_bytes) if mixed else (lib.bt_front_workspace_bytes, None)
        calls = (lib.bt_front_forward, lib.bt_front_backward)
    after = None
    for backward, fn in enumerate(calls):
        n = size(query, backward)
        assert n > 0 and (plain is None or n >= size(plain, backward))
        ws = guarded((n,), dtype=torch.uint8)
        a.ws, a.ws_bytes = ws.ptr(), n
        L.check(fn(L.stream_ptr(d), code, C.byref(a)))
        torch.cuda.synchronize()
        if batch and not backward:
            after = {k: g.t.clone().reshape(sd[k].shape) for k, g in stats.items()}
    for k in after or ():
        assert same_bits(stats[k].t.reshape(sd[k].shape), after[k]), f"{unit}: the backward touched {k}"
    assert_intact(*[(f"{unit} buffer {i}", g) for i, g in enumerate(keep)])
    res = {k: g.t.clone() for k, g in outs.items()}
    return (res, after) if batch else res


# ---- the 16-mixed gate --------------------------------------------------------------------------------------------------------------
def mixed_gate(name, got, truth, e_ref16, keys=None, extra=(), scale=None, report=None):
    """every gradient of ``keys`` (the truth's gradients) and every tensor of ``extra`` within 2 x e_ref16 of the fp64 truth and
    finite; prints the figures first -> the worst gradient's distance in e_ref16"""
    keys = RG.grad_keys(truth) if keys is None else list(keys)
    assert np.isfinite(e_ref16) and e_ref16 > 0 and set(keys) <= set(got), name
    errs = {k: RG.rel(got[k], truth[k]) for k in keys}
    k = max(errs, key=errs.get)
    at = "" if scale is None else f" (scale {scale:g})"
    print(f"{name}: e_ref16 = {e_ref16:.3e}{at}, worst device error = {errs[k]:.3e} ({errs[k] / e_ref16:.2f} x e_ref16, {k})")
    for key in extra:
        errs[key] = RG.rel(got[key], truth[key])
        print(f"{name}: {key} {errs[key]:.3e} ({errs[key] / e_ref16:.2f} x e_ref16)")
    if report is not None:
        report("front_mixed", case=name, e_ref16=e_ref16, worst_ratio=errs[k] / e_ref16, worst_tensor=k)
    for key, e in errs.items():
        assert torch.isfinite(got[key]).all(), f"{name}: {key} is not finite"
        assert e <= MIXED_GATE * e_ref16, f"{name}: {key} is {e:.3e} from the fp64 truth, the gate is 2 x e_ref16 = {MIXED_GATE * e_ref16:.3e}"
    return errs[k] / e_ref16
