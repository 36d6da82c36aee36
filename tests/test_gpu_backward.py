"""The GPU backward pass of the transformer trunk and the heads (csrc/train.hip, beat_this_amd/model/backward.py) against the
yardstick of route_grads.py: fp64 CPU autograd through the oracle is the truth, the fp32 oracle's worst tensor is e_ref,
and every device gradient has to be within 10 e_ref of the truth.

Tile edges of the kernels, each with a T on both sides (B = 1, so T is the number of rows):
  * attention key block = query block = 64 (BT_TRAIN_ATTN_BLOCK):            T = 63, 64, 65
  * GEMM row tile = 64 and the column sums' row chunk = 64 (BT_TRAIN_CS_ROWS): T = 63, 64, 65
  * the weight gradients' row chunk = 1024 (BT_TRAIN_DW_ROWS):                 T = 1023, 1024, 1025
and a batch-sized row count, (B, T) = (3, 700): 2100 rows, three chunks of the weight gradients, the last of 52 rows.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import route_grads as RG
import route_harness as H
from route_grads import shift_tolerant_bce
import route_reference as REF
from gpu_util import POISONS, Guarded, assert_intact, dev, report
from route_harness import make_batch, model_loss, randn
from beat_this_amd import weights as W
from oracle import beat_this_oracle as O

pytestmark = pytest.mark.gpu

SIZES = [(B, T) for T in (1, 31, 32, 33, 65, 100) for B in (1, 3)]
EDGES_64 = [(1, 63), (1, 64)]                   # (65 is in SIZES)
EDGES_1024 = [(1, 1023), (1, 1024), (1, 1025)]
BATCH = [(3, 700)]                              # more than two BT_TRAIN_DW_ROWS chunks
MODELS = {64: dict(transformer_dim=64, ff_mult=2), 192: dict(transformer_dim=192), 256: dict(transformer_dim=256)}


def make_model(D, n_layers=2, style="lively", sum_head=True, seed=3, ff_mult=None):
    """(model on the GPU with the trunk and the heads trainable, its state dict on the CPU), built once per configuration"""
    hp = dict(MODELS.get(D, dict(transformer_dim=D)), n_layers=n_layers, sum_head=sum_head)
    if ff_mult is not None:
        hp["ff_mult"] = ff_mult
    sd = H.state_dict(hp, seed, style)
    return H.make_model(hp, sd, cache=("backward", D, n_layers, style, sum_head, seed, ff_mult)), sd


def device_grads(outputs, weights, x, params):
    """gradients of sum_i (outputs[i] * weights[i]) in x and the named parameters"""
    names = [n for n, _ in params]
    grads = torch.autograd.grad(outputs, [x] + [p for _, p in params], weights, allow_unused=True)
    return {k: g for k, g in zip(["x"] + names, grads) if g is not None}


def unit_case(m, sd, kind, B, T, seed, sum_head=True):
    """one unit alone on the device and on the oracle -> (device grads, g32, g64)"""
    D = m.hparams["transformer_dim"]
    tb = m.transformer_blocks
    x = randn(B, T, D, seed=seed)
    xd = x.to(dev()).requires_grad_(True)
    if kind in ("attn", "ff"):
        layer = 1
        node = tb.layers[layer][0 if kind == "attn" else 1]
        prefix = f"transformer_blocks.layers.{layer}.{0 if kind == 'attn' else 1}."
        g = randn(B, T, D, seed=seed + 1)
        y = node(xd)
        params = [(prefix + n, p) for n, p in node.named_parameters() if not n.endswith("freqs")]
        got = device_grads([y], [g.to(dev())], xd, params)
        ref = [RG.oracle_unit_grads(kind, sd, prefix, x, g, dt, heads=D // 32) for dt in (torch.float32, torch.float64)]
    elif kind == "norm":
        g = randn(B, T, D, seed=seed + 1)
        y = tb.norm(xd)
        got = device_grads([y], [g.to(dev())], xd, [("transformer_blocks.norm.gamma", tb.norm.gamma)])
        ref = [RG.oracle_unit_grads("norm", sd, "", x, g, dt) for dt in (torch.float32, torch.float64)]
        ref = [{k: r[k] for k in ("x", "transformer_blocks.norm.gamma")} for r in ref]
    else:
        g = (randn(B, T, seed=seed + 1), randn(B, T, seed=seed + 2))
        out = m.task_heads(xd)
        params = [("task_heads." + n, p) for n, p in m.task_heads.named_parameters()]
        got = device_grads([out["beat"], out["downbeat"]], [t.to(dev()) for t in g], xd, params)
        ref = [RG.oracle_unit_grads("head", sd, "", x, g, dt, sum_head=sum_head) for dt in (torch.float32, torch.float64)]
        ref = [{k: r[k] for k in ["x"] + [n for n, _ in params]} for r in ref]
    return got, ref[0], ref[1]


# ---- 1. each unit alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style", ["lively", "init0"])
@pytest.mark.parametrize("D", [64, 192, 256])
@pytest.mark.parametrize("kind", ["ff", "attn", "norm", "head", "head_plain"])
def test_unit_against_the_yardstick(kind, D, style):
    sum_head = kind != "head_plain"
    m, sd = make_model(D, style=style, sum_head=sum_head)
    sizes = SIZES + EDGES_64 + (EDGES_1024 + BATCH if D == 64 else [])
    worst = (0.0, None)
    for i, (B, T) in enumerate(sizes):
        got, g32, g64 = unit_case(m, sd, kind.split("_")[0], B, T, seed=100 + 3 * i, sum_head=sum_head)
        e_ref, ratio = RG.check(f"unit {kind} D={D} {style} B={B} T={T}", got, g32, g64)
        worst = max(worst, (ratio, (B, T, e_ref)))
    report("backward_unit", kind=kind, D=D, style=style, worst_ratio=worst[0], at=str(worst[1]))


def test_outlier_weights_stay_finite():
    m, sd = make_model(192, style="outlier")
    B, T, D = 1, 100, 192
    x = randn(B, T, D, seed=7)
    g_b, g_d = randn(B, T, seed=8), randn(B, T, seed=9)
    got = trunk_device(m, x, g_b, g_d)
    g32, g64 = (RG.oracle_trunk_grads(sd, x, g_b, g_d, dt, 2) for dt in (torch.float32, torch.float64))
    e_ref, ratio = RG.check("trunk outlier D=192", got, g32, g64, report)


# ---- 2. whole trunk plus heads -----------------------------------------------------------------------------------------------
def trunk_device(m, x, g_b, g_d):
    xd = x.to(dev()).requires_grad_(True)
    out = m.task_heads(m.transformer_blocks(xd))
    params = [(n, p) for n, p in m.named_parameters()
              if n.startswith(("transformer_blocks.", "task_heads.")) and not n.endswith("freqs")]
    return device_grads([out["beat"], out["downbeat"]], [g_b.to(dev()), g_d.to(dev())], xd, params)


@pytest.mark.parametrize("D,L,B,T", [(128, 6, 2, 333), (512, 2, 1, 1500)])
def test_trunk_and_heads_against_the_yardstick(D, L, B, T):
    m, sd = make_model(D, n_layers=L)
    x = randn(B, T, D, seed=11)
    g_b, g_d = randn(B, T, seed=12), randn(B, T, seed=13)
    got = trunk_device(m, x, g_b, g_d)
    g32, g64 = (RG.oracle_trunk_grads(sd, x, g_b, g_d, dt, L) for dt in (torch.float32, torch.float64))
    RG.check(f"trunk D={D} L={L} B={B} T={T}", got, g32, g64, report)
    assert all(p.grad is None for p in m.parameters())   # (autograd.grad: nothing was accumulated)


# ---- 3. guard bands and poison (the C ABI directly) --------------------------------------------------------------------------
def _abi_unit(unit_name, poison, B=2, T=70, D=64, hidden=128):
    """forward + backward of one unit with every output, saved tensor and the workspace in guarded, poisoned buffers"""
    from beat_this_amd import _lib as L

    m, sd = make_model(64)
    d = dev()
    unit = dict(attn=L.UNIT_ATTN, ff=L.UNIT_FF, norm=L.UNIT_NORM, head=L.TRAIN_UNIT_HEAD)[unit_name]
    H = D // 32
    pfx = "transformer_blocks.layers.0."
    names = dict(attn=dict(gamma=pfx + "0.norm.gamma", w1=pfx + "0.to_qkv.weight", w2=pfx + "0.to_gates.weight",
                           b2=pfx + "0.to_gates.bias", w3=pfx + "0.to_out.0.weight"),
                 ff=dict(gamma=pfx + "1.net.0.gamma", w1=pfx + "1.net.1.weight", b1=pfx + "1.net.1.bias", w2=pfx + "1.net.4.weight",
                         b2=pfx + "1.net.4.bias"),
                 norm=dict(gamma="transformer_blocks.norm.gamma"),
                 head=dict(w1="task_heads.beat_downbeat_lin.weight", b1="task_heads.beat_downbeat_lin.bias"))[unit_name]
    keep = []

    def guarded(shape, data=None):
        g = Guarded(shape, torch.float32).fill(poison, data=data)
        keep.append(g)
        return g

    x = guarded((B, T, D), randn(B, T, D, seed=21).to(d))
    params = {f: guarded(sd[k].shape, sd[k].to(d)) for f, k in names.items()}
    outs = {"y": guarded((B, T) if unit_name == "head" else (B, T, D))}
    if unit_name == "head":
        outs["y2"] = guarded((B, T))
    if unit_name == "attn":
        outs["save_o"], outs["save_lse"] = guarded((B, T, D)), guarded((B, T, H))
    gy = guarded((B, T) if unit_name == "head" else (B, T, D), randn(B, T, *(() if unit_name == "head" else (D,)), seed=22).to(d))
    gy2 = guarded((B, T), randn(B, T, seed=23).to(d)) if unit_name == "head" else None
    grads = {"gx": guarded((B, T, D))}
    for f, g in params.items():
        grads["g_" + f] = guarded(g.t.shape)
    eng = m.engine()
    eng.ensure_positions(T)
    a = L.TrainArgs()
    a.B, a.T, a.dim, a.hidden, a.rope_len, a.sum_head = B, T, D, hidden, eng.packed.desc.rope_len, 1
    a.rope, a.x = eng.packed._rope_t.data_ptr(), x.ptr()
    for f, g in list(params.items()) + list(outs.items()) + list(grads.items()):
        setattr(a, f, g.ptr())
    a.gy = gy.ptr()
    a.gy2 = gy2.ptr() if gy2 is not None else None
    for backward, fn in ((0, L.lib().bt_train_forward), (1, L.lib().bt_train_backward)):
        n = L.lib().bt_train_workspace_bytes(unit, backward, B, T, D, hidden)
        ws = Guarded((n,), torch.uint8).fill(poison)
        keep.append(ws)
        a.ws, a.ws_bytes = ws.ptr(), n
        L.check(fn(L.stream_ptr(d), unit, C.byref(a)))
        torch.cuda.synchronize()
    assert_intact(*[(f"{unit_name} buffer {i}", g) for i, g in enumerate(keep)])
    return {k: g.t.clone() for k, g in list(outs.items()) + list(grads.items())}


@pytest.mark.parametrize("unit_name", ["attn", "ff", "norm", "head"])
def test_guard_bands_and_poison(unit_name):
    res = [_abi_unit(unit_name, p) for p in POISONS]
    for k in res[0]:
        assert torch.equal(res[0][k].view(torch.int32), res[1][k].view(torch.int32)), f"{unit_name}: {k} depends on the poison"
        assert torch.isfinite(res[0][k]).all(), f"{unit_name}: {k} keeps bytes of the 0xFF poison (or is not finite)"
        word = int.from_bytes(bytes([POISONS[1]] * 4), "little")
        assert not (res[1][k].view(torch.int32) == word).any(), f"{unit_name}: {k} keeps words of the 0x7B poison"


# ---- 4. reproducibility ------------------------------------------------------------------------------------------------------
def test_gradients_are_bitwise_reproducible_and_batch_invariant():
    m, sd = make_model(64)
    x = randn(3, 100, 64, seed=31)
    g_b, g_d = randn(3, 100, seed=32), randn(3, 100, seed=33)
    a = trunk_device(m, x, g_b, g_d)
    b = trunk_device(m, x, g_b, g_d)
    assert set(a) == set(b) and len(a) > 20
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    for i in range(3):
        alone = trunk_device(m, x[i:i + 1], g_b[i:i + 1], g_d[i:i + 1])
        assert torch.equal(alone["x"][0].view(torch.int32), a["x"][i].view(torch.int32)), f"sequence {i}"


# ---- 5. through the public interface -----------------------------------------------------------------------------------------
def oracle_loss_fn(batch, dtype, which=("beat", "downbeat")):
    t = {k: batch["truth_" + k].cpu().to(dtype) for k in ("beat", "downbeat")}
    mask = batch["padding_mask"].cpu().to(dtype)

    def fn(beat, down):
        o = dict(beat=beat, downbeat=down)
        return sum(shift_tolerant_bce(o[k], t[k], mask) for k in which)
    return fn


def param_grads(m):
    return {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


def test_through_the_public_interface():
    m, sd = make_model(64, seed=5)
    batch = make_batch(2, 150, seed=41)
    trunk = [n for n in RG.trainable_keys(sd)]
    with torch.no_grad():
        h = m.frontend(batch["spect"])
    refs = [RG.oracle_trunk_grads(sd, h, None, None, dt, 2, loss_fn=oracle_loss_fn(batch, dt)) for dt in (torch.float32, torch.float64)]
    refs = [{k: r[k] for k in trunk} for r in refs]
    m.zero_grad(set_to_none=True)
    loss, out = model_loss(m, batch)
    assert out["beat"].grad_fn is not None and out["downbeat"].grad_fn is not None
    loss.backward()
    got = param_grads(m)
    assert set(got) == set(trunk)
    for n, p in m.named_parameters():
        if n.startswith("frontend.") or n.endswith("freqs"):
            assert p.grad is None, n
    RG.check("public interface D=64", got, refs[0], refs[1], report)
    # the hooked route: the same gradients to within the gate
    seen = []
    hook = m.transformer_blocks.layers[0][0].register_forward_hook(lambda mod, i, o: seen.append(tuple(o.shape)))
    try:
        m.zero_grad(set_to_none=True)
        model_loss(m, batch)[0].backward()
    finally:
        hook.remove()
    assert seen == [(2, 150, 64)]
    RG.check("public interface, hooked", param_grads(m), refs[0], refs[1], report)
    # x.grad of a stage call; a loss on one output only; an expanded upstream gradient
    m.zero_grad(set_to_none=True)
    xd = h.clone().requires_grad_(True)
    y = m.transformer_blocks(xd)
    y.sum().backward()
    assert xd.grad is not None and torch.isfinite(xd.grad).all() and float(xd.grad.abs().max()) > 0
    for which, other in ((("beat",), 1), (("downbeat",), 0)):
        m.zero_grad(set_to_none=True)
        model_loss(m, batch, which)[0].backward()
        got = param_grads(m)
        r = [RG.oracle_trunk_grads(sd, h, None, None, dt, 2, loss_fn=oracle_loss_fn(batch, dt, which)) for dt in (torch.float32, torch.float64)]
        RG.check(f"public interface, only {which[0]}", got, *[{k: q[k] for k in trunk} for q in r], report)
    m.zero_grad(set_to_none=True)
    m(batch["spect"])["beat"].sum().backward()      # (the upstream gradient is an expanded scalar)
    got = param_grads(m)
    r = [RG.oracle_trunk_grads(sd, h, None, None, dt, 2, loss_fn=lambda b, d_: b.sum()) for dt in (torch.float32, torch.float64)]
    RG.check("public interface, expanded gradient", got, *[{k: q[k] for k in trunk} for q in r], report)
    m.zero_grad(set_to_none=True)
    # empty batches and zero frames keep a working backward
    for shape in ((0, 50, 128), (2, 0, 128)):
        out = m(torch.zeros(shape, device=dev()))
        assert out["beat"].shape == shape[:2] and out["downbeat"].shape == shape[:2]
        (out["beat"].sum() + out["downbeat"].sum()).backward()
    m.zero_grad(set_to_none=True)
    # the frontend is frozen
    m.frontend.linear.weight.requires_grad_(True)
    try:
        with pytest.raises(NotImplementedError, match="frontend is frozen"):
            m(batch["spect"])
        with torch.no_grad():
            m(batch["spect"])
    finally:
        m.frontend.linear.weight.requires_grad_(False)


# ---- 6. nothing existing moved -------------------------------------------------------------------------------------------------
def test_nothing_existing_moved():
    from beat_this_amd.model import BeatThis

    hp = W.resolve_hparams(dict(transformer_dim=64, ff_mult=2, n_layers=2))
    sd = W.random_state_dict(hp, seed=6, style="lively")
    m = BeatThis(**{k: hp[k] for k in ("spect_dim", "transformer_dim", "ff_mult", "n_layers", "head_dim", "stem_dim")})
    m.load_state_dict(sd)
    m = m.to(dev())
    untouched = copy.deepcopy(m)
    x = make_batch(2, 150, seed=51)["spect"]
    h = randn(2, 150, 64, seed=52).to(dev())

    def calls(model):
        out = model(x)
        fr = model.frontend(x)
        tb = model.transformer_blocks(fr)
        hd = model.task_heads(tb)
        return [out["beat"], out["downbeat"], fr, tb, hd["beat"], hd["downbeat"], model.transformer_blocks.layers[1][0](h),
                model.transformer_blocks.layers[0][1](h), model.transformer_blocks.norm(h)]

    with torch.no_grad():
        want = calls(untouched)
    default = calls(m)                                   # default parameters, grad mode on
    assert all(t.grad_fn is None and not t.requires_grad for t in default)
    m.transformer_blocks.requires_grad_(True)
    m.task_heads.requires_grad_(True)
    with torch.no_grad():
        frozen = calls(m)                                # trainable parameters under no_grad
    with torch.inference_mode():
        inference = calls(m)
    for name, res in (("default", default), ("no_grad", frozen), ("inference_mode", inference)):
        for i, (a, b) in enumerate(zip(res, want)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name}: call {i} moved"
    out = m(x)                                           # the differentiable route
    assert out["beat"].grad_fn is not None
    ob, od = O.model_forward(sd, x.cpu())
    err = max(float((out["beat"].detach().cpu() - ob).abs().max()), float((out["downbeat"].detach().cpu() - od).abs().max()))
    print(f"differentiable route: max |logit - oracle| = {err:.3e}")
    report("backward_route_logits", max_abs_err=err)
    assert err < 1e-3, err


# ---- 7. three plain SGD steps --------------------------------------------------------------------------------------------------
def test_three_sgd_steps():
    from beat_this_amd.model import BeatThis

    lr, steps = 0.02, 3
    hp = W.resolve_hparams(dict(transformer_dim=64, ff_mult=2, n_layers=2))
    sd = W.random_state_dict(hp, seed=8, style="lively")
    m = BeatThis(**{k: hp[k] for k in ("spect_dim", "transformer_dim", "ff_mult", "n_layers", "head_dim", "stem_dim")})
    m.load_state_dict(sd)
    m = m.to(dev())
    batch = make_batch(2, 150, seed=61)
    with torch.no_grad():
        before = m(batch["spect"])                       # (packs the inference engine with the initial weights)
        h = m.frontend(batch["spect"])
    m.transformer_blocks.requires_grad_(True)
    m.task_heads.requires_grad_(True)
    keys = RG.trainable_keys(sd)
    losses = []
    for _ in range(steps + 1):
        m.zero_grad(set_to_none=True)
        loss, _ = model_loss(m, batch)
        losses.append(float(loss.detach()))
        if len(losses) <= steps:
            loss.backward()
            with torch.no_grad():
                for n, p in m.named_parameters():
                    if p.grad is not None:
                        p -= lr * p.grad
    finals = {}
    for dt in (torch.float32, torch.float64):
        cur = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()}
        olosses = []
        for _ in range(steps + 1):
            leaf, _x = RG._leaves(cur, h, dt)
            beat, down = REF.trunk(leaf, h.cpu().to(dt), 2)
            ol = oracle_loss_fn(batch, dt)(beat, down)
            olosses.append(float(ol.detach()))
            if len(olosses) <= steps:
                ol.backward()
                cur = {k: ((leaf[k] - lr * leaf[k].grad).detach() if k in keys and leaf[k].grad is not None else leaf[k].detach())
                       for k in cur}
        finals[dt] = (cur, olosses)
    print("losses: device", losses, "fp32 oracle", finals[torch.float32][1])
    assert losses[-1] < losses[0], losses
    o32 = finals[torch.float32][1]
    assert o32[-1] < o32[0], o32
    delta = lambda cur: {k: cur[k].double().cpu() - sd[k].double() for k in keys}
    d32, d64 = delta(finals[torch.float32][0]), delta(finals[torch.float64][0])
    ddev = delta({n: p.detach() for n, p in m.named_parameters()})
    RG.check("three SGD steps, p_final - p_initial", ddev, d32, d64, report)
    m.eval()
    with torch.no_grad():
        after = m(batch["spect"])                        # (the packed weights are stale: the version check packs again)
    new_sd = dict(sd)
    new_sd.update({n: p.detach().cpu() for n, p in m.named_parameters()})
    ob, od = O.model_forward(new_sd, batch["spect"].cpu())
    err = max(float((after["beat"].cpu() - ob).abs().max()), float((after["downbeat"].cpu() - od).abs().max()))
    moved = float((after["beat"] - before["beat"]).abs().max())
    print(f"after training: max |logit - oracle(updated weights)| = {err:.3e}, moved from the initial logits by {moved:.3e}")
    report("backward_sgd", err_after=err, moved=moved, loss_first=losses[0], loss_last=losses[-1])
    assert err < 1e-3, err
    assert moved > 10 * err, (moved, err)


# ---- 8. graph capture ----------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay():
    from beat_this_amd.model import BeatThis

    hp = W.resolve_hparams(dict(transformer_dim=64, ff_mult=2, n_layers=2))
    sd = W.random_state_dict(hp, seed=9, style="lively")
    m = BeatThis(**{k: hp[k] for k in ("spect_dim", "transformer_dim", "ff_mult", "n_layers", "head_dim", "stem_dim")})
    m.load_state_dict(sd)
    m = m.to(dev())
    m.fp32_split_gemms = False     # (the hi + lo frontend looks at its range flag on the host after every forward)
    m.transformer_blocks.requires_grad_(True)
    m.task_heads.requires_grad_(True)
    batch = make_batch(2, 100, seed=71)
    x = batch["spect"]
    g_b, g_d = randn(2, 100, seed=72).to(dev()), randn(2, 100, seed=73).to(dev())

    def step():
        out = m(x)
        ((out["beat"] * g_b).sum() + (out["downbeat"] * g_d).sum()).backward()

    m.zero_grad(set_to_none=True)
    step()
    torch.cuda.synchronize()
    want = param_grads(m)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                        # (warm-up on a side stream, as torch asks for before a capture)
        m.zero_grad(set_to_none=True)
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    m.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for p in m.parameters():
        if p.grad is not None:
            p.grad.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    got = param_grads(m)
    assert set(got) == set(want) and len(got) > 20
    for k in want:
        assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), k
