"""The differentiable frontend on the GPU (csrc/train_front.hip, beat_this_amd/model/backward.py) against
the yardstick of route_grads.py: fp64 CPU autograd through the oracle is the truth, the fp32 oracle's worst tensor is e_ref,
and every device gradient has to be within 10 e_ref of the truth.

Shapes of the unit tests, B in {1, 2} x T in {1, 2, 3, 63, 64, 65, 150}:
  * T = 1 and 2: both zero pads of the time taps fall into one window;
  * B = 2: a convolution that flattens (b t) reads across the sequence boundary;
  * 63 / 64 / 65: an edge of the 64-row GEMM tile (rows = B T F');
  * B = 2, T = 65: the rows cross BT_TRAIN_DW_ROWS = 1024 and BT_TRAIN_CS_ROWS = 64 with a ragged last chunk.
"""
import copy
import shutil

import numpy as np
import pytest
import torch

import route_cases as RC
import route_grads as RG
import route_harness as H
import route_reference as REF
from gpu_util import dev, report
from route_harness import MODEL_KEYS, both_poisons, randn, same_bits
from beat_this_amd import weights as W
from oracle import beat_this_oracle as O

pytestmark = pytest.mark.gpu

HP = dict(transformer_dim=64, ff_mult=2, n_layers=2)
TS = (1, 2, 3, 63, 64, 65, 150)
UNITS = ("stem", "conv0", "conv1", "conv2", "linear", "swap")


def make_model(style="lively", sum_head=True, partial=True, seed=6, trainable=True):
    """(the model on the GPU, everything trainable behind the opt-in; its state dict on the CPU), once per configuration"""
    hp = dict(HP, sum_head=sum_head, partial_transformers=partial)
    sd = H.state_dict(hp, seed, style)
    return H.make_model(hp, sd, frontend=trainable, trunk=trainable, cache=("frontend_backward", style, sum_head, partial, seed, trainable)), sd


# ---- 1. each unit through the C ABI ------------------------------------------------------------------------------------------
def unit_spec(sd, unit, B, T):
    """(BT_FRONT_* unit, (F, C, dim), x shape, y shape, parameter fields -> state dict keys, gradient fields -> keys)"""
    from beat_this_amd import _lib as L

    bn = lambda field, p: {f"{field}_w": p + "weight", f"{field}_b": p + "bias", f"{field}_mean": p + "running_mean",
                           f"{field}_var": p + "running_var"}
    if unit == "stem":
        p = "frontend.stem."
        params = dict(w=p + "conv2d.weight", **bn("bn1", p + "bn1d."), **bn("bn", p + "bn2d."))
        grads = dict(g_w=p + "conv2d.weight", g_bn1_w=p + "bn1d.weight", g_bn1_b=p + "bn1d.bias", g_bn_w=p + "bn2d.weight",
                     g_bn_b=p + "bn2d.bias")
        return L.FRONT_STEM, (128, 32, 0), (B, T, 128), (B, T, 32, 32), params, grads
    if unit.startswith("conv"):
        i = int(unit[4])
        F_, C_ = 32 >> i, 32 << i
        p = f"frontend.blocks.{i}."
        params = dict(w=p + "conv2d.weight", **bn("bn", p + "norm."))
        grads = dict(g_w=p + "conv2d.weight", g_bn_w=p + "norm.weight", g_bn_b=p + "norm.bias")
        return L.FRONT_CONV, (F_, C_, 0), (B, T, F_, C_), (B, T, F_ // 2, 2 * C_), params, grads
    if unit == "linear":
        params = dict(w="frontend.linear.weight", b="frontend.linear.bias")
        grads = dict(g_w="frontend.linear.weight", g_b="frontend.linear.bias")
        return L.FRONT_LINEAR, (4, 256, 64), (B, T, 4, 256), (B, T, 64), params, grads
    return L.FRONT_SWAP, (16, 64, 0), (B, T, 16, 64), (B, 16, T, 64), {}, {}


def abi_unit(sd, unit, B, T, x, gy, poison):
    """forward + backward of one unit with every output, saved tensor, gradient and the workspace in guarded, poisoned buffers
    -> {"y", "save_pre" (conv), "x" (= gx), <state dict key>: gradient}"""
    _, (F_, C_, dim), *_ = unit_spec(sd, unit, B, T)
    if unit.startswith("conv"):
        return H.abi_front_unit(sd, "conv", (f"frontend.blocks.{unit[4]}.", F_, C_), B, T, x, gy, poison)
    return H.abi_front_unit(sd, unit, {"stem": None, "linear": (F_, C_, dim), "swap": (F_, C_)}[unit], B, T, x, gy, poison)


def unit_oracle(sd, unit, x, gy, dtype):
    """-> (y in the device's layout, gradients)"""
    if unit == "stem":
        y = O.stem(x.to(dtype), {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}).permute(0, 3, 2, 1)
        return y, RG.grads_only(RG.stem_grads(sd, x, gy, dtype))
    cast = {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}
    if unit.startswith("conv"):
        i = int(unit[4])
        y = REF.conv_unit(REF.to_oracle(x.to(dtype)), cast, f"frontend.blocks.{i}.").permute(0, 3, 2, 1)
        return y, RG.grads_only(RG.conv_grads(sd, i, x, gy, dtype))
    b, t, f, c = x.shape
    rows = x.to(dtype).permute(0, 1, 3, 2).reshape(b, t, c * f)
    return O._linear(rows, cast["frontend.linear.weight"], cast["frontend.linear.bias"]), RG.grads_only(RG.linear_grads(sd, x, gy, dtype))


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("unit", UNITS)
def test_unit_against_the_yardstick(unit, T):
    m, sd = make_model()
    for B in (1, 2):
        _, _, xs, ys, _, _ = unit_spec(sd, unit, B, T)
        x = RC.spect(B, T, seed=100 + T) if unit == "stem" else randn(*xs, seed=100 + T)
        gy = randn(*ys, seed=200 + T)
        got = both_poisons(f"{unit} B={B} T={T}", lambda p: abi_unit(sd, unit, B, T, x, gy, p))
        name = f"frontend {unit} B={B} T={T}"
        if unit == "swap":
            assert torch.equal(got["y"].cpu(), x.permute(0, 2, 1, 3)), name
            assert torch.equal(got["x"].cpu(), gy.permute(0, 2, 1, 3)), name
            continue
        (y32, g32), (y64, g64) = (unit_oracle(sd, unit, x, gy, dt) for dt in (torch.float32, torch.float64))
        assert all(float(v.abs().max()) > 0 for v in g64.values()), name
        RG.check(name, {k: v for k, v in got.items() if k in g64}, g32, g64, report)
        e_y = max(RG.rel(y32, y64), 1e-7)
        assert RG.rel(got["y"], y64) <= RG.GATE * e_y, (name, RG.rel(got["y"], y64), e_y)


def test_projection_over_several_weight_gradient_chunks():
    """B T = 1200 rows: the projection's weight gradient takes two BT_TRAIN_DW_ROWS chunks (the last of 176 rows) through the
    partials carved from the call's workspace, and its bias gradient 19 BT_TRAIN_CS_ROWS chunks (the last of 48 rows)"""
    m, sd = make_model()
    B, T = 2, 600
    x, gy = randn(B, T, 4, 256, seed=260), randn(B, T, 64, seed=261)
    got = both_poisons(f"linear B={B} T={T}", lambda p: abi_unit(sd, "linear", B, T, x, gy, p))
    (y32, g32), (y64, g64) = (unit_oracle(sd, "linear", x, gy, dt) for dt in (torch.float32, torch.float64))
    RG.check(f"frontend linear B={B} T={T}", {k: v for k, v in got.items() if k in g64}, g32, g64, report)
    assert RG.rel(got["y"], y64) <= RG.GATE * max(RG.rel(y32, y64), 1e-7)


def test_the_swap_serves_both_directions_at_full_length():
    """the way back from (b, f, t, c) has the 1500 time tokens in the second swapped extent"""
    from beat_this_amd.model import backward as bw

    x = randn(2, 8, 1500, 32, seed=250).to(dev()).requires_grad_(True)
    y = bw.SwapFn.apply(x)
    assert torch.equal(y, x.detach().permute(0, 2, 1, 3))
    g = randn(2, 1500, 8, 32, seed=251).to(dev())
    (gx,) = torch.autograd.grad([y], [x], [g])
    assert torch.equal(gx, g.permute(0, 2, 1, 3))
    assert torch.equal(bw.SwapFn.apply(y.detach()), x.detach())


# ---- 2. the conv GEMMs exactly ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(1, 1), (2, 2), (1, 64), (2, 65)])
@pytest.mark.parametrize("i", [0, 1, 2])
def test_conv_gemms_are_exact_on_integers(i, B, T):
    """Small integers, identity BatchNorm, and weights whose sign goes with the output channel, so that |pre| >= 64 and the
    GELU's derivative is exactly 1 (even channels) or 0 (odd ones): pre, y, g_x and g_W are integers below 2^24 and must equal
    the integer computation exactly."""
    F_, Cin = 32 >> i, 32 << i
    Cout, Fo = 2 * Cin, F_ // 2
    p = f"frontend.blocks.{i}."
    gen = torch.Generator().manual_seed(300 + i)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen)
    x = ri(1, 3, B, T, F_, Cin)
    w = ri(1, 3, Cout, Cin, 2, 3) * torch.where(torch.arange(Cout) % 2 == 0, 1, -1).view(-1, 1, 1, 1)
    gy = ri(-3, 3, B, T, Fo, Cout)
    sd = {p + "conv2d.weight": w.float(), p + "norm.weight": torch.ones(Cout), p + "norm.bias": torch.zeros(Cout),
          p + "norm.running_mean": torch.zeros(Cout), p + "norm.running_var": torch.full((Cout,), 1 - 1e-5)}
    got = both_poisons(f"conv{i} B={B} T={T}", lambda p: abi_unit(sd, f"conv{i}", B, T, x.float(), gy.float(), p))
    xp = np.zeros((B, T + 2, Fo, 2, Cin), dtype=np.int64)
    xp[:, 1:T + 1] = x.numpy().reshape(B, T, Fo, 2, Cin)
    P = np.stack([xp[:, dt:dt + T] for dt in range(3)], axis=3)            # [b, t, f', dt, df, ci]
    wn = w.numpy().astype(np.int64)                                          # [co, ci, df, dt]
    pre = np.einsum("btfdec,oced->btfo", P, wn)
    assert np.abs(pre).min() >= 64 and np.abs(pre).max() < 1 << 24
    gc = gy.numpy().astype(np.int64) * (pre > 0)
    gw = np.einsum("btfo,btfdec->oced", gc, P)
    gP = np.einsum("btfo,oced->btfdec", gc, wn)
    gxp = np.zeros_like(xp)
    for dt in range(3):
        gxp[:, dt:dt + T] += gP[:, :, :, dt]
    gx = gxp[:, 1:T + 1].reshape(B, T, F_, Cin)
    assert max(np.abs(gw).max(), np.abs(gx).max()) < 1 << 24
    for name, have, want in (("pre", got["save_pre"], pre), ("y", got["y"], pre * (pre > 0)), ("g_x", got["x"], gx),
                             ("g_W", got[p + "conv2d.weight"], gw)):
        assert np.array_equal(have.cpu().numpy().astype(np.float64), want.astype(np.float64)), f"conv{i} B={B} T={T}: {name}"
    assert np.array_equal(got[p + "norm.bias"].cpu().numpy().astype(np.float64), gc.sum((0, 1, 2)).astype(np.float64))


# ---- 3. a partial transformer block --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(2, 3), (2, 65)])
@pytest.mark.parametrize("i", [0, 1, 2])
def test_partial_transformer_against_the_yardstick(i, B, T):
    from beat_this_amd.model import backward as bw

    m, sd = make_model()
    F_, C_ = 32 >> i, 32 << i
    x, g = randn(B, T, F_, C_, seed=400 + i), randn(B, T, F_, C_, seed=410 + i)
    node = m.frontend.blocks[i].partial
    p = f"frontend.blocks.{i}.partial."

    def run():
        xd = x.to(dev()).requires_grad_(True)
        y = bw.partial_ft(node, xd, m._rope)
        params = [(p + n, q) for n, q in node.named_parameters() if not n.endswith("freqs")]
        grads = torch.autograd.grad([y], [xd] + [q for _, q in params], [g.to(dev())])
        return dict(zip(["x"] + [n for n, _ in params], grads)), y.detach()

    (got, y), (again, _) = run(), run()
    assert all(same_bits(got[k], again[k]) for k in got)
    g32, g64 = (RG.grads_only(RG.partial_grads(sd, i, x, g, dt)) for dt in (torch.float32, torch.float64))
    assert set(g64) == set(got) and len(got) == 21
    RG.check(f"frontend partial{i} B={B} T={T}", got, g32, g64, report)
    with torch.no_grad():
        want = O.partial_ft(REF.to_oracle(x.double()), {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, p)
    assert RG.rel(y, want.permute(0, 3, 2, 1)) < 1e-5


# ---- 4. the whole model ----------------------------------------------------------------------------------------------------------
def model_device(m, x, g_b, g_d):
    return H.weighted_backward(m, x, g_b, g_d)[:3]


@pytest.mark.parametrize("B,T", [(2, 150), (1, 1)])
@pytest.mark.parametrize("style,sum_head,partial", [("lively", True, True), ("init0", True, True), ("lively", False, True),
                                                    ("lively", True, False)])
def test_whole_model_against_the_yardstick(style, sum_head, partial, B, T):
    m, sd = make_model(style, sum_head, partial)
    x = RC.spect(B, T, seed=500 + T)
    g_b, g_d = randn(B, T, seed=501), randn(B, T, seed=502)
    got, beat, down = model_device(m, x, g_b, g_d)
    assert beat.shape == (B, T)
    g32, g64 = (RG.grads_only(RG.model_grads(sd, x, RG.weighted_sum(g_b, g_d, dt), dt, sum_head=sum_head)) for dt in (torch.float32, torch.float64))
    assert set(g64) == set(["x"] + RG.all_keys(sd)) and len(g64) == (100 if partial else 40)
    assert all(float(v.abs().max()) > 0 for v in g64.values())
    assert set(got) == set(g64), sorted(set(g64) ^ set(got))
    name = f"whole model {style}{'' if sum_head else ' Head'}{'' if partial else ' no partial'} B={B} T={T}"
    RG.check(name, got, g32, g64, report)
    ob, od = O.model_forward(sd, x, sum_head=sum_head)
    err = max(float((beat.cpu() - ob).abs().max()), float((down.cpu() - od).abs().max()))
    print(f"{name}: max |logit - oracle| = {err:.3e}")
    assert err < 1e-3, err
    again, beat2, _ = model_device(m, x, g_b, g_d)
    assert same_bits(beat, beat2) and all(same_bits(got[k], again[k]) for k in got), "two runs differ"
    alone, _, _ = model_device(m, x[:1], g_b[:1], g_d[:1])
    assert same_bits(alone["x"][0], got["x"][0]), "grad_x of item 0 depends on the batch"
    for n, b in m.named_buffers():
        assert torch.equal(b.cpu(), sd[n]), n


# ---- 5. nothing existing moved -----------------------------------------------------------------------------------------------------
def test_nothing_existing_moved():
    from beat_this_amd.model import BeatThis

    hp = W.resolve_hparams(HP)
    sd = W.random_state_dict(hp, seed=6, style="lively")
    m = BeatThis(**{k: hp[k] for k in MODEL_KEYS})
    m.load_state_dict(sd)
    m = m.to(dev())
    untouched = copy.deepcopy(m)
    x = torch.log1p(torch.rand(2, 150, 128, generator=torch.Generator().manual_seed(51)) * 30).to(dev())
    h = randn(2, 150, 64, seed=52).to(dev())

    def calls(model):
        out = model(x)
        fr = model.frontend(x)
        tb = model.transformer_blocks(fr)
        hd = model.task_heads(tb)
        stem = model.frontend.stem(x)
        return [out["beat"], out["downbeat"], fr, tb, hd["beat"], hd["downbeat"], model.transformer_blocks.layers[1][0](h),
                model.transformer_blocks.layers[0][1](h), model.transformer_blocks.norm(h), stem, model.frontend.blocks[0](stem)]

    def trunk_route(model):   # the trunk-only route: the frozen frontend on the fast path, gradients of the trunk and the heads
        model.zero_grad(set_to_none=True)
        out = model(x)
        (out["beat"].sum() + 2 * out["downbeat"].sum()).backward()
        res = [out["beat"].detach(), out["downbeat"].detach()] + [p.grad.clone() for p in model.parameters() if p.grad is not None]
        model.zero_grad(set_to_none=True)
        return res

    with torch.no_grad():
        want = calls(untouched)
    # without the opt-in a frontend parameter that requires grad still raises
    m.frontend.linear.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="frontend is frozen"):
        m(x)
    with pytest.raises(NotImplementedError, match="frontend is frozen"):
        m.frontend(x)
    m.frontend.linear.weight.requires_grad_(False)
    before = copy.deepcopy(m)
    before.transformer_blocks.requires_grad_(True)
    before.task_heads.requires_grad_(True)
    want_route = trunk_route(before)
    # with the opt-in, under no_grad and inference_mode: the inference paths, bit for bit
    m.set_frontend_trainable()
    m.transformer_blocks.requires_grad_(True)
    m.task_heads.requires_grad_(True)
    with torch.no_grad():
        frozen = calls(m)
    with torch.inference_mode():
        inference = calls(m)
    for name, res in (("no_grad", frozen), ("inference_mode", inference)):
        for i, (a, b) in enumerate(zip(res, want)):
            assert same_bits(a, b), f"{name}: call {i} moved"
    # in grad mode the nodes below the frontend stay inference-only
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.frontend.stem(x)
    assert m.frontend(x).grad_fn is not None and m(x)["beat"].grad_fn is not None
    # the flag off again: the trunk-only route gives the bits it gave before the flag was ever set
    m.set_frontend_trainable(False)
    assert all(not p.requires_grad for p in m.frontend.parameters())
    have_route = trunk_route(m)
    assert len(have_route) == len(want_route) == 2 + len(RG.trainable_keys(sd))
    for i, (a, b) in enumerate(zip(have_route, want_route)):
        assert same_bits(a, b), f"trunk-only route: result {i} moved"


def test_a_trained_frontend_frozen_again_runs_on_its_trained_weights():
    """The engine is packed with the initial weights by the first training step (the rotary table) and no no_grad call follows
    the optimiser step: after set_frontend_trainable(False) the frozen frontend, the trunk-only route and the inference path
    must run on the updated weights, not on the packed copies of the old ones."""
    from beat_this_amd.model import BeatThis

    hp = W.resolve_hparams(HP)
    sd = W.random_state_dict(hp, seed=9, style="lively")
    m = BeatThis(**{k: hp[k] for k in MODEL_KEYS})
    m.load_state_dict(sd)
    m = m.to(dev())
    x = RC.spect(2, 150, seed=71).to(dev())
    m.set_frontend_trainable()
    m.transformer_blocks.requires_grad_(True)
    m.task_heads.requires_grad_(True)
    out = m(x)
    (out["beat"].sum() + out["downbeat"].sum()).backward()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.grad is not None:
                p -= 0.05 * p.grad / p.grad.abs().max().clamp_min(1e-12)
    m.zero_grad(set_to_none=True)
    m.set_frontend_trainable(False)
    assert not any(p.requires_grad for p in m.frontend.parameters())
    new_sd = dict(sd)
    new_sd.update({n: p.detach().cpu() for n, p in m.named_parameters()})
    with torch.no_grad():
        ofr = O.frontend(x.cpu(), new_sd)
        ofr_old = O.frontend(x.cpu(), sd)
        ob, od = O.model_forward(new_sd, x.cpu())
    moved = float((ofr - ofr_old).abs().max())
    fr = m.frontend(x)                                   # grad mode, the flag off: the frozen frontend on the fast path
    assert fr.grad_fn is None
    e_fr = float((fr.cpu() - ofr).abs().max())
    route = m(x)                                         # the trunk-only route
    assert route["beat"].grad_fn is not None
    e_route = max(float((route["beat"].detach().cpu() - ob).abs().max()), float((route["downbeat"].detach().cpu() - od).abs().max()))
    with torch.no_grad():
        inf = m(x)
    e_inf = max(float((inf["beat"].cpu() - ob).abs().max()), float((inf["downbeat"].cpu() - od).abs().max()))
    print(f"frozen again: frontend {e_fr:.3e}, trunk-only route {e_route:.3e}, inference {e_inf:.3e} from the oracle on the "
          f"updated weights; the step moved the frontend's output by {moved:.3e}")
    assert moved > 1e-2, moved
    assert e_fr < 1e-3 and e_route < 1e-3 and e_inf < 1e-3, (e_fr, e_route, e_inf)


# ---- 6. the training loop ----------------------------------------------------------------------------------------------------------
def test_three_adamw_steps_on_all_parameters():
    from test_gpu_backward import make_batch, model_loss
    from beat_this_amd.model import BeatThis
    from beat_this_amd.optim import AdamW, param_groups_for

    hp = W.resolve_hparams(HP)
    sd = W.random_state_dict(hp, seed=8, style="lively")
    m = BeatThis(**{k: hp[k] for k in MODEL_KEYS})
    m.load_state_dict(sd)
    m = m.to(dev())
    batch = make_batch(2, 150, seed=61)
    with torch.no_grad():
        before = m(batch["spect"])                       # (packs the inference engine with the initial weights)
    m.set_frontend_trainable()
    m.transformer_blocks.requires_grad_(True)
    m.task_heads.requires_grad_(True)
    for n, p in m.named_parameters():                    # (the rotary tables are fixed, as in PLBeatThis)
        if n.endswith("rotary_embed.freqs"):
            p.requires_grad_(False)
    m.train()
    stats = {n: b.clone() for n, b in m.named_buffers()}
    assert len(stats) == 3 * 5
    opt = AdamW(param_groups_for(m, 0.01), lr=2e-3)
    assert sum(len(g["params"]) for g in opt.param_groups) == len(RG.all_keys(sd))
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss, _ = model_loss(m, batch)
        losses.append(float(loss.detach()))
        if len(losses) <= 3:
            loss.backward()
            opt.step()
    print("losses:", losses)
    assert losses[-1] < losses[0], losses
    for n, b in m.named_buffers():
        assert torch.equal(b, stats[n]) and b.dtype == stats[n].dtype, f"{n} changed in train() mode"
    moved = [n for n, p in m.named_parameters() if n.startswith("frontend.") and not torch.equal(p.detach().cpu(), sd[n])]
    assert len(moved) == len(RG.frontend_keys(sd)), "every frontend weight takes part in the step"
    m.eval()
    with torch.no_grad():
        after = m(batch["spect"])                        # (the packed frontend weights are stale: the version check packs again)
        fr = m.frontend(batch["spect"])
    new_sd = dict(sd)
    new_sd.update({n: p.detach().cpu() for n, p in m.named_parameters()})
    with torch.no_grad():
        ob, od = O.model_forward(new_sd, batch["spect"].cpu())
        ofr = O.frontend(batch["spect"].cpu(), new_sd)
    err = max(float((after["beat"].cpu() - ob).abs().max()), float((after["downbeat"].cpu() - od).abs().max()))
    moved_by = float((after["beat"] - before["beat"]).abs().max())
    print(f"after training: max |logit - oracle(updated weights)| = {err:.3e}, moved from the initial logits by {moved_by:.3e}")
    report("frontend_adamw", err_after=err, moved=moved_by, loss_first=losses[0], loss_last=losses[-1])
    assert err < 1e-3, err
    assert float((fr.cpu() - ofr).abs().max()) < 1e-3
    assert moved_by > 10 * err, (moved_by, err)


def test_fit_with_the_frontend_resumes_bit_for_bit(tmp_path):
    from dataset_reference import build_data_folder
    from beat_this_amd.inference import load_checkpoint, load_model
    from beat_this_amd.train import fit
    from test_gpu_finetune import EPOCHS, new_datamodule, new_module

    root = build_data_folder(str(tmp_path / "data"))
    ck, first, ck2 = (str(tmp_path / n) for n in ("run.ckpt", "epoch0.ckpt", "resumed.ckpt"))

    def log(line):
        if line.startswith("epoch 0:"):
            shutil.copy(ck, first)

    pl = new_module()
    np.random.seed(0)
    h = fit(pl, new_datamodule(root), EPOCHS, val_frequency=1, checkpoint_path=ck, log=log, train_frontend=True)
    print("train_loss per epoch:", h["train_loss"])     # (whether two epochs at this rate lower it is not what is checked here)
    assert pl.model.frontend_trainable and len(h["train_loss"]) == EPOCHS and all(np.isfinite(v) for v in h["train_loss"])
    pl2 = new_module()
    np.random.seed(99)
    h2 = fit(pl2, new_datamodule(root), EPOCHS, val_frequency=1, checkpoint_path=ck2, resume=first, log=lambda s: None,
             train_frontend=True)
    assert len(h2["train_loss"]) == 1
    a, b = load_checkpoint(ck), load_checkpoint(ck2)
    for k, v in a["state_dict"].items():
        assert torch.equal(v, b["state_dict"][k]), k
    sa, sb = a["optimizer_states"][0], b["optimizer_states"][0]
    n_all = len(RG.all_keys(pl.model.state_dict()))
    assert len(sa["state"]) == len(sb["state"]) == n_all     # (the larger optimiser state: the frontend's weights are in it)
    for i in sa["state"]:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(torch.as_tensor(sa["state"][i][k]), torch.as_tensor(sb["state"][i][k])), (i, k)
    fresh = new_module()
    moved = [n for (n, p), q in zip(fresh.model.named_parameters(), pl.model.parameters())
             if n.startswith("frontend.") and not torch.equal(p.detach(), q.detach())]
    assert len(moved) == len(RG.frontend_keys(fresh.model.state_dict())), len(moved)
    for (n, p), q in zip(fresh.model.named_buffers(), pl.model.buffers()):
        assert torch.equal(p, q), f"{n} changed during fit"
    loaded = load_model(ck, dev())
    x = torch.log1p(torch.rand(1, 150, 128, generator=torch.Generator().manual_seed(5)) * 30).to(dev())
    with torch.no_grad():
        assert same_bits(loaded(x)["beat"], pl.model(x)["beat"])


# ---- 7. errors ---------------------------------------------------------------------------------------------------------------------
def test_limits_and_misplaced_operands_raise_before_any_launch():
    from beat_this_amd.model import BeatThis

    m, sd = make_model()
    for B, T in ((1, 65536), (2, 32768), (16, 4096)):
        x = torch.zeros(1, 1, 128, device=dev()).expand(B, T, 128)    # (no memory behind it: nothing may read it)
        with pytest.raises(ValueError, match="65535 frames"):
            m.frontend(x)
        with pytest.raises(ValueError, match="65535 frames"):
            m(x)
    with pytest.raises(ValueError):
        m.frontend(torch.zeros(1, 8, 64, device=dev()))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m(torch.zeros(1, 8, 128))
    hp = W.resolve_hparams(HP)
    cpu = BeatThis(**{k: hp[k] for k in MODEL_KEYS})
    cpu.set_frontend_trainable()
    with pytest.raises(RuntimeError, match="ROCm GPU|no CPU implementation"):
        cpu(torch.zeros(1, 8, 128, device=dev()))
    # one operand left behind on the CPU
    from beat_this_amd.model import backward as bw

    blk = m.frontend.blocks[0]
    with pytest.raises(RuntimeError, match="same ROCm GPU"):
        bw.ConvUnitFn.apply(torch.zeros(1, 4, 32, 32, device=dev()), blk.conv2d.weight.detach().cpu(), blk.norm.weight, blk.norm.bias,
                            blk.norm.running_mean, blk.norm.running_var)
    # empty batches and zero frames keep a working backward
    for shape in ((0, 50, 128), (2, 0, 128)):
        out = m(torch.zeros(shape, device=dev()))
        assert out["beat"].shape == shape[:2]
        (out["beat"].sum() + out["downbeat"].sum()).backward()
    m.zero_grad(set_to_none=True)
