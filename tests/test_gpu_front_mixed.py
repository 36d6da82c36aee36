"""16-mixed in the differentiable frontend on the GPU (csrc/train_front_mixed.inc): the fp16 conv GEMMs
exactly on integers, the fp16 staging, then the units, the partial transformers and the whole model within 2 x e_ref16 of the fp64
truth (route_reference.py: e_ref16 is the autocast oracle's own error at the case's loss scale), and the contract and the
plumbing: determinism, isolation, refused arguments, the opt-in, AdamW steps under a LossScaler, ``fit`` and the command line.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import route_cases as RC
import route_grads as RG
import route_harness as H
from gpu_util import POISONS, dev, report
from route_harness import MIXED_GATE as GATE, MODEL_KEYS, both_poisons, make_batch, model_device, model_loss, new_datamodule, new_module, same_bits
from beat_this_amd import weights as W
from oracle import beat_this_oracle as O

pytestmark = pytest.mark.gpu
FAR = 0.25   # a mixed result is at least this many e_ref16 from the truth: the restatement sits at 0.8, the fp32 route at 1e-3


# ---- the units through the C ABI, guarded and poisoned -----------------------------------------------------------------------------
def conv_spec(i=None, F_=None, C_=None):
    """a conv unit: block i's shape, or any (F, C); -> (key prefix, F, C)"""
    if i is not None:
        F_, C_ = 32 >> i, 32 << i
    return f"frontend.blocks.{0 if i is None else i}.", F_, C_


def abi_front(sd, unit, dims, B, T, x, gy, poison, mixed):
    """forward + backward of BT_FRONT_CONV (dims = (prefix, F, C)) or BT_FRONT_LINEAR (dims = (F, C, dim)) through bt_front_*,
    fp32 or (``mixed``) on fp16 operands"""
    return H.abi_front_unit(sd, unit, dims, B, T, x, gy, poison, "fp16" if mixed else None)


def abi_conv_bn(sd, i, B, T, x, gy, poison, mixed):
    """the same of conv unit i through bt_front_bn_* -> (results, {<key>: running buffer after the forward})"""
    return H.abi_front_unit(sd, "conv", conv_spec(i), B, T, x, gy, poison, "fp16" if mixed else None, batch=True)


# ---- 1. exact on integers ----------------------------------------------------------------------------------------------------------
def integer_case(F_, Cin, B, T, seed):
    """Integers whose products all carry the sign of the output channel: x = sigma_ci |x| with |x| in 1 .. 4, w = s_co sigma_ci |w|
    with |w| in 1 .. 2, sigma and s random signs per input and alternating per output channel, so x covers [-4, 4] without 0 and
    w [-2, 2] without 0, and |pre| >= 2 Cin >= 64: the GELU is exactly pre or 0 and its derivative exactly 1 or 0.  g in [-3, 3].
    -> (state dict of an identity BatchNorm, x, g, the integer results)"""
    Cout, Fo = 2 * Cin, F_ // 2
    p = "frontend.blocks.0."
    gen = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen)
    sigma = ri(0, 1, Cin) * 2 - 1
    s_co = torch.where(torch.arange(Cout) % 2 == 0, 1, -1)
    x = ri(1, 4, B, T, F_, Cin) * sigma
    w = ri(1, 2, Cout, Cin, 2, 3) * sigma.view(1, -1, 1, 1) * s_co.view(-1, 1, 1, 1)
    gy = ri(-3, 3, B, T, Fo, Cout)
    sd = {p + "conv2d.weight": w.float(), p + "norm.weight": torch.ones(Cout), p + "norm.bias": torch.zeros(Cout),
          p + "norm.running_mean": torch.zeros(Cout), p + "norm.running_var": torch.full((Cout,), 1 - 1e-5)}
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
    want = {"save_pre": pre, "y": pre * (pre > 0), "x": gx, p + "conv2d.weight": gw, p + "norm.bias": gc.sum((0, 1, 2))}
    return sd, x.float(), gy.float(), want


def assert_exact(name, got, want):
    for k, v in want.items():
        assert np.array_equal(got[k].cpu().numpy().astype(np.float64), v.astype(np.float64)), f"{name}: {k}"


SHAPES_EXACT = [(32 >> i, 32 << i, B, T) for i in (0, 1, 2) for B, T in ((1, 1), (2, 2), (1, 64), (2, 65))] + [(6, 96, 2, 3), (2, 32, 2, 3)]


@pytest.mark.parametrize("F_,Cin,B,T", SHAPES_EXACT)
def test_conv_gemms_are_exact_on_integers(F_, Cin, B, T):
    """(32, 32) at (2, 65): 2080 rows, so g_W covers three BT_TRAIN_DW_ROWS chunks, the last of 32 rows; C = 96: 192 and 576
    columns; C = 32, F = 2: one output bin per frame"""
    sd, x, gy, want = integer_case(F_, Cin, B, T, 700 + Cin + T)
    name = f"mixed conv F={F_} C={Cin} B={B} T={T}"
    got = both_poisons(name, lambda p: abi_front(sd, "conv", ("frontend.blocks.0.", F_, Cin), B, T, x, gy, p, True))
    assert_exact(name, got, want)


@pytest.mark.parametrize("F_,Cin", [(32, 32), (16, 64), (8, 128), (6, 96), (2, 32)])
def test_operands_are_rounded_to_fp16_as_they_are_staged(F_, Cin):
    """x = n + 2^-13, n a non-zero integer in [-4, 4]: fp16 rounds that to n, so the mixed route gives the integer computation on
    n exactly -- and the fp32 route does not, which shows that the flag selects another kernel"""
    B, T = 2, 2
    sd, x, gy, want = integer_case(F_, Cin, B, T, 800 + Cin)
    xe = x + 2.0 ** -13
    assert not torch.equal(xe, x) and torch.equal(xe.to(torch.float16).float(), x)
    name = f"mixed conv staging F={F_} C={Cin}"
    got = both_poisons(name, lambda p: abi_front(sd, "conv", ("frontend.blocks.0.", F_, Cin), B, T, xe, gy, p, True))
    assert_exact(name, got, want)
    fp32 = abi_front(sd, "conv", ("frontend.blocks.0.", F_, Cin), B, T, xe, gy, POISONS[0], False)
    assert not np.array_equal(fp32["save_pre"].cpu().numpy().astype(np.float64), want["save_pre"].astype(np.float64))
    assert not np.array_equal(fp32["frontend.blocks.0.conv2d.weight"].cpu().numpy().astype(np.float64),
                              want["frontend.blocks.0.conv2d.weight"].astype(np.float64))


# ---- 2. the units against the yardstick --------------------------------------------------------------------------------------------
def gate(name, got, case, extra=("y",)):
    """every gradient (and y) within GATE x e_ref16 of the fp64 truth; -> the worst gradient's distance in e_ref16"""
    return H.mixed_gate(name, got, case["truth"], case["e_ref16"], None, extra, case["scale"], report)


def unscale(res, scale):
    return {k: (v if k in ("y", "save_pre") else v / scale) for k, v in res.items()}


@pytest.mark.parametrize("B,T", RC.CONV_SIZES)
@pytest.mark.parametrize("i", [0, 1, 2])
def test_conv_units_within_twice_e_ref16(i, B, T):
    case = RC.conv_case(i, B, T)
    name = f"mixed conv{i} B={B} T={T}"
    run = lambda p: abi_front(case["sd"], "conv", conv_spec(i), B, T, case["x"], case["g"] * case["scale"], p, True)
    got = unscale(both_poisons(name, run), case["scale"])
    away = gate(name, got, case)
    assert away >= FAR, f"{name}: {away:.3f} x e_ref16 from the truth -- the fp32 route's distance, not fp16 products'"


@pytest.mark.parametrize("B,T", RC.BN_SIZES)
@pytest.mark.parametrize("i", [0, 1, 2])
def test_conv_units_with_batch_statistics(i, B, T):
    """The moved running buffers by section 18's rule with the autocast oracle as the reference: within GATE x max(e, 1e-7) of
    the fp64 update, e the autocast oracle's own distance for that buffer (it takes the moments of products of rounded operands
    rounded once more; the device's products are not rounded again)."""
    case = RC.conv_case(i, B, T, batch=True)
    name = f"mixed conv{i} batch statistics B={B} T={T}"
    sd = dict(case["sd"])
    run = lambda p: abi_conv_bn(sd, i, B, T, case["x"], case["g"] * case["scale"], p, True)
    res, stats = both_poisons(name, run)
    away = gate(name, unscale(res, case["scale"]), case)
    assert away >= FAR, (name, away)
    for k, want in case["truth"]["stats"].items():
        if k.endswith("num_batches_tracked"):
            assert int(stats[k]) == int(want), k
            continue
        e = max(RG.rel(case["auto"]["stats"][k], want), 1e-7)
        err = RG.rel(stats[k], want)
        print(f"{name}: {k} autocast {e:.3e}, device {err:.3e} ({err / e:.2f} x)")
        assert torch.isfinite(stats[k]).all() and err <= GATE * e, (name, k, err, e)


@pytest.mark.parametrize("B,T", RC.LINEAR_SIZES)
def test_projection_within_twice_e_ref16(B, T):
    case = RC.linear_case(B, T)
    name = f"mixed projection B={B} T={T}"
    run = lambda p: abi_front(case["sd"], "linear", (4, 256, 64), B, T, case["x"], case["g"] * case["scale"], p, True)
    got = unscale(both_poisons(name, run), case["scale"])
    assert gate(name, got, case) >= FAR, name


def model_on_device(style="lively", partial=True):
    """the D = 64 model of route_cases.model_state_dict on the GPU, everything trainable; one per configuration"""
    return H.make_model(dict(RC.HP, partial_transformers=partial), RC.model_state_dict(style, partial), frontend=True, freeze_freqs=True,
                        cache=("front_mixed", style, partial))


@pytest.mark.parametrize("B,T", RC.PARTIAL_SIZES)
@pytest.mark.parametrize("i", [0, 1, 2])
def test_partial_transformers_within_twice_e_ref16(i, B, T):
    from beat_this_amd.model import backward as bw

    case = RC.partial_case(i, B, T)
    m = model_on_device()
    node, p = m.frontend.blocks[i].partial, f"frontend.blocks.{i}.partial."

    def run():
        xd = case["x"].to(dev()).requires_grad_(True)
        y = bw.partial_ft(node, xd, m._rope, mixed=True)
        params = [(p + n, q) for n, q in node.named_parameters() if not n.endswith("freqs")]
        grads = torch.autograd.grad([y], [xd] + [q for _, q in params], [(case["g"] * case["scale"]).to(dev())])
        res = {k: g / case["scale"] for k, g in zip(["x"] + [n for n, _ in params], grads)}
        res["y"] = y.detach()
        return res

    got, again = run(), run()
    assert len(got) == 22 and all(same_bits(got[k], again[k]) for k in got)
    assert gate(f"mixed partial{i} B={B} T={T}", got, case) >= FAR


# ---- 3. the whole model --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", RC.MODEL_SIZES)
@pytest.mark.parametrize("partial", [True, False])
@pytest.mark.parametrize("style", ["lively", "init0"])
def test_whole_model_within_twice_e_ref16(style, partial, B, T):
    case = RC.model_case(style, partial, B, T)
    m = model_on_device(style, partial)
    name = f"mixed whole model {style}{'' if partial else ' no partial'} B={B} T={T}"
    try:
        m.set_frontend_precision("16-mixed").set_train_precision("16-mixed")
        got = model_device(m, case["x"], case["beat"], case["down"], case["mask"], case["scale"])
    finally:
        m.set_frontend_precision("32-true").set_train_precision("32-true")
    keys = RG.grad_keys(case["truth"])
    assert set(keys) == set(got) - {"beat", "downbeat"} and len(keys) == (100 if partial else 40)
    gate(name, got, case, extra=())
    for k in ("beat", "downbeat"):
        e16, e = RG.rel(case["auto"][k], case["truth"][k]), RG.rel(got[k], case["truth"][k])
        print(f"{name} {k} logits: autocast {e16:.3e}, device {e:.3e}")
        assert e <= GATE * e16, (k, e, e16)


# ---- 4. the contract and the plumbing --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 2])
def test_a_sequence_alone_gives_the_same_input_gradient(i):
    case = RC.conv_case(i, 2, 65)
    g = case["g"] * case["scale"]
    both = abi_front(case["sd"], "conv", conv_spec(i), 2, 65, case["x"], g, POISONS[0], True)
    alone = abi_front(case["sd"], "conv", conv_spec(i), 1, 65, case["x"][:1], g[:1], POISONS[1], True)
    assert same_bits(alone["x"][0], both["x"][0]) and same_bits(alone["y"][0], both["y"][0])


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("B,T", [(2, 3), (1, 65)])
@pytest.mark.parametrize("i", [0, 2])
def test_save_pre_has_the_same_bits_on_both_statistics(i, B, T, mixed):
    """bt_front_bn_forward runs the conv GEMM of bt_front_forward with its GELU output suppressed: the saved ``pre`` of the same x
    and weight has the same bits on running and on batch statistics, fp32 and mixed.  Unit 0 has 96 and 1040 rows: across the
    64-row tile, no multiple of it, and across 1024."""
    x, g = RC.conv_inputs(i, B, T)
    sd = RC.model_state_dict()
    running = abi_front(sd, "conv", conv_spec(i), B, T, x, g, POISONS[0], mixed)
    batch, _ = abi_conv_bn(sd, i, B, T, x, g, POISONS[1], mixed)
    assert torch.isfinite(running["save_pre"]).all() and same_bits(batch["save_pre"], running["save_pre"])


def test_the_autograd_functions_pass_the_flag_on():
    """ConvUnitFn, ConvUnitBatchFn and ProjectionFn with mixed=True make the calls the C-ABI tests above make: the same bits"""
    from beat_this_amd.model import BeatThis
    from beat_this_amd.model import backward as bw

    hp = W.resolve_hparams(RC.HP)
    m = BeatThis(**{k: hp[k] for k in MODEL_KEYS})     # (its own: the batch-statistics call moves its running buffers)
    m.load_state_dict(RC.model_state_dict())
    m = m.to(dev()).set_frontend_trainable()
    i, B, T = 1, 2, 3
    case = RC.conv_case(i, B, T)
    blk, p, g = m.frontend.blocks[i], f"frontend.blocks.{i}.", case["g"] * case["scale"]
    for batch in (False, True):
        want = (abi_conv_bn(case["sd"], i, B, T, case["x"], g, POISONS[0], True)[0] if batch else
                abi_front(case["sd"], "conv", conv_spec(i), B, T, case["x"], g, POISONS[0], True))
        xd = case["x"].to(dev()).requires_grad_(True)
        y = bw.conv_unit(blk, xd, batch, True)
        grads = torch.autograd.grad([y], [xd, blk.conv2d.weight, blk.norm.weight, blk.norm.bias], [g.to(dev())])
        got = dict(zip(("x", p + "conv2d.weight", p + "norm.weight", p + "norm.bias"), grads), y=y.detach())
        for k, v in got.items():
            assert same_bits(v, want[k]), (batch, k)
    case = RC.linear_case(B, T)
    g = case["g"] * case["scale"]
    want = abi_front(case["sd"], "linear", (4, 256, 64), B, T, case["x"], g, POISONS[0], True)
    xd = case["x"].to(dev()).requires_grad_(True)
    y = bw.ProjectionFn.apply(xd, m.frontend.linear.weight, m.frontend.linear.bias, True)
    grads = torch.autograd.grad([y], [xd, m.frontend.linear.weight, m.frontend.linear.bias], [g.to(dev())])
    for k, v in dict(zip(("x", "frontend.linear.weight", "frontend.linear.bias"), grads), y=y.detach()).items():
        assert same_bits(v, want[k]), k


def test_refused_arguments():
    from beat_this_amd import _lib as L

    lib, s = L.lib(), L.stream_ptr(dev())
    shapes = {L.FRONT_STEM: (128, 32, 0), L.FRONT_SWAP: (16, 64, 0), L.FRONT_CONV: (32, 32, 0), L.FRONT_LINEAR: (4, 256, 64)}
    for unit, (F_, C_, dim) in shapes.items():
        for backward in (0, 1):
            n32, n16 = (q(unit, backward, 2, 3, F_, C_, dim) for q in (lib.bt_front_workspace_bytes, lib.bt_front_workspace_bytes_mixed))
            assert n32 > 0
            assert (n16 == 0) == (unit in (L.FRONT_STEM, L.FRONT_SWAP)), unit
            if unit == L.FRONT_CONV:
                assert n16 == n32 + 2 * 64 * 6 * 32      # the fp16 weight image
            if unit == L.FRONT_LINEAR:
                assert n16 == n32
    for unit in (L.FRONT_STEM, L.FRONT_CONV):
        F_, C_, _ = shapes[unit]
        n16 = lib.bt_front_bn_workspace_bytes_mixed(unit, 0, 2, 3, F_, C_)
        assert lib.bt_front_bn_workspace_bytes(unit, 0, 2, 3, F_, C_) > 0 and (n16 == 0) == (unit == L.FRONT_STEM)
    for backward in (0, 1):                               # the same weight image on batch statistics: 24 C^2 bytes
        n32, n16 = (q(L.FRONT_CONV, backward, 2, 3, 32, 32) for q in (lib.bt_front_bn_workspace_bytes, lib.bt_front_bn_workspace_bytes_mixed))
        assert n32 > 0 and n16 == n32 + 24 * 32 * 32
    assert lib.bt_front_workspace_bytes_mixed(L.FRONT_CONV, 0, 2, 3, 32, 48, 0) == 0      # an unsupported width
    assert lib.bt_front_bn_workspace_bytes_mixed(L.FRONT_CONV, 0, 1, 1, 2, 32) == 0       # one value per channel
    # refused before any launch: the pointers below are null, so a launch would be seen
    for unit, mixed in ((L.FRONT_STEM, 1), (L.FRONT_SWAP, 1), (L.FRONT_CONV, 2), (L.FRONT_LINEAR, 2), (L.FRONT_CONV, -1)):
        F_, C_, dim = shapes[unit]
        a = L.FrontArgs()
        a.B, a.T, a.F, a.C, a.dim, a.mixed = 2, 3, F_, C_, dim, mixed
        assert lib.bt_front_forward(s, unit, C.byref(a)) == L.BT_ERR_ARG
        assert lib.bt_front_backward(s, unit, C.byref(a)) == L.BT_ERR_ARG
        assert b"mixed" in lib.bt_last_error()
    for unit, mixed in ((L.FRONT_STEM, 1), (L.FRONT_CONV, 2)):
        F_, C_, _ = shapes[unit]
        b = L.FrontBnArgs(B=2, T=3, F=F_, C=C_, mixed=mixed)
        assert lib.bt_front_bn_forward(s, unit, C.byref(b)) == L.BT_ERR_ARG
        assert lib.bt_front_bn_backward(s, unit, C.byref(b)) == L.BT_ERR_ARG
        assert b"mixed" in lib.bt_last_error()
    torch.cuda.synchronize()


def fresh_model():
    return H.make_model(RC.HP, RC.model_state_dict("init0"), frontend=True, freeze_freqs=True)


def test_the_trunk_precision_alone_leaves_the_frontend_as_it_was():
    """set_train_precision("16-mixed") without the new opt-in: the whole-model gradients of a model that never opted in and of
    one that was switched to "16-mixed" and back are the same bits; with the opt-in they are others"""
    never, switched = fresh_model(), fresh_model()
    x, beat, down, mask = RC.model_inputs(2, 33, True)
    assert never.frontend_precision == switched.frontend_precision == "32-true"
    never.set_train_precision("16-mixed")
    want = model_device(never, x, beat, down, mask, 1024.0)
    assert switched.set_frontend_precision("16-mixed") is switched and switched.frontend_precision == "16-mixed"
    switched.set_train_precision("16-mixed")
    mixed = model_device(switched, x, beat, down, mask, 1024.0)
    front = [k for k in want if k.startswith("frontend.blocks")]
    assert len(want) == len(mixed) == 102 and all(not same_bits(mixed[k], want[k]) for k in front)
    with torch.no_grad():   # inference never looks at the switch
        a, b = never(x.to(dev())), switched(x.to(dev()))
    assert same_bits(a["beat"], b["beat"]) and same_bits(a["downbeat"], b["downbeat"])
    switched.set_frontend_precision("32-true")
    back = model_device(switched, x, beat, down, mask, 1024.0)
    for k in want:
        assert same_bits(back[k], want[k]), k
    for bad in ("bf16-mixed", "16", None):
        with pytest.raises(ValueError):
            switched.set_frontend_precision(bad)
    with pytest.raises(AttributeError):
        switched.frontend_precision = "16-mixed"


def test_three_adamw_steps_with_a_loss_scaler():
    from beat_this_amd.optim import AdamW, LossScaler, param_groups_for

    m = fresh_model().set_frontend_precision("16-mixed").set_train_precision("16-mixed")
    batch = make_batch(2, 150, seed=61)
    opt = AdamW(param_groups_for(m, 0.01), lr=2e-3)
    scaler = LossScaler(init_scale=4096.0)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss, _ = model_loss(m, batch)
        losses.append(float(loss.detach()))
        if len(losses) <= 3:
            (loss * scaler.scale).backward()
            opt.step(loss_scaler=scaler)
            assert not opt.last_step_skipped
    print("losses:", losses)
    assert losses[-1] < losses[0], losses
    with torch.no_grad():
        after = m(batch["spect"])
    sd = dict(RC.model_state_dict("init0"))
    moved = [n for n, p in m.named_parameters() if n.startswith("frontend.") and not torch.equal(p.detach().cpu(), sd[n])]
    assert len(moved) == len(RG.frontend_keys(sd)), "every frontend weight takes part in the step"
    sd.update({n: p.detach().cpu() for n, p in m.named_parameters()})
    with torch.no_grad():
        ob, od = O.model_forward(sd, batch["spect"].cpu())
    err = max(float((after["beat"].cpu() - ob).abs().max()), float((after["downbeat"].cpu() - od).abs().max()))
    print(f"after three mixed steps: max |logit - oracle(updated weights)| = {err:.3e}")
    assert err < 1e-3, err


def test_fit_with_both_precisions_mixed_resumes_bit_for_bit(tmp_path):
    from beat_this_amd.train import CHECKPOINT_KEYS, fit

    r = H.fit_and_resume(tmp_path, train_frontend=True, precision="16-mixed", frontend_precision="16-mixed")
    pl, h, h2, a, b, root = (r[k] for k in ("pl", "h", "h2", "a", "b", "root"))
    assert pl.model.frontend_precision == "16-mixed" and pl.model.train_precision == "16-mixed" and h["loss_scaler"] is not None
    assert all(np.isfinite(v) for v in h["train_loss"])
    assert set(a) == set(CHECKPOINT_KEYS) | {"loss_scaler"} and a["loss_scaler"] == b["loss_scaler"] == h2["loss_scaler"].state_dict()
    assert len(a["optimizer_states"][0]["state"]) == len(RG.all_keys(pl.model.state_dict()))
    # the frontend opt-in alone creates the scaler too, and PLBeatThis takes the setting
    from beat_this_amd.model.pl_module import PLBeatThis

    h3 = fit(new_module(), new_datamodule(root), 0, train_frontend=True, frontend_precision="16-mixed", log=lambda s: None)
    assert h3["loss_scaler"] is not None
    assert PLBeatThis(transformer_dim=64, n_layers=2, ff_mult=2, frontend_precision="16-mixed").model.frontend_precision == "16-mixed"
    assert PLBeatThis(transformer_dim=64, n_layers=2, ff_mult=2).model.frontend_precision == "32-true"
    assert "frontend_precision" not in PLBeatThis(transformer_dim=64, n_layers=2, ff_mult=2).hyper_parameters


def test_the_command_line_refuses_the_switch_without_a_trainable_frontend(capsys):
    from beat_this_amd import train

    with pytest.raises(SystemExit) as e:
        train.main(["--data-dir", "nowhere", "--output", "nothing.ckpt", "--frontend-precision", "16-mixed"])
    assert e.value.code == 2 and "--train-frontend" in capsys.readouterr().err
    args = train.get_parser().parse_args(["--data-dir", "d", "--output", "o", "--train-frontend", "--frontend-precision", "16-mixed"])
    assert args.frontend_precision == "16-mixed" and train.get_parser().parse_args(["--data-dir", "d", "--output", "o"]).frontend_precision == "32-true"
