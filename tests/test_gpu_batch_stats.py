"""Batch-statistics BatchNorm on the GPU (csrc/train_front.hip: bt_front_bn_*, backward.py: StemBatchFn / ConvUnitBatchFn,
BeatThis.set_batch_statistics) against the truth of route_grads.py: fp64 CPU autograd through the oracle's
frontend with torch's training-mode batch_norm, e_ref the same in fp32, every device tensor within 10 e_ref; the moved running
buffers by the same rule (floor 1e-7), the counters exactly.

Shapes of the unit tests: (2, 1) and (1, 2): both time pads inside one window, and n = 2 for bn1d; (1, 3), (2, 3); (1, 63) /
(1, 64) / (1, 65): an edge of the 64-row GEMM tile and of BT_TRAIN_CS_ROWS (bn1d's rows are B T); (2, 65): the rows cross
BT_TRAIN_DW_ROWS and BT_TRAIN_CS_ROWS with ragged last chunks, two sequences in one set of statistics; (2, 150); the conv units
also (1, 1) (n = F' >= 4 there).
"""
import copy
import ctypes as C
import shutil

import numpy as np
import pytest
import torch

import route_cases as RC
import route_grads as RG
import route_harness as H
from gpu_util import dev, report
from route_harness import both_poisons, randn, same_bits
from route_harness import weighted_backward as model_device
from oracle import beat_this_oracle as O

pytestmark = pytest.mark.gpu

HP = dict(transformer_dim=64, ff_mult=2, n_layers=2)
SHAPES = ((2, 1), (1, 2), (1, 3), (2, 3), (1, 63), (1, 64), (1, 65), (2, 65), (2, 150))


def state_dict(style="lively", partial=True, seed=6):
    """lively buffers are not the initial ones, and the counters start at 3: an update that overwrites instead of blending shows"""
    return H.state_dict(dict(HP, partial_transformers=partial), seed, style, counters=3)


def new_model(style="lively", partial=True, seed=6):
    sd = state_dict(style, partial, seed)
    return H.make_model(dict(HP, partial_transformers=partial), sd, frontend=True, freeze_freqs=True), sd


# ---- 1. each unit through the C ABI ------------------------------------------------------------------------------------------
def unit_spec(unit, B, T):
    """(BT_FRONT_* unit, F, C, x shape, y shape, {BatchNorm field prefix: state dict prefix}, conv weight key)"""
    from beat_this_amd import _lib as L

    if unit == "stem":
        p = "frontend.stem."
        return L.FRONT_STEM, 128, 32, (B, T, 128), (B, T, 32, 32), {"bn1": p + "bn1d.", "bn": p + "bn2d."}, p + "conv2d.weight"
    i = int(unit[4])
    F_, C_ = 32 >> i, 32 << i
    p = f"frontend.blocks.{i}."
    return L.FRONT_CONV, F_, C_, (B, T, F_, C_), (B, T, F_ // 2, 2 * C_), {"bn": p + "norm."}, p + "conv2d.weight"


def abi_unit(sd, unit, B, T, x, gy, poison):
    """forward + backward of one unit through bt_front_bn_*: every output, saved tensor, gradient, running buffer and the
    workspace in guarded, poisoned buffers -> ({"y", "x" (= gx), <key>: gradient}, {<key>: running buffer after the call})"""
    if unit == "stem":
        return H.abi_front_unit(sd, "stem", None, B, T, x, gy, poison, batch=True)
    _, F_, C_, *_ = unit_spec(unit, B, T)
    return H.abi_front_unit(sd, "conv", (f"frontend.blocks.{unit[4]}.", F_, C_), B, T, x, gy, poison, batch=True)


def unit_truth(sd, unit, x, gy, dtype):
    return RG.bn_stem(sd, x, gy, dtype) if unit == "stem" else RG.bn_conv(sd, int(unit[4]), x, gy, dtype)


def check_unit(unit, B, T, x, gy, name):
    sd = state_dict()
    got, stats = both_poisons(f"{unit} B={B} T={T}", lambda p: abi_unit(sd, unit, B, T, x, gy, p))
    r32, r64 = (unit_truth(sd, unit, x, gy, dt) for dt in (torch.float32, torch.float64))
    assert all(float(v.abs().max()) > 0 for v in r64["grads"].values()), name
    assert set(stats) == set(r64["stats"])
    RG.check_batch(name, {k: v for k, v in got.items() if k in r64["grads"]}, stats, r32, r64, report)
    e_y = max(RG.rel(r32["y"], r64["y"]), 1e-7)
    print(f"{name}: y e_ref = {e_y:.3e}, device error = {RG.rel(got['y'], r64['y']):.3e}")
    assert RG.rel(got["y"], r64["y"]) <= RG.GATE * e_y, (name, RG.rel(got["y"], r64["y"]), e_y)


@pytest.mark.parametrize("B,T", SHAPES + ((1, 1),))
@pytest.mark.parametrize("unit", ("stem", "conv0", "conv1", "conv2"))
def test_unit_against_the_truth(unit, B, T):
    from beat_this_amd import _lib as L

    code, F_, C_, xs, ys, _, _ = unit_spec(unit, B, T)
    if unit == "stem" and B * T == 1:   # one value per channel: refused like torch refuses it, before any launch
        assert L.lib().bt_front_bn_workspace_bytes(code, 0, B, T, F_, C_) == 0
        a = L.FrontBnArgs(B=B, T=T, F=F_, C=C_)
        assert L.lib().bt_front_bn_forward(L.stream_ptr(dev()), code, C.byref(a)) == L.BT_ERR_ARG
        assert L.lib().bt_front_bn_backward(L.stream_ptr(dev()), code, C.byref(a)) == L.BT_ERR_ARG
        return
    x = RC.spect(B, T, seed=100 + T) if unit == "stem" else randn(*xs, seed=100 + T)
    check_unit(unit, B, T, x, randn(*ys, seed=200 + T), f"batch statistics {unit} B={B} T={T}")


def test_cancellation_with_a_shifted_spectrogram():
    """x in [64, 67): E[v^2] - mean^2 in fp32 would lose bn1d's variance (0.75 against 4225) to cancellation; torch's fp32
    batch_norm does not (tests/test_bn_grad_reference.py), so it is the e_ref here as everywhere"""
    B, T = 2, 65
    x = RC.spect(B, T, seed=165) + 64
    check_unit("stem", B, T, x, randn(B, T, 32, 32, seed=265), "batch statistics stem B=2 T=65 shifted by 64")


# ---- 2. the whole model --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(2, 150), (2, 1)])
@pytest.mark.parametrize("style,partial", [("lively", True), ("init0", True), ("lively", False)])
def test_whole_model_against_the_truth(style, partial, B, T):
    """(At (2, 1) every channel of a conv unit's input holds a per-sequence constant in time, so ``partial.ffT.net.4.bias`` is
    removed by the BatchNorm that follows: its true gradient is 0, the fp32 reference's is rounding noise, e_ref of that case is
    of the order 1e8 and the gate says nothing there; the units' own tests cover n = 2.)"""
    m, sd = new_model(style, partial)
    m.train().set_batch_statistics()
    x = RC.spect(B, T, seed=500 + T)
    g_b, g_d = randn(B, T, seed=501), randn(B, T, seed=502)
    got, beat, down, stats = model_device(m, x, g_b, g_d)
    r32, r64 = (RG.bn_model(sd, x, RG.weighted_sum(g_b, g_d, dt), dt) for dt in (torch.float32, torch.float64))
    g64 = r64["grads"]
    assert set(g64) == set(["x"] + RG.all_keys(sd)) and len(g64) == (100 if partial else 40)
    assert set(got) == set(g64), sorted(set(g64) ^ set(got))
    assert len(stats) == 15 and set(stats) == set(r64["stats"])
    name = f"batch statistics whole model {style}{'' if partial else ' no partial'} B={B} T={T}"
    RG.check_batch(name, got, stats, r32, r64, report)
    for p in RG.BN_PREFIXES:
        assert int(stats[p + "num_batches_tracked"]) == int(sd[p + "num_batches_tracked"]) + 1 == 4
        assert stats[p + "num_batches_tracked"].dtype == torch.int64
        assert not torch.equal(stats[p + "running_mean"].cpu(), sd[p + "running_mean"]), p
    err = max(float((beat.cpu() - r64["beat"]).abs().max()), float((down.cpu() - r64["downbeat"]).abs().max()))
    print(f"{name}: max |logit - oracle| = {err:.3e}")
    assert err < 1e-3, err


def test_one_frame_alone_raises_like_torch():
    m, sd = new_model()
    m.train().set_batch_statistics()
    x = RC.spect(1, 1, seed=7).to(dev())
    for call in (m, m.frontend):
        with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
            call(x)
    for n, b in m.named_buffers():
        assert torch.equal(b.cpu(), sd[n]), n
    m.eval()
    assert m(x)["beat"].shape == (1, 1)      # the running statistics take one frame as ever


# ---- 3. bit identities -----------------------------------------------------------------------------------------------------------
def test_without_batch_statistics_nothing_moves():
    B, T = 2, 65
    x, g_b, g_d = RC.spect(B, T, seed=31), randn(B, T, seed=32), randn(B, T, seed=33)
    plain, sd = new_model()
    want = model_device(plain, x, g_b, g_d)
    opted = new_model()[0].set_batch_statistics()             # eval() with grad: the opt-in alone changes nothing
    assert opted.batch_statistics and not opted.training
    unopted = new_model()[0].train()                          # train() without the opt-in: nothing either
    for name, m in (("opted in, eval()", opted), ("train() without the opt-in", unopted)):
        got = model_device(m, x, g_b, g_d)
        assert set(got[0]) == set(want[0])
        assert all(same_bits(got[0][k], want[0][k]) for k in want[0]), name
        assert same_bits(got[1], want[1]) and same_bits(got[2], want[2]), name
        for n, b in m.named_buffers():
            assert torch.equal(b.cpu(), sd[n]) and same_bits(b, want[3][n]), f"{name}: {n} moved"
    opted.train()
    with torch.no_grad():                                     # the opt-in and train(), but no grad mode: the inference path
        quiet = opted(x.to(dev()))
    plain.train()
    with torch.no_grad():
        ref = plain(x.to(dev()))
    assert same_bits(quiet["beat"], ref["beat"]) and same_bits(quiet["downbeat"], ref["downbeat"])
    for n, b in opted.named_buffers():
        assert torch.equal(b.cpu(), sd[n]), f"no_grad: {n} moved"


def test_two_runs_from_the_same_state_are_bit_identical():
    B, T = 2, 65
    x, g_b, g_d = RC.spect(B, T, seed=41), randn(B, T, seed=42), randn(B, T, seed=43)
    runs = []
    for _ in range(2):
        m, _ = new_model()
        m.train().set_batch_statistics()
        first = model_device(m, x, g_b, g_d)
        second = model_device(m, x, g_b, g_d)               # a second call moves the buffers again
        runs.append((first, second))
        for p in RG.BN_PREFIXES:
            assert int(second[3][p + "num_batches_tracked"]) == 5
            assert not same_bits(first[3][p + "running_var"], second[3][p + "running_var"])
        # the batch's statistics do not depend on the running ones: outputs and gradients repeat, bit for bit
        assert same_bits(first[1], second[1]) and all(same_bits(first[0][k], second[0][k]) for k in first[0])
    for a, b in zip(runs[0], runs[1]):
        assert same_bits(a[1], b[1]) and same_bits(a[2], b[2])
        assert all(same_bits(a[0][k], b[0][k]) for k in a[0])
        assert all(same_bits(a[3][k], b[3][k]) for k in a[3])


# ---- 4. the engine's packed copies ---------------------------------------------------------------------------------------------
def test_the_inference_engine_sees_the_moved_statistics():
    from test_gpu_backward import make_batch, model_loss
    from beat_this_amd.optim import AdamW, param_groups_for

    m, sd = new_model("init0", seed=8)
    batch = make_batch(2, 150, seed=61)
    with torch.no_grad():
        m(batch["spect"])                                     # (packs the engine with the initial buffers)
    engine = m._engine
    m.train().set_batch_statistics()
    opt = AdamW(param_groups_for(m, 0.01), lr=2e-3)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss, _ = model_loss(m, batch)
        losses.append(float(loss.detach()))
        if len(losses) <= 3:
            loss.backward()
            opt.step()
        assert m._engine is engine, "the training forward packed the engine again"
    print("losses:", losses)
    assert losses[-1] < losses[0], losses
    now = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    for p in RG.BN_PREFIXES:
        assert int(now[p + "num_batches_tracked"]) == int(sd[p + "num_batches_tracked"]) + 4
    with torch.no_grad():                                     # train() mode still: no_grad alone selects the running statistics
        after = m(batch["spect"])
        again = m(batch["spect"])
    assert m._engine is not engine and same_bits(after["beat"], again["beat"])
    x = batch["spect"].cpu()
    with torch.no_grad():
        ob, od = O.model_forward(now, x)
        stale = dict(now)
        stale.update({k: v for k, v in sd.items() if k.endswith(RG.STAT_LEAVES)})
        sb, sdown = O.model_forward(stale, x)
    err = max(float((after["beat"].cpu() - ob).abs().max()), float((after["downbeat"].cpu() - od).abs().max()))
    apart = max(float((ob - sb).abs().max()), float((od - sdown).abs().max()))
    print(f"after three steps: max |logit - oracle(state_dict now)| = {err:.3e}; the initial buffers would be {apart:.3e} away")
    report("batch_stats_engine", err_after=err, stale_distance=apart, loss_first=losses[0], loss_last=losses[-1])
    assert err < 1e-3, err
    # "far more": ten times the bound on err, the margin test_three_adamw_steps_on_all_parameters asks between its two figures --
    # an engine left on the initial buffers would then miss the bound above by a decade
    assert apart > 10 * 1e-3, apart


# ---- 5. fit ---------------------------------------------------------------------------------------------------------------------
def test_fit_with_batch_statistics_resumes_bit_for_bit(tmp_path):
    from dataset_reference import build_data_folder
    from beat_this_amd.inference import load_checkpoint
    from beat_this_amd.train import fit
    from test_gpu_finetune import EPOCHS, new_datamodule, new_module

    root = build_data_folder(str(tmp_path / "data"))
    ck, first, ck2 = (str(tmp_path / n) for n in ("run.ckpt", "epoch0.ckpt", "resumed.ckpt"))

    def log(line):
        if line.startswith("epoch 0:"):
            shutil.copy(ck, first)

    pl = new_module()
    np.random.seed(0)
    h = fit(pl, new_datamodule(root), EPOCHS, val_frequency=1, checkpoint_path=ck, log=log, train_frontend=True, batch_statistics=True)
    print("train_loss per epoch:", h["train_loss"], "validation:", [v["val_loss"] for _, v in h["val"]])
    assert pl.model.batch_statistics and pl.training and all(np.isfinite(v) for v in h["train_loss"])
    assert len(h["val"]) == EPOCHS and all(np.isfinite(v["val_loss"]) for _, v in h["val"])
    pl2 = new_module()
    np.random.seed(99)
    h2 = fit(pl2, new_datamodule(root), EPOCHS, val_frequency=1, checkpoint_path=ck2, resume=first, log=lambda s: None,
             train_frontend=True, batch_statistics=True)
    assert len(h2["train_loss"]) == 1 and h2["train_loss"][0] == h["train_loss"][1]
    a, b = load_checkpoint(ck), load_checkpoint(ck2)
    assert set(a["state_dict"]) == set(b["state_dict"]) == set(new_module().state_dict())      # no new keys
    for k, v in a["state_dict"].items():
        assert same_bits(v, b["state_dict"][k]), k
    sa, sb = a["optimizer_states"][0], b["optimizer_states"][0]
    assert len(sa["state"]) == len(sb["state"]) == len(RG.all_keys(pl.model.state_dict()))
    for i in sa["state"]:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(torch.as_tensor(sa["state"][i][k]), torch.as_tensor(sb["state"][i][k])), (i, k)
    fresh = dict(new_module().model.named_buffers())
    steps = int(a["state_dict"]["model.frontend.stem.bn1d.num_batches_tracked"]) - int(fresh["frontend.stem.bn1d.num_batches_tracked"])
    assert steps == h["global_step"] > 0                      # (accumulate 1: one forward per optimiser step)
    for n, buf in pl.model.named_buffers():
        assert same_bits(buf, pl2.model.state_dict()[n]), n
        assert not torch.equal(buf, fresh[n]), f"{n} did not move during fit"
