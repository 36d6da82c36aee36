"""Dropout on the fine-tuning route (csrc/dropout.h, csrc/train.hip, BeatThis.enable_dropout, fit): the device against fp64
torch on the CPU that applies the masks of the numpy restatement (route_reference.py), with the yardstick of
route_grads.py -- e_ref is the same computation in fp32, and the outputs and every gradient have to be within 10 e_ref.
One wrong mask bit in the forward, the dQ or the dK / dV sweep moves an element by about 1 / T relative, decades over that.

Sizes: T = 1, 63, 64, 65, 130, 257 sit on both sides of the 64-wide attention blocks and GEMM tiles, cover T % 4 != 0 (a
query's last group of keys is ragged) and more than one block; D = 64 and 96 (two and three heads), ff_mult 2, B = 2; the units
also at D = 128 (four heads), ff_mult 4 -- the shipped model's hidden = 4 D -- for T = 65 and 130."""
import copy
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import route_grads as RG
import route_harness as H
import route_reference as REF
from conftest import ROOT
from dataset_reference import build_data_folder
from gpu_util import POISONS, dev, report
from route_grads import shift_tolerant_bce
from route_harness import FIELDS, Unit, make_batch, randn, same_bits, unit_state_dict
from route_reference import unit_masks
from beat_this_amd import weights as W

pytestmark = pytest.mark.gpu

TS = (1, 63, 64, 65, 130, 257)
B = 2
SEED = 0x5EED_0000_0000_0001          # (beyond 32 bits: both key words are in use)


def make_model(D, n_layers=2, seed=3):
    """(BeatThis on the GPU with the trunk and the heads trainable, its state dict on the CPU), once per configuration"""
    hp = dict(transformer_dim=D, ff_mult=2, n_layers=n_layers)
    sd = H.state_dict(hp, seed, "lively")
    return H.make_model(hp, sd, cache=("dropout", D, n_layers, seed)), sd


def unit_truth(kind, sd, pfx, x, g, dtype, masks, p, residual):
    """{"y", "x", <state dict key>: ..}: the unit's output and the gradients of sum(y g) in ``dtype`` on the CPU"""
    leaf, xl = RG._leaves(sd, x, dtype)
    y = REF.unit(kind, xl, leaf, pfx, None, REF.masks_as(masks, dtype), 1.0 / (1.0 - p))
    if residual:
        y = y + xl
    (y * g.to(dtype)).sum().backward()
    out = RG._collect(leaf, xl, [pfx + n for n in FIELDS[kind].values()])
    out["y"] = y.detach()
    return out


# ---- 1. units against the truth ---------------------------------------------------------------------------------------------------
# D -> (ff_mult, the T of TS, the rates): two and three heads at hidden = 2 D over every size; four heads at the shipped model's
# ratio hidden = 4 D on both sides of a second 64-row block
UNIT_CASES = {64: (2, TS, (0.2, 0.5)), 96: (2, TS, (0.2, 0.5)), 128: (4, (65, 130), (0.2,))}


@pytest.mark.parametrize("D", [64, 96, 128])
@pytest.mark.parametrize("kind", ["attn", "ff"])
def test_unit_against_the_truth(kind, D):
    ff_mult, sizes, rates = UNIT_CASES[D]
    sd = unit_state_dict(D, ff_mult)
    worst = (0.0, None)
    for i, T in enumerate(TS):
        if T not in sizes:
            continue
        x, g = randn(B, T, D, seed=200 + 2 * i), randn(B, T, D, seed=201 + 2 * i)
        for p in rates:
            for residual in (0, 1):
                stream = 1000 * i + int(10 * p) + residual
                u = Unit(kind, D, x, g, residual, ff_mult=ff_mult)
                got = u.run((p, SEED, stream))
                masks = unit_masks(kind, p, SEED, stream, B, T, D, ff_mult * D)
                g32, g64 = (unit_truth(kind, sd, u.pfx, x, g, dt, masks, p, residual) for dt in (torch.float32, torch.float64))
                e_ref, ratio = RG.check(f"dropout {kind} D={D} T={T} p={p} residual={residual}", got, g32, g64)
                worst = max(worst, (ratio, (T, p, residual, e_ref)))
    report("dropout_unit", kind=kind, D=D, worst_ratio=worst[0], at=str(worst[1]))


# ---- 2. NULL and p = 0 are the calls without dropout ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["attn", "ff"])
def test_null_and_zero_rate_are_the_plain_calls(kind):
    D = 64
    for T in (65, 130):
        x, g = randn(B, T, D, seed=31), randn(B, T, D, seed=32)
        for residual in (0, 1):
            want = Unit(kind, D, x, g, residual).run(None, entry="plain")
            for drop in (None, (0.0, SEED, 5)):
                got = Unit(kind, D, x, g, residual).run(drop, entry="dropout")
                assert set(got) == set(want)
                for k in want:
                    assert same_bits(got[k], want[k]), (kind, T, residual, drop, k)


# ---- 3. determinism, guard bands, poison, the workspace bound ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["attn", "ff"])
def test_determinism_guard_bands_and_poison(kind):
    D, T, p = 64, 65, 0.2
    x, g = randn(B, T, D, seed=41), randn(B, T, D, seed=42)
    res = [Unit(kind, D, x, g, 1, poison=q).run((p, SEED, 7)) for q in POISONS]
    again = Unit(kind, D, x, g, 1).run((p, SEED, 7))
    other = Unit(kind, D, x, g, 1).run((p, SEED, 8))
    word = int.from_bytes(bytes([POISONS[1]] * 4), "little")
    for k in res[0]:
        assert same_bits(res[0][k], res[1][k]), f"{kind}: {k} depends on the poison"
        assert same_bits(res[0][k], again[k]), f"{kind}: {k} differs between two runs with one (seed, stream)"
        assert torch.isfinite(res[0][k]).all(), f"{kind}: {k} keeps bytes of the 0xFF poison (or is not finite)"
        assert not (res[1][k].view(torch.int32) == word).any(), f"{kind}: {k} keeps words of the 0x7B poison"
    assert not same_bits(other["y"], again["y"])
    # one byte short of the dropout query: refused before any launch (the forward's query is the plain one)
    u = Unit(kind, D, x, g, 1)
    for backward in (0, 1):
        n = u.L.lib().bt_train_workspace_bytes_dropout(u.unit, backward, B, T, D, 2 * D)
        assert n == u.ws_bytes(backward, (p, SEED, 7))
        assert u.call(backward, (p, SEED, 7), "dropout", ws_bytes=n - 1) == u.L.BT_ERR_WORKSPACE


# ---- 4. the model -------------------------------------------------------------------------------------------------------------------
def model_loss(m, batch):
    from beat_this_amd.model.loss import ShiftTolerantBCELoss

    out = m(batch["spect"])
    fn = ShiftTolerantBCELoss().to(dev())
    return sum(fn(out[k], batch["truth_" + k].float(), batch["padding_mask"]) for k in ("beat", "downbeat")), out


def loss_and_grads(m, batch):
    m.zero_grad(set_to_none=True)
    loss, out = model_loss(m, batch)
    loss.backward()
    grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    return {k: v.detach().clone() for k, v in out.items()}, grads


def trunk_truth(sd, h, batch, dtype, n_layers, p, seed, first_stream):
    """gradients of the loss through the trunk with the masks of streams first_stream .. first_stream + 2 L - 1 and the heads"""
    leaf, xl = RG._leaves(sd, h, dtype)
    beat, down = REF.trunk(leaf, xl, n_layers, drop=(p, seed, first_stream))
    t = {k: batch["truth_" + k].cpu().to(dtype) for k in ("beat", "downbeat")}
    mask = batch["padding_mask"].cpu().to(dtype)
    (shift_tolerant_bce(beat, t["beat"], mask) + shift_tolerant_bce(down, t["downbeat"], mask)).backward()
    out = RG._collect(leaf, xl, RG.trainable_keys(sd))
    out.pop("x")
    return out


def test_the_model_opts_in_and_repeats_from_its_state():
    base, sd = make_model(64, seed=5)
    L_ = 2
    batch = make_batch(B, 130, seed=51)
    want_out, want_grads = loss_and_grads(base, batch)              # dropout never enabled
    m = copy.deepcopy(base)
    assert m.dropout_state() is None and m.dropout["transformer"] == 0.2
    m.enable_dropout(seed=SEED)
    try:
        out, grads = loss_and_grads(m, batch)                       # enabled, but in eval()
        assert m.dropout_state() == {"seed": SEED, "calls": 0}
        m.train()
        with torch.no_grad():                                       # the inference path never drops
            quiet = m(batch["spect"])
        assert m.dropout_state()["calls"] == 0
        first, g_first = loss_and_grads(m, batch)
        assert m.dropout_state()["calls"] == 2 * L_
        second, _ = loss_and_grads(m, batch)
        assert m.dropout_state()["calls"] == 4 * L_
        m.set_dropout_state({"seed": SEED, "calls": 0})
        first_again, g_again = loss_and_grads(m, batch)
        second_again, _ = loss_and_grads(m, batch)
        # against the fp64 truth with the masks of streams 0 .. 2 L - 1
        with torch.no_grad():
            h = m.frontend(batch["spect"])
        g32, g64 = (trunk_truth(sd, h, batch, dt, L_, 0.2, SEED, 0) for dt in (torch.float32, torch.float64))
        RG.check("dropout model D=64 L=2 T=130", g_first, g32, g64, report)
        # capture with dropout active is refused; the eval() model captures as ever (tests/test_gpu_backward.py)
        xd = h.clone().requires_grad_(True)
        m.transformer_blocks(xd)                                    # (warm: the rotary table and the allocator have seen the shapes)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            h * 2.0                                                 # (something to capture)
            with pytest.raises(RuntimeError, match="graph capture"):
                m.transformer_blocks.layers[0][0](xd)
        torch.cuda.synchronize()
    finally:
        m.eval()
    for k in want_out:
        assert same_bits(out[k], want_out[k]), f"eval(): {k} moved"
        assert not same_bits(first[k], want_out[k]) and not same_bits(first[k], second[k]), k
        assert same_bits(first[k], first_again[k]) and same_bits(second[k], second_again[k]), k
        assert torch.isfinite(quiet[k]).all()
    assert set(grads) == set(want_grads) == set(g_first) and len(grads) > 20
    for k in want_grads:
        assert same_bits(grads[k], want_grads[k]), f"eval(): gradient {k} moved"
        assert same_bits(g_first[k], g_again[k]), k
    assert base.dropout_state() is None


# ---- 5. the loop and the command line ---------------------------------------------------------------------------------------------
LR, WARMUP, EPOCHS = 2e-3, 2, 2


def new_module(apply_dropout, seed=11):
    from beat_this_amd.model.pl_module import PLBeatThis

    pl = PLBeatThis(transformer_dim=64, n_layers=2, ff_mult=2, lr=LR, warmup_steps=WARMUP, max_epochs=EPOCHS, eval_trim_beats=0,
                    apply_dropout=apply_dropout, dropout_seed=seed)
    sd = W.random_state_dict(W.resolve_hparams(dict(transformer_dim=64, ff_mult=2, n_layers=2)), seed=3, style="lively")
    pl.load_state_dict({"model." + k: v for k, v in sd.items()})
    return pl.to(dev())


def new_datamodule(root):
    from beat_this_amd.dataset import BeatDataModule

    return BeatDataModule(root, batch_size=2, train_length=150, augmentations={}, device=dev())


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from beat_this_amd.train import fit

    tmp = tmp_path_factory.mktemp("dropout_finetune")
    root = build_data_folder(str(tmp / "data"))
    ck, first = str(tmp / "run.ckpt"), str(tmp / "epoch0.ckpt")

    def log(line):   # (called after the epoch's checkpoint is written)
        if line.startswith("epoch 0:"):
            shutil.copy(ck, first)

    pl = new_module(True)
    np.random.seed(0)
    history = fit(pl, new_datamodule(root), EPOCHS, val_frequency=2, checkpoint_path=ck, log=log)
    return dict(tmp=tmp, root=root, ck=ck, first=first, pl=pl, history=history)


def test_fit_with_dropout_differs_resumes_and_loads(run):
    from beat_this_amd.inference import load_checkpoint, load_model
    from beat_this_amd.train import CHECKPOINT_KEYS, fit

    h = run["history"]
    assert run["pl"].model.training and len(h["train_loss"]) == EPOCHS and all(np.isfinite(h["train_loss"]))
    plain = new_module(False)
    np.random.seed(0)
    h0 = fit(plain, new_datamodule(run["root"]), 1, val_frequency=2, log=lambda line: None)
    assert not plain.model.training and plain.model.dropout_state() is None
    print("train loss of epoch 0: with dropout", h["train_loss"][0], "without", h0["train_loss"][0])
    assert h0["train_loss"][0] != h["train_loss"][0]
    # the checkpoint: the usual keys, the state inside rng, readable by load_model
    a = load_checkpoint(run["ck"])
    assert set(a) == set(CHECKPOINT_KEYS)
    calls = a["rng"]["dropout"]["calls"]
    assert a["rng"]["dropout"]["seed"] == 11 and calls > 0 and calls % 4 == 0          # 2 L per training forward
    assert load_checkpoint(run["first"])["rng"]["dropout"]["calls"] == calls // 2
    loaded = load_model(run["ck"], dev())
    x = torch.log1p(torch.rand(2, 150, 128, generator=torch.Generator().manual_seed(5)) * 30).to(dev())
    with torch.no_grad():
        want, got = run["pl"].model(x), loaded(x)
    for k in ("beat", "downbeat"):
        assert same_bits(got[k], want[k]), k
    # one epoch plus a resumed second one: the bits of the uninterrupted run
    ck2 = str(run["tmp"] / "resumed.ckpt")
    pl = new_module(True, seed=999)          # (whatever seed: the checkpoint's state replaces it)
    np.random.seed(1234)
    h2 = fit(pl, new_datamodule(run["root"]), EPOCHS, val_frequency=2, checkpoint_path=ck2, resume=run["first"], log=lambda line: None)
    assert h2["train_loss"] == h["train_loss"][1:]
    b = load_checkpoint(ck2)
    assert b["rng"]["dropout"] == a["rng"]["dropout"]
    for k, v in a["state_dict"].items():
        assert torch.equal(v, b["state_dict"][k]) and (not v.is_floating_point() or same_bits(v, b["state_dict"][k])), k
    for i, st in a["optimizer_states"][0]["state"].items():
        for k in ("exp_avg", "exp_avg_sq"):
            assert same_bits(st[k], b["optimizer_states"][0]["state"][i][k]), (i, k)
    # a checkpoint without the state resumes as before
    old = dict(load_checkpoint(run["first"]))
    old["rng"] = {k: v for k, v in old["rng"].items() if k != "dropout"}
    pl = new_module(True, seed=11)
    fit(pl, new_datamodule(run["root"]), EPOCHS, val_frequency=2, resume=old, log=lambda line: None)
    assert pl.model.dropout_state()["calls"] == calls // 2


def test_cli_trains_with_dropout(run):
    from beat_this_amd.inference import load_checkpoint

    start, out = str(run["tmp"] / "start.ckpt"), str(run["tmp"] / "cli" / "out.ckpt")
    fresh = new_module(False)
    torch.save({"state_dict": {k: v.cpu() for k, v in fresh.state_dict().items()}, "hyper_parameters": fresh.hyper_parameters}, start)
    r = subprocess.run([sys.executable, "-m", "beat_this_amd.train", "--data-dir", run["root"], "--checkpoint", start, "--output", out,
                        "--max-epochs", "1", "--batch-size", "2", "--train-length", "150", "--accumulate-grad-batches", "1",
                        "--warmup-steps", "2", "--val-frequency", "1", "--eval-trim-beats", "0", "--no-mask-augmentation",
                        "--dropout", "--transformer-dropout", "0.2", "--seed", "3"],
                       cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "epoch 0: train_loss" in r.stdout
    ckpt = load_checkpoint(out)
    assert ckpt["rng"]["dropout"]["seed"] == 3 and ckpt["rng"]["dropout"]["calls"] > 0
    assert ckpt["hyper_parameters"]["dropout"]["transformer"] == 0.2
