"""Fine-tuning end to end (beat_this_amd/train.py, beat_this_amd/model/pl_module.py): ``fit`` on the seeded synthetic data folder
with a D = 64, 2-layer, ff_mult 2 model (``lively`` weights), train_length 150, batch 2, 2 epochs, warm-up 2.  One 2-epoch run
is shared by the checks; its log callback keeps the checkpoint of the first epoch, from which a second run resumes."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from dataset_reference import build_data_folder
from gpu_util import dev
from route_harness import EPOCHS, new_datamodule, new_module   # (and for the modules that take them from here)

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from beat_this_amd.train import fit

    tmp = tmp_path_factory.mktemp("finetune")
    root = build_data_folder(str(tmp / "data"))
    ck, first = str(tmp / "run.ckpt"), str(tmp / "epoch0.ckpt")
    lines = []

    def log(line):   # (called after the epoch's checkpoint is written)
        lines.append(line)
        if line.startswith("epoch 0:"):
            shutil.copy(ck, first)

    pl = new_module()
    np.random.seed(0)
    history = fit(pl, new_datamodule(root), EPOCHS, val_frequency=1, checkpoint_path=ck, log=log)
    return dict(tmp=tmp, root=root, ck=ck, first=first, pl=pl, history=history, lines=lines)


@gpu
def test_the_loss_falls_and_validation_reports_the_metrics(run):
    from gpu_util import report

    h = run["history"]
    print("\n".join(run["lines"]))
    assert len(h["train_loss"]) == EPOCHS and h["global_step"] == 4 and h["epoch"] == EPOCHS - 1
    assert h["train_loss"][-1] < h["train_loss"][0], h["train_loss"]
    assert [e for e, _ in h["val"]] == [0, 1]
    for _, metrics in h["val"]:
        for target in ("beat", "downbeat"):
            for key in ("F-measure", "Cemgil"):
                v = metrics[f"val_{key}_{target}"]
                assert np.isfinite(v) and 0.0 <= v <= 1.0, (key, target, v)
        assert np.isfinite(metrics["val_loss"])
    report("finetune", loss_first=h["train_loss"][0], loss_last=h["train_loss"][-1],
           val_f_beat=h["val"][-1][1]["val_F-measure_beat"], val_loss=h["val"][-1][1]["val_loss"])
    # the schedule reached its last step: 4 optimiser steps over warm-up 2
    assert h["scheduler"].last_epoch == 4


@gpu
def test_the_checkpoint_loads_like_a_reference_checkpoint(run):
    from beat_this_amd.inference import load_checkpoint, load_model
    from beat_this_amd.model import BeatThis
    from beat_this_amd.loss import ShiftTolerantBCELoss, losses_from_hparams
    from beat_this_amd.train import CHECKPOINT_KEYS
    import inspect

    ckpt = load_checkpoint(run["ck"])    # torch.load(..., weights_only=True)
    assert set(ckpt) == set(CHECKPOINT_KEYS)
    assert ckpt["epoch"] == EPOCHS - 1 and ckpt["global_step"] == 4
    assert all(k.startswith("model.") for k in ckpt["state_dict"]) and len(ckpt["state_dict"]) == len(run["pl"].model.state_dict())
    hp = ckpt["hyper_parameters"]
    assert set(inspect.signature(BeatThis).parameters) <= set(hp)
    assert hp["transformer_dim"] == 64 and hp["ff_mult"] == 2 and hp["n_layers"] == 2 and hp["loss_type"] == "shift_tolerant_weighted_bce"
    beat_loss, down_loss = losses_from_hparams(hp)
    assert isinstance(beat_loss, ShiftTolerantBCELoss) and float(beat_loss.pos_weight) == hp["pos_weights"]["beat"]
    assert len(ckpt["optimizer_states"]) == 1 and set(ckpt["optimizer_states"][0]) == {"state", "param_groups"}
    assert len(ckpt["lr_schedulers"]) == 1 and ckpt["lr_schedulers"][0]["last_epoch"] == 4
    assert set(ckpt["rng"]) == {"kind", "keys", "pos", "has_gauss", "cached_gaussian"}
    loaded = load_model(run["ck"], dev())
    x = torch.log1p(torch.rand(2, 150, 128, generator=torch.Generator().manual_seed(5)) * 30).to(dev())
    with torch.no_grad():
        want = run["pl"].model(x)
        got = loaded(x)
    for k in ("beat", "downbeat"):
        assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), k


@gpu
def test_a_resumed_run_ends_where_the_uninterrupted_one_does(run):
    from beat_this_amd.inference import load_checkpoint
    from beat_this_amd.train import fit

    ck2 = str(run["tmp"] / "resumed.ckpt")
    lines = []
    pl = new_module()
    np.random.seed(1234)   # (whatever the generator holds: the checkpoint's state replaces it)
    h = fit(pl, new_datamodule(run["root"]), EPOCHS, val_frequency=1, checkpoint_path=ck2, resume=run["first"], log=lines.append)
    assert len(h["train_loss"]) == 1 and h["global_step"] == 4 and lines[0].startswith("resumed after epoch 0")
    assert h["train_loss"][0] == run["history"]["train_loss"][1]
    a, b = load_checkpoint(run["ck"]), load_checkpoint(ck2)
    for k, v in a["state_dict"].items():
        assert torch.equal(v, b["state_dict"][k]) and (not v.is_floating_point() or torch.equal(v.view(torch.int32), b["state_dict"][k].view(torch.int32))), k
    sa, sb = a["optimizer_states"][0], b["optimizer_states"][0]
    assert sa["param_groups"] == sb["param_groups"] and set(sa["state"]) == set(sb["state"])
    for i in sa["state"]:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(sa["state"][i][k].view(torch.int32), sb["state"][i][k].view(torch.int32)), (i, k)
    assert a["lr_schedulers"] == b["lr_schedulers"] and a["global_step"] == b["global_step"] and a["epoch"] == b["epoch"]
    assert torch.equal(a["rng"]["keys"], b["rng"]["keys"]) and a["rng"]["pos"] == b["rng"]["pos"]
    for (n, p), (_, q) in zip(run["pl"].named_parameters(), pl.named_parameters()):
        assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32)), n
    moved = [n for (n, p), (_, q) in zip(new_module().named_parameters(), pl.named_parameters()) if not torch.equal(p, q)]
    assert len(moved) > 20 and not any(n.startswith("model.frontend.") for n in moved)   # the trunk and heads trained, the frontend is frozen


def test_cli_help_exits_cleanly():
    r = subprocess.run([sys.executable, "-m", "beat_this_amd.train", "--help"], cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr
    for flag in ("--data-dir", "--checkpoint", "--output", "--lr", "--weight-decay", "--warmup-steps", "--max-epochs", "--batch-size",
                 "--accumulate-grad-batches", "--train-length", "--loss", "--fold", "--val", "--hung-data", "--seed", "--val-frequency",
                 "--dbn", "--eval-trim-beats", "--tempo-augmentation", "--pitch-augmentation", "--mask-augmentation",
                 "--max-grad-norm", "--resume-checkpoint"):
        assert flag in r.stdout, flag
    for absent in ("wandb", "--compile", "flash"):
        assert absent not in r.stdout


@gpu
def test_cli_writes_a_checkpoint(run):
    from beat_this_amd.inference import load_checkpoint
    from beat_this_amd.train import CHECKPOINT_KEYS

    start, out = str(run["tmp"] / "start.ckpt"), str(run["tmp"] / "cli" / "out.ckpt")
    fresh = new_module()
    torch.save({"state_dict": {k: v.cpu() for k, v in fresh.state_dict().items()}, "hyper_parameters": fresh.hyper_parameters}, start)
    r = subprocess.run([sys.executable, "-m", "beat_this_amd.train", "--data-dir", run["root"], "--checkpoint", start, "--output", out,
                        "--max-epochs", "1", "--batch-size", "2", "--train-length", "150", "--accumulate-grad-batches", "1",
                        "--warmup-steps", "2", "--val-frequency", "1", "--eval-trim-beats", "0", "--max-grad-norm", "1.0",
                        "--no-mask-augmentation"],
                       cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "epoch 0: train_loss" in r.stdout and "val_F-measure_beat" in r.stdout
    ckpt = load_checkpoint(out)
    assert set(ckpt) == set(CHECKPOINT_KEYS) and ckpt["epoch"] == 0 and ckpt["global_step"] >= 1
    assert ckpt["hyper_parameters"]["transformer_dim"] == 64 and ckpt["hyper_parameters"]["ff_mult"] == 2
    changed = [k for k, v in ckpt["state_dict"].items() if not torch.equal(v, fresh.state_dict()[k].cpu())]
    assert changed and not any(k.startswith("model.frontend.") for k in changed)
