"""``fit()`` end to end against an independent loop (tests/route_grads.py): data, model, losses, backward, accumulation,
clipping, AdamW and the schedule crossed in one run, on the seeded synthetic data folder with the D = 64, 2-layer, ff_mult 2
model (``lively`` weights of seed 3) at train_length 150 -- two full 64-row attention and GEMM tiles plus a ragged one, one padded
piece (``a_short``, 97 frames) and one without downbeat annotation (``b_one``).

``fit`` is observed, not changed: the batches it draws are cloned to the CPU, ``training_step`` leaves its losses,
``optimizer.step`` its gradient norm and the groups' rates, the ``log`` callback keeps each epoch's checkpoint.  The truth is the
helper in fp64 over the recorded batches (``h`` = the frozen frontend's output on the device); ``e_ref`` is the helper in fp32,
worst tensor; the gate is route_grads.GATE.  tests/test_finetune_reference.py shows what the gate separates.

Cases, one ``fit`` of two epochs each:
  A  batch 2, accumulate 1, no clipping, default decay, pos_weights 1, validation after every epoch
  B  batch 1, accumulate 2 (an epoch of five batches ends on a remainder of one), weight decay 0.05, pos_weights 2.5 / 6.0,
     max_grad_norm between the norms of the run
  C  B with dropout (seed beyond 32 bits, rate 0.2): the stream numbering across optimiser steps and epochs
"""
import math
import shutil

import numpy as np
import pytest
import torch

import route_grads as RG
import metrics_reference as MR
from dataset_reference import build_data_folder
from ddp_worker import TENSORS, RecordingLoader, observe_steps
from gpu_util import dev, report
from beat_this_amd import weights as W
from oracle import beat_this_oracle as O

pytestmark = pytest.mark.gpu

HP = dict(transformer_dim=64, ff_mult=2, n_layers=2)
LR, WARMUP, EPOCHS, T = 2e-3, 2, 2, 150
DROPOUT_SEED = 0x5EED_0000_0000_0001
# B and C: 0.68 lies between the norms of both runs -- 0.47 | 0.77 0.94 1.09 | 0.30 | 1.27 without dropout, 0.58 | 0.82 0.84 1.09 |
# 0.42 | 1.29 with it (fp64 helper): steps 1, 2, 3 and 5 clip, steps 0 and 4 do not, and none is within 13 % of the limit
CASES = {
    "A": dict(batch_size=2, accumulate=1, max_grad_norm=None, weight_decay=0.01, pos_weights={"beat": 1, "downbeat": 1},
              val_frequency=1, dropout=False),
    "B": dict(batch_size=1, accumulate=2, max_grad_norm=0.68, weight_decay=0.05, pos_weights={"beat": 2.5, "downbeat": 6.0},
              val_frequency=EPOCHS + 1, dropout=False),
    "C": dict(batch_size=1, accumulate=2, max_grad_norm=0.68, weight_decay=0.05, pos_weights={"beat": 2.5, "downbeat": 6.0},
              val_frequency=EPOCHS + 1, dropout=True),
}
_RUNS = {}


def initial_state_dict():
    return W.random_state_dict(W.resolve_hparams(HP), seed=3, style="lively")


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return build_data_folder(str(tmp_path_factory.mktemp("trajectory") / "data"))


def observed_fit(case, folder, tmp):
    """one ``fit`` of ``case`` with the observers attached -> everything the checks need"""
    from beat_this_amd.dataset import BeatDataModule
    from beat_this_amd.inference import load_checkpoint
    from beat_this_amd.model.pl_module import PLBeatThis
    from beat_this_amd.train import fit

    c = CASES[case]
    sd = initial_state_dict()
    pl = PLBeatThis(**HP, lr=LR, weight_decay=c["weight_decay"], pos_weights=c["pos_weights"], warmup_steps=WARMUP, max_epochs=EPOCHS,
                    eval_trim_beats=0, apply_dropout=c["dropout"], dropout_seed=DROPOUT_SEED)
    pl.load_state_dict({"model." + k: v for k, v in sd.items()})
    pl = pl.to(dev())
    dm = BeatDataModule(folder, batch_size=c["batch_size"], train_length=T, augmentations={}, device=dev())
    dm.setup("fit")
    rec = dict(case=case, sd=sd, pl=pl, dm=dm, batches=[], losses=[], steps=[], checkpoints=[], configured=[])

    train_dataloader = dm.train_dataloader
    dm.train_dataloader = lambda: RecordingLoader(train_dataloader(), rec["batches"])
    training_step = pl.training_step

    def recording_training_step(batch, batch_idx=0):
        loss = training_step(batch, batch_idx)
        rec["losses"].append({k: float(v) for k, v in pl.last_losses.items()})
        assert float(loss.detach()) == rec["losses"][-1]["total"]
        return loss

    pl.training_step = recording_training_step
    observe_steps(pl, rec["steps"], configured=rec["configured"])
    ck = str(tmp / f"{case}.ckpt")

    def log(line):   # (called after the epoch's checkpoint is written)
        if line.startswith("epoch "):
            epoch = int(line.split()[1].rstrip(":"))
            shutil.copy(ck, str(tmp / f"{case}.epoch{epoch}.ckpt"))
            rec["checkpoints"].append(load_checkpoint(str(tmp / f"{case}.epoch{epoch}.ckpt")))

    np.random.seed(0)
    rec["history"] = fit(pl, dm, EPOCHS, accumulate_grad_batches=c["accumulate"], val_frequency=c["val_frequency"],
                         max_grad_norm=c["max_grad_norm"], checkpoint_path=ck, log=log)
    rec["optimizer"] = rec["history"]["optimizer"]
    rec["checkpoint_paths"] = [str(tmp / f"{case}.epoch{e}.ckpt") for e in range(EPOCHS)]
    # the helper's inputs: the frozen frontend's output for every recorded batch, and its two runs
    with torch.no_grad():
        for b in rec["batches"]:
            b["h"] = pl.model.frontend(b["spect"].to(dev())).cpu()
    per_epoch = len(rec["batches"]) // EPOCHS
    rec["per_epoch"], rec["steps_per_epoch"] = per_epoch, math.ceil(per_epoch / c["accumulate"])
    settings = dict(n_layers=HP["n_layers"], lr=LR, weight_decay=c["weight_decay"], warmup=WARMUP, total_steps=EPOCHS * rec["steps_per_epoch"],
                    accumulate=c["accumulate"], max_grad_norm=c["max_grad_norm"], pos_weights=c["pos_weights"], epochs=EPOCHS,
                    batches_per_epoch=per_epoch, dropout=(0.2, DROPOUT_SEED) if c["dropout"] else None)
    rec["truth"], rec["yard"] = (RG.run(sd, rec["batches"], dt, **settings) for dt in (torch.float64, torch.float32))
    return rec


@pytest.fixture(scope="module")
def observed(folder, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("trajectory_runs")

    def get(case):
        if case not in _RUNS:
            _RUNS[case] = observed_fit(case, folder, tmp)
        return _RUNS[case]

    yield get
    _RUNS.clear()


def names_by_index(rec):
    """optimiser state index -> state-dict key of the model, through the optimiser's groups (torch's layout counts the
    parameters group after group)"""
    name = {id(p): n[len("model."):] for n, p in rec["pl"].named_parameters()}
    return [name[id(p)] for g in rec["optimizer"].param_groups for p in g["params"]]


def vector(values):
    return torch.tensor(list(values), dtype=torch.float64)


@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_fit_follows_the_fp64_loop(observed, case):
    rec = observed(case)
    c, sd, truth, yard, history = CASES[case], rec["sd"], rec["truth"], rec["yard"], rec["history"]
    keys = RG.trainable_keys(sd)
    # ---- what the run was made of -------------------------------------------------------------------------------------------------
    per_epoch, n_steps = rec["per_epoch"], EPOCHS * rec["steps_per_epoch"]
    assert per_epoch == 5 // c["batch_size"] and len(rec["batches"]) == EPOCHS * per_epoch == len(rec["losses"])
    for e in range(EPOCHS):
        drawn = rec["batches"][e * per_epoch:(e + 1) * per_epoch]
        assert any(not bool(b["padding_mask"].all()) for b in drawn), f"epoch {e} has no padded excerpt"
        assert any(not bool(b["downbeat_mask"].all()) for b in drawn), f"epoch {e} has no piece without downbeat annotation"
    # ---- exact: counts, schedule, groups, frozen tensors -------------------------------------------------------------------------
    assert len(rec["steps"]) == n_steps == history["global_step"] == len(truth["steps"])
    assert history["scheduler"].last_epoch == n_steps
    assert rec["configured"] == [dict(total_steps=n_steps, max_grad_norm=c["max_grad_norm"], accumulate=c["accumulate"])]
    for s, (step, want) in enumerate(zip(rec["steps"], truth["steps"])):
        # the scheduler multiplies the base rate by numpy's cosine, the helper by math's: equal once both are rounded to fp32
        closed = np.float32(LR * RG.lr_factor(s, WARMUP, n_steps))
        assert closed == np.float32(want["lr"])
        assert [np.float32(r) for r in step["lrs"]] == [closed, closed], (s, step["lrs"], closed)
        assert step["accumulated"] == want["count"], (s, step["accumulated"], want["count"])
    assert rec["steps"][0]["lrs"] == [0.0, 0.0]
    groups = rec["optimizer"].param_groups
    name = {id(p): n for n, p in rec["pl"].named_parameters()}
    assert len(groups) == 2 and [g["weight_decay"] for g in groups] == [c["weight_decay"], 0]
    assert sorted(name[id(p)][len("model."):] for g in groups for p in g["params"]) == sorted(keys)
    assert all(p.ndim >= 2 for p in groups[0]["params"]) and all(p.ndim <= 1 for p in groups[1]["params"])
    assert len(groups[0]["params"]) > 10 and len(groups[1]["params"]) > 10
    frozen = [k for k in sd if k.startswith("frontend.") or k.endswith("rotary_embed.freqs")]
    final = rec["pl"].model.state_dict()
    assert len(frozen) > 20
    for k in frozen:
        a, b = final[k].detach().cpu().reshape(-1), sd[k].reshape(-1)
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"{k} changed its bits"
    for e, ckpt in enumerate(rec["checkpoints"]):
        assert ckpt["epoch"] == e and ckpt["global_step"] == (e + 1) * rec["steps_per_epoch"]
        assert ckpt["lr_schedulers"][0]["last_epoch"] == ckpt["global_step"]
    if c["dropout"]:
        assert rec["pl"].model.dropout_state() == {"seed": DROPOUT_SEED, "calls": 2 * HP["n_layers"] * len(rec["batches"])}
    # ---- the trajectory: displacement and both moments of every tensor after each epoch ----------------------------------------
    index = names_by_index(rec)
    assert len(rec["checkpoints"]) == EPOCHS
    for e, ckpt in enumerate(rec["checkpoints"]):
        got = {k: ckpt["state_dict"]["model." + k] for k in keys}
        RG.check(f"trajectory {case} epoch {e}: p - p_initial", RG.displacement(got, sd),
                RG.displacement(yard["epochs"][e]["params"], sd), RG.displacement(truth["epochs"][e]["params"], sd), report)
        state = ckpt["optimizer_states"][0]["state"]
        assert sorted(state) == list(range(len(index)))
        for moment in ("exp_avg", "exp_avg_sq"):
            got = {index[i]: state[i][moment] for i in state}
            RG.check(f"trajectory {case} epoch {e}: {moment}", got, yard["epochs"][e][moment], truth["epochs"][e][moment], report)
    # ---- per batch: the losses; per step: the norms and which steps clip -------------------------------------------------------
    for j, which in enumerate(("beat", "downbeat", "total")):
        RG.check(f"trajectory {case}: {which} loss per batch", {which: vector(l[which] for l in rec["losses"])},
                {which: vector(l[j] for l in yard["losses"])}, {which: vector(l[j] for l in truth["losses"])}, report)
    for b, got, want in zip(rec["batches"], rec["losses"], truth["losses"]):
        if not bool(b["downbeat_mask"].any()):
            assert got["downbeat"] == 0.0 == want[1]
    e_loss = RG.rel(vector(l[2] for l in yard["losses"]), vector(l[2] for l in truth["losses"]))
    for e in range(EPOCHS):
        mean = float(np.mean([l["total"] for l in rec["losses"][e * per_epoch:(e + 1) * per_epoch]]))
        assert abs(history["train_loss"][e] - mean) <= RG.GATE * e_loss * abs(mean), (e, history["train_loss"][e], mean)
    if c["max_grad_norm"] is not None:
        limit = c["max_grad_norm"]
        norms = [s["norm"] for s in truth["steps"]]
        clipped = [s["coef"] < 1.0 for s in truth["steps"]]
        print("gradient norms, fp64:", norms, "device:", [s["norm"] for s in rec["steps"]])
        assert any(clipped) and not all(clipped)
        assert all(abs(n - limit) > 0.05 * limit for n in norms), norms
        RG.check(f"trajectory {case}: gradient norm per step", {"norm": vector(s["norm"] for s in rec["steps"])},
                {"norm": vector(s["norm"] for s in yard["steps"])}, {"norm": vector(norms)}, report)
        assert [s["norm"] + 1e-6 > limit for s in rec["steps"]] == clipped
    else:
        assert all(s["coef"] == 1.0 for s in truth["steps"])


def oracle_validation(rec, sd, batches, dtype):
    """the three validation losses of the weights ``sd``: the CPU oracle's logits, the loss restated, the mean over the
    validation set weighted by batch size"""
    c = CASES[rec["case"]]
    sums, count = np.zeros(3), 0
    for b in batches:
        beat, down = O.model_forward(sd, b["spect"], dtype)
        n = b["spect"].shape[0]
        sums += n * np.array([float(v) for v in RG.batch_losses(beat, down, b, dtype, c["pos_weights"])])
        count += n
    return dict(zip(("val_loss_beat", "val_loss_downbeat", "val_loss"), sums / count))


def reference_metrics(model, batches):
    """the four validation metrics from the DEVICE's logits: the oracle's post-processor, tests/metrics_reference.py, the mean
    over the pieces of a batch (Cemgil: over both entries of its tuple), the batches weighted by their sizes"""
    sums, count = {}, 0
    for b in batches:
        with torch.no_grad():
            out = model(b["spect"].to(dev()))
        logits = {k: out[k].float().cpu().masked_fill(~b["padding_mask"], -1000.0) for k in ("beat", "downbeat")}
        rows = {"beat": [], "downbeat": []}
        for i in range(b["spect"].shape[0]):
            n = int(b["padding_mask"][i].sum())
            events = dict(zip(("beat", "downbeat"), O.postp_minimal(logits["beat"][i, :n], logits["downbeat"][i, :n])))
            for target in rows:
                truth = np.frombuffer(b["truth_orig_" + target][i], dtype=np.float64)
                rows[target].append(MR.row(truth, np.asarray(events[target], np.float64), min_beat_time=0))
        n = b["spect"].shape[0]
        for target, r in rows.items():
            sums[f"val_F-measure_{target}"] = sums.get(f"val_F-measure_{target}", 0.0) + n * float(np.mean([x[0] for x in r]))
            sums[f"val_Cemgil_{target}"] = sums.get(f"val_Cemgil_{target}", 0.0) + n * float(np.mean([(x[3], x[4]) for x in r]))
        count += n
    return {k: v / count for k, v in sums.items()}


def validation_batches(dm):
    return [dict({k: b[k].detach().cpu().clone() for k in TENSORS}, truth_orig_beat=b["truth_orig_beat"],
                 truth_orig_downbeat=b["truth_orig_downbeat"]) for b in dm.val_dataloader()]


def test_validation_against_the_oracle(observed, folder):
    """``validate()`` after each epoch of case A, and once more over batches of unequal sizes (3 + 1), where a mean over batches
    is not the mean over pieces"""
    from beat_this_amd.dataset import BeatDataModule
    from beat_this_amd.inference import load_model
    from beat_this_amd.train import validate

    rec = observed("A")
    history = rec["history"]
    assert [e for e, _ in history["val"]] == list(range(EPOCHS))
    batches = validation_batches(rec["dm"])
    assert [b["spect"].shape[0] for b in batches] == [2, 2]
    runs = [(f"epoch {e}", metrics, e, batches) for e, metrics in history["val"]]
    dm3 = BeatDataModule(folder, batch_size=3, train_length=T, augmentations={}, device=dev())
    dm3.setup("validate")
    uneven = validation_batches(dm3)
    assert [b["spect"].shape[0] for b in uneven] == [3, 1]
    runs.append(("final, batches of 3 + 1", validate(rec["pl"], dm3), EPOCHS - 1, uneven))
    got, l32, l64 = {}, {}, {}
    for label, metrics, epoch, val_batches in runs:
        model = load_model(rec["checkpoint_paths"][epoch], dev())   # (the epoch's weights on the device, for its logits)
        sd = {k[len("model."):]: v for k, v in rec["checkpoints"][epoch]["state_dict"].items()}
        assert set(metrics) == {"val_loss", "val_loss_beat", "val_loss_downbeat", "val_F-measure_beat", "val_Cemgil_beat",
                                "val_F-measure_downbeat", "val_Cemgil_downbeat"}
        want = reference_metrics(model, val_batches)
        for k, v in want.items():
            print(f"{label}: {k} = {metrics[k]:.6f} (reference {v:.6f})")
            assert abs(metrics[k] - v) <= 1e-12, (label, k, metrics[k], v)
        o32, o64 = (oracle_validation(rec, sd, val_batches, dt) for dt in (torch.float32, torch.float64))
        for k in o64:
            got.setdefault(k, []).append(metrics[k])
            l32.setdefault(k, []).append(o32[k])
            l64.setdefault(k, []).append(o64[k])
    RG.check("trajectory A: validation losses", *({k: vector(v) for k, v in d.items()} for d in (got, l32, l64)), report)
