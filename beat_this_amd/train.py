#!/usr/bin/env python3
"""Fine-tuning loop: ``fit`` drives a ``PLBeatThis`` over a ``BeatDataModule`` the way the reference's Lightning trainer is set
up in launch_scripts/train.py:118-131 -- epochs over the training loader, gradient accumulation, one optimiser and scheduler
step per accumulated batch group, validation with the package's own metrics every few epochs, one checkpoint per epoch -- and
``python -m beat_this_amd.train`` is the command line around it.  Every step's arithmetic runs in the package's kernels: the
differentiable route of ``BeatThis`` (fp32 or, with ``precision="16-mixed"``, fp16 matrix products under a dynamic loss scale, or
with ``mixed_operand="bf16"`` bfloat16 ones, which need none;
frozen frontend or, with ``train_frontend``, the whole model, its frontend in fp32 or with ``frontend_precision="16-mixed"`` on
fp16 products too; dropout in the main layers when enabled and, with ``frontend_dropout``, in the leaves of the frontend's
partial transformers as well), the losses, and the fused AdamW of ``beat_this_amd.optim``.  The checkpoint is a plain dictionary that ``torch.load(..., weights_only=True)``, ``load_checkpoint``
and ``load_model`` read as it is.

``fit(..., process_group=...)`` and ``--gpus N`` train data-parallel, one process per GPU: the ranks' gradients are added in rank
order (csrc/reduce.hip), so N ranks with one batch each per step repeat the single-process run with N accumulated batches bit
for bit.

Not offered: the reference's wandb logger, ``--compile`` and ``--force-flash-attention`` (nothing here is compiled by torch or
runs torch's attention), and the test run after training (``beat_this_amd.evaluate`` scores a checkpoint).
"""
from __future__ import annotations

import argparse
import contextlib
import os
import sys

import numpy as np
import torch

FPS = 50
# the augmentation settings and the target widening of the class weights that the reference trains with
# (launch_scripts/train.py:42-57, 75); the three --*-augmentation switches pick from the table
AUGMENTATIONS = {
    "tempo": {"min": -20, "max": 20, "stride": 4},
    "pitch": {"min": -5, "max": 6},
    "mask": {"kind": "permute", "min_count": 1, "max_count": 6, "min_len": 0.1, "max_len": 2, "min_parts": 5, "max_parts": 9},
}
POS_WEIGHT_WIDEN = 3
CHECKPOINT_KEYS = ("state_dict", "hyper_parameters", "optimizer_states", "lr_schedulers", "epoch", "global_step", "rng")
# what fit() and the command line call the switches of model.settings.TrainSettings.violations when they refuse a recipe
_FIT_NAMES = {"frontend_dropout": "frontend_dropout=True", "train_frontend": "a trainable frontend (train_frontend=True)",
              "dropout": "dropout enabled (PLBeatThis(apply_dropout=True) or model.enable_dropout())"}
_FLAGS = {"batch_statistics": "--batch-statistics", "frontend_precision": "--frontend-precision", "dropout": "--dropout",
          "frontend_dropout": "--apply-frontend-dropout", "train_frontend": "--train-frontend", "train_operand": "--mixed-operand",
          "train_mixed": "--precision 16-mixed", "frontend_operand": "--frontend-mixed-operand",
          "frontend_mixed": "--frontend-precision 16-mixed"}


def _rng_state() -> dict:
    """numpy's global generator (the data pipeline's only source of randomness) as tensors and plain numbers"""
    kind, keys, pos, has_gauss, cached = np.random.get_state()
    return {"kind": str(kind), "keys": torch.from_numpy(np.asarray(keys, dtype=np.int64)), "pos": int(pos),
            "has_gauss": int(has_gauss), "cached_gaussian": float(cached)}


def _set_rng_state(state: dict) -> None:
    np.random.set_state((state["kind"], state["keys"].numpy().astype(np.uint32), int(state["pos"]), int(state["has_gauss"]),
                         float(state["cached_gaussian"])))


def _to_cpu(obj):
    if isinstance(obj, torch.Tensor):
        return obj.detach().cpu()
    if isinstance(obj, dict):
        return {k: _to_cpu(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_to_cpu(v) for v in obj)
    return obj


def save_checkpoint(path, pl_module, optimizer, scheduler, epoch: int, global_step: int, loss_scaler=None) -> None:
    """One file with the reference's (Lightning's) top-level keys: ``state_dict`` (``model.`` prefix), ``hyper_parameters``,
    ``optimizer_states`` and ``lr_schedulers`` (one entry each), ``epoch`` (the last finished one), ``global_step`` (optimiser
    steps so far) and ``rng`` (numpy's generator; with dropout enabled also ``rng["dropout"]`` = the model's
    ``dropout_state()``, which carries the frontend's opt-in when it is set); a 16-mixed run adds ``loss_scaler`` (the ``LossScaler``'s state).
    An optimiser that averages the weights (``ema_decay``) and has taken a step adds ``ema_state_dict``: the whole ``state_dict``
    with every optimised parameter replaced by its average -- buffers (BatchNorm statistics among them) and frozen parameters
    are the live ones; ``state_dict`` stays the live weights, and the average itself travels in the optimiser's state (so the
    file holds the averages twice: it grows by two copies of the trained weights).  Written
    next to ``path`` first and then moved over it."""
    ckpt = {"state_dict": _to_cpu(dict(pl_module.state_dict())), "hyper_parameters": dict(pl_module.hyper_parameters),
            "optimizer_states": [_to_cpu(optimizer.state_dict())], "lr_schedulers": [_to_cpu(scheduler.state_dict())],
            "epoch": int(epoch), "global_step": int(global_step), "rng": _rng_state()}
    dropout = pl_module.model.dropout_state()
    if dropout is not None:
        ckpt["rng"]["dropout"] = dropout
    if loss_scaler is not None:
        ckpt["loss_scaler"] = loss_scaler.state_dict()
    if getattr(optimizer, "ema_decay", None) is not None and optimizer.flat_state()["n_averaged"] > 0:
        names = {id(p): n.replace("_orig_mod.", "") for n, p in pl_module.named_parameters()}
        averaged = dict(ckpt["state_dict"])
        for p, e in zip((p for g in optimizer.param_groups for p in g["params"]), optimizer.ema_parameters()):
            if id(p) not in names:
                raise ValueError("the optimiser averages a parameter that is not one of pl_module's: ema_state_dict cannot name it")
            averaged[names[id(p)]] = e.detach().cpu()
        ckpt["ema_state_dict"] = averaged
    path = os.fspath(path)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = path + ".part"
    torch.save(ckpt, tmp)
    os.replace(tmp, path)


def _validation_values(pl_module, batch, i):
    """one validation batch -> (its size, {name: value as a Python float})"""
    losses, metrics = pl_module.validation_step(batch, i)
    values = {"val_loss": losses["total"], "val_loss_beat": losses["beat"], "val_loss_downbeat": losses["downbeat"]}
    values.update({f"val_{k}": v for k, v in metrics.items()})
    return int(batch["spect"].shape[0]), {k: float(v) for k, v in values.items()}


def _ranks(group) -> tuple:
    """(world, rank) of this process in ``group``; (1, 0) without one -- and without importing torch.distributed"""
    if group is None:
        return 1, 0
    import torch.distributed as dist

    return dist.get_world_size(group), dist.get_rank(group)


def validate(pl_module, datamodule, process_group=None) -> dict:
    """The mean over the validation set (weighted by batch size) of the losses and of what the reference's ``step="val"``
    reports: F-measure and Cemgil for beats and downbeats.  ``process_group``: batch ``j`` is computed by rank ``j % world``,
    the per-batch values are gathered and every rank adds them in batch order -- the single-process numbers exactly, on
    every rank."""
    world, rank = _ranks(process_group)
    loader = datamodule.val_dataloader()
    own = enumerate(loader) if process_group is None else loader.shard(rank, world)
    per_batch = {j: _validation_values(pl_module, batch, j) for j, batch in own}
    if process_group is not None:
        import torch.distributed as dist

        gathered = [None] * world
        dist.all_gather_object(gathered, per_batch, group=process_group)
        per_batch = {j: v for part in gathered for j, v in part.items()}
    sums, count = {}, 0
    for j in sorted(per_batch):
        n, values = per_batch[j]
        for k, v in values.items():
            sums[k] = sums.get(k, 0.0) + n * v
        count += n
    return {k: v / count for k, v in sums.items()} if count else {}


def step_groups(batches: int, accumulate: int, world: int = 1) -> list:
    """The optimiser steps of one epoch of ``batches`` global batches on ``world`` ranks: [(first, count)], consecutive runs of
    ``accumulate * world`` global batches and, last, the remainder with its own count.  Global batch ``j`` is rank
    ``j % world``'s; a rank that owns none of a group's batches still takes part in the group's step."""
    size = int(accumulate) * int(world)
    if size < 1 or batches < 0:
        raise ValueError("accumulate and world must be at least 1, batches at least 0")
    return [(first, min(size, batches - first)) for first in range(0, batches, size)]


def _broadcast(tensors, group, staged: bool) -> None:
    """rank 0's values into every rank's ``tensors`` (in place)"""
    import torch.distributed as dist

    src = dist.get_global_rank(group, 0)
    with torch.no_grad():
        for t in tensors:
            if staged:
                host = t.detach().cpu()
                dist.broadcast(host, src, group=group)
                t.copy_(host)
            else:
                dist.broadcast(t.detach(), src, group=group)
                torch.autograd.graph.increment_version(t)   # (written behind autograd's back, as the optimiser's step is)


def _fingerprint(optimizer) -> tuple:
    """A cheap bit fingerprint of a rank's training state: exp_avg's bits summed as integers, and where numpy's generator is"""
    kind, keys, pos, has_gauss, cached = np.random.get_state()
    moments = int(optimizer.flat_state()["exp_avg"].view(torch.int32).sum(dtype=torch.int64))
    return moments, int(pos), int(np.asarray(keys, dtype=np.uint64).sum()), int(has_gauss)


def _apply_settings(model, *, precision, mixed_operand, train_frontend, batch_statistics, frontend_precision, frontend_mixed_operand,
                    frontend_dropout) -> None:
    """``fit``'s requests to the model, in ``fit``'s order; None leaves a setting as it is"""
    if precision is None and mixed_operand is not None:
        precision = model.train_precision
    if frontend_precision is None and frontend_mixed_operand is not None:
        frontend_precision = model.frontend_precision
    if precision is not None:
        model.set_train_precision(precision, mixed_operand)
    if train_frontend is not None:
        model.set_frontend_trainable(train_frontend)
    if batch_statistics is not None:
        model.set_batch_statistics(batch_statistics)
    if frontend_precision is not None:
        model.set_frontend_precision(frontend_precision, frontend_mixed_operand)
    if frontend_dropout is not None:
        model.train_settings.changed("recipe", ValueError, _FIT_NAMES, only="frontend_dropout", frontend_dropout=bool(frontend_dropout))
        state = model.dropout_state()
        if state is not None:
            model.set_dropout_state(dict(state, frontend=bool(frontend_dropout)))


def _restore(resume, pl_module, optimizer, scheduler, scaler, log) -> tuple:
    """``resume`` (a checkpoint of ``fit``: path or loaded dict) into the run's objects and numpy's generator -> (the epoch to
    go on with, the optimiser steps so far)"""
    from .inference import load_checkpoint

    ckpt = resume if isinstance(resume, dict) else load_checkpoint(resume, "cpu")
    missing = [k for k in CHECKPOINT_KEYS if k not in ckpt]
    if missing:
        raise ValueError(f"cannot resume: the checkpoint has no {missing} (written by fit()?)")
    pl_module.load_state_dict(ckpt["state_dict"])
    optimizer.load_state_dict(ckpt["optimizer_states"][0])
    scheduler.load_state_dict(ckpt["lr_schedulers"][0])
    _set_rng_state(ckpt["rng"])
    if "dropout" in ckpt["rng"] and pl_module.model.dropout_state() is not None:
        pl_module.model.set_dropout_state(ckpt["rng"]["dropout"])
    if scaler is not None and "loss_scaler" in ckpt:
        scaler.load_state_dict(ckpt["loss_scaler"])
    log(f"resumed after epoch {ckpt['epoch']} ({int(ckpt['global_step'])} optimiser steps)")
    return int(ckpt["epoch"]) + 1, int(ckpt["global_step"])


def fit(pl_module, datamodule, max_epochs, accumulate_grad_batches=1, val_frequency=5, max_grad_norm=None, checkpoint_path=None,
        resume=None, log=print, precision=None, train_frontend=None, batch_statistics=None, frontend_precision=None,
        frontend_dropout=None, ema_decay=None, mixed_operand=None, frontend_mixed_operand=None, process_group=None,
        staged=False) -> dict:
    """Train ``pl_module`` (on a ROCm GPU) for ``max_epochs`` epochs over ``datamodule.train_dataloader()``.  The rules behind
    each argument are DESIGN.md's: the loop in section 14, then the section named with the argument.

    ``accumulate_grad_batches``: one ``optimizer.step()`` and ``scheduler.step()`` per that many batches, and one for an
    epoch's remainder with its own count (``step_groups``); the schedule spans ``max_epochs`` times an epoch's steps.
    ``max_grad_norm``: the optimiser clips to that global gradient norm (None: no clipping).
    ``val_frequency``: ``validate`` runs after every that-many-th epoch.
    ``checkpoint_path``: ``save_checkpoint`` writes there at each epoch's end (None: nowhere).
    ``resume``: such a checkpoint, path or loaded dict: the run continues with the next epoch, bit for bit as if it had not
    stopped; it needs the settings of the run that wrote it.
    ``log``: called with one line per epoch (and one after a resume).
    ``precision`` ("16-mixed", "32-high", "32-true"), ``train_frontend``, ``batch_statistics`` (True / False),
    ``frontend_precision`` (as ``precision``), ``frontend_dropout`` (True / False; True needs dropout enabled and a trainable
    frontend, ``ValueError`` otherwise): the model's settings, applied in this order before the optimiser is built; None leaves
    the model as it is.  Sections 16 and 25, 17, 18, 19, 21; ``model.settings.TrainSettings`` says what each means.  A
    ``LossScaler`` scales the loss iff some part is 16-mixed on fp16 operands; the losses reported are unscaled.
    ``mixed_operand``, ``frontend_mixed_operand``: "fp16" or "bf16", the ``operand`` of ``set_train_precision`` /
    ``set_frontend_precision``, set together with the part's precision (given alone: with the precision the part has).
    Section 24.
    ``ema_decay``: a float in [0, 1): the optimiser averages the weights it trains, ``validate`` runs on the averages and the
    checkpoint gains ``ema_state_dict``; None: off, and every call is the one of a run without it.  Section 22.
    ``process_group``: a ``torch.distributed`` group, one rank per process, every rank with the same module settings, the same
    numpy seed and, with ``resume``, the same file: data-parallel training, in which rank ``j % world`` runs global batch ``j``
    and one step closes ``accumulate_grad_batches * world`` batches.  ``staged``: its collectives go through host copies
    (gloo, ranks that share one GPU).  None: ``torch.distributed`` is not imported, and the run is the ``world = 1`` case of
    the same loop.  Section 26.

    A module whose model has dropout enabled or uses batch statistics is put into ``train()`` mode here and stays in it.  A
    training loader that yields another number of batches than its ``len()`` is a ``RuntimeError``.

    -> dict: ``train_loss`` (one mean per epoch run), ``val`` ([(epoch, metrics)]), ``epoch``, ``global_step``, ``optimizer``,
    ``scheduler``, ``loss_scaler`` (None without a loss scale); in a group the same on every rank."""
    from .optim import LossScaler

    model, group = pl_module.model, process_group
    _apply_settings(model, precision=precision, mixed_operand=mixed_operand, train_frontend=train_frontend,
                    batch_statistics=batch_statistics, frontend_precision=frontend_precision,
                    frontend_mixed_operand=frontend_mixed_operand, frontend_dropout=frontend_dropout)
    scaler = LossScaler() if model.train_settings.needs_loss_scale() else None   # (16-mixed on fp16 operands somewhere)
    accumulate, max_epochs, val_frequency = int(accumulate_grad_batches), int(max_epochs), int(val_frequency)
    if accumulate < 1 or max_epochs < 0 or val_frequency < 1:
        raise ValueError("accumulate_grad_batches and val_frequency must be at least 1, max_epochs at least 0")
    datamodule.setup("fit")   # (returns at once when the caller has set the data up already)
    loader = datamodule.train_dataloader()
    world, rank = _ranks(group)
    batches = len(loader)
    groups = step_groups(batches, accumulate, world)
    extra = {} if ema_decay is None else {"ema_decay": ema_decay}
    if group is not None:
        extra.update(process_group=group, staged=staged)
    conf = pl_module.configure_optimizers(max(1, len(groups) * max_epochs), max_grad_norm=max_grad_norm,
                                          accumulate=accumulate * world, **extra)
    optimizer, scheduler = conf["optimizer"], conf["lr_scheduler"]["scheduler"]
    first_epoch, global_step = (0, 0) if resume is None else _restore(resume, pl_module, optimizer, scheduler, scaler, log)
    if model.dropout_state() is not None or model.batch_statistics:
        pl_module.train()
    history = {"train_loss": [], "val": [], "optimizer": optimizer, "scheduler": scheduler, "loss_scaler": scaler}
    optimizer.zero_grad()
    if group is not None:
        import torch.distributed as dist

        _broadcast(list(pl_module.parameters()) + list(pl_module.buffers()), group, staged)

    scaled = {} if scaler is None else {"loss_scaler": scaler}

    def close(count):
        optimizer.step(accumulated=count, **scaled)
        scheduler.step()

    for epoch in range(first_epoch, max_epochs):
        losses = torch.zeros(max(batches, 1), dtype=torch.float32, device=optimizer.device)
        # in a group the forward of global batch j draws the single process's streams: the model's counter follows j
        rng = None if group is None else model.train_settings.dropout_rng   # (None, or the live {"seed", "calls"})
        if rng is not None:
            calls0 = int(rng["calls"])
            advance = 2 * len(model.transformer_blocks.layers) + (12 if model.frontend_dropout else 0)
        done = seen = 0
        mine = len(range(rank, batches, world))   # (how many of the epoch's batches are this process's)
        for j, batch in (enumerate(loader) if group is None else loader.shard(rank, world)):
            if j >= batches:
                raise RuntimeError(f"the training loader has {batches} batches (len) and yielded batch {j}")
            while j >= groups[done][0] + groups[done][1]:
                close(groups[done][1])
                done += 1
            if rng is not None:
                rng["calls"] = calls0 + j * advance
            loss = pl_module.training_step(batch, j)
            if rng is not None and rng["calls"] != calls0 + (j + 1) * advance:
                raise RuntimeError(f"a training forward drew {rng['calls'] - calls0 - j * advance} dropout streams, {advance} were "
                                   "expected: the ranks' streams would not be the single-process ones")
            (loss if scaler is None else loss * scaler.scale).backward()
            losses[j] = loss.detach()
            seen += 1
        if seen != mine:
            raise RuntimeError(f"the training loader has {batches} batches (len), {mine} of them this process's, and ended after {seen}")
        for _, count in groups[done:]:   # the groups no batch of this process came after: the epoch's last, with its own count
            close(count)
        global_step += len(groups)
        if rng is not None:
            rng["calls"] = calls0 + batches * advance
        if group is not None and model.batch_statistics:
            _broadcast(list(pl_module.buffers()), group, staged)
        # the epoch's only read-back: every process's losses, added in global batch order as a chain of fp32 additions from 0
        parts = [losses.cpu().numpy()]
        if group is not None:
            gathered = [None] * world
            dist.all_gather_object(gathered, (parts[0], _fingerprint(optimizer)), group=group)
            parts, prints = [g[0] for g in gathered], [g[1] for g in gathered]
            if any(p != prints[0] for p in prints):
                odd = [r for r, p in enumerate(prints) if p != prints[0]]
                raise RuntimeError(f"epoch {epoch}: ranks {odd} have diverged from rank 0 (optimiser moments or numpy's generator): "
                                   f"fingerprints {prints}")
        total = np.float32(0.0)
        for j in range(batches):
            total = total + parts[j % world][j]
        mean = float(total) / max(batches, 1)
        history["train_loss"].append(mean)
        line = f"epoch {epoch}: train_loss {mean:.6f}, {global_step} steps, lr {scheduler.get_last_lr()[0]:.3e}"
        if group is not None:
            line += f", {world} ranks"
        if (epoch + 1) % val_frequency == 0:
            averaged = ema_decay is not None and optimizer.flat_state()["n_averaged"] > 0
            with optimizer.averaged_weights() if averaged else contextlib.nullcontext():
                metrics = validate(pl_module, datamodule, group)
            history["val"].append((epoch, metrics))
            if averaged:
                line += f", validated on the averaged weights (decay {ema_decay:g})"
            line += "".join(f", {k} {v:.4f}" for k, v in metrics.items())
        if checkpoint_path is not None:
            if rank == 0:
                save_checkpoint(checkpoint_path, pl_module, optimizer, scheduler, epoch, global_step, scaler)
            if group is not None:
                dist.barrier(group=group)
        if rank == 0:
            log(line)
    history["epoch"], history["global_step"] = max(first_epoch, max_epochs) - 1, global_step
    return history


# ---- command line (launch_scripts/train.py:135-291) ------------------------------------------------------------------------------
def _ema_decay(text: str) -> float:
    value = float(text)
    if not 0.0 <= value < 1.0:
        raise argparse.ArgumentTypeError(f"the decay of the weight average must lie in [0, 1), got {text}")
    return value


def get_parser() -> argparse.ArgumentParser:
    from .loss import LOSS_TYPES

    p = argparse.ArgumentParser(description="Fine-tune Beat This! on the MI355X kernels (frozen frontend unless --train-frontend, fp32 or --precision "
                                            "16-mixed, dropout in the main transformer with --dropout, in the frontend too with "
                                            "--apply-frontend-dropout).")
    toggle = argparse.BooleanOptionalAction
    p.add_argument("--data-dir", type=str, required=True, help="data folder: annotations/ and the spectrogram bundles")
    p.add_argument("--checkpoint", type=str, default=None,
                   help="checkpoint (name, path or URL) to start from; default: a new model with the reference's initialisation")
    p.add_argument("--output", type=str, required=True, help="where the checkpoint is written at each epoch's end")
    p.add_argument("--gpu", type=int, default=0, help="index of the GPU to use (default: %(default)s)")
    p.add_argument("--gpus", metavar="N", type=int, default=1,
                   help="data-parallel training on N GPUs of this node, one process each: the run launches itself under "
                        "torch.distributed.run (a run already started by torchrun is taken as it is); one optimiser step then "
                        "closes --accumulate-grad-batches x N batches (default: %(default)s, a single process without a process group)")
    p.add_argument("--share-gpu", action="store_true",
                   help="development / tests, with --gpus N > 1: all N ranks run on --gpu and the collectives go over gloo through "
                        "host copies -- the N-rank code path on a node with one GPU; not a measurement")
    p.add_argument("--n-layers", type=int, default=6, help="main transformer layers of a new model (default: %(default)s)")
    p.add_argument("--transformer-dim", type=int, default=512, help="width of a new model (default: %(default)s)")
    p.add_argument("--lr", type=float, default=0.0008)
    p.add_argument("--weight-decay", type=float, default=0.01)
    p.add_argument("--loss", type=str, default="shift_tolerant_weighted_bce", choices=list(LOSS_TYPES), help="the loss to use")
    p.add_argument("--warmup-steps", type=int, default=1000, help="warm-up steps of the schedule")
    p.add_argument("--max-epochs", type=int, default=100)
    p.add_argument("--batch-size", type=int, default=8)
    p.add_argument("--accumulate-grad-batches", type=int, default=8)
    p.add_argument("--train-length", type=int, default=1500, help="excerpt length in frames")
    p.add_argument("--max-grad-norm", type=float, default=None, help="clip the global gradient norm to this (default: no clipping)")
    p.add_argument("--dropout", default=False, action=toggle,
                   help="train the main transformer layers with dropout, seeded by --seed (default: off)")
    p.add_argument("--transformer-dropout", metavar="RATE", type=float, default=None,
                   help="dropout rate of the main transformer layers, 0 <= RATE < 1 (default: the checkpoint's, or 0.2 for a new model)")
    p.add_argument("--frontend-dropout", metavar="RATE", type=float, default=None,
                   help="dropout rate of the frontend's partial transformers, 0 <= RATE < 1; used with --apply-frontend-dropout "
                        "(default: the checkpoint's, or 0.1 for a new model)")
    p.add_argument("--apply-frontend-dropout", default=False, action=toggle,
                   help="with --dropout and --train-frontend: the attention / feed-forward leaves of the frontend's partial "
                        "transformers drop too, at --frontend-dropout (default: off)")
    p.add_argument("--precision", type=str, default="32-true", choices=["32-true", "32-high", "16-mixed"],
                   help="16-mixed: the reference's training precision -- fp16 matrix products in the main layers, fp32 master "
                        "weights, a dynamic loss scale; 32-high: the same products with every fp32 operand as two bfloat16 "
                        "halves on three bfloat16 MFMAs, no loss scale (default: %(default)s)")
    p.add_argument("--mixed-operand", type=str, default=None, choices=["fp16", "bf16"],
                   help="with --precision 16-mixed: the format its matrix products round their operands to; bf16 has fp32's "
                        "exponent range and needs no loss scale (default: fp16)")
    p.add_argument("--train-frontend", default=False, action=toggle,
                   help="whole-model fine-tuning: also train the frontend (frozen BatchNorm statistics unless --batch-statistics, "
                        "no frontend dropout unless --apply-frontend-dropout, fp32 frontend unless --frontend-precision 16-mixed; default: the frontend stays frozen)")
    p.add_argument("--frontend-precision", type=str, default="32-true", choices=["32-true", "32-high", "16-mixed"],
                   help="with --train-frontend: 16-mixed runs the matrix products of the frontend's conv units, partial "
                        "transformers and projection on fp16 operands too, under the same loss scale; 32-high: on split "
                        "bfloat16 operands (default: %(default)s)")
    p.add_argument("--frontend-mixed-operand", type=str, default=None, choices=["fp16", "bf16"],
                   help="with --frontend-precision 16-mixed: the same choice for the frontend's products (default: fp16)")
    p.add_argument("--batch-statistics", default=False, action=toggle,
                   help="with --train-frontend: the frontend's BatchNorms use each batch's statistics and update their running "
                        "ones, as training from scratch needs (default: frozen running statistics)")
    p.add_argument("--ema-decay", metavar="D", type=_ema_decay, default=None,
                   help="keep an exponential moving average of the trained weights with this decay, 0 <= D < 1: validation runs "
                        "on it and the checkpoint gains ema_state_dict (default: off)")
    p.add_argument("--dbn", default=False, action=toggle, help="DBN post-processing in validation")
    p.add_argument("--eval-trim-beats", metavar="SECONDS", type=float, default=5,
                   help="skip the first seconds of each piece in the metrics (default: %(default)s)")
    p.add_argument("--val-frequency", metavar="N", type=int, default=5, help="validate every N epochs (default: %(default)s)")
    p.add_argument("--tempo-augmentation", default=True, action=toggle, help="use the precomputed tempo variants")
    p.add_argument("--pitch-augmentation", default=True, action=toggle, help="use the precomputed pitch variants")
    p.add_argument("--mask-augmentation", default=True, action=toggle, help="mask stretches of the excerpts")
    p.add_argument("--length-based-oversampling-factor", type=float, default=0.65,
                   help="oversampling of long pieces; 0 takes one excerpt per piece (default: %(default)s)")
    p.add_argument("--val", default=True, action=toggle,
                   help="--no-val trains on the validation data as well (the validation metrics then mean nothing)")
    p.add_argument("--hung-data", default=False, action=toggle, help="train on the datasets of Hung et al. only")
    p.add_argument("--fold", type=int, default=None, help="the cross-validation fold NOT to train on (0-based)")
    p.add_argument("--seed", type=int, default=0, help="seed of the random number generators")
    p.add_argument("--init-seed", metavar="N", type=int, default=0,
                   help="seed of a new model's initial weights; unused with --checkpoint or --resume-checkpoint (default: %(default)s)")
    p.add_argument("--resume-checkpoint", type=str, default=None, help="continue the run that wrote this checkpoint")
    return p


def _free_port() -> int:
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _launch_ranks(args, argv) -> int:
    """--gpus N outside torchrun: check the node's GPUs, then run this command line once per rank under torch.distributed.run"""
    import subprocess

    have = torch.cuda.device_count()
    if have < args.gpus and not (args.share_gpu and have >= 1):
        raise SystemExit(f"beat_this_amd.train: --gpus {args.gpus} but this node shows {have} GPU(s) (torch.cuda.device_count()); "
                         "run with --gpus <= that, one process per GPU")
    env = dict(os.environ)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # (the ranks import the package this process runs)
    env["PYTHONPATH"] = os.pathsep.join([root] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), "-m", "beat_this_amd.train", *(sys.argv[1:] if argv is None else argv)]
    return subprocess.run(cmd, env=env).returncode


def _join_ranks(args):
    """A rank of a --gpus N run under torchrun: its device, its share of the cores, and the process group -> (device, group,
    rank); the rules are bench.py's"""
    import torch.distributed as dist
    from datetime import timedelta

    world, rank, local_rank = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", "1"), ("RANK", "0"), ("LOCAL_RANK", "0")))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    index = args.gpu if args.share_gpu else local_rank
    if index >= torch.cuda.device_count():
        raise SystemExit(f"beat_this_amd.train: LOCAL_RANK {local_rank} but this node shows {torch.cuda.device_count()} GPU(s)")
    try:   # every rank its own slice of the cores, torch's intra-op pool sized to it
        cores = sorted(os.sched_getaffinity(0))
        per_rank = max(1, len(cores) // int(os.environ.get("LOCAL_WORLD_SIZE", world)))
        mine = cores[local_rank * per_rank: (local_rank + 1) * per_rank] or cores
        os.sched_setaffinity(0, mine)
        torch.set_num_threads(max(1, min(len(mine), 16)))
    except (AttributeError, OSError) as e:   # (no affinity interface: leave the scheduler alone)
        print(f"rank {rank}: host threads not pinned ({type(e).__name__})", file=sys.stderr)
    torch.cuda.set_device(index)
    device = torch.device("cuda", index)
    # (a collective whose peer died is aborted after three minutes; a rank that RAISES takes the job down at once, see main)
    if args.share_gpu:
        dist.init_process_group("gloo", timeout=timedelta(seconds=180))
    else:
        dist.init_process_group("nccl", device_id=device, timeout=timedelta(seconds=180))
    return device, dist.group.WORLD, rank


def main(argv=None) -> int:
    parser = get_parser()
    args = parser.parse_args(argv)
    if args.gpus < 1:
        parser.error(f"--gpus must be at least 1, got {args.gpus}")
    if args.share_gpu and args.gpus < 2:
        parser.error("--share-gpu needs --gpus N with N > 1: it puts the N ranks of a data-parallel run on one GPU")
    _check_recipe(parser, args)
    if args.gpus > 1 and "RANK" not in os.environ:
        return _launch_ranks(args, argv)
    if args.gpus == 1:
        return _run(args)
    return run_rank(lambda: _run(args, ranks=True))


def run_rank(body):
    """``body()`` as one rank of a multi-process job.  A rank that raises takes the whole job down AT ONCE (bench.py's rule):
    the traceback is printed and the process leaves through ``os._exit``, without the interpreter's teardown -- which would
    wait for the process group, while the peers wait in a collective for this rank -- so the launcher sees a dead rank and
    ends the others."""
    try:
        return body()
    except BaseException:   # noqa: BLE001
        import traceback

        traceback.print_exc()
        sys.stderr.flush()
        sys.stdout.flush()
        os._exit(1)


def _check_recipe(parser, args) -> None:
    from .model.settings import TrainSettings

    asked = TrainSettings(frontend_trainable=args.train_frontend, batch_statistics=args.batch_statistics,
                          train_precision=args.precision, train_operand=args.mixed_operand or "fp16",
                          frontend_precision=args.frontend_precision, frontend_operand=args.frontend_mixed_operand or "fp16",
                          dropout_rng={"seed": args.seed, "calls": 0} if args.dropout else None,
                          frontend_dropout=args.apply_frontend_dropout)
    for violation in asked.violations("recipe"):   # (before the data folder is touched)
        parser.error(violation.message(_FLAGS))
    for flag, operand, part, precision in (("--mixed-operand", args.mixed_operand, "--precision", args.precision),
                                           ("--frontend-mixed-operand", args.frontend_mixed_operand, "--frontend-precision",
                                            args.frontend_precision)):
        if operand is not None and precision != "16-mixed":   # (fp16 too: the flag says nothing about a 32-true part)
            parser.error(f"{flag} needs {part} 16-mixed: it is the operand format of 16-mixed products")


def _run(args, ranks: bool = False) -> int:
    """the run of one process: the whole of a --gpus 1 run, or (``ranks``) one rank of a data-parallel one"""
    from .dataset import BeatDataModule
    from .inference import load_checkpoint
    from .model.pl_module import PLBeatThis

    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    if not torch.cuda.is_available():
        print("beat_this_amd.train needs a ROCm GPU: this package has no CPU path", file=sys.stderr)
        return 2
    group, rank = None, 0
    if ranks:
        device, group, rank = _join_ranks(args)
    else:
        device = torch.device(f"cuda:{args.gpu}")
    say = print if rank == 0 else (lambda *a, **k: None)   # (only rank 0 prints the run's lines)
    say("Starting a run with:", vars(args))
    enabled = {name: dict(settings) for name, settings in AUGMENTATIONS.items() if getattr(args, f"{name}_augmentation")}
    datamodule = BeatDataModule(args.data_dir, batch_size=args.batch_size, train_length=args.train_length, spect_fps=FPS,
                                test_dataset="gtzan", length_based_oversampling_factor=args.length_based_oversampling_factor,
                                augmentations=enabled, hung_data=args.hung_data, no_val=not args.val, fold=args.fold,
                                device=device)
    datamodule.setup("fit")   # (the class weights below need the training set; fit()'s own setup call then returns at once)
    pos_weights = datamodule.get_train_positive_weights(widen_target_mask=POS_WEIGHT_WIDEN)
    say("Using positive weights:", pos_weights)
    start = args.resume_checkpoint or args.checkpoint
    ckpt = load_checkpoint(start, "cpu") if start else None
    arch = dict(transformer_dim=args.transformer_dim, n_layers=args.n_layers)
    if ckpt is not None:   # the architecture is the checkpoint's
        keys = ("spect_dim", "transformer_dim", "ff_mult", "n_layers", "stem_dim", "head_dim", "sum_head", "partial_transformers", "dropout")
        arch = {k: ckpt["hyper_parameters"][k] for k in keys if k in ckpt["hyper_parameters"]}
    if args.transformer_dropout is not None:
        arch["dropout"] = dict(arch.get("dropout", {"frontend": 0.1}), transformer=args.transformer_dropout)
    if args.frontend_dropout is not None:
        arch["dropout"] = dict(arch.get("dropout", {"transformer": 0.2}), frontend=args.frontend_dropout)
    pl_module = PLBeatThis(**arch, apply_dropout=args.dropout, dropout_seed=args.seed, fps=FPS, lr=args.lr,
                           weight_decay=args.weight_decay, pos_weights=pos_weights, loss_type=args.loss,
                           warmup_steps=args.warmup_steps, max_epochs=args.max_epochs, use_dbn=args.dbn,
                           eval_trim_beats=args.eval_trim_beats, precision=args.precision, train_frontend=args.train_frontend,
                           batch_statistics=args.batch_statistics, frontend_precision=args.frontend_precision,
                           mixed_operand=args.mixed_operand, frontend_mixed_operand=args.frontend_mixed_operand,
                           apply_frontend_dropout=args.apply_frontend_dropout, init_seed=0 if ckpt is not None else args.init_seed)
    if ckpt is not None and not args.resume_checkpoint:   # (a resumed run's weights are restored by fit() with the rest)
        pl_module.load_state_dict(ckpt["state_dict"])
    pl_module.to(device)
    extra = {}
    if group is not None:
        extra.update(process_group=group, staged=args.share_gpu)
    with torch.cuda.device(device):
        fit(pl_module, datamodule, args.max_epochs, accumulate_grad_batches=args.accumulate_grad_batches,
            val_frequency=args.val_frequency, max_grad_norm=args.max_grad_norm, checkpoint_path=args.output,
            resume=ckpt if args.resume_checkpoint else None, ema_decay=args.ema_decay, log=say, **extra)
    say("wrote", args.output)
    if group is not None:
        import torch.distributed as dist

        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
