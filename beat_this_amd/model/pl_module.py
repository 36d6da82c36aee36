"""``PLBeatThis`` -- the reference's training module (beat_this/model/pl_module.py:21-317) without Lightning: a plain
``nn.Module`` that wraps a ``BeatThis`` model with its loss pair, post-processor, metrics and optimiser, and is driven by
``beat_this_amd.train.fit``.  Same constructor arguments, same ``state_dict`` keys (``model.`` prefix) and the same
``hyper_parameters``, so the checkpoints ``fit`` writes are read by ``load_model`` and ``losses_from_hparams`` like the
reference's.  The schedule and the parameter grouping live in ``beat_this_amd.optim``.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from .. import optim as _optim
from ..loss import losses_from_hparams
from ..metrics import Metrics
from ..postprocessor import Postprocessor
from . import BeatThis
from .settings import TrainSettings

CosineWarmupScheduler = _optim.CosineWarmupScheduler   # (the reference defines it in this module)
_SWITCHES = {"frontend_dropout": "apply_frontend_dropout", "dropout": "apply_dropout=True", "train_frontend": "train_frontend=True"}


def _plain(value):
    """hyper-parameters as plain Python values (what ``torch.load(..., weights_only=True)`` reads back)"""
    if isinstance(value, dict):
        return {str(k): _plain(v) for k, v in value.items()}
    if isinstance(value, (list, tuple)):
        return [_plain(v) for v in value]
    if isinstance(value, (bool, np.bool_)):
        return bool(value)
    if isinstance(value, (int, np.integer)):
        return int(value)
    if isinstance(value, (float, np.floating)):
        return float(value)
    return value


TARGETS = ("beat", "downbeat")
_MODEL_KEYS = ("spect_dim", "transformer_dim", "ff_mult", "stem_dim", "n_layers", "head_dim", "dropout", "sum_head", "partial_transformers")


class PLBeatThis(nn.Module):
    """The model and everything a training run needs around it.

    The six main layers, the final RMSNorm and the task heads are trainable; everything else about the training route is a
    switch that maps onto one field of the model's ``settings.TrainSettings``, which says what it means: ``train_frontend``
    (``BeatThis.set_frontend_trainable``: whole-model fine-tuning, else the frontend is frozen), on top of it
    ``batch_statistics`` (``set_batch_statistics``: what training from scratch needs) and ``frontend_precision`` ("16-mixed", "32-high" or
    "32-true"; None leaves the model's default, "32-true"; ``set_frontend_precision``); ``precision`` ("32-true", the default,
    "32-high" -- fp32 products on three bfloat16 MFMAs, no loss scale -- or "16-mixed", the reference's trainer setting:
    ``set_train_precision``, and ``fit`` then scales the loss with an ``optim.LossScaler``); ``mixed_operand`` / ``frontend_mixed_operand`` ("fp16", "bf16" or None = "fp16": the ``operand`` of those
    two setters -- the format a 16-mixed part rounds its products' operands to; "bf16" needs no loss scale and is a ``ValueError``
    on a part that is not "16-mixed"); ``apply_dropout`` (``enable_dropout`` under ``dropout_seed``: the main layers drop at
    ``dropout["transformer"]`` like the reference's, with this package's own masks) and on top of it and of ``train_frontend``
    (``ValueError`` without either) ``apply_frontend_dropout`` (``enable_dropout(frontend=True)``: the frontend's leaves drop at
    ``dropout["frontend"]`` too, the reference's full recipe; without it that rate stays unused).  With dropout or batch
    statistics ``fit`` trains in ``train()`` mode.  ``dropout`` itself is stored in the hyper-parameters and handed to the model;
    the switches and ``init_seed`` -- the seed of a new model's initial weights (``BeatThis.init_weights``; 0 is what it always
    was) -- are no hyper-parameters: a checkpoint carries the reference's keys only.  ``max_epochs`` is stored only; ``fit`` takes
    the number of epochs to run."""

    def __init__(self, spect_dim=128, fps=50, transformer_dim=512, ff_mult=4, n_layers=6, stem_dim=32,
                 dropout={"frontend": 0.1, "transformer": 0.2}, lr=0.0008, weight_decay=0.01,
                 pos_weights={"beat": 1, "downbeat": 1}, head_dim=32, loss_type="shift_tolerant_weighted_bce",
                 warmup_steps=1000, max_epochs=100, use_dbn=False, eval_trim_beats=5, sum_head=True, partial_transformers=True,
                 apply_dropout=False, dropout_seed=0, precision="32-true", train_frontend=False,
                 batch_statistics=False, frontend_precision=None, apply_frontend_dropout=False, init_seed=0,
                 mixed_operand=None, frontend_mixed_operand=None):
        given = {k: v for k, v in locals().items()
                 if k not in ("self", "__class__", "apply_dropout", "dropout_seed", "precision", "train_frontend",
                              "batch_statistics", "frontend_precision", "apply_frontend_dropout", "init_seed", "mixed_operand",
                              "frontend_mixed_operand")}
        # what is asked for, checked as a recipe before anything is built (batch statistics: the model's own refusal, below)
        want =TrainSettings().changed(
            "recipe", ValueError, _SWITCHES, only="frontend_dropout", train_precision=precision,
            frontend_trainable=bool(train_frontend), batch_statistics=bool(batch_statistics),
            dropout_rng={"seed": dropout_seed, "calls": 0} if apply_dropout else None, frontend_dropout=bool(apply_frontend_dropout))
        super().__init__()
        hp = self.hyper_parameters = _plain(given)   # what a checkpoint carries: every constructor argument, as plain values
        for key in ("lr", "weight_decay", "fps", "warmup_steps", "max_epochs", "pos_weights", "eval_trim_beats"):
            setattr(self, key, hp[key])
        self.model = BeatThis(**{k: hp[k] for k in _MODEL_KEYS})
        if int(init_seed) != 0:   # (0: the state a new BeatThis holds, to the bit)
            self.model.init_weights(init_seed)
        if want.dropout_rng is not None:   # (applied in this order: init_weights and the requires_grad loop sit in between)
            self.model.enable_dropout(seed=dropout_seed, frontend=want.frontend_dropout)
        self.model.set_train_precision(want.train_precision, mixed_operand)
        if frontend_precision is not None or frontend_mixed_operand is not None:   # BeatThis.set_frontend_precision; no hyper-parameter, like precision
            self.model.set_frontend_precision(self.model.frontend_precision if frontend_precision is None else frontend_precision,
                                              frontend_mixed_operand)
        # trainable: the trunk and the heads, without the rotary tables (fixed in the reference too); frozen: the frontend
        for name, p in self.model.named_parameters():
            p.requires_grad_(not name.startswith("frontend.") and not name.endswith("rotary_embed.freqs"))
        if want.frontend_trainable:   # whole-model fine-tuning (BeatThis.set_frontend_trainable; no hyper-parameter, like apply_dropout)
            self.model.set_frontend_trainable(True)
        if want.batch_statistics:   # training-mode BatchNorm in the frontend (BeatThis.set_batch_statistics; raises without train_frontend)
            self.model.set_batch_statistics(True)
        self.beat_loss, self.downbeat_loss = losses_from_hparams(hp)
        self.postprocessor = Postprocessor(("minimal", "dbn")[bool(use_dbn)], fps)
        self.metrics = Metrics(eval_trim_beats)
        self.lr_scheduler = None

    # ---- losses and metrics ------------------------------------------------------------------------------------------------------
    @staticmethod
    def _loss_masks(batch) -> dict:
        """Which frames count, per target: everything that is not padding; for downbeats only in pieces whose dataset
        annotates them (the reference multiplies the two masks, pl_module.py:100-105)."""
        frames = batch["padding_mask"]
        annotated = batch["downbeat_mask"].reshape(-1, 1)
        return {"beat": frames, "downbeat": torch.logical_and(frames, annotated)}

    def _compute_loss(self, batch, model_prediction) -> dict:
        """-> {"beat", "downbeat", "total"}: each target's loss on its float targets and mask, and their sum"""
        masks = self._loss_masks(batch)
        fns = dict(zip(TARGETS, (self.beat_loss, self.downbeat_loss)))
        out = {t: fns[t](model_prediction[t], batch["truth_" + t].float(), masks[t]) for t in TARGETS}
        out["total"] = out["beat"] + out["downbeat"]
        return out

    def _compute_metrics(self, batch, postp_beat, postp_downbeat, step="val") -> dict:
        """Batch means of ``Metrics`` per target, keyed "<metric>_<target>".  The truth is the annotations in seconds
        (``truth_orig_*``: float64 bytes, one entry per piece), not the quantised frame targets; a tuple-valued metric (Cemgil)
        is averaged over its entries too, as the reference's np.mean does (pl_module.py:156-160)."""
        out = {}
        for target, events in zip(TARGETS, (postp_beat, postp_downbeat)):
            pieces = events if isinstance(events, tuple) else (events,)   # (an unbatched post-processor call gives one array)
            truths = batch["truth_orig_" + target]
            if len(truths) != len(pieces):
                raise ValueError(f"{len(pieces)} predicted {target} sequences for {len(truths)} annotated pieces")
            rows = [self.metrics(np.frombuffer(t, dtype=np.float64), e, step=step) for t, e in zip(truths, pieces)]
            for name in rows[0]:
                out[f"{name}_{target}"] = float(np.mean([r[name] for r in rows]))
        return out

    def _postprocess(self, prediction, padding_mask):
        return self.postprocessor(*(prediction[t] for t in TARGETS), padding_mask)

    # ---- the steps: what the reference's steps compute (pl_module.py:199-277), returned instead of logged ------------------------
    def training_step(self, batch, batch_idx=0):
        """-> the total loss (differentiable); the three losses of the batch stay in ``self.last_losses`` (detached)"""
        losses = self._compute_loss(batch, self.model(batch["spect"]))
        self.last_losses = {k: v.detach() for k, v in losses.items()}
        return losses["total"]

    @torch.no_grad()
    def validation_step(self, batch, batch_idx=0):
        """-> (losses, metrics): F-measure and Cemgil of beats and downbeats on the batch's excerpts"""
        prediction = self.model(batch["spect"])
        events = self._postprocess(prediction, batch["padding_mask"])
        return self._compute_loss(batch, prediction), self._compute_metrics(batch, *events, step="val")

    @torch.no_grad()
    def test_step(self, batch, batch_idx=0):
        """-> (losses, metrics) of one whole piece, through ``predict_step``"""
        metrics, prediction = self.predict_step(batch, batch_idx)[:2]
        return self._compute_loss(batch, prediction), metrics

    @torch.no_grad()
    def predict_step(self, batch, batch_idx=0, dataloader_idx=0, chunk_size=1500, overlap_mode="keep_first"):
        """One whole piece (a batch of one, unpadded) in chunks of ``chunk_size`` frames -> (metrics, prediction, dataset,
        spect_path); where chunks overlap, ``overlap_mode`` keeps the first ("keep_first") or the last one's frames.  The
        frames the loss crops at a chunk's edges (twice its tolerance) are the chunks' borders."""
        from ..inference import split_predict_aggregate

        spect = batch["spect"]
        if spect.dim() != 3 or spect.shape[0] != 1:
            raise ValueError(f"predict_step takes one whole piece per call, got a batch of shape {tuple(spect.shape)}: "
                             "use a loader with batch_size=1")
        if not bool(batch["padding_mask"].all()):
            raise ValueError("predict_step takes an unpadded piece: build the dataset with train_length=None")
        border = 2 * getattr(self.beat_loss, "tolerance", 0)
        logits = split_predict_aggregate(spect[0], chunk_size, border, overlap_mode, self.model)
        prediction = {t: logits[t][None] for t in TARGETS}
        metrics = self._compute_metrics(batch, *self._postprocess(prediction, None), step="test")
        return metrics, prediction, batch["dataset"], batch["spect_path"]

    def configure_optimizers(self, total_steps, max_grad_norm=None, accumulate=1, ema_decay=None, process_group=None, staged=False):
        """The reference's optimiser and schedule (pl_module.py:279-306) on this package's kernels: AdamW at ``lr`` with
        ``weight_decay`` on the matrices only, and the cosine schedule with ``warmup_steps`` over ``total_steps`` optimiser
        steps (what Lightning's ``estimated_stepping_batches`` is there), stepped once per optimiser step.  ``ema_decay``: the
        optimiser also keeps an exponential moving average of the weights (``AdamW(ema_decay=...)``).  ``process_group``,
        ``staged``: the optimiser sums the gradients over that group's ranks at every step (``AdamW(process_group=...)``)."""
        extra = {} if process_group is None else {"process_group": process_group, "staged": staged}
        optimizer = _optim.AdamW(_optim.param_groups_for(self, self.weight_decay), lr=self.lr, max_grad_norm=max_grad_norm,
                                 accumulate=accumulate, ema_decay=ema_decay, **extra)
        self.lr_scheduler = _optim.CosineWarmupScheduler(optimizer, self.warmup_steps, total_steps)
        return {"optimizer": optimizer, "lr_scheduler": {"scheduler": self.lr_scheduler, "interval": "step"}}

    # ---- state dict: the reference's keys ("model." prefix; torch.compile's "_orig_mod." never appears) ----------------------------
    def state_dict(self, *args, **kwargs):
        return {k.replace("_orig_mod.", ""): v for k, v in super().state_dict(*args, **kwargs).items()}

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """Hands the "model." entries to ``BeatThis.load_state_dict`` (which drops its packed inference engine)"""
        clean = {k.replace("_orig_mod.", ""): v for k, v in state_dict.items()}
        inner = {k[len("model."):]: v for k, v in clean.items() if k.startswith("model.")}
        if strict and len(inner) != len(clean):
            raise RuntimeError(f"unexpected keys in the state dict: {sorted(k for k in clean if not k.startswith('model.'))[:5]}")
        return self.model.load_state_dict(inner, strict=strict, assign=assign)
