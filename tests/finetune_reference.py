"""The fine-tuning loop restated in plain torch on the CPU, in any float dtype: what ``beat_this_amd.train.fit`` has to compute
over a list of recorded batches, written from DESIGN.md sections 11, 14 and 15 and the reference's training module
(beat_this/model/pl_module.py:100-105 the masks, :279-306 the optimiser and its two groups, :342-369 the schedule) without
anything of beat_this_amd.optim, .train, .loss or .model.pl_module.  In fp64 it is the truth of the trajectory tests
(tests/test_finetune_reference.py, tests/test_gpu_finetune_trajectory.py), in fp32 their yardstick ``e_ref``
(trunk_grad_util.py); ``mutant=`` switches on one deviation at a time, to show that the yardstick tells them apart.

Also the pieces the tests of the backward pass and of dropout share with it: the shift-tolerant loss and the masked units.
"""
import math

import torch
import torch.nn.functional as F

import dropout_reference as R
import trunk_grad_util as U
from oracle import beat_this_oracle as O

MUTANTS = ("decay_all", "remainder_by_accumulate", "schedule_shift", "ignore_downbeat_mask", "pos_weight_1", "no_clip")


# ---- the loss -------------------------------------------------------------------------------------------------------------------
def shift_tolerant_bce(preds, targets, mask, pos_weight=1.0, tol=3):
    """the shift-tolerant loss as DESIGN.md section 11 states it, in torch on the CPU (differentiable, any float dtype)"""
    X = F.max_pool1d(preds[:, None], 1 + 2 * tol, 1)[:, 0][:, tol:preds.shape[1] - 3 * tol]
    S = F.max_pool1d(targets[:, None], 1 + 4 * tol, 1)[:, 0]
    y = targets[:, 2 * tol:targets.shape[1] - 2 * tol]
    w = (y + (1 - S)) * mask[:, 2 * tol:mask.shape[1] - 2 * tol]
    return F.binary_cross_entropy_with_logits(X, y, weight=w, pos_weight=torch.tensor(pos_weight, dtype=preds.dtype))


def batch_losses(beat, down, batch, dtype, pos_weights, tol=3, use_downbeat_mask=True):
    """-> (beat, downbeat, total): the beat loss counts every frame that is not padding, the downbeat loss those of the pieces
    whose dataset annotates downbeats (pl_module.py:100-105); the total is their sum"""
    frames = batch["padding_mask"].to(dtype)
    annotated = batch["downbeat_mask"].reshape(-1, 1).to(dtype) if use_downbeat_mask else 1.0
    lb = shift_tolerant_bce(beat, batch["truth_beat"].to(dtype), frames, float(pos_weights["beat"]), tol)
    ld = shift_tolerant_bce(down, batch["truth_downbeat"].to(dtype), frames * annotated, float(pos_weights["downbeat"]), tol)
    return lb, ld, lb + ld


# ---- the units with masks, in torch on the CPU (any float dtype) ------------------------------------------------------------------
def attention_drop(x, sd, pfx, heads, mask_p, mask_out, c):
    """oracle.attention with the softmax written out, the probabilities times mask_p c and to_out's result times mask_out c"""
    b, n, dim = x.shape
    xn = O.rmsnorm(x, sd[pfx + "norm.gamma"])
    qkv = O._linear(xn, sd[pfx + "to_qkv.weight"]).view(b, n, 3, heads, 32).permute(2, 0, 3, 1, 4)
    fr = sd[pfx + "rotary_embed.freqs"]
    q, k, v = O.rope(qkv[0], fr), O.rope(qkv[1], fr), qkv[2]
    att = torch.softmax((q @ k.transpose(-1, -2)) * (32 ** -0.5), dim=-1)
    out = (att * mask_p * c) @ v
    gates = O._linear(xn, sd[pfx + "to_gates.weight"], sd[pfx + "to_gates.bias"])
    out = (out * torch.sigmoid(gates).permute(0, 2, 1)[..., None]).permute(0, 2, 1, 3).reshape(b, n, dim)
    return O._linear(out, sd[pfx + "to_out.0.weight"]) * mask_out * c


def feedforward_drop(x, sd, pfx, mask_hidden, mask_out, c):
    h = O.rmsnorm(x, sd[pfx + "net.0.gamma"])
    h = F.gelu(O._linear(h, sd[pfx + "net.1.weight"], sd[pfx + "net.1.bias"])) * mask_hidden * c
    return O._linear(h, sd[pfx + "net.4.weight"], sd[pfx + "net.4.bias"]) * mask_out * c


def unit_masks(kind, p, seed, stream, Bn, T, D, hidden):
    """the two masks of one unit call as numpy arrays in the shapes the restatements multiply by"""
    if kind == "attn":
        return (R.mask(p, seed, stream, R.ATTN_P, Bn, T, D), R.mask(p, seed, stream, R.ATTN_OUT, Bn, T, D).reshape(Bn, T, D))
    return (R.mask(p, seed, stream, R.FF_HIDDEN, Bn, T, D, hidden).reshape(Bn, T, hidden),
            R.mask(p, seed, stream, R.FF_OUT, Bn, T, D).reshape(Bn, T, D))


def trunk_forward_drop(leaf, x, n_layers, p, seed, first_stream):
    """(beat, downbeat) of the trunk and the summing head with the masks of streams first_stream .. first_stream + 2 L - 1: the
    attention of layer l takes stream first_stream + 2 l, its feed-forward first_stream + 2 l + 1"""
    Bn, T, D = x.shape
    dtype, c = x.dtype, 1.0 / (1.0 - p)
    for l in range(n_layers):
        pfx = f"transformer_blocks.layers.{l}."
        hidden = leaf[pfx + "1.net.1.weight"].shape[0]
        ma = [torch.from_numpy(t).to(dtype) for t in unit_masks("attn", p, seed, first_stream + 2 * l, Bn, T, D, hidden)]
        mf = [torch.from_numpy(t).to(dtype) for t in unit_masks("ff", p, seed, first_stream + 2 * l + 1, Bn, T, D, hidden)]
        x = attention_drop(x, leaf, pfx + "0.", D // 32, *ma, c) + x
        x = feedforward_drop(x, leaf, pfx + "1.", *mf, c) + x
    return U.head_outputs(O.rmsnorm(x, leaf["transformer_blocks.norm.gamma"]), leaf, True)


# ---- the schedule -----------------------------------------------------------------------------------------------------------------
def lr_factor(s, warmup, total):
    """DESIGN.md section 14 (pl_module.py:342-369 without the final re-raise): the factor on the base rate of the optimiser
    step taken after ``s`` earlier ones.  0 for the first step."""
    return 0.5 * (1.0 + math.cos(math.pi * s / total)) * (s / warmup if s <= warmup else 1.0)


# ---- the loop ---------------------------------------------------------------------------------------------------------------------
def run(sd, batches, dtype, *, n_layers, lr, weight_decay, warmup, total_steps, accumulate, max_grad_norm, pos_weights, epochs,
        batches_per_epoch, tol=3, dropout=None, first_forward=0, mutant=None):
    """Train the trunk and the heads of ``sd`` over ``batches`` (epoch after epoch, ``batches_per_epoch`` each; every batch a dict
    of CPU tensors: ``h`` = the frontend's output, ``truth_beat``, ``truth_downbeat``, ``padding_mask`` (B, T) and
    ``downbeat_mask`` (B,)) in ``dtype``.

    Every batch: forward, the two losses, backward into the summed gradients.  Every ``accumulate`` batches, and for what is left
    at an epoch's end, one step: the sum is divided by the group's own count; the global L2 norm over all trainable tensors is
    taken in fp64 and, with ``max_grad_norm``, the gradients are multiplied by coef = min(1, max_norm / (norm + 1e-6));
    ``torch.optim.AdamW(foreach=False)`` at torch's betas and eps, weight decay on the tensors with two or more dimensions only,
    at the rate lr * lr_factor(steps taken so far).  ``dropout``: (p, seed) -- training forward number n (``first_forward`` for
    the first one here) draws the masks of streams 2 L n .. 2 L n + 2 L - 1.

    -> {"steps": [{"norm", "coef", "lr", "count"}], "losses": [(beat, downbeat, total)] per batch as floats, "epochs":
    [{"params", "exp_avg", "exp_avg_sq"}] = dicts by state-dict key at each epoch's end}"""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError(f"unknown mutant {mutant!r}")
    if len(batches) != epochs * batches_per_epoch:
        raise ValueError(f"{len(batches)} batches for {epochs} epochs of {batches_per_epoch}")
    keys = U.trainable_keys(sd)
    leaf = {}
    for k, v in sd.items():
        if k in keys:
            leaf[k] = v.detach().cpu().to(dtype).clone().requires_grad_(True)
        elif k.startswith("transformer_blocks."):   # (the rotary tables: fixed, and kept in their own dtype)
            leaf[k] = v.detach().cpu()
    decayed, plain = [k for k in keys if leaf[k].ndim >= 2], [k for k in keys if leaf[k].ndim <= 1]
    opt = torch.optim.AdamW([{"params": [leaf[k] for k in decayed], "weight_decay": weight_decay},
                             {"params": [leaf[k] for k in plain], "weight_decay": weight_decay if mutant == "decay_all" else 0.0}],
                            lr=lr, foreach=False)
    pw = {"beat": 1.0, "downbeat": 1.0} if mutant == "pos_weight_1" else pos_weights
    out = {"steps": [], "losses": [], "epochs": []}
    forward = first_forward

    def step(count):
        s = len(out["steps"])
        scale = 1.0 / (accumulate if mutant == "remainder_by_accumulate" else count)
        for k in keys:
            leaf[k].grad.mul_(scale)
        norm = math.sqrt(sum(float(leaf[k].grad.double().pow(2).sum()) for k in keys))
        coef = 1.0
        if max_grad_norm is not None and mutant != "no_clip":
            coef = min(1.0, max_grad_norm / (norm + 1e-6))
            for k in keys:
                leaf[k].grad.mul_(coef)
        rate = lr * lr_factor(s + 1 if mutant == "schedule_shift" else s, warmup, total_steps)
        for group in opt.param_groups:
            group["lr"] = rate
        opt.step()
        opt.zero_grad(set_to_none=False)
        out["steps"].append({"norm": norm, "coef": coef, "lr": rate, "count": count})

    for k in keys:
        leaf[k].grad = torch.zeros_like(leaf[k])
    for epoch in range(epochs):
        pending = 0
        for batch in batches[epoch * batches_per_epoch:(epoch + 1) * batches_per_epoch]:
            h = batch["h"].detach().cpu().to(dtype)
            if dropout is None:
                beat, down = U.oracle_trunk_forward(leaf, h, n_layers)
            else:
                beat, down = trunk_forward_drop(leaf, h, n_layers, dropout[0], dropout[1], 2 * n_layers * forward)
            forward += 1
            lb, ld, total = batch_losses(beat, down, batch, dtype, pw, tol, use_downbeat_mask=mutant != "ignore_downbeat_mask")
            total.backward()
            out["losses"].append(tuple(float(v.detach()) for v in (lb, ld, total)))
            pending += 1
            if pending == accumulate:
                step(pending)
                pending = 0
        if pending:
            step(pending)
        state = opt.state
        out["epochs"].append({"params": {k: leaf[k].detach().clone() for k in keys},
                              "exp_avg": {k: state[leaf[k]]["exp_avg"].clone() for k in keys},
                              "exp_avg_sq": {k: state[leaf[k]]["exp_avg_sq"].clone() for k in keys}})
    return out


def displacement(params, sd):
    """p - p_initial in fp64, by key"""
    return {k: v.detach().double().cpu() - sd[k].detach().double().cpu() for k, v in params.items()}
