"""Gradients through tests/route_reference.py on the CPU, the yardsticks the training route's tests gate on, and the fine-tuning
loop restated in plain torch.

The yardstick (DESIGN.md sections 11 to 21): truth is fp64 autograd on the CPU; the reference's own precision is the same
computation in fp32.  For one case ``e_ref`` is the LARGEST, over all gradient tensors, of |g32 - g64| / |g64|; a device gradient
passes when |g_dev - g64| / |g64| <= 10 e_ref (``GATE``) for every tensor.  The decade covers other summation orders over up to
thousands of rows, the device's own exp2 / erf and recomputed activations; a wrong or missing term is at least four decades above
it (the test_the_yardstick_discriminates tests).  Running buffers moved by a batch-statistics forward are judged by the same rule
against the fp64 update, with a floor of 1e-7 on e_ref; ``num_batches_tracked`` exactly.  For 16-mixed the yardstick is
``e_ref16``: the worst gradient tensor's relative distance from the fp64 truth of the oracle run in fp32 under
``torch.autocast("cpu", dtype=torch.float16)`` with the loss multiplied by the loss scale and the result divided by it, which is
what the reference's 16-mixed run computes.

Every ``*_grads`` function goes through ``_run`` and returns one flat dict: the gradients under "x" and their state dict keys
(``grad_keys``), the outputs under "y" (or "beat" / "downbeat") and, with ``batch``, the running buffers after the call under
"stats".  ``on``: route_reference.py's (None = the oracle).  The frontend's functions take and return activations in the device's
(b, t, f, c).
"""
import contextlib
import math

import torch
import torch.nn.functional as F

import route_reference as REF
from oracle import beat_this_oracle as O

GATE = 10.0
STAT_FLOOR = 1e-7
SCALE = 65536.0
FIELDS = dict(attn=("norm.gamma", "to_qkv.weight", "to_gates.weight", "to_gates.bias", "to_out.0.weight"),
              ff=("net.0.gamma", "net.1.weight", "net.1.bias", "net.4.weight", "net.4.bias"))
STAT_LEAVES = ("running_mean", "running_var", "num_batches_tracked")
BN_PREFIXES = ("frontend.stem.bn1d.", "frontend.stem.bn2d.", "frontend.blocks.0.norm.", "frontend.blocks.1.norm.",
               "frontend.blocks.2.norm.")


def rel(a, b):
    """|a - b| / |b| in fp64"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


# ---- which tensors ----------------------------------------------------------------------------------------------------------------
def trainable_keys(sd, prefixes=("transformer_blocks.", "task_heads.")):
    return [k for k in sd if k.startswith(prefixes) and not k.endswith("rotary_embed.freqs")]


def frontend_keys(sd, prefix="frontend."):
    """the trainable keys below ``prefix``: weights, no rotary tables, no running statistics"""
    return [k for k, v in sd.items() if k.startswith(prefix) and v.is_floating_point() and not k.endswith("rotary_embed.freqs")
            and not k.endswith(STAT_LEAVES)]


def all_keys(sd):
    return frontend_keys(sd) + trainable_keys(sd)


def conv_keys(i):
    p = f"frontend.blocks.{i}."
    return [p + "conv2d.weight", p + "norm.weight", p + "norm.bias"]


def leaf_keys(i, leaf):
    p = f"frontend.blocks.{i}.partial.{leaf}."
    return [p + n for n in FIELDS["attn" if leaf.startswith("attn") else "ff"]]


def grad_keys(d):
    """the gradients of a ``*_grads`` result"""
    return [k for k in d if k not in ("y", "beat", "downbeat", "stats")]


# ---- one differentiation ----------------------------------------------------------------------------------------------------------
def _leaves(sd, x, dtype):
    leaf = {}
    for k, v in sd.items():
        v = v.detach().cpu()
        if k.endswith("rotary_embed.freqs") or not v.is_floating_point():
            leaf[k] = v
        else:
            leaf[k] = v.to(dtype).clone().requires_grad_(True)
    return leaf, x.detach().cpu().to(dtype).clone().requires_grad_(True)


def _collect(leaf, xl, keys):
    out = {"x": xl.grad.detach().clone()}
    for k in keys:
        if leaf[k].grad is not None:
            out[k] = leaf[k].grad.detach().clone()
    return out


def _run(sd, x, keys, dtype, forward, scale=1.0, autocast=False, batch=False):
    """forward(leaf, xl) -> (outputs, loss).  -> {"x", <key>: gradient of loss (taken of loss * scale and divided by scale),
    <output name>: value, and with ``batch`` "stats": the running buffers a batch-statistics forward moved}.  ``autocast``: under
    CPU fp16 autocast; ``batch``: True, or another stand-in than ``REF.training_batchnorm`` (the discrimination tests)"""
    leaf, xl = _leaves(sd, x, dtype)
    stats = {}
    batchnorm = REF.training_batchnorm if batch is True else batch
    with (REF.swapped(batchnorm(stats)) if batch else contextlib.nullcontext()):
        with torch.autocast("cpu", dtype=torch.float16, enabled=autocast):
            outs, loss = forward(leaf, xl)
            (loss * scale).backward()
    res = {k: v / scale for k, v in _collect(leaf, xl, keys).items()}
    res.update({k: v.detach() for k, v in outs.items()})
    if batch:
        res["stats"] = stats
    return res


def grads_only(res):
    return {k: res[k] for k in grad_keys(res)}


def nested(res):
    """a result with its gradients under "grads": the form ``check_batch`` and the batch-statistics tests read"""
    out = {k: v for k, v in res.items() if k not in grad_keys(res)}
    out["grads"] = grads_only(res)
    return out


def weighted_sum(g_b, g_d, dtype):
    """the loss sum(beat g_b) + sum(downbeat g_d)"""
    cast = lambda t: t.detach().cpu().to(dtype)
    return lambda beat, down: (beat * cast(g_b)).sum() + (down * cast(g_d)).sum()


# ---- the trunk --------------------------------------------------------------------------------------------------------------------
def oracle_unit_grads(kind, sd, prefix, x, g, dtype, heads=None, sum_head=True):
    """Gradients of sum(unit(x) * g) through the oracle.  kind: "attn" / "ff" (the branch without the residual; prefix =
    "transformer_blocks.layers.<l>.<0|1>."), "norm", "head" (g = (g_beat or None, g_downbeat or None)).  Gradients only."""
    assert heads in (None, x.shape[-1] // 32)
    cast = lambda t: t.detach().cpu().to(dtype)

    def forward(leaf, xl):
        if kind in ("attn", "ff"):
            return {}, (REF.unit(kind, xl, leaf, prefix) * cast(g)).sum()
        if kind == "norm":
            return {}, (O.rmsnorm(xl, leaf["transformer_blocks.norm.gamma"]) * cast(g)).sum()
        beat, down = REF.head_outputs(xl, leaf, sum_head)
        return {}, sum((o * cast(w)).sum() for o, w in ((beat, g[0]), (down, g[1])) if w is not None)
    keys = [k for k in trainable_keys(sd) if k.startswith(prefix)] if kind in ("attn", "ff") else trainable_keys(sd)
    return _run(sd, x, keys, dtype, forward)


def unit_grads(kind, sd, pfx, x, g, dtype, on, scale=1.0, masks=None, p=0.0, autocast=False):
    """one unit of the trunk: {"y", "x", <state dict key>}; ``masks``: REF.unit_masks' at rate ``p``"""
    def forward(leaf, xl):
        m = None if masks is None else REF.masks_as(masks, xl.dtype)
        y = REF.unit(kind, xl, leaf, pfx, on, m, 1.0 / (1.0 - p) if masks is not None else 1.0)
        return {"y": y}, (y.to(dtype) * g.to(dtype)).sum()
    return _run(sd, x, [pfx + n for n in FIELDS[kind]], dtype, forward, scale, autocast)


def trunk_grads(sd, x, dtype, n_layers, loss_fn, on, scale=1.0, autocast=False, sum_head=True):
    """the whole trunk and the heads with a loss: {"beat", "downbeat", "x", <state dict key>}"""
    def forward(leaf, xl):
        beat, down = REF.trunk(leaf, xl, n_layers, on, sum_head=sum_head)
        return {"beat": beat, "downbeat": down}, loss_fn(beat.to(dtype), down.to(dtype))
    return _run(sd, x, trainable_keys(sd), dtype, forward, scale, autocast)


def oracle_trunk_grads(sd, x, g_b, g_d, dtype, n_layers, sum_head=True, loss_fn=None):
    """Gradients of sum(beat g_b) + sum(downbeat g_d) -- or of loss_fn(beat, downbeat) -- through transformer_blocks and
    task_heads of the oracle.  Gradients only."""
    return grads_only(trunk_grads(sd, x, dtype, n_layers, loss_fn or weighted_sum(g_b, g_d, dtype), None, sum_head=sum_head))


# ---- the frontend and the whole model -----------------------------------------------------------------------------------------------
def _to_device(y):   # (b, c, f, t) -> (b, t, f, c)
    return y.permute(0, 3, 2, 1)


def stem_grads(sd, x, g, dtype, batch=False):
    """x (B, T, 128), g (B, T, 32, 32)"""
    def forward(leaf, xl):
        y = O.stem(xl, leaf)
        return {"y": _to_device(y)}, (y * REF.to_oracle(g.to(dtype))).sum()
    return _run(sd, x, frontend_keys(sd, "frontend.stem."), dtype, forward, batch=batch)


def conv_grads(sd, i, x, g, dtype, on=None, scale=1.0, autocast=False, batch=False):
    """conv unit i: x (B, T, F, C), g (B, T, F / 2, 2 C)"""
    def forward(leaf, xl):
        y = REF.conv_unit(REF.to_oracle(xl), leaf, f"frontend.blocks.{i}.", on).to(dtype)
        return {"y": _to_device(y)}, (y * REF.to_oracle(g.to(dtype))).sum()
    return _run(sd, x, conv_keys(i), dtype, forward, scale, autocast, batch)


def partial_grads(sd, i, x, g, dtype, on=None, scale=1.0, autocast=False, drops=None):
    """partial transformer i: x, g (B, T, F, C); ``drops`` = {leaf: None or (p, seed, stream)}"""
    def forward(leaf, xl):
        y = REF.partial_ft(REF.to_oracle(xl), leaf, i, drops, on).to(dtype)
        return {"y": _to_device(y)}, (y * REF.to_oracle(g.to(dtype))).sum()
    return _run(sd, x, frontend_keys(sd, f"frontend.blocks.{i}.partial."), dtype, forward, scale, autocast)


def leaf_grads(sd, i, leaf, x, g, dtype, drop, on=None, scale=1.0, autocast=False):
    """one leaf of block i as the unit call with its residual runs it: x, g (B', T', C) are the call's own rows, ``drop`` = None
    or (p, seed, stream) with the masks over that (B', T', C) -> {"y" = x + f(x), "x", <state dict key>}"""
    pfx = f"frontend.blocks.{i}.partial."
    hidden = sd[pfx + "ffF.net.1.weight"].shape[0]

    def forward(lf, xl):
        y = (xl + REF.dropped_unit(leaf[:-1], xl, lf, pfx + leaf + ".", on, drop, hidden)).to(dtype)
        return {"y": y}, (y * g.to(dtype)).sum()
    return _run(sd, x, leaf_keys(i, leaf), dtype, forward, scale, autocast)


def linear_grads(sd, x, g, dtype, on=None, scale=1.0, autocast=False):
    """concat + frontend.linear: x (B, T, F, C), g (B, T, D)"""
    def forward(leaf, xl):
        y = REF.projection(REF.to_oracle(xl), leaf, on).to(dtype)
        return {"y": y}, (y * g.to(dtype)).sum()
    return _run(sd, x, ["frontend.linear.weight", "frontend.linear.bias"], dtype, forward, scale, autocast)


def frontend_grads(sd, x, g, dtype, plan_=None, on=None, batch=False):
    """gradients of sum(frontend(x) g) in x (B, T, 128) and every trainable frontend key; g (B, T, D)"""
    def forward(leaf, xl):
        y = REF.frontend(xl, leaf, plan_, on).to(dtype)
        return {"y": y}, (y * g.to(dtype)).sum()
    return _run(sd, x, frontend_keys(sd), dtype, forward, batch=batch)


def model_grads(sd, x, loss_fn, dtype, on=None, scale=1.0, autocast=False, plan_=None, trunk_drop=None, batch=False, sum_head=True):
    """the whole model with a loss: {"beat", "downbeat", "x", <state dict key>}; the frontend under ``plan_``, the trunk under
    ``trunk_drop`` (REF.model_plan's)"""
    def forward(leaf, xl):
        trunk_drop_ = trunk_drop if trunk_drop is not None and trunk_drop[0] > 0 else None
        beat, down = REF.trunk(leaf, REF.frontend(xl, leaf, plan_, on), REF.n_layers_of(sd), on, trunk_drop_, sum_head)
        beat, down = beat.to(dtype), down.to(dtype)
        return {"beat": beat, "downbeat": down}, loss_fn(beat, down)
    return _run(sd, x, all_keys(sd), dtype, forward, scale, autocast, batch)


def batch_statistics(grads_fn):
    """``grads_fn`` under batch statistics, ``nested``; ``batchnorm(stats)``: another stand-in than torch's"""
    def run(*args, batchnorm=None, **kw):
        return nested(grads_fn(*args, batch=batchnorm or True, **kw))
    return run


bn_stem, bn_conv, bn_frontend, bn_model = (batch_statistics(f) for f in (stem_grads, conv_grads, frontend_grads, model_grads))


# ---- the yardsticks -----------------------------------------------------------------------------------------------------------------
def yardstick(g32, g64):
    """e_ref of a case: the worst tensor of the fp32 oracle against the fp64 one, over every tensor of ``g64``"""
    return max(rel(g32[k], g64[k]) for k in g64)


def worst(got, truth, keys=None):
    """(largest relative distance over the gradient tensors, its key)"""
    errs = {k: rel(got[k], truth[k]) for k in (keys or grad_keys(truth)) if k in got}
    k = max(errs, key=errs.get)
    return errs[k], k


def check(name, dev, g32, g64, report=None):
    """Every device tensor within GATE * e_ref of the fp64 truth, over every tensor of ``g64`` (hand it ``grads_only`` of a result
    to leave the outputs out); returns (e_ref, worst ratio).  Prints the figures first."""
    e_ref = yardstick(g32, g64)
    errs = {k: rel(dev[k], g64[k]) for k in g64 if k in dev}
    worst_key = max(errs, key=errs.get)
    worst_ratio = errs[worst_key] / e_ref
    print(f"{name}: e_ref = {e_ref:.3e}, worst device error = {errs[worst_key]:.3e} ({worst_ratio:.2f} x e_ref, {worst_key})")
    if report is not None:
        report(name, e_ref=e_ref, worst_ratio=worst_ratio, worst_tensor=worst_key)
    missing = [k for k in g64 if k not in dev]
    assert not missing, f"{name}: no device gradient for {missing}"
    for k, e in errs.items():
        assert torch.isfinite(dev[k]).all(), f"{name}: {k} is not finite"
        assert e <= GATE * e_ref, f"{name}: {k} is {e:.3e} from the fp64 truth, the gate is 10 x e_ref = {GATE * e_ref:.3e}"
    return e_ref, worst_ratio


def check_batch(name, dev_grads, dev_stats, r32, r64, report=None):
    """``nested`` results: the gradients through ``check``; every moved running buffer within GATE x max(e_ref, 1e-7) of the fp64
    update, e_ref that buffer's fp32 error; the counters exactly.  Prints each figure before it asserts; -> (e_ref, worst gradient
    ratio, worst buffer ratio)."""
    e_ref, worst_ratio = check(name, dev_grads, r32["grads"], r64["grads"], report)
    worst_stat = 0.0
    for k, want in r64["stats"].items():
        assert k in dev_stats, f"{name}: no device value for {k}"
        if k.endswith("num_batches_tracked"):
            assert int(dev_stats[k]) == int(want), f"{name}: {k} is {int(dev_stats[k])}, expected {int(want)}"
            continue
        e = max(rel(r32["stats"][k], want), STAT_FLOOR)
        err = rel(dev_stats[k], want)
        worst_stat = max(worst_stat, err / e)
        print(f"{name}: {k} e_ref = {e:.3e}, device error = {err:.3e} ({err / e:.2f} x)")
        assert torch.isfinite(dev_stats[k]).all() and err <= GATE * e, f"{name}: {k} is {err:.3e} from the fp64 update, gate {GATE * e:.3e}"
    if report is not None:
        report(name + " running statistics", worst_ratio=worst_stat)
    return e_ref, worst_ratio, worst_stat


def mixed_yardstick(run, start=SCALE):
    """run(dtype, scale, autocast) -> a ``*_grads`` result.  -> (truth fp64, the autocast oracle, scale, e_ref16): the loss scale
    is the largest power of two <= ``start`` at which every gradient of the autocast oracle is finite (where a GradScaler settles;
    at 65536 the autocast oracle's frontend gradients overflow and the gate would say nothing), e_ref16 its worst gradient
    tensor's relative distance from the truth"""
    truth = run(torch.float64, 1.0, False)
    keys = grad_keys(truth)
    scale = start
    while True:
        auto = run(torch.float32, scale, True)
        if all(bool(torch.isfinite(auto[k]).all()) for k in keys) or scale <= 1.0:
            break
        scale /= 2.0
    return truth, auto, scale, worst(auto, truth, keys)[0]


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


def trunk_loss(beat_t, down_t, mask):
    def loss(beat, down):
        dt = beat.dtype
        return shift_tolerant_bce(beat, beat_t.to(dt), mask.to(dt)) + shift_tolerant_bce(down, down_t.to(dt), mask.to(dt))
    return loss


# ---- the fine-tuning loop: what ``beat_this_amd.train.fit`` has to compute over a list of recorded batches, written from DESIGN.md
# sections 11, 14 and 15 and the reference's training module (beat_this/model/pl_module.py:100-105 the masks, :279-306 the
# optimiser and its two groups, :342-369 the schedule) without anything of beat_this_amd.optim, .train, .loss or .model.pl_module.
# In fp64 it is the truth of the trajectory tests (tests/test_finetune_reference.py, tests/test_gpu_finetune_trajectory.py), in
# fp32 their e_ref; ``mutant=`` switches on one deviation at a time, to show that the yardstick tells them apart. ---------------
MUTANTS = ("decay_all", "remainder_by_accumulate", "schedule_shift", "ignore_downbeat_mask", "pos_weight_1", "no_clip")


def lr_factor(s, warmup, total):
    """DESIGN.md section 14 (pl_module.py:342-369 without the final re-raise): the factor on the base rate of the optimiser
    step taken after ``s`` earlier ones.  0 for the first step."""
    return 0.5 * (1.0 + math.cos(math.pi * s / total)) * (s / warmup if s <= warmup else 1.0)


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
    keys = trainable_keys(sd)
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
            drop = None if dropout is None else (dropout[0], dropout[1], 2 * n_layers * forward)
            beat, down = REF.trunk(leaf, h, n_layers, drop=drop)
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
