"""Frontend dropout (the dropout section of include/beat_this_amd.h) restated in torch on the CPU, in any
float dtype: the oracle's frontend with the masks of the host twin's contract applied to the twelve attention / feed-forward
leaves of the three partial transformers.  Built from ``finetune_reference.attention_drop`` / ``feedforward_drop`` /
``unit_masks`` and the oracle's stem, conv units and projection, which never drop.

Row orders: a frequency-direction leaf (attnF, ffF) is a unit call on (B T, F, C) -- row (b T + t) F + f -- and a time-direction
leaf (attnT, ffT) one on (B F, T, C) -- row (b F + f) T + t.  Streams: a ``plan`` maps (block, leaf) to None or (p, seed, stream);
``plan(p, seed, first)`` numbers the leaves in forward order, block 0 attnF, ffF, attnT, ffT = first .. first + 3, block 1 from
first + 4, block 2 from first + 8; the trunk's units follow (``finetune_reference.trunk_forward_drop``).  A leaf whose entry is None
is the oracle's own call, so with every rate 0 the helper IS ``O.frontend``.

``on``: None = the oracle's arithmetic (run it under ``torch.autocast("cpu", dtype=torch.float16)`` for the reference's own
16-mixed error, the way front_mixed_reference.py and mixed_reference.py build theirs), True / False = mixed_reference.py's
restatement of the 16-mixed contract with / without its rounding.  Activations are the oracle's (b, c, f, t) inside; the
``*_grads`` functions take and return the device's (b, t, f, c).
"""
import contextlib

import torch

import bn_grad_util as BU
import front_grad_util as FU
import front_mixed_reference as FM
import mixed_reference as R
import trunk_grad_util as U
from finetune_reference import attention_drop, feedforward_drop, unit_masks
from oracle import beat_this_oracle as O

LEAVES = ("attnF", "ffF", "attnT", "ffT")
BLOCK_SHAPES = ((32, 32), (16, 64), (8, 128))          # (F, C) at the input of block i


def leaf_shape(i, leaf, B, T):
    """(B', T', C) of a leaf call of block i on a (B, T) batch"""
    F_, C_ = BLOCK_SHAPES[i]
    return (B * T, F_, C_) if leaf.endswith("F") else (B * F_, T, C_)


def plan(p, seed, first=0, blocks=(0, 1, 2)):
    """{(block, leaf): (p, seed, stream) or None}: the streams of one frontend forward, in call order; rate 0 takes no number"""
    out, stream = {}, first
    for i in blocks:
        for leaf in LEAVES:
            out[i, leaf] = (p, seed, stream) if p > 0 else None
            stream += int(p > 0)
    return out


def leaf_masks(i, leaf, drop, B, T, hidden):
    """the two masks of a leaf call as ``unit_masks`` shapes them: over (B', T', C) of the contract"""
    Bp, Tp, C_ = leaf_shape(i, leaf, B, T)
    return unit_masks("attn" if leaf.startswith("attn") else "ff", drop[0], drop[1], drop[2], Bp, Tp, C_, hidden)


def _leaf(y, sd, pfx, i, leaf, drop, B, T, on):
    """the branch of one leaf on its (B', T', C) rows, without the residual"""
    heads, p = y.shape[2] // 32, pfx + leaf + "."
    attn = leaf.startswith("attn")
    if drop is None:
        if on is None:
            return O.attention(y, sd, p, heads) if attn else O.feedforward(y, sd, p)
        return R.attention(y, sd, p, heads, on) if attn else R.feedforward(y, sd, p, on)
    hidden = sd[pfx + "ffF.net.1.weight"].shape[0]
    m0, m1 = (torch.from_numpy(m).to(y.dtype) for m in leaf_masks(i, leaf, drop, B, T, hidden))
    c = 1.0 / (1.0 - drop[0])
    if on is None:
        return attention_drop(y, sd, p, heads, m0, m1, c) if attn else feedforward_drop(y, sd, p, m0, m1, c)
    return R.attention(y, sd, p, heads, on, m0, m1, c) if attn else R.feedforward(y, sd, p, on, m0, m1, c)


def partial_ft(x, sd, i, drops, on=None):
    """O.partial_ft of block i on (b, c, f, t) with ``drops`` = {leaf: None or (p, seed, stream)}"""
    pfx = f"frontend.blocks.{i}.partial."
    b, c, f, t = x.shape
    y = x.permute(0, 3, 2, 1).reshape(b * t, f, c)                              # (b t) f c
    y = y + _leaf(y, sd, pfx, i, "attnF", drops.get("attnF"), b, t, on)
    y = y + _leaf(y, sd, pfx, i, "ffF", drops.get("ffF"), b, t, on)
    y = y.view(b, t, f, c).permute(0, 2, 1, 3).reshape(b * f, t, c)             # (b f) t c
    y = y + _leaf(y, sd, pfx, i, "attnT", drops.get("attnT"), b, t, on)
    y = y + _leaf(y, sd, pfx, i, "ffT", drops.get("ffT"), b, t, on)
    return y.view(b, f, t, c).permute(0, 3, 1, 2)                               # b c f t


def frontend(x, sd, plan_, on=None):
    """O.frontend with the leaves of ``plan_`` dropped: (B, T, 128) -> (B, T, D)"""
    h = O.stem(x, sd)
    for i in range(3):
        p = f"frontend.blocks.{i}."
        if p + "partial.attnF.norm.gamma" in sd:
            h = partial_ft(h, sd, i, {leaf: plan_.get((i, leaf)) for leaf in LEAVES}, on)
        h = FM.conv_unit(h, sd, p, on)
    return FM.projection(h, sd, on)


def _trunk(leaf, h, n_layers, drop, on):
    """(beat, downbeat); ``drop`` = None or (p, seed, first stream of the trunk)"""
    if drop is None or not drop[0] > 0:
        return U.oracle_trunk_forward(leaf, h, n_layers) if on is None else R.trunk_forward(leaf, h, n_layers, on)
    Bn, T, D = h.shape
    p, seed, first = drop
    c = 1.0 / (1.0 - p)
    x = h
    for l in range(n_layers):
        pfx = f"transformer_blocks.layers.{l}."
        hidden = leaf[pfx + "1.net.1.weight"].shape[0]
        ma = [torch.from_numpy(t).to(h.dtype) for t in unit_masks("attn", p, seed, first + 2 * l, Bn, T, D, hidden)]
        mf = [torch.from_numpy(t).to(h.dtype) for t in unit_masks("ff", p, seed, first + 2 * l + 1, Bn, T, D, hidden)]
        if on is None:
            x = attention_drop(x, leaf, pfx + "0.", D // 32, *ma, c) + x
            x = feedforward_drop(x, leaf, pfx + "1.", *mf, c) + x
        else:
            x = R.attention(x, leaf, pfx + "0.", D // 32, on, *ma, c) + x
            x = R.feedforward(x, leaf, pfx + "1.", on, *mf, c) + x
    return U.head_outputs(O.rmsnorm(x, leaf["transformer_blocks.norm.gamma"]), leaf, True)


def model(x, sd, plan_, trunk_drop, on=None):
    """(beat, downbeat), summing head: the frontend under ``plan_``, the trunk under ``trunk_drop``"""
    n_layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("transformer_blocks.layers."))
    return _trunk(sd, frontend(x, sd, plan_, on), n_layers, trunk_drop, on)


def model_plan(sd, p_front, p_trunk, seed, first=0):
    """(plan, trunk_drop, streams used) of one whole-model forward from counter ``first``: the leaves first, then the trunk"""
    blocks = tuple(i for i in range(3) if f"frontend.blocks.{i}.partial.attnF.norm.gamma" in sd)
    pl = plan(p_front, seed, first, blocks)
    used = 4 * len(blocks) * int(p_front > 0)
    n_layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("transformer_blocks.layers."))
    trunk = (p_trunk, seed, first + used) if p_trunk > 0 else None
    return pl, trunk, used + 2 * n_layers * int(p_trunk > 0)


# ---- gradients --------------------------------------------------------------------------------------------------------------------
def _run(sd, x, keys, dtype, forward, scale=1.0, autocast=False, batch=False):
    """forward(leaf, xl) -> (outputs, loss) -> {"x", <key>: gradient of loss (taken of loss * scale and divided by it), <output
    name>: value, "stats": the running buffers a batch-statistics forward moved}"""
    leaf, xl = U._leaves(sd, x, dtype)
    stats = {}
    with (BU.swapped(FM.training_batchnorm(stats)) if batch else contextlib.nullcontext()):
        with torch.autocast("cpu", dtype=torch.float16, enabled=autocast):
            outs, loss = forward(leaf, xl)
            (loss * scale).backward()
    res = {k: v / scale for k, v in U._collect(leaf, xl, keys).items()}
    res.update({k: v.detach() for k, v in outs.items()})
    res["stats"] = stats
    return res


def leaf_keys(i, leaf):
    p = f"frontend.blocks.{i}.partial.{leaf}."
    return [p + n for n in R.FIELDS["attn" if leaf.startswith("attn") else "ff"]]


def leaf_grads(sd, i, leaf, x, g, dtype, drop, on=None, scale=1.0, autocast=False):
    """one leaf of block i as the unit call with its residual runs it: x, g (B', T', C) are the call's own rows, ``drop`` = None
    or (p, seed, stream) with the masks over that (B', T', C) -> {"y" = x + f(x), "x", <state dict key>}"""
    pfx = f"frontend.blocks.{i}.partial."
    hidden = sd[pfx + "ffF.net.1.weight"].shape[0]
    Bp, Tp, C_ = x.shape

    def forward(lf, xl):
        if drop is None:
            f = _leaf(xl, lf, pfx, i, leaf, None, 0, 0, on)
        else:
            m0, m1 = (torch.from_numpy(m).to(dtype) for m in
                      unit_masks("attn" if leaf.startswith("attn") else "ff", drop[0], drop[1], drop[2], Bp, Tp, C_, hidden))
            c, p, heads = 1.0 / (1.0 - drop[0]), pfx + leaf + ".", C_ // 32
            if leaf.startswith("attn"):
                f = attention_drop(xl, lf, p, heads, m0, m1, c) if on is None else R.attention(xl, lf, p, heads, on, m0, m1, c)
            else:
                f = feedforward_drop(xl, lf, p, m0, m1, c) if on is None else R.feedforward(xl, lf, p, on, m0, m1, c)
        y = (xl + f).to(dtype)
        return {"y": y}, (y * g.to(dtype)).sum()
    return _run(sd, x, leaf_keys(i, leaf), dtype, forward, scale, autocast)


def partial_grads(sd, i, x, g, dtype, drops, on=None, scale=1.0, autocast=False):
    """partial transformer i: x, g (B, T, F, C) in (b, t, f, c); ``drops`` = {leaf: None or (p, seed, stream)}"""
    p = f"frontend.blocks.{i}.partial."

    def forward(leaf, xl):
        y = partial_ft(FU.to_oracle(xl), leaf, i, drops, on).to(dtype)
        return {"y": y.permute(0, 3, 2, 1)}, (y * FU.to_oracle(g.to(dtype))).sum()
    return _run(sd, x, FU.frontend_keys(sd, p), dtype, forward, scale, autocast)


def frontend_grads(sd, x, g, dtype, plan_, on=None):
    """gradients of sum(frontend(x) g) in x and every trainable frontend key"""
    def forward(leaf, xl):
        y = frontend(xl, leaf, plan_, on).to(dtype)
        return {"y": y}, (y * g.to(dtype)).sum()
    return _run(sd, x, FU.frontend_keys(sd), dtype, forward)


def model_grads(sd, x, loss_fn, dtype, plan_, trunk_drop, on=None, scale=1.0, autocast=False, batch=False):
    """the whole model with a loss: {"beat", "downbeat", "x", <state dict key>, "stats"}"""
    def forward(leaf, xl):
        beat, down = model(xl, leaf, plan_, trunk_drop, on)
        beat, down = beat.to(dtype), down.to(dtype)
        return {"beat": beat, "downbeat": down}, loss_fn(beat, down)
    return _run(sd, x, FU.all_keys(sd), dtype, forward, scale, autocast, batch)


def grad_keys(d):
    return [k for k in d if k not in ("y", "beat", "downbeat", "stats")]


def mixed_yardstick(run, start=R.SCALE):
    """run(dtype, scale, autocast) -> a ``*_grads`` result.  -> (truth fp64, the autocast oracle, scale, e_ref16): the loss scale
    is the largest power of two <= ``start`` at which every gradient of the autocast oracle is finite (front_mixed_reference.py's
    rule), e_ref16 its worst gradient tensor's relative distance from the truth"""
    truth = run(torch.float64, 1.0, False)
    keys = grad_keys(truth)
    scale = start
    while True:
        auto = run(torch.float32, scale, True)
        if all(bool(torch.isfinite(auto[k]).all()) for k in keys) or scale <= 1.0:
            break
        scale /= 2.0
    return truth, auto, scale, R.worst(auto, truth, keys)[0]
