"""The forward arithmetic of the training route restated in torch on the CPU, in any float dtype: what the device's training
kernels have to compute, from the contracts in include/beat_this_amd.h and DESIGN.md sections 15 (dropout), 16 and 19 (16-mixed),
18 (batch statistics) and 21 (frontend dropout).  tests/route_grads.py differentiates it, tests/route_cases.py holds the cases.

A unit (an attention or feed-forward branch, without its residual) exists in three forms that are separate implementations on
purpose -- the CPU tests hold them against each other:
  * the oracle's own ``O.attention`` / ``O.feedforward``;
  * the masked oracle, ``attention_drop`` / ``feedforward_drop``: the oracle's lines with the dropout masks multiplied in;
  * the 16-mixed restatement, ``attention`` / ``feedforward`` over ``linear``, ``_MatMul``, ``_AttnCore`` (and ``_Conv`` for the
    conv units): BOTH operands of every matrix product rounded to fp16, in the forward and in the hand-written backward, and
    everything else in the working dtype; ``on=False`` switches the rounding off.
``unit`` picks among them, and ``partial_ft``, ``frontend``, ``trunk`` and ``model`` are built on it.  ``on``: None = the
oracle's arithmetic (run it under ``torch.autocast("cpu", dtype=torch.float16)`` for the reference's own 16-mixed error),
True / False = the restatement with / without its rounding.  Where nothing is dropped and ``on`` is None the compositions ARE the
oracle's own (``O.partial_ft``, ``O.frontend``, ``O.transformer``), not a restated loop.

Batch statistics: ``swapped(training_batchnorm(stats))`` puts torch's training-mode BatchNorm in place of ``O.batchnorm`` for the
duration of a call.

Dropout masks: Philox4x32-10 over (group, site, stream) counters under the seed as key, keep iff word >= floor(p 2^32), in numpy.
Row orders in the frontend: a frequency-direction leaf (attnF, ffF) is a unit call on (B T, F, C) -- row (b T + t) F + f -- and a
time-direction leaf (attnT, ffT) one on (B F, T, C) -- row (b F + f) T + t.  Streams: a ``plan`` maps (block, leaf) to None or
(p, seed, stream); ``plan(p, seed, first)`` numbers the leaves in forward order, block 0 attnF, ffF, attnT, ffT = first ..
first + 3, block 1 from first + 4, block 2 from first + 8; the trunk's units follow: the attention of layer l takes stream
first + 2 l, its feed-forward first + 2 l + 1.

The device's activations are (b, t, f, c), the oracle's (b, c, f, t): everything here is in the oracle's layout.
"""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import beat_this_oracle as O

# ---- the dropout masks (test_dropout_rng.py holds them against bt_dropout_mask_host) -------------------------------------------
ATTN_P, ATTN_OUT, FF_HIDDEN, FF_OUT = range(4)
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays of one shape (or scalars), key: two Python ints -> four uint32 arrays"""
    c = [np.asarray(v, dtype=np.uint64) & MASK32 for v in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def threshold(p):
    """floor(p 2^32) in double, p as the fp32 value the library receives"""
    return int(np.floor(float(np.float32(p)) * 4294967296.0))


def _words(groups, site, seed, stream):
    """uint32 [..., 4]: the four words of every group"""
    g = np.asarray(groups, dtype=np.uint64)
    ctr = [g & MASK32, np.uint64(site << 24) | (g >> S32), np.uint64(stream & 0xFFFFFFFF), np.uint64((stream >> 32) & 0xFFFFFFFF)]
    ctr = [np.broadcast_to(v, g.shape) for v in ctr]
    return np.stack(philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)), axis=-1)


def mask(p, seed, stream, site, B, T, dim, hidden=0):
    """uint8, 1 = kept: [B, dim / 32, T, T] (query by key) for ATTN_P, [B T, dim or hidden] for the row sites"""
    thr = threshold(p)
    if site == ATTN_P:
        H, G = dim // 32, (T + 3) // 4
        rows = np.arange(B * H * T, dtype=np.uint64)                      # (b H + h) T + q
        groups = rows[:, None] * np.uint64(G) + np.arange(G, dtype=np.uint64)[None, :]
        w = _words(groups, site, seed, stream).reshape(B * H * T, 4 * G)[:, :T]   # word k mod 4 of group k / 4
        return (w >= thr).astype(np.uint8).reshape(B, H, T, T)
    n = hidden if site == FF_HIDDEN else dim
    groups = np.arange(B * T * n // 4, dtype=np.uint64)                   # row (n / 4) + col / 4
    return (_words(groups, site, seed, stream).reshape(B * T, n) >= thr).astype(np.uint8)


def unit_masks(kind, p, seed, stream, Bn, T, D, hidden):
    """the two masks of one unit call as numpy arrays in the shapes the restatements multiply by"""
    if kind == "attn":
        return (mask(p, seed, stream, ATTN_P, Bn, T, D), mask(p, seed, stream, ATTN_OUT, Bn, T, D).reshape(Bn, T, D))
    return (mask(p, seed, stream, FF_HIDDEN, Bn, T, D, hidden).reshape(Bn, T, hidden),
            mask(p, seed, stream, FF_OUT, Bn, T, D).reshape(Bn, T, D))


def masks_as(masks, dtype):
    """numpy masks -> torch tensors of ``dtype``"""
    return tuple(torch.from_numpy(m).to(dtype) for m in masks)


# ---- the masked oracle ------------------------------------------------------------------------------------------------------------
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


# ---- the 16-mixed restatement ---------------------------------------------------------------------------------------------------
def r16(t, on=True):
    """round to fp16 (to nearest even; beyond its range: inf) and back"""
    return t.to(torch.float16).to(t.dtype) if on else t


class _MatMul(torch.autograd.Function):
    """C = r(A) r(B); dA = r(dC) r(B)^T, dB = r(A)^T r(dC)"""

    @staticmethod
    def forward(ctx, a, b, on):
        ctx.save_for_backward(a, b)
        ctx.on = on
        return r16(a, on) @ r16(b, on)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        gr = r16(g, ctx.on)
        return gr @ r16(b, ctx.on).transpose(-1, -2), r16(a, ctx.on).transpose(-1, -2) @ gr, None


def linear(x, w, b=None, on=True):
    """Y = A W^T (+ b) on the rows of x; dA = dY W and dW = dY^T A round their operands too"""
    y = _MatMul.apply(x.reshape(-1, x.shape[-1]), w.t(), on).view(*x.shape[:-1], w.shape[0])
    return y if b is None else y + b


class _AttnCore(torch.autograd.Function):
    """O = r(P m c) r(V) with P = softmax(r(q) r(k)^T / sqrt(32)), and the two-sweep backward of the device: delta = dO . O,
    dP = m c (r(dO) r(V)^T), dS = P (dP - delta), dV = r(P m c)^T r(dO), dQ = r(dS) r(K) / sqrt(32), dK = r(dS)^T r(Q) / sqrt(32)"""

    @staticmethod
    def forward(ctx, q, k, v, mc, on):
        scale = q.shape[-1] ** -0.5
        p = torch.softmax((r16(q, on) @ r16(k, on).transpose(-1, -2)) * scale, dim=-1)
        pm = p if mc is None else p * mc
        o = r16(pm, on) @ r16(v, on)
        ctx.save_for_backward(q, k, v, p, o, mc)
        ctx.on = on
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, p, o, mc = ctx.saved_tensors
        on, scale = ctx.on, q.shape[-1] ** -0.5
        pm = p if mc is None else p * mc
        dor = r16(do, on)
        delta = (do * o).sum(-1, keepdim=True)
        dp = dor @ r16(v, on).transpose(-1, -2)
        if mc is not None:
            dp = dp * mc
        ds = r16(p * (dp - delta), on)
        dv = r16(pm, on).transpose(-1, -2) @ dor
        return (ds @ r16(k, on)) * scale, (ds.transpose(-1, -2) @ r16(q, on)) * scale, dv, None, None


def attention(x, sd, pfx, heads, on=True, mask_p=None, mask_out=None, c=1.0):
    """oracle.attention under the contract (masks: attention_drop's)"""
    b, n, dim = x.shape
    xn = O.rmsnorm(x, sd[pfx + "norm.gamma"])
    qkv = linear(xn, sd[pfx + "to_qkv.weight"], on=on).view(b, n, 3, heads, 32).permute(2, 0, 3, 1, 4)
    fr = sd[pfx + "rotary_embed.freqs"]
    q, k, v = O.rope(qkv[0], fr), O.rope(qkv[1], fr), qkv[2]
    out = _AttnCore.apply(q, k, v, None if mask_p is None else mask_p * c, on)
    gates = linear(xn, sd[pfx + "to_gates.weight"], sd[pfx + "to_gates.bias"], on=on)
    out = (out * torch.sigmoid(gates).permute(0, 2, 1)[..., None]).permute(0, 2, 1, 3).reshape(b, n, dim)
    y = linear(out, sd[pfx + "to_out.0.weight"], on=on)
    return y if mask_out is None else y * mask_out * c


def feedforward(x, sd, pfx, on=True, mask_hidden=None, mask_out=None, c=1.0):
    h = O.rmsnorm(x, sd[pfx + "net.0.gamma"])
    h = F.gelu(linear(h, sd[pfx + "net.1.weight"], sd[pfx + "net.1.bias"], on=on))
    if mask_hidden is not None:
        h = h * mask_hidden * c
    y = linear(h, sd[pfx + "net.4.weight"], sd[pfx + "net.4.bias"], on=on)
    return y if mask_out is None else y * mask_out * c


class _Conv(torch.autograd.Function):
    """the conv unit's convolution on (b, c, f, t): kernel (2, 3), stride (2, 1), padding (0, 1), both operands of each of its
    three products rounded: forward conv2d(r(x), r(w)); backward conv2d_input(r(w), r(g)) and conv2d_weight(r(x), r(g)), g being
    the gradient at the convolution's output"""

    @staticmethod
    def forward(ctx, x, w, on):
        ctx.save_for_backward(x, w)
        ctx.on = on
        return F.conv2d(r16(x, on), r16(w, on), stride=(2, 1), padding=(0, 1))

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gr = r16(g, ctx.on)
        gx = torch.nn.grad.conv2d_input(x.shape, r16(w, ctx.on), gr, stride=(2, 1), padding=(0, 1))
        gw = torch.nn.grad.conv2d_weight(r16(x, ctx.on), w.shape, gr, stride=(2, 1), padding=(0, 1))
        return gx, gw, None


# ---- training-mode BatchNorm ----------------------------------------------------------------------------------------------------
class _PlainGrad(torch.autograd.Function):
    """Identity whose backward hands on a freshly laid out, contiguous copy of the gradient.  torch's CPU batch_norm backward
    misreads a grad_output whose strides look channels-last, which is what a permuted gradient with a last extent of 1 (T = 1)
    does: its gradients then disagree with plain autograd through the same formula (tests/test_bn_grad_reference.py holds the
    two against each other at T = 1)."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return torch.empty(g.shape, dtype=g.dtype).copy_(g)


def training_batchnorm(stats):
    """-> a stand-in for O.batchnorm: ``torch.nn.functional.batch_norm(..., training=True, momentum=0.1, eps=1e-5)`` on CLONES of
    the running buffers; the moved buffers land in ``stats``.  The buffers are kept in fp32 when the input is fp16 (under autocast
    a BatchNorm's buffers and parameters stay fp32, as in the reference's 16-mixed run; torch's CPU kernel takes that mixture and
    no other)."""
    def batchnorm(x, sd, pfx, ch_dim):
        assert ch_dim == 1
        dt = torch.float32 if x.dtype == torch.float16 else x.dtype
        mean = sd[pfx + "running_mean"].detach().to(dt).clone()
        var = sd[pfx + "running_var"].detach().to(dt).clone()
        y = F.batch_norm(x, mean, var, sd[pfx + "weight"], sd[pfx + "bias"], training=True, momentum=0.1, eps=1e-5)
        stats[pfx + "running_mean"], stats[pfx + "running_var"] = mean, var
        if pfx + "num_batches_tracked" in sd:
            stats[pfx + "num_batches_tracked"] = sd[pfx + "num_batches_tracked"].detach().clone() + 1
        return _PlainGrad.apply(y)
    return batchnorm


@contextlib.contextmanager
def swapped(batchnorm):
    """``O.batchnorm`` = ``batchnorm`` inside the block; the oracle's file stays as it is"""
    real = O.batchnorm
    O.batchnorm = batchnorm
    try:
        yield
    finally:
        O.batchnorm = real


# ---- one unit, and what is built from it ------------------------------------------------------------------------------------------
def unit(kind, x, sd, pfx, on=None, masks=None, c=1.0):
    """the branch of one attention ("attn") or feed-forward ("ff") unit on (B, T, C) rows, without the residual: the oracle
    (on = None), the masked oracle (on = None with ``masks`` = the unit's two masks as tensors) or the restatement"""
    heads, attn = x.shape[-1] // 32, kind == "attn"
    if on is not None:
        m = (None, None) if masks is None else masks
        return attention(x, sd, pfx, heads, on, *m, c) if attn else feedforward(x, sd, pfx, on, *m, c)
    if masks is None:
        return O.attention(x, sd, pfx, heads) if attn else O.feedforward(x, sd, pfx)
    return attention_drop(x, sd, pfx, heads, *masks, c) if attn else feedforward_drop(x, sd, pfx, *masks, c)


def dropped_unit(kind, x, sd, pfx, on, drop, hidden, dtype=None):
    """``unit`` with the masks of ``drop`` = None or (p, seed, stream) over x's own (B, T, C), as tensors of ``dtype`` (x's own)"""
    if drop is None:
        return unit(kind, x, sd, pfx, on)
    masks = masks_as(unit_masks(kind, drop[0], drop[1], drop[2], *x.shape, hidden), dtype or x.dtype)
    return unit(kind, x, sd, pfx, on, masks, 1.0 / (1.0 - drop[0]))


LEAVES = ("attnF", "ffF", "attnT", "ffT")
BLOCK_SHAPES = ((32, 32), (16, 64), (8, 128))          # (F, C) at the input of block i


def to_oracle(t):   # (b, t, f, c) -> (b, c, f, t)
    return t.permute(0, 3, 2, 1)


def leaf_shape(i, leaf, B, T):
    """(B', T', C) of a leaf call of block i on a (B, T) batch"""
    F_, C_ = BLOCK_SHAPES[i]
    return (B * T, F_, C_) if leaf.endswith("F") else (B * F_, T, C_)


def leaf_masks(i, leaf, drop, B, T, hidden):
    """the two masks of a leaf call as ``unit_masks`` shapes them: over (B', T', C) of the contract"""
    Bp, Tp, C_ = leaf_shape(i, leaf, B, T)
    return unit_masks("attn" if leaf.startswith("attn") else "ff", drop[0], drop[1], drop[2], Bp, Tp, C_, hidden)


def plan(p, seed, first=0, blocks=(0, 1, 2)):
    """{(block, leaf): (p, seed, stream) or None}: the streams of one frontend forward, in call order; rate 0 takes no number"""
    out, stream = {}, first
    for i in blocks:
        for leaf in LEAVES:
            out[i, leaf] = (p, seed, stream) if p > 0 else None
            stream += int(p > 0)
    return out


def n_layers_of(sd):
    return 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("transformer_blocks.layers."))


def model_plan(sd, p_front, p_trunk, seed, first=0):
    """(plan, trunk_drop, streams used) of one whole-model forward from counter ``first``: the leaves first, then the trunk"""
    blocks = tuple(i for i in range(3) if f"frontend.blocks.{i}.partial.attnF.norm.gamma" in sd)
    pl = plan(p_front, seed, first, blocks)
    used = 4 * len(blocks) * int(p_front > 0)
    trunk_drop = (p_trunk, seed, first + used) if p_trunk > 0 else None
    return pl, trunk_drop, used + 2 * n_layers_of(sd) * int(p_trunk > 0)


def conv_unit(x, sd, p, on=None):
    """blocks.i.conv2d + norm + GELU on (b, c, f, t), as O.frontend runs it; BatchNorm and GELU in the working dtype
    (``O.batchnorm`` is looked up at call time: ``swapped`` puts the training-mode one there)"""
    w = sd[p + "conv2d.weight"]
    y = F.conv2d(x, w, stride=(2, 1), padding=(0, 1)) if on is None else _Conv.apply(x, w, on)
    return F.gelu(O.batchnorm(y, sd, p + "norm.", 1))


def partial_ft(x, sd, i, drops=None, on=None):
    """O.partial_ft of block i on (b, c, f, t): the oracle's own with on = None and ``drops`` = None, else its loop over ``unit``
    with ``drops`` = {leaf: None or (p, seed, stream)}"""
    pfx = f"frontend.blocks.{i}.partial."
    if on is None and drops is None:
        return O.partial_ft(x, sd, pfx)
    drops = drops or {}
    hidden = sd[pfx + "ffF.net.1.weight"].shape[0]
    leaf = lambda y, name: dropped_unit(name[:-1], y, sd, pfx + name + ".", on, drops.get(name), hidden)
    b, c, f, t = x.shape
    y = x.permute(0, 3, 2, 1).reshape(b * t, f, c)                              # (b t) f c
    y = y + leaf(y, "attnF")
    y = y + leaf(y, "ffF")
    y = y.view(b, t, f, c).permute(0, 2, 1, 3).reshape(b * f, t, c)             # (b f) t c
    y = y + leaf(y, "attnT")
    y = y + leaf(y, "ffT")
    return y.view(b, f, t, c).permute(0, 3, 1, 2)                               # b c f t


def projection(x, sd, on=None):
    """concat + frontend.linear: (b, c, f, t) -> (b, t, D)"""
    b, c, f, t = x.shape
    rows = x.permute(0, 3, 1, 2).reshape(b, t, c * f)
    w, bias = sd["frontend.linear.weight"], sd["frontend.linear.bias"]
    return O._linear(rows, w, bias) if on is None else linear(rows, w, bias, on)


def frontend(x, sd, plan_=None, on=None):
    """(B, T, 128) -> (B, T, D): O.frontend itself with on = None and no plan, else its loop with the leaves of ``plan_`` dropped;
    the stem is the oracle's (fp32 on the device too)"""
    if on is None and plan_ is None:
        return O.frontend(x, sd)
    h = O.stem(x, sd)
    for i in range(3):
        p = f"frontend.blocks.{i}."
        if p + "partial.attnF.norm.gamma" in sd:
            h = partial_ft(h, sd, i, {leaf: (plan_ or {}).get((i, leaf)) for leaf in LEAVES}, on)
        h = conv_unit(h, sd, p, on)
    return projection(h, sd, on)


def head_outputs(h, leaf, sum_head):
    bd = O._linear(h, leaf["task_heads.beat_downbeat_lin.weight"], leaf["task_heads.beat_downbeat_lin.bias"])
    beat, down = bd[..., 0], bd[..., 1]
    return (beat + down if sum_head else beat), down


def trunk(leaf, x, n_layers, on=None, drop=None, sum_head=True):
    """(beat, downbeat) of the transformer and the head on (B, T, D): ``O.transformer`` with on = None and no ``drop``, else the
    layers over ``unit`` -- with ``drop`` = (p, seed, first stream) under masks -- the final norm and the head in the working dtype"""
    if on is None and drop is None:
        return head_outputs(O.transformer(x, leaf, n_layers, leaf["transformer_blocks.norm.gamma"].shape[0] // 32), leaf, sum_head)
    dtype = x.dtype
    for l in range(n_layers):
        pfx = f"transformer_blocks.layers.{l}."
        hidden = leaf[pfx + "1.net.1.weight"].shape[0]
        drops = (None, None) if drop is None else ((drop[0], drop[1], drop[2] + 2 * l), (drop[0], drop[1], drop[2] + 2 * l + 1))
        x = dropped_unit("attn", x, leaf, pfx + "0.", on, drops[0], hidden, dtype) + x
        x = dropped_unit("ff", x, leaf, pfx + "1.", on, drops[1], hidden, dtype) + x
    return head_outputs(O.rmsnorm(x, leaf["transformer_blocks.norm.gamma"]), leaf, sum_head)


def model(x, sd, plan_=None, trunk_drop=None, on=None):
    """(beat, downbeat), summing head: the frontend under ``plan_``, the trunk under ``trunk_drop`` (a rate of 0 drops nothing)"""
    trunk_drop = trunk_drop if trunk_drop is not None and trunk_drop[0] > 0 else None
    return trunk(sd, frontend(x, sd, plan_, on), n_layers_of(sd), on, trunk_drop)
