"""The differentiable route of ``BeatThis``: the six main transformer layers, the final RMSNorm and the task heads as
``torch.autograd.Function``s over the training entry points of the HIP library (bt_train_forward / bt_train_backward,
csrc/train.hip).  One Function per unit, each ``once_differentiable``; the reference's container loop composes them
(``x = attn(x) + x; x = ff(x) + x; norm; head``, roformer.py:176-181).

The kernels read the parameters' own storage at call time (the reference's layout and values, not the engine's packed
copies), so an optimizer step is seen by the next forward.  The arithmetic is fp32 whatever ``fp32_split_gemms`` says and
also under ``torch.autocast``.  Gradients are overwritten by the library and handed to autograd, which accumulates into
``.grad``; they are bitwise reproducible (no atomics anywhere).

Dropout and 16-mixed (DESIGN.md sections 15, 16): the attention and the feed-forward take ``drop`` = None (the calls and launches
of a model without dropout) or ``(p, seed, stream)``, which goes from ``ctx`` unchanged to the backward -- the kernels recompute
the masks from those three numbers, nothing is stored -- and ``mixed``: both operands of every matrix product rounded to fp16,
fp32 accumulation, everything else fp32 (True or "fp16"; "bf16" rounds them to bfloat16 instead, section 24: ``_operand``).  ``_run`` picks the entry points for the two; ``BeatThis._route`` decides both per
call (``torch.autocast`` does not) and ``BeatThis`` hands out the streams.

The frontend (the lower part of this file): ``StemFn``, ``ConvUnitFn``, ``SwapFn`` and ``ProjectionFn`` over
bt_front_forward / bt_front_backward (csrc/train_front.hip), composed by ``frontend_train`` with ``AttentionFn`` /
``FeedForwardFn`` for the twelve leaves of the partial transformers; BatchNorm on its running statistics; dropout in the leaves
alone and only when ``BeatThis.enable_dropout(frontend=True)`` opted in (section 21: ``partial_ft`` takes the ``drop`` values); fp32, or
with ``BeatThis.set_frontend_precision("16-mixed")`` the conv units, the leaves and the projection take ``mixed`` (section 19).
``BeatThis.set_frontend_trainable`` decides whether it runs.  ``StemBatchFn`` / ``ConvUnitBatchFn`` (section 18, bt_front_bn_*)
are the same two units on the statistics of the call's batch; their forward moves the running buffers in place
(``BeatThis.set_batch_statistics``).
"""
from __future__ import annotations

import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from .. import _lib


def _f32(t: torch.Tensor) -> torch.Tensor:
    """fp32 and contiguous (a parameter already is: its own storage is what the kernels read)"""
    return t.detach().to(torch.float32).contiguous()


def _on_device_of(x: torch.Tensor, *tensors) -> None:
    """Checked before any launch: the kernels take raw pointers, so every operand has to live on the input's GPU."""
    _lib.require_gpu(x, "input of the differentiable route")
    for t in tensors:
        if t is not None and t.device != x.device:
            raise RuntimeError(f"the differentiable route got an operand on '{t.device}' and its input on '{x.device}': "
                               "move the model and the input to the same ROCm GPU")


def _args(x: torch.Tensor, hidden: int = 0, rope=None, rope_len: int = 0) -> _lib.TrainArgs:
    if rope is not None and (rope.dim() != 3 or rope.shape[0] < max(int(rope_len), int(x.shape[1])) or tuple(rope.shape[1:]) != (16, 2)):
        raise ValueError(f"rotary table of shape {tuple(rope.shape)} for {int(x.shape[1])} frames (rope_len {rope_len})")
    a = _lib.TrainArgs()
    a.B, a.T, a.dim = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    a.hidden, a.rope_len = int(hidden), int(rope_len)
    a.rope = _lib.ptr(rope)
    a.x = x.data_ptr()
    return a


# (mixed, drop is None) -> the family of entry points (bt_train_forward / _backward / _workspace_bytes + this); the plain one takes
# no dropout argument, "_dropout" takes (p, seed, stream), "_mixed" takes them or NULL and its workspace query whether they come
_FAMILY = {(False, True): "", (False, False): "_dropout", (True, True): "_mixed", (True, False): "_mixed"}


def _operand(mixed) -> int:
    """BT_OPERAND_* of a ``mixed`` value, by _lib.OPERAND_FORMATS: False (fp32: the field is not read), True or "fp16", "bf16"
    (section 24) or "bf16x3" (section 25: the split operands of "32-high")"""
    name = "fp16" if mixed is True or not mixed else mixed
    if name not in _lib.OPERAND_FORMATS:
        raise ValueError(f"mixed must be False, True, 'fp16', 'bf16' or 'bf16x3', got {mixed!r}")
    return _lib.OPERAND_FORMATS[name][0]


def _run(backward: bool, unit: int, a: _lib.TrainArgs, device, drop=None, mixed=False) -> None:
    """One call of a unit of the trunk -- attention, feed-forward, final norm, head -- with its workspace; ``drop``: None or
    (p, seed, stream); ``mixed``: 16-mixed (the attention and the feed-forward alone take either), True or the operand format"""
    lib, family = _lib.lib(), _FAMILY[bool(mixed), drop is None]
    a.operand = _operand(mixed)
    extra = (int(drop is not None),) if mixed else ()
    need = getattr(lib, "bt_train_workspace_bytes" + family)(unit, int(backward), a.B, a.T, a.dim, a.hidden, *extra)
    if need == 0:
        raise ValueError(f"the differentiable route supports widths that are multiples of 32 from 32 to 1024 and ff_mult 1 .. 16, "
                         f"got batch {a.B}, {a.T} frames, width {a.dim}, hidden width {a.hidden}")
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
    d = None if drop is None else C.byref(_lib.TrainDropout(p=drop[0], seed=drop[1], stream=drop[2]))
    fn = getattr(lib, ("bt_train_backward" if backward else "bt_train_forward") + family)
    with torch.cuda.device(device):
        _lib.check(fn(_lib.stream_ptr(device), unit, C.byref(a), *((d,) if family else ())))


def _grad_like(p: torch.Tensor, wanted: bool):
    return torch.empty(p.shape, dtype=torch.float32, device=p.device) if wanted else None


class AttentionFn(torch.autograd.Function):
    """Attention.forward (roformer.py:114-132) on (B, T, D): the branch without the residual, or with ``residual`` the unit's
    own x + f(x) (the frontend's leaves)."""

    @staticmethod
    def forward(ctx, x, gamma, w_qkv, w_gates, b_gates, w_out, rope, rope_len, drop=None, mixed=False, residual=False):
        xf = _f32(x)
        B, T, D = xf.shape
        ps = [_f32(p) for p in (gamma, w_qkv, w_gates, b_gates, w_out)]
        _on_device_of(xf, rope, *ps)
        y = torch.empty_like(xf)
        o = torch.empty_like(xf)
        lse = torch.empty((B, T, D // 32), dtype=torch.float32, device=xf.device)
        a = _args(xf, rope=rope, rope_len=rope_len)
        a.residual = int(bool(residual))
        a.gamma, a.w1, a.w2, a.b2, a.w3 = (p.data_ptr() for p in ps)
        a.y, a.save_o, a.save_lse = y.data_ptr(), o.data_ptr(), lse.data_ptr()
        _run(False, _lib.UNIT_ATTN, a, xf.device, drop, mixed)
        ctx.save_for_backward(xf, o, lse, rope, *ps)
        ctx.rope_len, ctx.drop, ctx.mixed, ctx.residual = rope_len, drop, mixed, int(bool(residual))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xf, o, lse, rope, gamma, w_qkv, w_gates, b_gates, w_out = ctx.saved_tensors
        need = ctx.needs_input_grad
        gyf = _f32(gy)
        gx, g_gamma, g_qkv, g_wg, g_bg, g_out = (_grad_like(t, need[i]) for i, t in
                                                 enumerate((xf, gamma, w_qkv, w_gates, b_gates, w_out)))
        a = _args(xf, rope=rope, rope_len=ctx.rope_len)
        a.residual = ctx.residual
        a.gamma, a.w1, a.w2, a.b2, a.w3 = (p.data_ptr() for p in (gamma, w_qkv, w_gates, b_gates, w_out))
        a.save_o, a.save_lse, a.gy = o.data_ptr(), lse.data_ptr(), gyf.data_ptr()
        a.gx, a.g_gamma, a.g_w1, a.g_w2, a.g_b2, a.g_w3 = (_lib.ptr(g) for g in (gx, g_gamma, g_qkv, g_wg, g_bg, g_out))
        _run(True, _lib.UNIT_ATTN, a, xf.device, ctx.drop, ctx.mixed)
        return gx, g_gamma, g_qkv, g_wg, g_bg, g_out, None, None, None, None, None


class FeedForwardFn(torch.autograd.Function):
    """FeedForward.forward (roformer.py:38-61) on (B, T, D): the branch without the residual, or with ``residual`` x + f(x)."""

    @staticmethod
    def forward(ctx, x, gamma, w1, b1, w2, b2, drop=None, mixed=False, residual=False):
        xf = _f32(x)
        ps = [_f32(p) for p in (gamma, w1, b1, w2, b2)]
        _on_device_of(xf, *ps)
        y = torch.empty_like(xf)
        a = _args(xf, hidden=ps[1].shape[0])
        a.residual = int(bool(residual))
        a.gamma, a.w1, a.b1, a.w2, a.b2 = (p.data_ptr() for p in ps)
        a.y = y.data_ptr()
        _run(False, _lib.UNIT_FF, a, xf.device, drop, mixed)
        ctx.save_for_backward(xf, *ps)
        ctx.drop, ctx.mixed, ctx.residual = drop, mixed, int(bool(residual))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xf, gamma, w1, b1, w2, b2 = ctx.saved_tensors
        gyf = _f32(gy)
        grads = [_grad_like(t, ctx.needs_input_grad[i]) for i, t in enumerate((xf, gamma, w1, b1, w2, b2))]
        a = _args(xf, hidden=w1.shape[0])
        a.residual = ctx.residual
        a.gamma, a.w1, a.b1, a.w2, a.b2 = (p.data_ptr() for p in (gamma, w1, b1, w2, b2))
        a.gy = gyf.data_ptr()
        a.gx, a.g_gamma, a.g_w1, a.g_b1, a.g_w2, a.g_b2 = (_lib.ptr(g) for g in grads)
        _run(True, _lib.UNIT_FF, a, xf.device, ctx.drop, ctx.mixed)
        return (*grads, None, None, None)


class NormFn(torch.autograd.Function):
    """The trunk's final RMSNorm (roformer.py:22-32, 181)."""

    @staticmethod
    def forward(ctx, x, gamma):
        xf, g = _f32(x), _f32(gamma)
        _on_device_of(xf, g)
        y = torch.empty_like(xf)
        a = _args(xf)
        a.gamma, a.y = g.data_ptr(), y.data_ptr()
        _run(False, _lib.UNIT_NORM, a, xf.device)
        ctx.save_for_backward(xf, g)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xf, gamma = ctx.saved_tensors
        gyf = _f32(gy)
        gx, g_gamma = _grad_like(xf, ctx.needs_input_grad[0]), _grad_like(gamma, ctx.needs_input_grad[1])
        a = _args(xf)
        a.gamma, a.gy, a.gx, a.g_gamma = gamma.data_ptr(), gyf.data_ptr(), _lib.ptr(gx), _lib.ptr(g_gamma)
        _run(True, _lib.UNIT_NORM, a, xf.device)
        return gx, g_gamma


class HeadFn(torch.autograd.Function):
    """SumHead / Head (beat_tracker.py:304-346): (B, T, D) -> beat, downbeat (B, T)."""

    @staticmethod
    def forward(ctx, x, w, b, sum_head):
        xf, wf, bf = _f32(x), _f32(w), _f32(b)
        _on_device_of(xf, wf, bf)
        B, T, D = xf.shape
        beat = torch.empty((B, T), dtype=torch.float32, device=xf.device)
        down = torch.empty_like(beat)
        a = _args(xf)
        a.sum_head = int(bool(sum_head))
        a.w1, a.b1, a.y, a.y2 = wf.data_ptr(), bf.data_ptr(), beat.data_ptr(), down.data_ptr()
        _run(False, _lib.TRAIN_UNIT_HEAD, a, xf.device)
        ctx.save_for_backward(xf, wf, bf)
        ctx.sum_head = int(bool(sum_head))
        ctx.set_materialize_grads(False)   # (a loss on one of the two outputs: the other's gradient is None, not zeros)
        return beat, down

    @staticmethod
    @once_differentiable
    def backward(ctx, g_beat, g_down):
        xf, w, b = ctx.saved_tensors
        gb = None if g_beat is None else _f32(g_beat)
        gd = None if g_down is None else _f32(g_down)
        gx, gw, gbias = (_grad_like(t, ctx.needs_input_grad[i]) for i, t in enumerate((xf, w, b)))
        a = _args(xf)
        a.sum_head = ctx.sum_head
        a.w1, a.b1, a.gy, a.gy2 = w.data_ptr(), b.data_ptr(), _lib.ptr(gb), _lib.ptr(gd)
        a.gx, a.g_w1, a.g_b1 = _lib.ptr(gx), _lib.ptr(gw), _lib.ptr(gbias)
        _run(True, _lib.TRAIN_UNIT_HEAD, a, xf.device)
        return gx, gw, gbias, None


def empty_with_graph(shape, x: torch.Tensor, params) -> torch.Tensor:
    """An empty batch or zero frames: an empty fp32 result that still hangs in the graph, so that ``backward`` runs and leaves
    zero gradients."""
    out = torch.zeros(shape, dtype=torch.float32, device=x.device)
    for t in (x, *params):
        if t.requires_grad and t.is_floating_point():
            out = out + t.reshape(-1)[:0].sum().to(torch.float32)
    return out


def attention(node, x, rope, rope_len, drop=None, mixed=False, residual=False):
    """``transformer_blocks.layers[l][0]`` of the differentiable route; ``drop``: None or (p, seed, stream); ``mixed``: 16-mixed;
    ``residual``: x + f(x) in the unit's own kernels (``residual = 1`` of bt_train_args)"""
    return AttentionFn.apply(x, node.norm.gamma, node.to_qkv.weight, node.to_gates.weight, node.to_gates.bias,
                             node.to_out[0].weight, rope, rope_len, drop, mixed, residual)


def feedforward(node, x, drop=None, mixed=False, residual=False):
    """``transformer_blocks.layers[l][1]``"""
    net = node.net
    return FeedForwardFn.apply(x, net[0].gamma, net[1].weight, net[1].bias, net._modules["4"].weight, net._modules["4"].bias, drop,
                               mixed, residual)


def final_norm(node, x):
    return NormFn.apply(x, node.gamma)


def head(node, x, sum_head: bool):
    lin = node.beat_downbeat_lin
    return HeadFn.apply(x, lin.weight, lin.bias, sum_head)


# ---- the differentiable frontend (csrc/train_front.hip) -----------------------------------------------------
# Activations are the library's (b, t, f, c), channels last, fp32.  BatchNorm runs on its running statistics, only the leaves
# of the partial transformers can drop (section 21), and the arithmetic is fp32 whatever the train precision says; ``mixed`` (BeatThis.set_frontend_precision) puts the conv
# units', the leaves' and the projection's matrix products on fp16 operands.
def check_front_limits(B: int, T: int) -> None:
    """Raised before any launch: the frequency direction runs B T sequences, every unit B T 32 rows at the most."""
    if B * T > _lib.FRONT_MAX_FRAMES or B * T * 32 > _lib.FRONT_MAX_ROWS:
        raise ValueError(f"the differentiable frontend takes at most {_lib.FRONT_MAX_FRAMES} frames per call (batch x time, "
                         f"{_lib.FRONT_MAX_ROWS} rows of 32 frequency tokens), got batch {B} x {T} frames: split the batch")


def check_batch_statistics(B: int, T: int) -> None:
    """torch's own refusal, raised before any launch: a BatchNorm in training mode needs two values per channel, and
    ``stem.bn1d`` has B T of them"""
    if B * T < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {(B, 128, T)}: batch statistics "
                         "need batch x time >= 2")


def _front_args(B, T, F, Cc, dim=0, mixed=False, batch=False):
    """The argument struct of bt_front_forward / _backward or, with ``batch`` (the stem and the conv unit on
    the statistics of the call's batch), of bt_front_bn_forward / _backward, which has no ``dim``"""
    if batch:
        return _lib.FrontBnArgs(B=int(B), T=int(T), F=int(F), C=int(Cc), mixed=int(bool(mixed)), operand=_operand(mixed))
    return _lib.FrontArgs(B=int(B), T=int(T), F=int(F), C=int(Cc), dim=int(dim), mixed=int(bool(mixed)), operand=_operand(mixed))


def _front_call(backward: bool, unit: int, a, device) -> None:
    """One call of the frontend's own units: the struct's type picks the family of entry points, its ``mixed`` the workspace query"""
    batch = isinstance(a, _lib.FrontBnArgs)
    family = "bt_front_bn" if batch else "bt_front"
    shape = (a.B, a.T, a.F, a.C) if batch else (a.B, a.T, a.F, a.C, a.dim)
    query = dict(_lib.OPERAND_FORMATS.values())[a.operand] if a.mixed else ""   # (BT_OPERAND_* -> suffix: the split format has two weight images)
    need = getattr(_lib.lib(), f"{family}_workspace_bytes{query}")(unit, int(backward), *shape)
    if need == 0:
        check_front_limits(a.B, a.T)
        if batch:
            check_batch_statistics(a.B, a.T * (1 if unit == _lib.FRONT_STEM else a.F // 2))
        raise ValueError(f"the differentiable frontend does not support batch {a.B}, {a.T} frames, {a.F} frequency bins, {a.C} channels"
                         + (f" (unit {unit}, batch statistics)" if batch else f", width {a.dim} (unit {unit})"))
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
    fn = getattr(_lib.lib(), f"{family}_backward" if backward else f"{family}_forward")
    with torch.cuda.device(device):
        _lib.check(fn(_lib.stream_ptr(device), unit, C.byref(a)))


def _running(mean, var, tracked, C_):
    """The three buffers of a BatchNorm as the kernels update them: in place, in their own storage."""
    for t, dtype in ((mean, torch.float32), (var, torch.float32), (tracked, torch.int64)):
        if t.dtype != dtype or not t.is_contiguous() or t.numel() != (1 if t is tracked else C_):
            raise ValueError(f"batch statistics update the running buffers in place: expected contiguous {dtype} buffers of "
                             f"{C_} channels, got {t.dtype} {tuple(t.shape)}")
    return mean.data_ptr(), var.data_ptr(), tracked.data_ptr()


# What the two Functions of a unit share, running and batch statistics alike: the struct with the unit's input, conv weight,
# gains and biases; the forward's outputs; the gradients of a backward.
def _stem_args(xf, w, w1, b1, w2, b2, batch):
    B, T, F = xf.shape
    a = _front_args(B, T, F, int(w.shape[0]), batch=batch)
    a.x, a.w, a.bn1_w, a.bn1_b, a.bn_w, a.bn_b = (t.data_ptr() for t in (xf, w, w1, b1, w2, b2))
    return a


def _stem_forward(a, xf):
    y = torch.empty((xf.shape[0], xf.shape[1], 32, 32), dtype=torch.float32, device=xf.device)
    a.y = y.data_ptr()
    _front_call(False, _lib.FRONT_STEM, a, xf.device)
    return y


def _stem_backward(a, gy, grads, device):
    """``grads``: gx, g_w, then gain and bias gradient of bn1d and of bn2d (None: not wanted)"""
    gyf = _f32(gy)
    a.gy = gyf.data_ptr()
    a.gx, a.g_w, a.g_bn1_w, a.g_bn1_b, a.g_bn_w, a.g_bn_b = (_lib.ptr(g) for g in grads)
    _front_call(True, _lib.FRONT_STEM, a, device)


def _conv_args(xf, w, nw, nb, mixed, batch):
    B, T, F, Cc = xf.shape
    a = _front_args(B, T, F, Cc, mixed=mixed, batch=batch)
    a.x, a.w, a.bn_w, a.bn_b = (t.data_ptr() for t in (xf, w, nw, nb))
    return a


def _conv_forward(a, xf, w):
    """Returns y and the convolution's result ``pre``, which the backward takes"""
    B, T, F, Cc = xf.shape
    if tuple(w.shape) != (2 * Cc, Cc, 2, 3) or F % 2:
        raise ValueError(f"conv unit: input {tuple(xf.shape)} against a weight of shape {tuple(w.shape)}")
    y = torch.empty((B, T, F // 2, 2 * Cc), dtype=torch.float32, device=xf.device)
    pre = torch.empty_like(y)
    a.y, a.save_pre = y.data_ptr(), pre.data_ptr()
    _front_call(False, _lib.FRONT_CONV, a, xf.device)
    return y, pre


def _conv_backward(a, pre, gy, grads, device):
    """``grads``: gx, g_w, the norm's gain and bias gradient (None: not wanted)"""
    gyf = _f32(gy)
    a.save_pre, a.gy = pre.data_ptr(), gyf.data_ptr()
    a.gx, a.g_w, a.g_bn_w, a.g_bn_b = (_lib.ptr(g) for g in grads)
    _front_call(True, _lib.FRONT_CONV, a, device)


class StemFn(torch.autograd.Function):
    """make_stem (beat_tracker.py:108-126): (B, T, 128) -> (B, T, 32, 32) = (b, t, f, c).  Inputs: x, conv weight, bn1d weight,
    bias, running_mean, running_var, bn2d weight, bias, running_mean, running_var."""

    @staticmethod
    def _args(xf, w, w1, b1, m1, v1, w2, b2, m2, v2):
        a = _stem_args(xf, w, w1, b1, w2, b2, batch=False)
        a.bn1_mean, a.bn1_var, a.bn_mean, a.bn_var = (t.data_ptr() for t in (m1, v1, m2, v2))
        return a

    @staticmethod
    def forward(ctx, x, w, w1, b1, m1, v1, w2, b2, m2, v2):
        xf = _f32(x)
        ps = [_f32(p) for p in (w, w1, b1, m1, v1, w2, b2, m2, v2)]
        _on_device_of(xf, *ps)
        y = _stem_forward(StemFn._args(xf, *ps), xf)
        ctx.save_for_backward(xf, *ps)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xf, *ps = ctx.saved_tensors
        need = ctx.needs_input_grad
        gx, g_w, g_w1, g_b1, g_w2, g_b2 = grads = [_grad_like(t, need[i]) for i, t in
                                                   ((0, xf), (1, ps[0]), (2, ps[1]), (3, ps[2]), (6, ps[5]), (7, ps[6]))]
        _stem_backward(StemFn._args(xf, *ps), gy, grads, xf.device)
        return gx, g_w, g_w1, g_b1, None, None, g_w2, g_b2, None, None


class ConvUnitFn(torch.autograd.Function):
    """blocks.i.conv2d + .norm + GELU (beat_tracker.py:155-166): (B, T, F, C) -> (B, T, F / 2, 2 C).  Saves its input and the
    convolution's result ``pre``.  Inputs: x, conv weight, norm weight, bias, running_mean, running_var; ``mixed``: the three
    products on fp16 operands (section 19), in the forward and, remembered, in the backward."""

    @staticmethod
    def _args(xf, w, nw, nb, nm, nv, mixed):
        a = _conv_args(xf, w, nw, nb, mixed, batch=False)
        a.bn_mean, a.bn_var = nm.data_ptr(), nv.data_ptr()
        return a

    @staticmethod
    def forward(ctx, x, w, nw, nb, nm, nv, mixed=False):
        xf = _f32(x)
        ps = [_f32(p) for p in (w, nw, nb, nm, nv)]
        _on_device_of(xf, *ps)
        y, pre = _conv_forward(ConvUnitFn._args(xf, *ps, mixed), xf, ps[0])
        ctx.save_for_backward(xf, pre, *ps)
        ctx.mixed = mixed
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xf, pre, *ps = ctx.saved_tensors
        grads = [_grad_like(t, ctx.needs_input_grad[i]) for i, t in enumerate((xf, ps[0], ps[1], ps[2]))]
        _conv_backward(ConvUnitFn._args(xf, *ps, ctx.mixed), pre, gy, grads, xf.device)
        return (*grads, None, None, None)


# ---- batch-statistics BatchNorm: the same two units over bt_front_bn_forward / _backward --------------------
class StemBatchFn(torch.autograd.Function):
    """``StemFn`` with bn1d and bn2d on the statistics of the call's batch.  Inputs: x, conv weight, bn1d weight, bias, bn2d
    weight, bias, then the six buffers (bn1d running_mean, running_var, num_batches_tracked, bn2d likewise), which the forward
    updates in place, once, and which take no part in the graph.  Saves the batch's mean and 1 / sqrt(var + eps) of both."""

    @staticmethod
    def _args(xf, ps, stats):
        a = _stem_args(xf, *ps, batch=True)
        a.save1_mean, a.save1_rstd, a.save_mean, a.save_rstd = (t.data_ptr() for t in stats)
        return a

    @staticmethod
    def forward(ctx, x, w, w1, b1, w2, b2, m1, v1, n1, m2, v2, n2):
        xf = _f32(x)
        ps = [_f32(p) for p in (w, w1, b1, w2, b2)]
        _on_device_of(xf, *ps, m1, v1, n1, m2, v2, n2)
        F = xf.shape[2]
        stats = [torch.empty(n, dtype=torch.float32, device=xf.device) for n in (F, F, 32, 32)]
        a = StemBatchFn._args(xf, ps, stats)
        a.bn1_mean, a.bn1_var, a.bn1_tracked = _running(m1, v1, n1, F)
        a.bn_mean, a.bn_var, a.bn_tracked = _running(m2, v2, n2, 32)
        y = _stem_forward(a, xf)
        ctx.save_for_backward(xf, *ps, *stats)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xf, w, w1, b1, w2, b2, *stats = ctx.saved_tensors
        grads = [_grad_like(t, ctx.needs_input_grad[i]) for i, t in enumerate((xf, w, w1, b1, w2, b2))]
        _stem_backward(StemBatchFn._args(xf, (w, w1, b1, w2, b2), stats), gy, grads, xf.device)
        return (*grads, None, None, None, None, None, None)


class ConvUnitBatchFn(torch.autograd.Function):
    """``ConvUnitFn`` with the norm on the statistics of the call's batch.  Inputs: x, conv weight, norm weight, bias, then
    running_mean, running_var, num_batches_tracked (updated in place by the forward, outside the graph); ``mixed`` as
    ``ConvUnitFn``'s (the moments are those of the fp16-product ``pre``)."""

    @staticmethod
    def _args(xf, ps, stats, mixed):
        a = _conv_args(xf, *ps, mixed, batch=True)
        a.save_mean, a.save_rstd = (t.data_ptr() for t in stats)
        return a

    @staticmethod
    def forward(ctx, x, w, nw, nb, nm, nv, nn_, mixed=False):
        xf = _f32(x)
        ps = [_f32(p) for p in (w, nw, nb)]
        _on_device_of(xf, *ps, nm, nv, nn_)
        Cout = 2 * xf.shape[3]
        stats = [torch.empty(Cout, dtype=torch.float32, device=xf.device) for _ in range(2)]
        a = ConvUnitBatchFn._args(xf, ps, stats, mixed)
        a.bn_mean, a.bn_var, a.bn_tracked = _running(nm, nv, nn_, Cout)
        y, pre = _conv_forward(a, xf, ps[0])
        ctx.save_for_backward(xf, pre, *ps, *stats)
        ctx.mixed = mixed
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xf, pre, w, nw, nb, *stats = ctx.saved_tensors
        grads = [_grad_like(t, ctx.needs_input_grad[i]) for i, t in enumerate((xf, w, nw, nb))]
        _conv_backward(ConvUnitBatchFn._args(xf, (w, nw, nb), stats, ctx.mixed), pre, gy, grads, xf.device)
        return (*grads, None, None, None, None)


class SwapFn(torch.autograd.Function):
    """(B, P, Q, C) -> (B, Q, P, C): between the frequency and the time direction of a partial transformer"""

    @staticmethod
    def forward(ctx, x):
        xf = _f32(x)
        _on_device_of(xf)
        B, P, Q, Cc = xf.shape
        y = torch.empty((B, Q, P, Cc), dtype=torch.float32, device=xf.device)
        a = _front_args(B, P, Q, Cc)
        a.x, a.y = xf.data_ptr(), y.data_ptr()
        _front_call(False, _lib.FRONT_SWAP, a, xf.device)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        gyf = _f32(gy)
        B, Q, P, Cc = gyf.shape
        gx = torch.empty((B, P, Q, Cc), dtype=torch.float32, device=gyf.device)
        a = _front_args(B, P, Q, Cc)
        a.gy, a.gx = gyf.data_ptr(), gx.data_ptr()
        _front_call(True, _lib.FRONT_SWAP, a, gyf.device)
        return gx


class ProjectionFn(torch.autograd.Function):
    """concat + frontend.linear (beat_tracker.py:71-76): (B, T, F, C) -> (B, T, D); the weight's columns are c F + f;
    ``mixed``: the three GEMMs of the forward and the backward on fp16 operands (section 19)"""

    @staticmethod
    def forward(ctx, x, w, b, mixed=False):
        xf, wf, bf = _f32(x), _f32(w), _f32(b)
        _on_device_of(xf, wf, bf)
        B, T, F, Cc = xf.shape
        D = int(wf.shape[0])
        if int(wf.shape[1]) != F * Cc:
            raise ValueError(f"projection: input {tuple(xf.shape)} against a weight of shape {tuple(wf.shape)}")
        y = torch.empty((B, T, D), dtype=torch.float32, device=xf.device)
        a = _front_args(B, T, F, Cc, D, mixed)
        a.x, a.y, a.w, a.b = xf.data_ptr(), y.data_ptr(), wf.data_ptr(), bf.data_ptr()
        _front_call(False, _lib.FRONT_LINEAR, a, xf.device)
        ctx.save_for_backward(xf, wf, bf)
        ctx.mixed = mixed
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xf, wf, bf = ctx.saved_tensors
        B, T, F, Cc = xf.shape
        gyf = _f32(gy)
        gx, g_w, g_b = (_grad_like(t, ctx.needs_input_grad[i]) for i, t in enumerate((xf, wf, bf)))
        a = _front_args(B, T, F, Cc, int(wf.shape[0]), ctx.mixed)
        a.x, a.gy, a.w, a.b = xf.data_ptr(), gyf.data_ptr(), wf.data_ptr(), bf.data_ptr()
        a.gx, a.g_w, a.g_b = (_lib.ptr(g) for g in (gx, g_w, g_b))
        _front_call(True, _lib.FRONT_LINEAR, a, xf.device)
        return gx, g_w, g_b, None


def _bn(node):
    return node.weight, node.bias, node.running_mean, node.running_var


def _stats(node):
    return node.running_mean, node.running_var, node.num_batches_tracked


def stem(node, x, batch_statistics=False):
    """``frontend.stem``: (B, T, 128) -> (b, t, f, c)"""
    if batch_statistics:
        return StemBatchFn.apply(x, node.conv2d.weight, node.bn1d.weight, node.bn1d.bias, node.bn2d.weight, node.bn2d.bias,
                                 *_stats(node.bn1d), *_stats(node.bn2d))
    return StemFn.apply(x, node.conv2d.weight, *_bn(node.bn1d), *_bn(node.bn2d))


def conv_unit(block, x, batch_statistics=False, mixed=False):
    """``frontend.blocks[i]`` behind its partial transformer: conv2d, norm, GELU on (b, t, f, c)"""
    if batch_statistics:
        return ConvUnitBatchFn.apply(x, block.conv2d.weight, block.norm.weight, block.norm.bias, *_stats(block.norm), mixed)
    return ConvUnitFn.apply(x, block.conv2d.weight, *_bn(block.norm), mixed)


def partial_ft(node, x, rope_for, mixed=False, drops=None):
    """PartialFTTransformer.forward (beat_tracker.py:290-301) on (b, t, f, c): attention and feed-forward over the frequency
    tokens of every frame, then over the time tokens of every bin -- the trunk's unit code with its residual on (B T, F, C) and
    (B F, T, C); fp32, or with ``mixed`` the 16-mixed unit calls.  ``rope_for(n)``: the rotary table for n tokens.  ``drops``:
    None (no dropout: the calls and launches as ever), four ``drop`` values -- None or (p, seed, stream) -- for attnF, ffF,
    attnT, ffT, or a callable that yields the next one (asked once per leaf, in that order).  A frequency-direction leaf's mask
    rows are (b T + t) F + f, a time-direction leaf's (b F + f) T + t (include/beat_this_amd.h)."""
    if drops is None:
        nxt = lambda: None
    elif callable(drops):
        nxt = drops
    else:
        four = list(drops)
        if len(four) != 4:
            raise ValueError(f"a partial transformer has four leaves (attnF, ffF, attnT, ffT), got {len(four)} drop values")
        nxt = iter(four).__next__
    B, T, F, Cc = x.shape
    y = x.reshape(B * T, F, Cc)
    y = attention(node.attnF, y, *rope_for(F), drop=nxt(), mixed=mixed, residual=True)
    y = feedforward(node.ffF, y, drop=nxt(), mixed=mixed, residual=True)
    y = SwapFn.apply(y.reshape(B, T, F, Cc)).reshape(B * F, T, Cc)
    y = attention(node.attnT, y, *rope_for(T), drop=nxt(), mixed=mixed, residual=True)
    y = feedforward(node.ffT, y, drop=nxt(), mixed=mixed, residual=True)
    return SwapFn.apply(y.reshape(B, F, T, Cc))


def frontend_train(model, x, batch_statistics=False, mixed=None, drops=None):
    """``BeatThis.frontend`` on the differentiable route, in the reference's order (beat_tracker.py:54-80, 290-301): stem, three
    times (partial transformer, conv unit), projection.  (B, T, 128) -> (B, T, D).  ``batch_statistics``: the five BatchNorms
    normalise with this call's batch and move their running buffers (section 18).  ``mixed``: the conv units, the leaves and the
    projection on fp16 operands (section 19), with "bf16" on bfloat16 ones (section 24), with "bf16x3" on split ones (section 25); None reads ``model.frontend_precision``
    and ``model.frontend_operand``.  The stem is fp32 either way.  ``drops``:
    None, or a callable that yields the ``drop`` of the next leaf call (section 21: ``BeatThis`` hands out the streams in forward
    order); the stem, the conv units and the projection never drop."""
    if mixed is None:
        mixed = {"16-mixed": model.frontend_operand, "32-high": "bf16x3"}.get(model.frontend_precision, False)
    fr = model.frontend
    check_front_limits(int(x.shape[0]), int(x.shape[1]))
    if batch_statistics:
        check_batch_statistics(int(x.shape[0]), int(x.shape[1]))
    h = stem(fr.stem, x, batch_statistics)
    for blk in fr.blocks:
        if "partial" in blk._modules:
            h = partial_ft(blk.partial, h, model._rope, mixed, drops)
        h = conv_unit(blk, h, batch_statistics, mixed)
    return ProjectionFn.apply(h, fr.linear.weight, fr.linear.bias, mixed)
