"""The differentiable route of ``BeatThis``: the six main transformer layers, the final RMSNorm and the task heads as
``torch.autograd.Function``s over the training entry points of the HIP library (bt_train_forward / bt_train_backward,
csrc/train.hip).  One Function per unit, each ``once_differentiable``; the reference's container loop composes them
(``x = attn(x) + x; x = ff(x) + x; norm; head``, roformer.py:176-181).

The kernels read the parameters' own storage at call time (the reference's layout and values, not the engine's packed
copies), so an optimizer step is seen by the next forward.  The arithmetic is fp32 whatever ``fp32_split_gemms`` says and
also under ``torch.autocast``.  Gradients are overwritten by the library and handed to autograd, which accumulates into
``.grad``; they are bitwise reproducible (no atomics anywhere).

Dropout: the attention and the feed-forward take ``drop`` = None (the calls and launches of a model without dropout) or
``(p, seed, stream)``, which goes to bt_train_forward_dropout and, from ``ctx``, unchanged to bt_train_backward_dropout: the
kernels recompute the masks from those three numbers, nothing is stored.  ``BeatThis`` decides when dropout is active and
hands out the streams.

16-mixed: the attention and the feed-forward take ``mixed``; True sends the same arguments to
bt_train_forward_mixed / bt_train_backward_mixed (both operands of every matrix product rounded to fp16, fp32 accumulation,
everything else fp32), False -- the default -- makes the calls above.  ``BeatThis.set_train_precision`` decides it;
``torch.autocast`` does not.
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


def _workspace(unit: int, backward: bool, B: int, T: int, D: int, hidden: int, device, drop=None, mixed=False) -> torch.Tensor:
    if mixed:
        need = _lib.lib().bt_train_workspace_bytes_mixed(unit, int(backward), B, T, D, hidden, int(drop is not None))
    else:
        query = _lib.lib().bt_train_workspace_bytes if drop is None else _lib.lib().bt_train_workspace_bytes_dropout
        need = query(unit, int(backward), B, T, D, hidden)
    if need == 0:
        raise ValueError(f"the differentiable route supports widths that are multiples of 32 from 32 to 1024 and ff_mult 1 .. 16, "
                         f"got batch {B}, {T} frames, width {D}, hidden width {hidden}")
    return torch.empty(need, dtype=torch.uint8, device=device)


def _args(x: torch.Tensor, hidden: int = 0, rope=None, rope_len: int = 0) -> _lib.TrainArgs:
    if rope is not None and (rope.dim() != 3 or rope.shape[0] < max(int(rope_len), int(x.shape[1])) or tuple(rope.shape[1:]) != (16, 2)):
        raise ValueError(f"rotary table of shape {tuple(rope.shape)} for {int(x.shape[1])} frames (rope_len {rope_len})")
    a = _lib.TrainArgs()
    a.B, a.T, a.dim = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    a.hidden, a.rope_len = int(hidden), int(rope_len)
    a.rope = _lib.ptr(rope)
    a.x = x.data_ptr()
    return a


def _call(fn, unit: int, a: _lib.TrainArgs, ws: torch.Tensor, device) -> None:
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
    with torch.cuda.device(device):
        _lib.check(fn(_lib.stream_ptr(device), unit, C.byref(a)))


def _run(backward: bool, unit: int, a: _lib.TrainArgs, shape, hidden: int, device, drop, mixed=False) -> None:
    """One attention / feed-forward call: the usual entry point, or with ``drop`` = (p, seed, stream) the dropout one;
    ``mixed``: the 16-mixed entry point, which takes the dropout or NULL"""
    B, T, D = shape
    ws = _workspace(unit, backward, B, T, D, hidden, device, drop, mixed)
    lib = _lib.lib()
    if mixed:
        fn = lib.bt_train_backward_mixed if backward else lib.bt_train_forward_mixed
        d = None if drop is None else C.byref(_lib.TrainDropout(p=drop[0], seed=drop[1], stream=drop[2]))
        return _call(lambda stream, u, args: fn(stream, u, args, d), unit, a, ws, device)
    if drop is None:
        return _call(lib.bt_train_backward if backward else lib.bt_train_forward, unit, a, ws, device)
    d = _lib.TrainDropout(p=drop[0], seed=drop[1], stream=drop[2])
    fn = lib.bt_train_backward_dropout if backward else lib.bt_train_forward_dropout
    _call(lambda stream, u, args: fn(stream, u, args, C.byref(d)), unit, a, ws, device)


def _grad_like(p: torch.Tensor, wanted: bool):
    return torch.empty(p.shape, dtype=torch.float32, device=p.device) if wanted else None


class AttentionFn(torch.autograd.Function):
    """Attention.forward (roformer.py:114-132) on (B, T, D): the branch without the residual."""

    @staticmethod
    def forward(ctx, x, gamma, w_qkv, w_gates, b_gates, w_out, rope, rope_len, drop=None, mixed=False):
        xf = _f32(x)
        B, T, D = xf.shape
        ps = [_f32(p) for p in (gamma, w_qkv, w_gates, b_gates, w_out)]
        _on_device_of(xf, rope, *ps)
        y = torch.empty_like(xf)
        o = torch.empty_like(xf)
        lse = torch.empty((B, T, D // 32), dtype=torch.float32, device=xf.device)
        a = _args(xf, rope=rope, rope_len=rope_len)
        a.gamma, a.w1, a.w2, a.b2, a.w3 = (p.data_ptr() for p in ps)
        a.y, a.save_o, a.save_lse = y.data_ptr(), o.data_ptr(), lse.data_ptr()
        _run(False, _lib.UNIT_ATTN, a, (B, T, D), 0, xf.device, drop, mixed)
        ctx.save_for_backward(xf, o, lse, rope, *ps)
        ctx.rope_len, ctx.drop, ctx.mixed = rope_len, drop, bool(mixed)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xf, o, lse, rope, gamma, w_qkv, w_gates, b_gates, w_out = ctx.saved_tensors
        B, T, D = xf.shape
        need = ctx.needs_input_grad
        gyf = _f32(gy)
        gx, g_gamma, g_qkv, g_wg, g_bg, g_out = (_grad_like(t, need[i]) for i, t in
                                                 enumerate((xf, gamma, w_qkv, w_gates, b_gates, w_out)))
        a = _args(xf, rope=rope, rope_len=ctx.rope_len)
        a.gamma, a.w1, a.w2, a.b2, a.w3 = (p.data_ptr() for p in (gamma, w_qkv, w_gates, b_gates, w_out))
        a.save_o, a.save_lse, a.gy = o.data_ptr(), lse.data_ptr(), gyf.data_ptr()
        a.gx, a.g_gamma, a.g_w1, a.g_w2, a.g_b2, a.g_w3 = (_lib.ptr(g) for g in (gx, g_gamma, g_qkv, g_wg, g_bg, g_out))
        _run(True, _lib.UNIT_ATTN, a, (B, T, D), 0, xf.device, ctx.drop, ctx.mixed)
        return gx, g_gamma, g_qkv, g_wg, g_bg, g_out, None, None, None, None


class FeedForwardFn(torch.autograd.Function):
    """FeedForward.forward (roformer.py:38-61) on (B, T, D): the branch without the residual."""

    @staticmethod
    def forward(ctx, x, gamma, w1, b1, w2, b2, drop=None, mixed=False):
        xf = _f32(x)
        B, T, D = xf.shape
        ps = [_f32(p) for p in (gamma, w1, b1, w2, b2)]
        _on_device_of(xf, *ps)
        hidden = int(ps[1].shape[0])
        y = torch.empty_like(xf)
        a = _args(xf, hidden=hidden)
        a.gamma, a.w1, a.b1, a.w2, a.b2 = (p.data_ptr() for p in ps)
        a.y = y.data_ptr()
        _run(False, _lib.UNIT_FF, a, (B, T, D), hidden, xf.device, drop, mixed)
        ctx.save_for_backward(xf, *ps)
        ctx.drop, ctx.mixed = drop, bool(mixed)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xf, gamma, w1, b1, w2, b2 = ctx.saved_tensors
        B, T, D = xf.shape
        hidden = int(w1.shape[0])
        gyf = _f32(gy)
        grads = [_grad_like(t, ctx.needs_input_grad[i]) for i, t in enumerate((xf, gamma, w1, b1, w2, b2))]
        a = _args(xf, hidden=hidden)
        a.gamma, a.w1, a.b1, a.w2, a.b2 = (p.data_ptr() for p in (gamma, w1, b1, w2, b2))
        a.gy = gyf.data_ptr()
        a.gx, a.g_gamma, a.g_w1, a.g_b1, a.g_w2, a.g_b2 = (_lib.ptr(g) for g in grads)
        _run(True, _lib.UNIT_FF, a, (B, T, D), hidden, xf.device, ctx.drop, ctx.mixed)
        return (*grads, None, None)


class NormFn(torch.autograd.Function):
    """The trunk's final RMSNorm (roformer.py:22-32, 181)."""

    @staticmethod
    def forward(ctx, x, gamma):
        xf, g = _f32(x), _f32(gamma)
        _on_device_of(xf, g)
        B, T, D = xf.shape
        y = torch.empty_like(xf)
        a = _args(xf)
        a.gamma, a.y = g.data_ptr(), y.data_ptr()
        _call(_lib.lib().bt_train_forward, _lib.UNIT_NORM, a, _workspace(_lib.UNIT_NORM, False, B, T, D, 0, xf.device), xf.device)
        ctx.save_for_backward(xf, g)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xf, gamma = ctx.saved_tensors
        B, T, D = xf.shape
        gyf = _f32(gy)
        gx, g_gamma = _grad_like(xf, ctx.needs_input_grad[0]), _grad_like(gamma, ctx.needs_input_grad[1])
        a = _args(xf)
        a.gamma, a.gy, a.gx, a.g_gamma = gamma.data_ptr(), gyf.data_ptr(), _lib.ptr(gx), _lib.ptr(g_gamma)
        _call(_lib.lib().bt_train_backward, _lib.UNIT_NORM, a, _workspace(_lib.UNIT_NORM, True, B, T, D, 0, xf.device), xf.device)
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
        _call(_lib.lib().bt_train_forward, _lib.TRAIN_UNIT_HEAD, a, _workspace(_lib.TRAIN_UNIT_HEAD, False, B, T, D, 0, xf.device),
              xf.device)
        ctx.save_for_backward(xf, wf, bf)
        ctx.sum_head = int(bool(sum_head))
        ctx.set_materialize_grads(False)   # (a loss on one of the two outputs: the other's gradient is None, not zeros)
        return beat, down

    @staticmethod
    @once_differentiable
    def backward(ctx, g_beat, g_down):
        xf, w, b = ctx.saved_tensors
        B, T, D = xf.shape
        gb = None if g_beat is None else _f32(g_beat)
        gd = None if g_down is None else _f32(g_down)
        gx, gw, gbias = (_grad_like(t, ctx.needs_input_grad[i]) for i, t in enumerate((xf, w, b)))
        a = _args(xf)
        a.sum_head = ctx.sum_head
        a.w1, a.b1, a.gy, a.gy2 = w.data_ptr(), b.data_ptr(), _lib.ptr(gb), _lib.ptr(gd)
        a.gx, a.g_w1, a.g_b1 = _lib.ptr(gx), _lib.ptr(gw), _lib.ptr(gbias)
        _call(_lib.lib().bt_train_backward, _lib.TRAIN_UNIT_HEAD, a, _workspace(_lib.TRAIN_UNIT_HEAD, True, B, T, D, 0, xf.device),
              xf.device)
        return gx, gw, gbias, None


def empty_with_graph(shape, x: torch.Tensor, params) -> torch.Tensor:
    """An empty batch or zero frames: an empty fp32 result that still hangs in the graph, so that ``backward`` runs and leaves
    zero gradients."""
    out = torch.zeros(shape, dtype=torch.float32, device=x.device)
    for t in (x, *params):
        if t.requires_grad and t.is_floating_point():
            out = out + t.reshape(-1)[:0].sum().to(torch.float32)
    return out


def attention(node, x, rope, rope_len, drop=None, mixed=False):
    """``transformer_blocks.layers[l][0]`` of the differentiable route; ``drop``: None or (p, seed, stream); ``mixed``: 16-mixed"""
    return AttentionFn.apply(x, node.norm.gamma, node.to_qkv.weight, node.to_gates.weight, node.to_gates.bias,
                             node.to_out[0].weight, rope, rope_len, drop, mixed)


def feedforward(node, x, drop=None, mixed=False):
    """``transformer_blocks.layers[l][1]``"""
    net = node.net
    return FeedForwardFn.apply(x, net[0].gamma, net[1].weight, net[1].bias, net._modules["4"].weight, net._modules["4"].bias, drop,
                               mixed)


def final_norm(node, x):
    return NormFn.apply(x, node.gamma)


def head(node, x, sum_head: bool):
    lin = node.beat_downbeat_lin
    return HeadFn.apply(x, lin.weight, lin.bias, sum_head)
