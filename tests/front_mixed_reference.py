"""The arithmetic contract of 16-mixed in the differentiable frontend (include/beat_this_amd.h) restated in
torch on the CPU, in any float dtype, on top of mixed_reference.py: the conv unit's three products as a custom autograd Function
(forward conv2d(r16(x), r16(w)); backward conv2d_input(r16(w), r16(g)) and conv2d_weight(r16(x), r16(g)), g being the gradient at
the convolution's output, i.e. g_pre s multiplied in the working dtype first), the partial transformers over
``mixed_reference.attention`` / ``feedforward`` with their residual, the projection over ``mixed_reference.linear``; the stem is
the oracle's (fp32 on the device too).  ``on=False`` switches the rounding off, ``on=None`` runs the oracle itself.

Also here: the cases of tests/test_gpu_front_mixed.py with their inputs, and ``e_ref16`` -- the worst gradient tensor's relative
distance from fp64 autograd of the fp32 oracle run under ``torch.autocast("cpu", dtype=torch.float16)`` with the upstream gradient
(or the loss) multiplied by the loss scale and the result divided by it.  The scale is 65536 for the unit cases; for a
whole-model case it is the largest power of two <= 65536 at which every gradient of the autocast oracle is finite (where a
GradScaler settles; at 65536 the autocast oracle's frontend gradients overflow and the gate would say nothing).  The device is
fed the same scale.

Activations are taken and returned in the device's (b, t, f, c); the oracle's are (b, c, f, t).
"""
import contextlib

import torch
import torch.nn.functional as F

import bn_grad_util as BU
import front_grad_util as FU
import mixed_reference as R
import trunk_grad_util as U
from oracle import beat_this_oracle as O

SCALE = R.SCALE
GATE_CPU = 1.5          # the restatement alone, in fp32, against e_ref16 (test_front_mixed_reference.py)
HP = dict(transformer_dim=64, ff_mult=2, n_layers=2)
WEIGHT_SEED = 3


class _Conv(torch.autograd.Function):
    """the conv unit's convolution on (b, c, f, t): kernel (2, 3), stride (2, 1), padding (0, 1), both operands of each of its
    three products rounded"""

    @staticmethod
    def forward(ctx, x, w, on):
        ctx.save_for_backward(x, w)
        ctx.on = on
        return F.conv2d(R.r16(x, on), R.r16(w, on), stride=(2, 1), padding=(0, 1))

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gr = R.r16(g, ctx.on)
        gx = torch.nn.grad.conv2d_input(x.shape, R.r16(w, ctx.on), gr, stride=(2, 1), padding=(0, 1))
        gw = torch.nn.grad.conv2d_weight(R.r16(x, ctx.on), w.shape, gr, stride=(2, 1), padding=(0, 1))
        return gx, gw, None


def conv_unit(x, sd, p, on):
    """blocks.i.conv2d + norm + GELU on (b, c, f, t); BatchNorm and GELU in the working dtype (``O.batchnorm`` is looked up at
    call time: bn_grad_util.swapped puts the training-mode one there)"""
    if on is None:
        return FU.conv_unit(x, sd, p)
    return F.gelu(O.batchnorm(_Conv.apply(x, sd[p + "conv2d.weight"], on), sd, p + "norm.", 1))


def partial_ft(x, sd, pfx, on):
    """O.partial_ft with the leaves under the contract"""
    if on is None:
        return O.partial_ft(x, sd, pfx)
    b, c, f, t = x.shape
    heads = c // 32
    y = x.permute(0, 3, 2, 1).reshape(b * t, f, c)
    y = y + R.attention(y, sd, pfx + "attnF.", heads, on)
    y = y + R.feedforward(y, sd, pfx + "ffF.", on)
    y = y.view(b, t, f, c).permute(0, 2, 1, 3).reshape(b * f, t, c)
    y = y + R.attention(y, sd, pfx + "attnT.", heads, on)
    y = y + R.feedforward(y, sd, pfx + "ffT.", on)
    return y.view(b, f, t, c).permute(0, 3, 1, 2)


def projection(x, sd, on):
    """(b, c, f, t) -> (b, t, D)"""
    b, c, f, t = x.shape
    rows = x.permute(0, 3, 1, 2).reshape(b, t, c * f)
    w, bias = sd["frontend.linear.weight"], sd["frontend.linear.bias"]
    return O._linear(rows, w, bias) if on is None else R.linear(rows, w, bias, on)


def frontend(x, sd, on):
    if on is None:
        return O.frontend(x, sd)
    h = O.stem(x, sd)
    for i in range(3):
        p = f"frontend.blocks.{i}."
        if p + "partial.attnF.norm.gamma" in sd:
            h = partial_ft(h, sd, p + "partial.", on)
        h = conv_unit(h, sd, p, on)
    return projection(h, sd, on)


def model(x, sd, on):
    """(beat, downbeat), summing head"""
    n_layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("transformer_blocks.layers."))
    h = frontend(x, sd, on)
    return U.oracle_trunk_forward(sd, h, n_layers) if on is None else R.trunk_forward(sd, h, n_layers, on)


def training_batchnorm(stats):
    """bn_grad_util.training_batchnorm with the running buffers kept in fp32 when the input is fp16 (under autocast a
    BatchNorm's buffers and parameters stay fp32, as in the reference's 16-mixed run; torch's CPU kernel takes that mixture and
    no other)"""
    def batchnorm(x, sd, pfx, ch_dim):
        assert ch_dim == 1
        dt = torch.float32 if x.dtype == torch.float16 else x.dtype
        mean = sd[pfx + "running_mean"].detach().to(dt).clone()
        var = sd[pfx + "running_var"].detach().to(dt).clone()
        y = F.batch_norm(x, mean, var, sd[pfx + "weight"], sd[pfx + "bias"], training=True, momentum=0.1, eps=1e-5)
        stats[pfx + "running_mean"], stats[pfx + "running_var"] = mean, var
        if pfx + "num_batches_tracked" in sd:
            stats[pfx + "num_batches_tracked"] = sd[pfx + "num_batches_tracked"].detach().clone() + 1
        return BU._PlainGrad.apply(y)
    return batchnorm


# ---- gradients ------------------------------------------------------------------------------------------------------------------
def _run(sd, x, keys, dtype, forward, scale=1.0, autocast=False, batch=False):
    """forward(leaf, xl) -> (outputs, loss).  -> {"x", <key>: gradient of loss (taken of loss * scale and divided by scale),
    <output name>: value, "stats": the moved running buffers with ``batch``}"""
    leaf, xl = U._leaves(sd, x, dtype)
    stats = {}
    with (BU.swapped(training_batchnorm(stats)) if batch else contextlib.nullcontext()):
        with torch.autocast("cpu", dtype=torch.float16, enabled=autocast):
            outs, loss = forward(leaf, xl)
            (loss * scale).backward()
    res = {k: v / scale for k, v in U._collect(leaf, xl, keys).items()}
    res.update({k: v.detach() for k, v in outs.items()})
    res["stats"] = stats
    return res


def conv_grads(sd, i, x, g, dtype, on, scale=1.0, autocast=False, batch=False):
    p = f"frontend.blocks.{i}."

    def forward(leaf, xl):
        y = conv_unit(FU.to_oracle(xl), leaf, p, on).to(dtype)
        return {"y": y.permute(0, 3, 2, 1)}, (y * FU.to_oracle(g.to(dtype))).sum()
    return _run(sd, x, [p + "conv2d.weight", p + "norm.weight", p + "norm.bias"], dtype, forward, scale, autocast, batch)


def partial_grads(sd, i, x, g, dtype, on, scale=1.0, autocast=False):
    p = f"frontend.blocks.{i}.partial."

    def forward(leaf, xl):
        y = partial_ft(FU.to_oracle(xl), leaf, p, on).to(dtype)
        return {"y": y.permute(0, 3, 2, 1)}, (y * FU.to_oracle(g.to(dtype))).sum()
    return _run(sd, x, FU.frontend_keys(sd, p), dtype, forward, scale, autocast)


def linear_grads(sd, x, g, dtype, on, scale=1.0, autocast=False):
    def forward(leaf, xl):
        y = projection(FU.to_oracle(xl), leaf, on).to(dtype)
        return {"y": y}, (y * g.to(dtype)).sum()
    return _run(sd, x, ["frontend.linear.weight", "frontend.linear.bias"], dtype, forward, scale, autocast)


def model_grads(sd, x, loss_fn, dtype, on, scale=1.0, autocast=False):
    def forward(leaf, xl):
        beat, down = model(xl, leaf, on)
        beat, down = beat.to(dtype), down.to(dtype)
        return {"beat": beat, "downbeat": down}, loss_fn(beat, down)
    return _run(sd, x, FU.all_keys(sd), dtype, forward, scale, autocast)


def grad_keys(d):
    return [k for k in d if k not in ("y", "beat", "downbeat", "stats")]


def worst(got, truth):
    return R.worst(got, truth, grad_keys(truth))


# ---- the cases of tests/test_gpu_front_mixed.py ------------------------------------------------------------------------------------
CONV_SIZES = ((1, 1), (1, 2), (2, 3), (1, 63), (1, 64), (1, 65), (2, 65), (2, 150))
BN_SIZES = ((2, 3), (2, 65), (2, 1))
LINEAR_SIZES = ((2, 3), (2, 65), (2, 600))
PARTIAL_SIZES = ((2, 3), (2, 65))
MODEL_SIZES = ((2, 150), (2, 33))
MODEL_SEEDS = {True: 62, False: 61}     # with / without partial transformers
_SD, _CASES = {}, {}


def state_dict(style="lively", partial=True):
    from beat_this_amd import weights as W

    if (style, partial) not in _SD:
        _SD[style, partial] = W.random_state_dict(W.resolve_hparams(dict(HP, partial_transformers=partial)), seed=WEIGHT_SEED,
                                                  style=style)
    return _SD[style, partial]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def conv_inputs(i, B, T):
    F_, C_ = 32 >> i, 32 << i
    gen = _gen(100 * i + 10 * T + B)
    x = torch.rand(B, T, F_, C_, generator=gen) * 3
    return x, torch.randn(B, T, F_ // 2, 2 * C_, generator=gen) * 2.0 ** -14


def partial_inputs(i, B, T):
    F_, C_ = 32 >> i, 32 << i
    gen = _gen(1000 * i + 10 * T + B)
    x = torch.randn(B, T, F_, C_, generator=gen)
    return x, torch.randn(B, T, F_, C_, generator=gen) * 2.0 ** -14


def linear_inputs(B, T):
    """the projection's own (the cases above leave them open): the last conv unit's output shape at width 64"""
    gen = _gen(5000 + 10 * T + B)
    x = torch.randn(B, T, 4, 256, generator=gen)
    return x, torch.randn(B, T, 64, generator=gen) * 2.0 ** -14


def model_inputs(B, T, partial):
    gen = _gen(MODEL_SEEDS[partial])
    x = torch.rand(B, T, 128, generator=gen) * 3
    beat = (torch.rand(B, T, generator=gen) < 0.06).float()
    down = beat * (torch.rand(B, T, generator=gen) < 0.3).float()
    mask = torch.ones(B, T)
    mask[0, 3 * T // 4:] = 0
    mask[1, T // 3:] = 0
    return x, beat, down, mask


def _case(key, make):
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


def _unit_case(fn, sd, x, g, **kw):
    truth = fn(sd, x, g, torch.float64, None, **kw)
    auto = fn(sd, x, g, torch.float32, None, SCALE, autocast=True, **kw)
    return dict(sd=sd, x=x, g=g, truth=truth, auto=auto, scale=SCALE, e_ref16=worst(auto, truth)[0])


def conv_case(i, B, T, batch=False):
    """-> dict(sd, x, g, truth (fp64 oracle), auto (the autocast oracle), scale, e_ref16)"""
    x, g = conv_inputs(i, B, T)
    fn = lambda *a, **kw: conv_grads(a[0], i, *a[1:], **kw)
    return _case(("conv", i, B, T, batch), lambda: _unit_case(fn, state_dict(), x, g, batch=batch))


def partial_case(i, B, T):
    x, g = partial_inputs(i, B, T)
    fn = lambda *a, **kw: partial_grads(a[0], i, *a[1:], **kw)
    return _case(("partial", i, B, T), lambda: _unit_case(fn, state_dict(), x, g))


def linear_case(B, T):
    x, g = linear_inputs(B, T)
    return _case(("linear", B, T), lambda: _unit_case(linear_grads, state_dict(), x, g))


def model_case(style, partial, B, T):
    """-> dict(sd, x, beat, down, mask, loss_fn, truth, auto, scale, e_ref16); the scale is searched downwards from 65536"""
    def make():
        sd = state_dict(style, partial)
        x, beat, down, mask = model_inputs(B, T, partial)
        loss_fn = R.trunk_loss(beat, down, mask)
        truth = model_grads(sd, x, loss_fn, torch.float64, None)
        scale = SCALE
        while True:
            auto = model_grads(sd, x, loss_fn, torch.float32, None, scale, autocast=True)
            if all(bool(torch.isfinite(auto[k]).all()) for k in grad_keys(truth)) or scale <= 1.0:
                break
            scale /= 2.0
        return dict(sd=sd, x=x, beat=beat, down=down, mask=mask, loss_fn=loss_fn, truth=truth, auto=auto, scale=scale,
                    e_ref16=worst(auto, truth)[0])
    return _case(("model", style, partial, B, T), make)


def restate(case, kind, *ident, dtype=torch.float32, on=True, batch=False):
    """the restatement (or, on = None, the oracle) on a case's inputs at the case's scale"""
    sd, scale = case["sd"], case["scale"]
    if kind == "conv":
        return conv_grads(sd, ident[0], case["x"], case["g"], dtype, on, scale, batch=batch)
    if kind == "partial":
        return partial_grads(sd, ident[0], case["x"], case["g"], dtype, on, scale)
    if kind == "linear":
        return linear_grads(sd, case["x"], case["g"], dtype, on, scale)
    return model_grads(sd, case["x"], case["loss_fn"], dtype, on, scale)
