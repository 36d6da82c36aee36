"""The accuracy yardstick of the frontend's backward pass (tests/test_frontend_grad_reference.py,
tests/test_gpu_frontend_backward.py): trunk_grad_util.py's rule on the oracle's frontend.  Truth is fp64 autograd on the CPU
through ``O.frontend`` / ``O.model_forward`` (or one of its units alone), e_ref the fp32 oracle's worst tensor against it, and a
device tensor passes at <= 10 e_ref (``trunk_grad_util.GATE``, ``trunk_grad_util.check``).

The device's activations are (b, t, f, c), the oracle's (b, c, f, t): the helpers take and return the device's layout.
"""
import torch
import torch.nn.functional as F

import trunk_grad_util as U
from oracle import beat_this_oracle as O

STAT_LEAVES = ("running_mean", "running_var", "num_batches_tracked")


def frontend_keys(sd, prefix="frontend."):
    """the trainable keys below ``prefix``: weights, no rotary tables, no running statistics"""
    return [k for k, v in sd.items() if k.startswith(prefix) and v.is_floating_point() and not k.endswith("rotary_embed.freqs")
            and not k.endswith(STAT_LEAVES)]


def all_keys(sd):
    return frontend_keys(sd) + U.trainable_keys(sd)


def to_oracle(t):   # (b, t, f, c) -> (b, c, f, t)
    return t.permute(0, 3, 2, 1)


def _cast(t, dtype):
    return t.detach().cpu().to(dtype)


def frontend_grads(sd, x, g, dtype):
    """gradients of sum(frontend(x) g) in x and every trainable frontend key"""
    leaf, xl = U._leaves(sd, x, dtype)
    (O.frontend(xl, leaf) * _cast(g, dtype)).sum().backward()
    return U._collect(leaf, xl, frontend_keys(sd))


def model_grads(sd, x, g_b, g_d, dtype, sum_head=True, loss_fn=None):
    """gradients of sum(beat g_b) + sum(downbeat g_d) -- or loss_fn(beat, downbeat) -- through the whole model"""
    leaf, xl = U._leaves(sd, x, dtype)
    dim = leaf["transformer_blocks.norm.gamma"].shape[0]
    n_layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("transformer_blocks.layers."))
    h = O.transformer(O.frontend(xl, leaf), leaf, n_layers, dim // 32)
    beat, down = U.head_outputs(h, leaf, sum_head)
    loss = loss_fn(beat, down) if loss_fn is not None else (beat * _cast(g_b, dtype)).sum() + (down * _cast(g_d, dtype)).sum()
    loss.backward()
    return U._collect(leaf, xl, all_keys(sd))


def stem_grads(sd, x, g, dtype):
    """x (B, T, 128), g (B, T, 32, 32) in (b, t, f, c)"""
    leaf, xl = U._leaves(sd, x, dtype)
    (O.stem(xl, leaf) * to_oracle(_cast(g, dtype))).sum().backward()
    return U._collect(leaf, xl, frontend_keys(sd, "frontend.stem."))


def conv_unit(x, sd, p):
    """blocks.i.conv2d + norm + GELU on the oracle's (b, c, f, t), as O.frontend runs it"""
    y = F.conv2d(x, sd[p + "conv2d.weight"], stride=(2, 1), padding=(0, 1))
    return F.gelu(O.batchnorm(y, sd, p + "norm.", 1))


def conv_grads(sd, i, x, g, dtype):
    """conv unit i: x (B, T, F, C), g (B, T, F / 2, 2 C) in (b, t, f, c); grad x comes back in that layout"""
    p = f"frontend.blocks.{i}."
    leaf, xl = U._leaves(sd, x, dtype)
    (conv_unit(to_oracle(xl), leaf, p) * to_oracle(_cast(g, dtype))).sum().backward()
    return U._collect(leaf, xl, [p + "conv2d.weight", p + "norm.weight", p + "norm.bias"])


def partial_grads(sd, i, x, g, dtype):
    """partial transformer i: x, g (B, T, F, C) in (b, t, f, c)"""
    p = f"frontend.blocks.{i}.partial."
    leaf, xl = U._leaves(sd, x, dtype)
    (O.partial_ft(to_oracle(xl), leaf, p) * to_oracle(_cast(g, dtype))).sum().backward()
    return U._collect(leaf, xl, frontend_keys(sd, p))


def linear_grads(sd, x, g, dtype):
    """concat + frontend.linear: x (B, T, F, C) in (b, t, f, c), g (B, T, D)"""
    leaf, xl = U._leaves(sd, x, dtype)
    b, t, f, c = xl.shape
    rows = xl.permute(0, 1, 3, 2).reshape(b, t, c * f)   # "b c f t -> b t (c f)"
    (O._linear(rows, leaf["frontend.linear.weight"], leaf["frontend.linear.bias"]) * _cast(g, dtype)).sum().backward()
    return U._collect(leaf, xl, ["frontend.linear.weight", "frontend.linear.bias"])


def spect(B, T, seed):
    """inputs uniform in [0, 3)"""
    return torch.rand(B, T, 128, generator=torch.Generator().manual_seed(seed)) * 3
