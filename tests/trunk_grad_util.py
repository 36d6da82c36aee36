"""The accuracy yardstick of the trunk's backward pass (tests/test_trunk_grad_reference.py, tests/test_gpu_backward.py).

Truth is fp64 autograd through the oracle's restatement of the transformer (oracle/beat_this_oracle.py) plus the head linear,
on the CPU; the reference's own precision is the same computation in fp32.  For one case ``e_ref`` is the LARGEST, over all
gradient tensors, of |g32 - g64| / |g64|; a device gradient passes when |g_dev - g64| / |g64| <= 10 e_ref for every tensor.
The decade covers other summation orders over up to thousands of rows, the device's own exp2 / erf and recomputed
activations; a wrong or missing term is at least four decades above it (test_the_yardstick_discriminates).
"""
import torch

from oracle import beat_this_oracle as O

GATE = 10.0


def rel(a, b):
    """|a - b| / |b| in fp64"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def trainable_keys(sd, prefixes=("transformer_blocks.", "task_heads.")):
    return [k for k in sd if k.startswith(prefixes) and not k.endswith("rotary_embed.freqs")]


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


def head_outputs(h, leaf, sum_head):
    bd = O._linear(h, leaf["task_heads.beat_downbeat_lin.weight"], leaf["task_heads.beat_downbeat_lin.bias"])
    beat, down = bd[..., 0], bd[..., 1]
    return (beat + down if sum_head else beat), down


def oracle_unit_grads(kind, sd, prefix, x, g, dtype, heads=None, sum_head=True):
    """Gradients of sum(unit(x) * g) in ``dtype`` on the CPU.  kind: "attn" / "ff" (the branch without the residual; prefix
    = "transformer_blocks.layers.<l>.<0|1>."), "norm", "head" (g = (g_beat or None, g_downbeat or None))."""
    leaf, xl = _leaves(sd, x, dtype)
    cast = lambda t: t.detach().cpu().to(dtype)
    if kind == "attn":
        loss = (O.attention(xl, leaf, prefix, heads) * cast(g)).sum()
    elif kind == "ff":
        loss = (O.feedforward(xl, leaf, prefix) * cast(g)).sum()
    elif kind == "norm":
        loss = (O.rmsnorm(xl, leaf["transformer_blocks.norm.gamma"]) * cast(g)).sum()
    else:
        beat, down = head_outputs(xl, leaf, sum_head)
        loss = sum((o * cast(w)).sum() for o, w in ((beat, g[0]), (down, g[1])) if w is not None)
    loss.backward()
    keys = [k for k in trainable_keys(sd) if k.startswith(prefix)] if kind in ("attn", "ff") else trainable_keys(sd)
    return _collect(leaf, xl, keys)


def oracle_trunk_forward(leaf, x, n_layers, sum_head=True):
    dim = leaf["transformer_blocks.norm.gamma"].shape[0]
    h = O.transformer(x, leaf, n_layers, dim // 32)
    return head_outputs(h, leaf, sum_head)


def oracle_trunk_grads(sd, x, g_b, g_d, dtype, n_layers, sum_head=True, loss_fn=None):
    """Gradients of sum(beat g_b) + sum(downbeat g_d) -- or of loss_fn(beat, downbeat) -- through transformer_blocks and
    task_heads, in ``dtype`` on the CPU: {"x": .., <state dict key>: ..}."""
    leaf, xl = _leaves(sd, x, dtype)
    beat, down = oracle_trunk_forward(leaf, xl, n_layers, sum_head)
    if loss_fn is not None:
        loss = loss_fn(beat, down)
    else:
        loss = (beat * g_b.detach().cpu().to(dtype)).sum() + (down * g_d.detach().cpu().to(dtype)).sum()
    loss.backward()
    return _collect(leaf, xl, trainable_keys(sd))


def yardstick(g32, g64):
    """e_ref of a case: the worst tensor of the fp32 oracle against the fp64 one"""
    return max(rel(g32[k], g64[k]) for k in g64)


def check(name, dev, g32, g64, report=None):
    """Every device gradient within GATE * e_ref of the fp64 truth; returns (e_ref, worst ratio).  Prints the figures first."""
    e_ref = yardstick(g32, g64)
    errs = {k: rel(dev[k], g64[k]) for k in g64 if k in dev}
    worst_key = max(errs, key=errs.get)
    worst = errs[worst_key] / e_ref
    print(f"{name}: e_ref = {e_ref:.3e}, worst device error = {errs[worst_key]:.3e} ({worst:.2f} x e_ref, {worst_key})")
    if report is not None:
        report(name, e_ref=e_ref, worst_ratio=worst, worst_tensor=worst_key)
    missing = [k for k in g64 if k not in dev]
    assert not missing, f"{name}: no device gradient for {missing}"
    for k, e in errs.items():
        assert torch.isfinite(dev[k]).all(), f"{name}: {k} is not finite"
        assert e <= GATE * e_ref, f"{name}: {k} is {e:.3e} from the fp64 truth, the gate is 10 x e_ref = {GATE * e_ref:.3e}"
    return e_ref, worst
