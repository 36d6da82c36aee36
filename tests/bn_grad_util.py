"""The truth for batch-statistics BatchNorm (tests/test_bn_grad_reference.py, tests/test_gpu_batch_stats.py):
the oracle's frontend with ``oracle.beat_this_oracle.batchnorm`` swapped, for the duration of a call, for
``torch.nn.functional.batch_norm(..., training=True, momentum=0.1, eps=1e-5)`` on CLONES of the running buffers.  The yardstick is
trunk_grad_util.py's: fp64 CPU autograd is the truth, the same computation in fp32 gives e_ref, a device tensor passes at
<= GATE x e_ref.  The moved running buffers are judged by the same rule against the fp64 update, with a floor of 1e-7 on e_ref;
``num_batches_tracked`` exactly.

Every function returns a dict: the outputs under "y" (or "beat" / "downbeat"), the gradients under "x" and their state dict keys
in ``["grads"]``, the buffers after the call in ``["stats"]``.  Activations are taken and returned in the device's (b, t, f, c).
"""
import contextlib

import torch
import torch.nn.functional as F

import front_grad_util as FU
import trunk_grad_util as U
from oracle import beat_this_oracle as O

STAT_FLOOR = 1e-7
BN_PREFIXES = ("frontend.stem.bn1d.", "frontend.stem.bn2d.", "frontend.blocks.0.norm.", "frontend.blocks.1.norm.",
               "frontend.blocks.2.norm.")


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
    """-> a stand-in for O.batchnorm: torch's training-mode BatchNorm; the moved buffers land in ``stats``"""
    def batchnorm(x, sd, pfx, ch_dim):
        assert ch_dim == 1
        mean = sd[pfx + "running_mean"].detach().to(x.dtype).clone()
        var = sd[pfx + "running_var"].detach().to(x.dtype).clone()
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


def _run(sd, x, dtype, keys, forward, batchnorm=None):
    """forward(leaf, xl) -> (outputs, loss); ``batchnorm(stats)``: another stand-in than torch's (the discrimination test)"""
    leaf, xl = U._leaves(sd, x, dtype)
    stats = {}
    with swapped((batchnorm or training_batchnorm)(stats)):
        outs, loss = forward(leaf, xl)
        loss.backward()
    res = {k: v.detach() for k, v in outs.items()}
    res["grads"] = U._collect(leaf, xl, keys)
    res["stats"] = stats
    return res


def _upstream(g, dtype):
    """the upstream gradient in the oracle's (b, c, f, t)"""
    return FU.to_oracle(FU._cast(g, dtype))


def stem(sd, x, g, dtype, batchnorm=None):
    """x (B, T, 128), g (B, T, 32, 32)"""
    def forward(leaf, xl):
        y = O.stem(xl, leaf)
        return {"y": y.permute(0, 3, 2, 1)}, (y * _upstream(g, dtype)).sum()
    return _run(sd, x, dtype, FU.frontend_keys(sd, "frontend.stem."), forward, batchnorm)


def conv(sd, i, x, g, dtype, batchnorm=None):
    """conv unit i: x (B, T, F, C), g (B, T, F / 2, 2 C)"""
    p = f"frontend.blocks.{i}."

    def forward(leaf, xl):
        y = FU.conv_unit(FU.to_oracle(xl), leaf, p)
        return {"y": y.permute(0, 3, 2, 1)}, (y * _upstream(g, dtype)).sum()
    return _run(sd, x, dtype, [p + "conv2d.weight", p + "norm.weight", p + "norm.bias"], forward, batchnorm)


def frontend(sd, x, g, dtype, batchnorm=None):
    """x (B, T, 128), g (B, T, D)"""
    def forward(leaf, xl):
        y = O.frontend(xl, leaf)
        return {"y": y}, (y * FU._cast(g, dtype)).sum()
    return _run(sd, x, dtype, FU.frontend_keys(sd), forward, batchnorm)


def model(sd, x, g_b, g_d, dtype, sum_head=True, loss_fn=None):
    """the whole model: "beat", "downbeat" (B, T) and all its gradients"""
    def forward(leaf, xl):
        dim = leaf["transformer_blocks.norm.gamma"].shape[0]
        n_layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("transformer_blocks.layers."))
        h = O.transformer(O.frontend(xl, leaf), leaf, n_layers, dim // 32)
        beat, down = U.head_outputs(h, leaf, sum_head)
        loss = loss_fn(beat, down) if loss_fn is not None else (beat * FU._cast(g_b, dtype)).sum() + (down * FU._cast(g_d, dtype)).sum()
        return {"beat": beat, "downbeat": down}, loss
    return _run(sd, x, dtype, FU.all_keys(sd), forward)


def check(name, dev_grads, dev_stats, r32, r64, report=None):
    """The gradients through trunk_grad_util.check; every moved running buffer within GATE x max(e_ref, 1e-7) of the fp64 update,
    e_ref that buffer's fp32 error; the counters exactly.  Prints each figure before it asserts; -> (e_ref, worst gradient ratio,
    worst buffer ratio)."""
    e_ref, worst = U.check(name, dev_grads, r32["grads"], r64["grads"], report)
    worst_stat = 0.0
    for k, want in r64["stats"].items():
        assert k in dev_stats, f"{name}: no device value for {k}"
        if k.endswith("num_batches_tracked"):
            assert int(dev_stats[k]) == int(want), f"{name}: {k} is {int(dev_stats[k])}, expected {int(want)}"
            continue
        e = max(U.rel(r32["stats"][k], want), STAT_FLOOR)
        err = U.rel(dev_stats[k], want)
        worst_stat = max(worst_stat, err / e)
        print(f"{name}: {k} e_ref = {e:.3e}, device error = {err:.3e} ({err / e:.2f} x)")
        assert torch.isfinite(dev_stats[k]).all() and err <= U.GATE * e, f"{name}: {k} is {err:.3e} from the fp64 update, gate {U.GATE * e:.3e}"
    if report is not None:
        report(name + " running statistics", worst_ratio=worst_stat)
    return e_ref, worst, worst_stat
