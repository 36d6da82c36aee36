"""The contract of the averaging AdamW step (include/beat_this_amd.h) restated in numpy, and its yardstick.

``EmaReference`` does what bt_adamw_ema_step does, one rounded fp32 operation at a time: the AdamW element update with the
per-group scalars computed in fp64 and rounded once, then the average from the new parameter -- a copy on the first step taken,
e + (p - e) * w with w = fp32(1 - decay) afterwards -- and nothing at all on a skipped step.  It knows nothing of the package.

``yardstick``: the truth is an fp64 AdamW plus an fp64 EMA over the same fp32 gradients; e_ref is the relative L2 distance, over
the displacement from p0, of torch's own fp32 path (``torch.optim.AdamW`` followed by ``AveragedModel(multi_avg_fn=
get_ema_multi_avg_fn(decay)).update_parameters``) from that truth.  The code under test has to be within 2 e_ref, the gate of
tests/test_optim.py for the step, for the same reason: torch's CPU lerp contracts to an FMA and the contract here does not.
"""
import math

import numpy as np
import torch

F = np.float32


def group_scalars(settings, t):
    """decay, 1 - beta1, beta2, 1 - beta2, step size, sqrt of the second bias correction, eps: fp64, rounded to fp32 once"""
    lr, (b1, b2), eps, wd = float(settings["lr"]), settings["betas"], float(settings["eps"]), float(settings["weight_decay"])
    return dict(decay=F(1.0 - lr * wd), omb1=F(1.0 - b1), b2=F(b2), omb2=F(1.0 - b2), step_size=F(lr / (1.0 - b1 ** t)),
                bias2_sqrt=F(math.sqrt(1.0 - b2 ** t)), eps=F(eps))


class EmaReference:
    """parameters (a list of fp32 arrays, copied), the group index of each, the groups' settings, the decay"""

    def __init__(self, params, groups, settings, decay):
        self.p = [np.array(p, dtype=F).ravel().copy() for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.e = [np.zeros_like(p) for p in self.p]
        self.groups, self.settings = list(groups), settings
        self.w = F(1.0 - float(decay))
        self.t = self.n_averaged = 0

    def step(self, grads, grad_scale=1.0, coef=None, skipped=False):
        if skipped:   # (the loss scaler found a non-finite gradient: nothing moves, nothing is counted)
            return
        self.t += 1
        gs = F(grad_scale) if coef is None else F(grad_scale) * F(coef)
        with np.errstate(all="ignore"):
            for i, grad in enumerate(grads):
                h = group_scalars(self.settings[self.groups[i]], self.t)
                g = np.asarray(grad, dtype=F).ravel() * gs
                p = self.p[i] * h["decay"]
                m = self.m[i] + (g - self.m[i]) * h["omb1"]
                v = self.v[i] * h["b2"] + (g * g) * h["omb2"]
                denom = np.sqrt(v) / h["bias2_sqrt"] + h["eps"]
                p = p - h["step_size"] * (m / denom)
                self.p[i], self.m[i], self.v[i] = p, m, v
                self.e[i] = p.copy() if self.n_averaged == 0 else self.e[i] + (p - self.e[i]) * self.w
                assert p.dtype == F and self.e[i].dtype == F
        self.n_averaged += 1


def adamw_ema64(p0, grads, settings, decay):
    """fp64 AdamW (torch.optim.AdamW's defaults) and fp64 EMA over the fp32 gradients of every step -> (p, e)"""
    lr, (b1, b2), eps, wd = settings["lr"], settings["betas"], settings["eps"], settings["weight_decay"]
    p = p0.astype(np.float64)
    m, v, e = np.zeros_like(p), np.zeros_like(p), None
    for t, g32 in enumerate(grads, 1):
        g = g32.astype(np.float64)
        p = p * (1 - lr * wd)
        m = m + (g - m) * (1 - b1)
        v = v * b2 + g * g * (1 - b2)
        p = p - lr / (1 - b1 ** t) * (m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps))
        e = p.copy() if e is None else e + (p - e) * (1 - decay)
    return p, e


def torch_adamw_ema32(p0, grads, settings, decay):
    """torch's own fp32 path on the CPU -> the averaged parameter"""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

    net = torch.nn.Module()
    net.w = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.AdamW([net.w], foreach=False, **settings)
    avg = AveragedModel(net, multi_avg_fn=get_ema_multi_avg_fn(decay))
    for g in grads:
        net.w.grad = torch.from_numpy(g.copy())
        opt.step()
        avg.update_parameters(net)
    assert int(avg.n_averaged) == len(grads)
    return avg.module.w.detach().numpy()


def rel(a, truth):
    return float(np.linalg.norm(a.astype(np.float64) - truth) / np.linalg.norm(truth))


def yardstick(p0, grads, settings, decay):
    """-> (e_ref, measure): e_ref as above; measure(e32) is the same distance of another fp32 average"""
    _, e64 = adamw_ema64(p0, grads, settings, decay)
    d64 = e64 - p0.astype(np.float64)
    measure = lambda e32: rel(np.asarray(e32).astype(np.float64) - p0.astype(np.float64), d64)
    return measure(torch_adamw_ema32(p0, grads, settings, decay)), measure
