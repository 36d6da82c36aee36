"""No-GPU checks of weight averaging (csrc/optim.hip through bt_adamw_ema_step_host, beat_this_amd/optim.py).

1. The host twin against bt_adamw_step_host (p, m, v: the same bits) and against the numpy restatement of the contract
   (tests/ema_reference.py: the average, bit for bit), over 1, 2 and 20 steps of one plan whose tensor sizes sit on both sides of
   the chunk and of the 16-byte access width, with a view at a 4-byte offset, two groups and a clip coefficient.
2. The yardstick of tests/ema_reference.py: the twin within 2 e_ref of an fp64 AdamW + EMA, e_ref being torch's own fp32 path.
3. Refusals, ``averaged_checkpoint``, the command lines and the binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ema_reference as R
from conftest import ROOT


def _L():
    from beat_this_amd import _lib as L

    L.build()
    return L


def _optim():
    _L()
    from beat_this_amd import optim

    return optim


CHUNK = 4096
SIZES = [0, 1, 3, 4, 5, 1023, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7, CHUNK + 6]
VIEW_AT = len(SIZES) - 1   # this parameter starts 4 bytes into its buffer: the one-element path of the device kernel
DEFAULTS = dict(lr=8e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
SETTINGS = [dict(DEFAULTS), dict(DEFAULTS, lr=2e-4, weight_decay=0.0)]
GROUPS = [i % 2 for i in range(len(SIZES))]
DECAY, COEF, POISON = 0.9, 0.37, 0xFF


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


class Plan:
    """the parameters of SIZES as numpy arrays (one of them a view at a 4-byte offset), flat buffers, the planner's tables"""

    def __init__(self, seed=0):
        O = _optim()
        rng = np.random.default_rng(seed)
        self.bufs = [(rng.standard_normal(n + 4) * 0.05).astype(np.float32) for n in SIZES]
        self.params = [b[1:1 + n] if i == VIEW_AT else b[:n] for i, (b, n) in enumerate(zip(self.bufs, SIZES))]
        assert self.params[VIEW_AT].ctypes.data % 16 == 4
        self.tensors, self.chunks, self.total, self.n_chunks = O.plan([p.ctypes.data for p in self.params], SIZES, GROUPS, 2)
        self.offsets = [int(self.tensors[i].offset) for i in range(len(SIZES))]
        self.grad, self.m, self.v = (np.zeros(self.total, np.float32) for _ in range(3))
        self.ema = np.frombuffer(bytes([POISON]) * (4 * self.total), np.float32).copy()
        self.covered = np.zeros(self.total, bool)
        for o, n in zip(self.offsets, SIZES):
            self.covered[o:o + n] = True

    def set_grads(self, grads):
        self.grad[:] = 0
        for o, g in zip(self.offsets, grads):
            self.grad[o:o + g.size] = g

    def part(self, buf, i):
        return buf[self.offsets[i]:self.offsets[i] + SIZES[i]]


def gradients(steps, seed=1, scale=1e-2):
    rng = np.random.default_rng(seed)
    return [[(rng.standard_normal(n) * scale).astype(np.float32) for n in SIZES] for _ in range(steps)]


@pytest.mark.parametrize("steps", [1, 2, 20])
def test_host_twin_equals_the_plain_twin_and_the_restatement(steps):
    O = _optim()
    ema, plain = Plan(), Plan()
    ref = R.EmaReference(ema.params, GROUPS, SETTINGS, DECAY)
    for t, grads in enumerate(gradients(steps), 1):
        coef = COEF if t % 2 else None   # (a clip coefficient on every other step)
        h = O.hyper(SETTINGS, t, grad_scale=0.5)
        ema.set_grads(grads)
        plain.set_grads(grads)
        O.adamw_ema_step_host(ema.tensors, len(SIZES), ema.chunks, ema.n_chunks, ema.grad, ema.m, ema.v, ema.ema, h, 1.0 - DECAY,
                              t == 1, coef=coef)
        O.adamw_step_host(plain.tensors, len(SIZES), plain.chunks, plain.n_chunks, plain.grad, plain.m, plain.v, h, coef=coef)
        ref.step(grads, grad_scale=0.5, coef=coef)
        assert not ema.grad.any()
    assert ref.n_averaged == steps
    for name in ("m", "v"):
        assert np.array_equal(bits(getattr(ema, name)), bits(getattr(plain, name))), name
    for i in range(len(SIZES)):
        assert np.array_equal(bits(ema.bufs[i]), bits(plain.bufs[i])), f"parameter {i} differs from bt_adamw_step_host"
        assert np.array_equal(bits(ema.params[i]), bits(ref.p[i])), f"parameter {i} differs from the restatement"
        assert np.array_equal(bits(ema.part(ema.ema, i)), bits(ref.e[i])), f"average {i} differs from the restatement"
    assert (ema.ema[~ema.covered].view(np.uint8) == POISON).all(), "padding of the averages written"
    assert np.isfinite(ema.ema[ema.covered]).all()
    if steps > 1:   # (the average is not the last iterate)
        assert not np.array_equal(ema.part(ema.ema, 7), ema.params[7])
    else:
        assert all(np.array_equal(bits(ema.part(ema.ema, i)), bits(ema.params[i])) for i in range(len(SIZES)))


def test_a_copying_step_ignores_the_old_average_and_a_decay_of_zero_follows_the_weights():
    O = _optim()
    a = Plan()
    ref = R.EmaReference(a.params, GROUPS, SETTINGS, 0.0)
    for t, grads in enumerate(gradients(3, seed=2), 1):
        a.set_grads(grads)
        O.adamw_ema_step_host(a.tensors, len(SIZES), a.chunks, a.n_chunks, a.grad, a.m, a.v, a.ema, O.hyper(SETTINGS, t), 1.0, t == 1)
        ref.step(grads)
    for i in range(len(SIZES)):   # weight 1: e + (p - e) is p only up to the roundings of the two operations, restated exactly
        assert np.array_equal(bits(a.part(a.ema, i)), bits(ref.e[i]))
        assert np.abs(a.part(a.ema, i) - a.params[i]).max(initial=0.0) <= 2.0 ** -23 * 0.5   # (|p|, |e| < 0.5 here: an ulp of 0.25)
    b = Plan()
    b.set_grads(gradients(1, seed=2)[0])
    O.adamw_ema_step_host(b.tensors, len(SIZES), b.chunks, b.n_chunks, b.grad, b.m, b.v, b.ema, O.hyper(SETTINGS, 1), 0.25, True)
    for i in range(len(SIZES)):   # (the poison of the old average, NaN, did not leak into the copy)
        assert np.array_equal(bits(b.part(b.ema, i)), bits(b.params[i]))


YARD = [(decay, steps, lr) for decay in (0.9, 0.999, 0.9999) for steps in (2, 20, 200) for lr in (1e-3, 1e-5)] + [(0.9999, 1000, 1e-5)]


@pytest.mark.parametrize("decay,steps,lr", YARD)
def test_twin_against_the_fp64_yardstick(decay, steps, lr):
    O = _optim()
    n = CHUNK + 1000
    settings = dict(DEFAULTS, lr=lr)
    rng = np.random.default_rng(3)
    p = (rng.standard_normal(n) * 0.05).astype(np.float32)
    p0 = p.copy()
    grads = [(rng.standard_normal(n) * 1e-3).astype(np.float32) for _ in range(steps)]
    tensors, chunks, total, n_chunks = O.plan([p.ctypes.data], [n], [0], 1)
    grad, m, v, ema = (np.zeros(total, np.float32) for _ in range(4))
    ref = R.EmaReference([p0], [0], [settings], decay)
    for t, g in enumerate(grads, 1):
        grad[:n] = g
        O.adamw_ema_step_host(tensors, 1, chunks, n_chunks, grad, m, v, ema, O.hyper([settings], t), 1.0 - decay, t == 1)
        ref.step([g])
    e_ref, measure = R.yardstick(p0, grads, settings, decay)
    e_twin, e_restated = measure(ema[:n]), measure(ref.e[0])
    print(f"decay {decay}, {steps} steps, lr {lr:g}: e_ref {e_ref:.3e}, twin {e_twin:.3e} = {e_twin / e_ref:.3f} e_ref, "
          f"restatement {e_restated / e_ref:.3f} e_ref")
    assert np.array_equal(bits(ema[:n]), bits(ref.e[0]))
    assert e_twin <= 2 * e_ref, (e_twin, e_ref)


def test_refusals():
    L = _L()
    O = _optim()
    lib, ARG = L.lib(), L.BT_ERR_ARG
    buf = np.zeros(64, np.float32)
    a = buf.ctypes.data
    assert a % 16 == 0
    tensors, chunks, total, n_chunks = O.plan([a, a + 128], [8, 8], [0, 1], 2)
    h = O.hyper([DEFAULTS, DEFAULTS], 1)
    good = [C.addressof(tensors), 2, C.addressof(chunks), 2, a, a, a, a, 16, C.byref(h), None, 0.1, 0]
    twin = lib.bt_adamw_ema_step_host
    device = lambda *args: lib.bt_adamw_ema_step(None, *args)   # (refused before anything is launched: no GPU needed)
    for fn in (twin, device):
        for w in (0.0, 1.5, -0.1, float("nan"), float("inf")):
            for copy in (0, 1):
                assert fn(*(good[:11] + [w, copy])) == ARG and b"ema_weight" in lib.bt_last_error(), (w, copy)
        for i in (0, 2, 4, 5, 6, 7, 9):
            bad = list(good)
            bad[i] = None
            assert fn(*bad) == ARG, i
        for i in (4, 5, 6, 7):
            bad = list(good)
            bad[i] = a + 4
            assert fn(*bad) == ARG and b"16-byte" in lib.bt_last_error(), i
        assert fn(*(good[:8] + [15] + good[9:])) == ARG
    assert twin(*good) == L.BT_OK and twin(*(good[:11] + [1.0, 1])) == L.BT_OK
    swap = lambda *args: lib.bt_ema_exchange(None, *args)
    ok = [C.addressof(tensors), 2, C.addressof(chunks), 2, a, 16]
    for i in (0, 2, 4):
        bad = list(ok)
        bad[i] = None
        assert swap(*bad) == ARG, i
    assert swap(*(ok[:4] + [a + 4, 16])) == ARG and b"16-byte" in lib.bt_last_error()
    assert swap(*(ok[:5] + [15])) == ARG and swap(*(ok[:3] + [-1] + ok[4:])) == ARG


def test_averaged_checkpoint():
    _L()
    import torch

    from beat_this_amd.inference import averaged_checkpoint

    live, avg = {"model.w": torch.ones(3)}, {"model.w": torch.zeros(3)}
    ckpt = {"state_dict": live, "ema_state_dict": avg, "hyper_parameters": {"n_layers": 2}, "epoch": 4}
    out = averaged_checkpoint(ckpt)
    assert out["state_dict"] is avg and "ema_state_dict" not in out
    assert out["hyper_parameters"] == {"n_layers": 2} and out["epoch"] == 4
    assert ckpt["state_dict"] is live and "ema_state_dict" in ckpt   # (the input is left as it was)
    with pytest.raises(ValueError, match="ema_state_dict"):
        averaged_checkpoint({"state_dict": live, "hyper_parameters": {}})


def test_command_lines():
    _L()
    from beat_this_amd import evaluate, train

    base = ["--data-dir", "d", "--output", "o"]
    assert train.get_parser().parse_args(base).ema_decay is None
    assert train.get_parser().parse_args(base + ["--ema-decay", "0.999"]).ema_decay == 0.999
    assert train.get_parser().parse_args(base + ["--ema-decay", "0"]).ema_decay == 0.0
    for bad in ("1.0", "-0.1", "nan"):
        with pytest.raises(SystemExit):
            train.get_parser().parse_args(base + ["--ema-decay", bad])
    ev = ["--models", "m.ckpt", "--bundle", "b.npz", "--annotations", "a"]
    assert evaluate.get_parser().parse_args(ev).ema is False and evaluate.get_parser().parse_args(ev + ["--ema"]).ema is True


def test_optimizer_refuses_a_bad_decay_before_it_looks_at_the_parameters():
    O = _optim()
    import torch

    for bad in (1.0, -0.01, 2, float("nan"), "0.9", True):
        with pytest.raises(ValueError, match="ema_decay"):
            O.AdamW([torch.nn.Parameter(torch.zeros(4))], ema_decay=bad)


def test_binding_and_header_list_the_exports():
    L = _L()
    header = open(os.path.join(ROOT, "include", "beat_this_amd.h")).read()
    declared = set(re.findall(r"\b(bt_[a-z_0-9]+)\s*\(", header))
    new = {"bt_adamw_ema_step", "bt_adamw_ema_step_host", "bt_ema_exchange"}
    assert new <= declared and new <= set(L.EXPORTS) and set(L.EXPORTS) == declared
    for name in new:
        assert hasattr(L.lib(), name)
    assert L.lib().bt_version() == 600 == L.ABI_VERSION and CHUNK == L.OPTIM_CHUNK
    assert len(L.EXPORTS["bt_adamw_ema_step"][1]) == 14 and len(L.EXPORTS["bt_adamw_ema_step_host"][1]) == 13
    assert len(L.EXPORTS["bt_ema_exchange"][1]) == 7
