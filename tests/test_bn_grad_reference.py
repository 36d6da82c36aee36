"""CPU side of batch-statistics BatchNorm: the binding of the bt_front_bn_* entry points, what they refuse
before any launch, the opt-in's bookkeeping, the command line, and the yardstick of route_grads.py shown to discriminate the
three mistakes a training-mode BatchNorm makes most easily."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

import route_cases as RC
import route_grads as RG
from conftest import ROOT
from route_harness import MODEL_KEYS
from beat_this_amd import weights as W

HP = dict(transformer_dim=64, ff_mult=2, n_layers=2)
NEW = ("bt_front_bn_struct_sizes", "bt_front_bn_workspace_bytes", "bt_front_bn_forward", "bt_front_bn_backward")


def new_model(**more):
    from beat_this_amd.model import BeatThis

    hp = W.resolve_hparams(dict(HP, **more))
    return BeatThis(**{k: hp[k] for k in MODEL_KEYS})


def test_binding_of_the_batch_statistics_entry_points():
    from beat_this_amd import _lib as L

    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "beat_this_amd.h")).read()
    assert re.search(r"#define BT_ABI_VERSION 600\b", header) and lib.bt_version() == 600
    P = C.POINTER(L.FrontBnArgs)
    assert L.EXPORTS["bt_front_bn_forward"] == (C.c_int, [C.c_void_p, C.c_int, P])
    assert L.EXPORTS["bt_front_bn_backward"] == (C.c_int, [C.c_void_p, C.c_int, P])
    assert L.EXPORTS["bt_front_bn_workspace_bytes"] == (C.c_size_t, [C.c_int] * 6)
    for name in NEW:
        assert hasattr(lib, name) and re.search(r"\b%s\(" % name, header), name
    assert "} bt_front_bn_args;" in header
    out = (C.c_int32 * 9)()
    lib.bt_front_bn_struct_sizes(out)
    T = L.FrontBnArgs
    assert list(out) == [C.sizeof(T), T.w.offset, T.bn_tracked.offset, T.save_mean.offset, T.x.offset, T.gy.offset, T.gx.offset,
                         T.ws.offset, T.ws_bytes.offset]


def test_workspace_queries():
    """multiples of 256 bytes, non-decreasing in B and T; 8 x 1500 frames are inside the limits"""
    from beat_this_amd import _lib as L

    lib = L.lib()
    for unit, F_, C_ in ((L.FRONT_STEM, 128, 32), (L.FRONT_CONV, 32, 32), (L.FRONT_CONV, 16, 64), (L.FRONT_CONV, 8, 128)):
        for backward in (0, 1):
            prev_T = 0
            for T_ in (2, 3, 63, 64, 65, 150, 1500):
                prev_B = 0
                for B in (1, 2, 8):
                    n = lib.bt_front_bn_workspace_bytes(unit, backward, B, T_, F_, C_)
                    assert n > 0 and n % 256 == 0 and n >= prev_B, (unit, backward, B, T_, n)
                    prev_B = n
                n1 = lib.bt_front_bn_workspace_bytes(unit, backward, 1, T_, F_, C_)
                assert n1 >= prev_T
                prev_T = n1
    assert lib.bt_front_bn_workspace_bytes(L.FRONT_CONV, 0, 1, 1, 32, 32) > 0      # 16 values per channel
    assert lib.bt_front_bn_workspace_bytes(L.FRONT_STEM, 1, 3, 21845, 128, 32) > 0
    assert lib.bt_front_bn_workspace_bytes(L.FRONT_STEM, 1, 4, 16384, 128, 32) == 0


def test_refused_before_any_launch():
    """(no GPU here: a call that reached a launch would fail differently)  One value per channel, unsupported shapes, the units
    without a BatchNorm and NULL pointers are BT_ERR_ARG; the query returns 0."""
    from beat_this_amd import _lib as L

    lib = L.lib()
    some = C.cast((C.c_float * 64)(), C.c_void_p).value    # a non-NULL address that no refused call may touch
    pointers = [n for n, t in L.FrontBnArgs._fields_ if t is C.c_void_p and n != "ws"]

    def full(unit, B, T_, F_, C_):
        a = L.FrontBnArgs(B=B, T=T_, F=F_, C=C_)
        for n in pointers:
            setattr(a, n, some)
        a.ws, a.ws_bytes = some, 1 << 40
        return a

    for fn in (lib.bt_front_bn_forward, lib.bt_front_bn_backward):
        # torch: "Expected more than 1 value per channel when training"
        assert fn(None, L.FRONT_STEM, C.byref(full(L.FRONT_STEM, 1, 1, 128, 32))) == L.BT_ERR_ARG
        assert b"more than 1 value per channel" in lib.bt_last_error()
        assert fn(None, L.FRONT_CONV, C.byref(full(L.FRONT_CONV, 1, 1, 2, 32))) == L.BT_ERR_ARG
        assert b"more than 1 value per channel" in lib.bt_last_error()
        for field, value in (("B", 0), ("T", 0), ("T", 32768), ("B", 65536), ("F", 31), ("F", 34), ("C", 48), ("C", 0), ("C", 544)):
            a = full(L.FRONT_CONV, 2, 8, 32, 32)
            setattr(a, field, value)
            assert fn(None, L.FRONT_CONV, C.byref(a)) == L.BT_ERR_ARG, (field, value)
            assert lib.bt_front_bn_workspace_bytes(L.FRONT_CONV, 0, a.B, a.T, a.F, a.C) == 0, (field, value)
        assert fn(None, L.FRONT_STEM, C.byref(full(L.FRONT_STEM, 2, 8, 32, 32))) == L.BT_ERR_ARG     # (the stem takes 128 bins)
        for unit in (L.FRONT_LINEAR, L.FRONT_SWAP, 4, -1):
            assert fn(None, unit, C.byref(full(L.FRONT_CONV, 2, 8, 32, 32))) == L.BT_ERR_ARG, unit
            assert lib.bt_front_bn_workspace_bytes(unit, 0, 2, 8, 32, 32) == 0
        assert fn(None, L.FRONT_CONV, None) == L.BT_ERR_ARG
    assert lib.bt_front_bn_workspace_bytes(L.FRONT_STEM, 0, 1, 1, 128, 32) == 0
    # every required pointer, one at a time
    optional = {"bn_tracked", "bn1_tracked", "gx", "g_w", "g_bn_w", "g_bn_b", "g_bn1_w", "g_bn1_b"}
    needs = {(0, L.FRONT_STEM): {"w", "bn_w", "bn_b", "bn_mean", "bn_var", "bn1_w", "bn1_b", "bn1_mean", "bn1_var", "save_mean",
                                 "save_rstd", "save1_mean", "save1_rstd", "x", "y", "ws"},
             (0, L.FRONT_CONV): {"w", "bn_w", "bn_b", "bn_mean", "bn_var", "save_mean", "save_rstd", "x", "y", "save_pre", "ws"},
             (1, L.FRONT_STEM): {"w", "bn_w", "bn_b", "bn1_w", "bn1_b", "save_mean", "save_rstd", "save1_mean", "save1_rstd", "x", "gy",
                                 "ws"},
             (1, L.FRONT_CONV): {"w", "bn_w", "bn_b", "save_mean", "save_rstd", "x", "save_pre", "gy", "ws"}}
    for (backward, unit), names in needs.items():
        fn = lib.bt_front_bn_backward if backward else lib.bt_front_bn_forward
        assert not names & optional
        for n in sorted(names):
            a = full(unit, 2, 8, 128, 32) if unit == L.FRONT_STEM else full(unit, 2, 8, 32, 32)
            setattr(a, n, None)
            assert fn(None, unit, C.byref(a)) == L.BT_ERR_ARG, (backward, unit, n)
    a = full(L.FRONT_CONV, 2, 8, 32, 32)
    a.ws_bytes = 256
    assert lib.bt_front_bn_forward(None, L.FRONT_CONV, C.byref(a)) == L.BT_ERR_WORKSPACE


def test_the_opt_in_keeps_its_books_on_a_cpu_model():
    import copy
    import pickle

    m = new_model()
    assert not m.batch_statistics
    with pytest.raises(RuntimeError, match="set_frontend_trainable"):
        m.set_batch_statistics()
    assert not m.batch_statistics
    m.set_frontend_trainable()
    assert not m.batch_statistics                      # never inferred
    assert m.set_batch_statistics() is m and m.batch_statistics
    m.train()
    assert m.batch_statistics and m._batch_route()
    with torch.no_grad():
        assert not m._batch_route()
    m.eval()
    assert m.batch_statistics and not m._batch_route()
    with pytest.raises(AttributeError):
        m.batch_statistics = True                      # read-only
    assert copy.deepcopy(m).batch_statistics and pickle.loads(pickle.dumps(m)).batch_statistics
    m.set_batch_statistics(False)
    assert not m.batch_statistics and m.frontend_trainable
    m.set_batch_statistics()
    m.set_frontend_trainable(False)
    assert not m.batch_statistics and not m.frontend_trainable
    m.set_frontend_trainable()
    assert not m.batch_statistics                      # cleared for good, not remembered
    m.train().set_batch_statistics()
    with pytest.raises(RuntimeError, match="ROCm GPU"):     # the route has no CPU implementation either
        m(torch.zeros(2, 16, 128))
    # train() alone changes nothing
    m2 = new_model().train()
    assert not m2.batch_statistics and not m2._batch_route()


def test_the_module_and_the_command_line(capsys):
    from beat_this_amd.model.pl_module import PLBeatThis
    from beat_this_amd.train import get_parser, main

    kw = dict(transformer_dim=64, n_layers=2, ff_mult=2)
    plain, batch = PLBeatThis(**kw, train_frontend=True), PLBeatThis(**kw, train_frontend=True, batch_statistics=True)
    assert not plain.model.batch_statistics and batch.model.batch_statistics
    assert "batch_statistics" not in batch.hyper_parameters and batch.hyper_parameters == plain.hyper_parameters
    assert set(batch.state_dict()) == set(plain.state_dict())      # the buffers travel already: no new keys
    assert sum(k.endswith(RG.STAT_LEAVES) for k in batch.state_dict()) == 15
    with pytest.raises(RuntimeError, match="set_frontend_trainable"):
        PLBeatThis(**kw, batch_statistics=True)
    p = get_parser()
    base = ["--data-dir", "d", "--output", "o"]
    assert p.parse_args(base).batch_statistics is False
    assert p.parse_args(base + ["--train-frontend", "--batch-statistics"]).batch_statistics is True
    assert p.parse_args(base + ["--batch-statistics", "--no-batch-statistics"]).batch_statistics is False
    with pytest.raises(SystemExit) as e:
        main(base + ["--batch-statistics"])
    assert e.value.code == 2 and "--batch-statistics needs --train-frontend" in capsys.readouterr().err


# ---- the yardstick discriminates -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    sd = W.random_state_dict(W.resolve_hparams(HP), seed=6, style="lively")
    B, T = 2, 3
    x = RC.spect(B, T, seed=11)
    g = torch.randn(B, T, 64, generator=torch.Generator().manual_seed(12))
    r32, r64 = (RG.bn_frontend(sd, x, g, dt) for dt in (torch.float32, torch.float64))
    return sd, x, g, r32, r64


def test_the_truth_is_torchs_training_mode(case):
    """every frontend tensor has a gradient, every buffer moves, and the oracle itself is left as it was"""
    from oracle import beat_this_oracle as O

    sd, x, g, r32, r64 = case
    assert O.batchnorm.__module__ == O.__name__
    assert set(r64["grads"]) == set(["x"] + RG.frontend_keys(sd)) and len(r64["grads"]) == 77
    assert all(float(v.abs().max()) > 0 for v in r64["grads"].values())
    assert len(r64["stats"]) == 15
    for p in RG.BN_PREFIXES:
        assert int(r64["stats"][p + "num_batches_tracked"]) == int(sd[p + "num_batches_tracked"]) + 1
        for leaf in ("running_mean", "running_var"):
            assert not torch.equal(r64["stats"][p + leaf], sd[p + leaf].double()), p + leaf
    # against nn.BatchNorm1d in train(): the stand-in is torch's own module arithmetic
    bn = torch.nn.BatchNorm1d(128).double().train()
    p = "frontend.stem.bn1d."
    bn.load_state_dict({k[len(p):]: v.double() if v.is_floating_point() else v for k, v in sd.items() if k.startswith(p)})
    bn(x.double().transpose(1, 2))
    assert torch.allclose(bn.running_var, r64["stats"][p + "running_var"], rtol=1e-12, atol=0)
    assert torch.allclose(bn.running_mean, r64["stats"][p + "running_mean"], rtol=1e-12, atol=1e-15)
    e_ref = RG.yardstick(r32["grads"], r64["grads"])
    print(f"e_ref = {e_ref:.3e}")
    assert 1e-7 < e_ref < 1e-4, e_ref


def _mistaken(mistake):
    def make(stats):
        def batchnorm(x, sd, pfx, ch_dim):
            dims = [d for d in range(x.dim()) if d != 1]
            shape = [1, -1] + [1] * (x.dim() - 2)
            n = x.numel() // x.shape[1]
            mean, var = x.mean(dims), x.var(dims, unbiased=False)
            use = var * (n / (n - 1)) if mistake == "normalising with the unbiased variance" else var
            if mistake == "no centring terms in the backward":
                mean, use = mean.detach(), use.detach()
            y = (x - mean.view(shape)) / torch.sqrt(use.view(shape) + 1e-5) * sd[pfx + "weight"].view(shape) + sd[pfx + "bias"].view(shape)
            moved = var if mistake == "running_var moved with the biased variance" else var * (n / (n - 1))
            stats[pfx + "running_mean"] = (0.9 * sd[pfx + "running_mean"] + 0.1 * mean).detach()
            stats[pfx + "running_var"] = (0.9 * sd[pfx + "running_var"] + 0.1 * moved).detach()
            return y
        return batchnorm
    return make


@pytest.mark.parametrize("mistake", [None, "no centring terms in the backward", "normalising with the unbiased variance",
                                     "running_var moved with the biased variance"])
def test_the_yardstick_discriminates(case, mistake):
    """Each mistake, made on the fp32 reference, is at least 1000 e_ref from the fp64 truth (100 x the gate of 10 e_ref); the same
    hand-written BatchNorm without a mistake (None) is inside the gate, so the distance is the mistake's."""
    sd, x, g, r32, r64 = case
    bad = RG.bn_frontend(sd, x, g, torch.float32, batchnorm=_mistaken(mistake))
    e_ref = RG.yardstick(r32["grads"], r64["grads"])
    e_grad = RG.yardstick(bad["grads"], r64["grads"]) / e_ref
    stat_keys = [k for k in r64["stats"] if not k.endswith("num_batches_tracked")]
    e_stat = max(RG.rel(bad["stats"][k], r64["stats"][k]) / max(RG.rel(r32["stats"][k], r64["stats"][k]), RG.STAT_FLOOR) for k in stat_keys)
    print(f"{mistake}: gradients {e_grad:.1f} x e_ref ({e_ref:.3e}), running statistics {e_stat:.1f} x their e_ref")
    if mistake is None:
        assert e_grad <= RG.GATE and e_stat <= RG.GATE
    elif mistake == "running_var moved with the biased variance":
        assert e_grad <= RG.GATE and e_stat >= 100 * RG.GATE, (e_grad, e_stat)
    else:
        assert e_grad >= 100 * RG.GATE, (mistake, e_grad)


@pytest.mark.parametrize("B,T", [(2, 1), (1, 2), (2, 3)])
def test_the_truth_agrees_with_plain_autograd(B, T):
    """torch's batch_norm backward against autograd through the formula written out, in fp64: the same gradients to 1e-10, also
    at T = 1, where a permuted upstream gradient has channels-last strides (route_reference._PlainGrad)"""
    sd = W.random_state_dict(W.resolve_hparams(HP), seed=6, style="lively")
    x, gy = RC.spect(B, T, seed=100 + T), torch.randn(B, T, 32, 32, generator=torch.Generator().manual_seed(200 + T))
    a, b = RG.bn_stem(sd, x, gy, torch.float64), RG.bn_stem(sd, x, gy, torch.float64, batchnorm=_mistaken(None))
    assert RG.yardstick(a["grads"], b["grads"]) < 1e-10 and RG.rel(a["y"], b["y"]) < 1e-12
    xc = torch.randn(B, T, 16, 64, generator=torch.Generator().manual_seed(1))
    gc = torch.randn(B, T, 8, 128, generator=torch.Generator().manual_seed(2))
    a, b = RG.bn_conv(sd, 1, xc, gc, torch.float64), RG.bn_conv(sd, 1, xc, gc, torch.float64, batchnorm=_mistaken(None))
    assert RG.yardstick(a["grads"], b["grads"]) < 1e-10


def test_torchs_fp32_batch_norm_is_a_sound_reference_for_shifted_input():
    """The cancellation case of the GPU tests: the spectrogram shifted by +64 (values in [64, 67)).  torch's fp32 batch_norm on
    the CPU must itself stay close to the fp64 one there, or its error would be no yardstick: its running_var and its output are
    within 1e-5 of fp64, where E[v^2] - mean^2 in fp32 (4225 +- 0.75 at 2^-24 relative: 2.5e-4 absolute) would be 1e-3 off."""
    x = RC.spect(2, 65, seed=165) + 64
    assert 64 <= float(x.min()) and float(x.max()) < 67
    out = {}
    for dt in (torch.float32, torch.float64):
        mean, var = torch.zeros(128, dtype=dt), torch.ones(128, dtype=dt)
        y = F.batch_norm(x.to(dt).transpose(1, 2), mean, var, None, None, training=True, momentum=0.1, eps=1e-5)
        out[dt] = (y, mean, var)
    e_y, e_mean, e_var = (RG.rel(a, b) for a, b in zip(out[torch.float32], out[torch.float64]))
    print(f"shift +64: fp32 batch_norm against fp64: y {e_y:.3e}, running_mean {e_mean:.3e}, running_var {e_var:.3e}")
    assert e_y < 1e-5 and e_mean < 1e-6 and e_var < 1e-5
    naive = (x * x).mean((0, 1)) - x.mean((0, 1)) ** 2               # fp32
    true = x.double().var((0, 1), unbiased=False)
    print(f"           E[v^2] - mean^2 in fp32: {RG.rel(naive, true):.3e}")
    assert RG.rel(naive, true) > 100 * e_var
