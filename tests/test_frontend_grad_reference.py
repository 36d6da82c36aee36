"""CPU side of the differentiable frontend: the binding of the bt_front_* entry points, the opt-in's
bookkeeping, the wiring through PLBeatThis / param_groups_for / the command line, and the yardstick of route_grads.py shown
to discriminate the three mistakes a conv backward makes most easily."""
import ctypes as C
import os
import re

import pytest
import torch

import route_cases as RC
import route_grads as RG
from conftest import ROOT
from route_harness import MODEL_KEYS
from beat_this_amd import weights as W
from oracle import beat_this_oracle as O

HP = dict(transformer_dim=64, ff_mult=2, n_layers=2)


def new_model(**more):
    from beat_this_amd.model import BeatThis

    hp = W.resolve_hparams(dict(HP, **more))
    return BeatThis(**{k: hp[k] for k in MODEL_KEYS}), hp


def test_binding_of_the_frontend_entry_points():
    from beat_this_amd import _lib as L

    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "beat_this_amd.h")).read()
    assert re.search(r"#define BT_ABI_VERSION 600\b", header) and lib.bt_version() == 600 and L.ABI_VERSION == 600
    assert "train_front.hip" in L.SOURCES
    P = C.POINTER(L.FrontArgs)
    assert L.EXPORTS["bt_front_forward"] == (C.c_int, [C.c_void_p, C.c_int, P])
    assert L.EXPORTS["bt_front_backward"] == (C.c_int, [C.c_void_p, C.c_int, P])
    assert L.EXPORTS["bt_front_workspace_bytes"] == (C.c_size_t, [C.c_int] * 7)
    for name in ("bt_front_forward", "bt_front_backward", "bt_front_workspace_bytes", "bt_front_struct_sizes"):
        assert hasattr(lib, name) and re.search(r"\b%s\(" % name, header), name
    for name, value in (("BT_FRONT_STEM", L.FRONT_STEM), ("BT_FRONT_CONV", L.FRONT_CONV), ("BT_FRONT_LINEAR", L.FRONT_LINEAR),
                        ("BT_FRONT_SWAP", L.FRONT_SWAP)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    out = (C.c_int32 * 7)()
    lib.bt_front_struct_sizes(out)
    T = L.FrontArgs
    assert list(out) == [C.sizeof(T), T.w.offset, T.x.offset, T.gy.offset, T.gx.offset, T.ws.offset, T.ws_bytes.offset]
    # workspace queries: multiples of 256 bytes, non-decreasing in B and T; 8 x 1500 frames are inside the limits
    shapes = ((L.FRONT_STEM, 128, 32, 0), (L.FRONT_CONV, 32, 32, 0), (L.FRONT_CONV, 16, 64, 0), (L.FRONT_CONV, 8, 128, 0),
              (L.FRONT_LINEAR, 4, 256, 64), (L.FRONT_LINEAR, 4, 256, 512), (L.FRONT_SWAP, 32, 32, 0), (L.FRONT_SWAP, 8, 128, 0))
    for unit, F_, C_, dim in shapes:
        for backward in (0, 1):
            prev_T = 0
            for T_ in (1, 2, 63, 64, 65, 150, 1500):
                prev_B = 0
                for B in (1, 2, 8):
                    n = lib.bt_front_workspace_bytes(unit, backward, B, T_, F_, C_, dim)
                    assert n > 0 and n % 256 == 0 and n >= prev_B, (unit, backward, B, T_, n)
                    prev_B = n
                n1 = lib.bt_front_workspace_bytes(unit, backward, 1, T_, F_, C_, dim)
                assert n1 >= prev_T
                prev_T = n1
    # unsupported shapes and sizes beyond the limits: the query returns 0 and the calls refuse before any launch (no GPU here)
    a = L.FrontArgs()
    a.B, a.T, a.F, a.C, a.dim = 2, 8, 32, 32, 0
    bad = (("B", 0), ("T", 0), ("T", 32768), ("B", 65536), ("F", 31), ("F", 34), ("C", 48), ("C", 0), ("C", 544))
    for fn in (lib.bt_front_forward, lib.bt_front_backward):
        for field, value in bad:
            b = L.FrontArgs.from_buffer_copy(a)
            setattr(b, field, value)
            assert fn(None, L.FRONT_CONV, C.byref(b)) == L.BT_ERR_ARG, (field, value)
            assert lib.bt_last_error()
            assert lib.bt_front_workspace_bytes(L.FRONT_CONV, 0, b.B, b.T, b.F, b.C, b.dim) == 0, (field, value)
        assert fn(None, L.FRONT_CONV, C.byref(a)) == L.BT_ERR_ARG      # (a supported shape with null pointers: still no launch)
        assert fn(None, L.FRONT_STEM, C.byref(a)) == L.BT_ERR_ARG      # (the stem takes 128 bins)
        assert fn(None, 4, C.byref(a)) == L.BT_ERR_ARG and fn(None, L.FRONT_CONV, None) == L.BT_ERR_ARG
    assert lib.bt_front_workspace_bytes(L.FRONT_STEM, 1, 8, 1500, 128, 32, 0) > 0
    assert lib.bt_front_workspace_bytes(L.FRONT_STEM, 1, 3, 21845, 128, 32, 0) > 0     # 65535 frames
    assert lib.bt_front_workspace_bytes(L.FRONT_STEM, 1, 4, 16384, 128, 32, 0) == 0    # 65536 frames
    assert lib.bt_front_workspace_bytes(L.FRONT_LINEAR, 0, 1, 8, 4, 256, 48) == 0
    # the swap's row count is bounded factor by factor: extents whose product leaves 64 bits are refused like any other
    big = 2 ** 31 - 1
    for B, T_, F_ in ((big, big, big), (1 << 21, 1 << 21, 1 << 22), (1, 1, big), (4, 1 << 20, 2)):
        assert lib.bt_front_workspace_bytes(L.FRONT_SWAP, 0, B, T_, F_, 32, 0) == 0, (B, T_, F_)
    assert lib.bt_front_workspace_bytes(L.FRONT_SWAP, 0, 4, 1 << 20, 1, 32, 0) > 0


def test_the_opt_in_keeps_its_books_on_a_cpu_model():
    m, hp = new_model()
    assert not m.frontend_trainable and all(not p.requires_grad for p in m.parameters())
    front = dict(m.frontend.named_parameters())
    weights = [n for n in front if not n.endswith("rotary_embed.freqs")]
    assert len(weights) == len(RG.frontend_keys(m.state_dict())) == 76
    assert m.set_frontend_trainable() is m and m.frontend_trainable
    for n, p in front.items():
        assert p.requires_grad == (n in weights), n
    for n, b in m.named_buffers():
        assert n.endswith(RG.STAT_LEAVES) and not b.requires_grad, n
    assert all(not p.requires_grad for n, p in m.named_parameters() if not n.startswith("frontend."))
    # the route has no CPU implementation either
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m(torch.zeros(1, 16, 128))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m.frontend(torch.zeros(1, 16, 128))
    m.set_frontend_trainable(False)
    assert not m.frontend_trainable and all(not p.requires_grad for p in m.parameters())
    # the opt-in is never inferred from requires_grad
    m.frontend.linear.weight.requires_grad_(True)
    assert not m.frontend_trainable
    # a deep copy and a pickle keep the flag
    import copy
    import pickle

    m.set_frontend_trainable()
    assert copy.deepcopy(m).frontend_trainable and pickle.loads(pickle.dumps(m)).frontend_trainable
    # a model without partial transformers has the convolutions, the BatchNorms and the projection only
    m2, _ = new_model(partial_transformers=False)
    m2.set_frontend_trainable()
    assert sum(p.requires_grad for p in m2.parameters()) == 5 + 3 * 3 + 2


def test_the_module_the_groups_and_the_command_line():
    from beat_this_amd.model.pl_module import PLBeatThis
    from beat_this_amd.optim import param_groups_for
    from beat_this_amd.train import get_parser

    kw = dict(transformer_dim=64, n_layers=2, ff_mult=2)
    frozen, whole = PLBeatThis(**kw), PLBeatThis(**kw, train_frontend=True)
    assert not frozen.model.frontend_trainable and whole.model.frontend_trainable
    assert "train_frontend" not in whole.hyper_parameters and whole.hyper_parameters == frozen.hyper_parameters
    sd = whole.model.state_dict()
    trunk = RG.trainable_keys(sd)
    front = RG.frontend_keys(sd)
    count = lambda groups: [len(g["params"]) for g in groups]
    ndim2 = lambda keys: sum(sd[k].ndim >= 2 for k in keys)
    assert count(param_groups_for(frozen, 0.01)) == [ndim2(trunk), len(trunk) - ndim2(trunk)]
    groups = param_groups_for(whole, 0.01)
    assert count(groups) == [ndim2(trunk + front), len(trunk + front) - ndim2(trunk + front)]
    assert groups[0]["weight_decay"] == 0.01 and groups[1]["weight_decay"] == 0
    # the convolutions and the projection are decayed, the BatchNorm gains and biases are not
    decayed = {id(p) for p in groups[0]["params"]}
    named = dict(whole.model.named_parameters())
    assert id(named["frontend.blocks.1.conv2d.weight"]) in decayed and id(named["frontend.stem.conv2d.weight"]) in decayed
    assert id(named["frontend.blocks.1.norm.weight"]) not in decayed and id(named["frontend.stem.bn1d.bias"]) not in decayed
    p = get_parser()
    base = ["--data-dir", "d", "--output", "o"]
    assert p.parse_args(base).train_frontend is False
    assert p.parse_args(base + ["--train-frontend"]).train_frontend is True
    assert p.parse_args(base + ["--no-train-frontend"]).train_frontend is False


# ---- the yardstick discriminates -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    sd = W.random_state_dict(W.resolve_hparams(HP), seed=6, style="lively")
    B, T = 2, 3
    x = RC.spect(B, T, seed=11)
    g = torch.randn(B, T, 64, generator=torch.Generator().manual_seed(12))
    g32, g64 = (RG.grads_only(RG.frontend_grads(sd, x, g, dt)) for dt in (torch.float32, torch.float64))
    return sd, x, g, g32, g64


def test_every_frontend_tensor_has_a_gradient(case):
    sd, x, g, g32, g64 = case
    assert set(g64) == set(["x"] + RG.frontend_keys(sd)) and len(g64) == 77
    assert all(float(v.abs().max()) > 0 for v in g64.values())
    e_ref = RG.yardstick(g32, g64)
    print(f"e_ref = {e_ref:.3e}")
    assert 1e-7 < e_ref < 1e-4, e_ref   # (2.8e-6 .. 1.6e-5 over the cases of the issue)


def _conv_patch(monkeypatch, variant):
    real = torch.nn.functional.conv2d

    def conv2d(x, w, *args, **kw):
        if w.shape[-1] != 3:
            return real(x, w, *args, **kw)
        if variant == "flipped taps in backward-data":
            # the value and the weight gradient of the convolution; the input gradient through time-flipped taps
            through = real(x, w.detach().flip(-1), *args, **kw)
            return real(x.detach(), w, *args, **kw) + through - through.detach()
        # "(b t)" flattened: the time taps read the neighbouring sequence instead of the padding
        b, c, f, t = x.shape
        flat = x.permute(1, 2, 0, 3).reshape(1, c, f, b * t)
        y = real(flat, w, *args, **kw)
        return y.reshape(y.shape[1], y.shape[2], b, t).permute(2, 0, 1, 3)

    monkeypatch.setattr(O.F, "conv2d", conv2d)


@pytest.mark.parametrize("mistake", ["no BatchNorm scale in g_conv", "flipped taps in backward-data", "conv across the sequence boundary"])
def test_the_yardstick_discriminates(case, monkeypatch, mistake):
    """Each mistake, made on the fp32 oracle, is at least 1000 e_ref from the fp64 truth."""
    sd, x, g, g32, g64 = case
    e_ref = RG.yardstick(g32, g64)
    if mistake == "no BatchNorm scale in g_conv":
        real_bn = O.batchnorm

        def batchnorm(t, sd_, pfx, ch_dim):   # the value of the BatchNorm, the input gradient without its scale
            return real_bn(t.detach(), sd_, pfx, ch_dim) + t - t.detach()

        monkeypatch.setattr(O, "batchnorm", batchnorm)
    else:
        _conv_patch(monkeypatch, mistake)
    bad = RG.frontend_grads(sd, x, g, torch.float32)
    monkeypatch.undo()
    changed = [k for k in g64 if not torch.equal(bad[k], g32[k])]
    worst = RG.yardstick(bad, g64)
    print(f"{mistake}: {len(changed)} tensors changed, worst {worst:.3e} = {worst / e_ref:.0f} x e_ref")
    assert "x" in changed and len(changed) >= 10, changed
    assert worst >= 1000 * e_ref, (mistake, worst, e_ref)
    again = RG.frontend_grads(sd, x, g, torch.float32)     # (the patches are gone)
    assert all(torch.equal(again[k], g32[k]) for k in g64)
