"""The optimiser step on the GPU (csrc/optim.hip, beat_this_amd/optim.py).

1. The C ABI against its host twins, bit for bit: parameters, both moments, the cleared gradients, the norm and the clip
   coefficient, with every buffer between guard bands under both poison bytes.  Tensor sizes sit on both sides of the chunk
   (BT_OPTIM_CHUNK elements per workgroup) and of the 16-byte access width; one parameter is a view at a 4-byte offset.
2. ``beat_this_amd.optim.AdamW`` on a D = 64, 2-layer model with real gradients, against the yardstick of tests/test_optim.py:
   the truth is an fp64 numpy AdamW over the same gradients, e_ref the distance of torch.optim.AdamW(foreach=False) on CPU
   fp32 from it on p_final - p_initial, and the device has to be within 2 e_ref.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_util import POISONS, Guarded, assert_intact, dev, report
from route_harness import make_batch
from beat_this_amd import weights as W
from oracle import beat_this_oracle as O

pytestmark = pytest.mark.gpu

DEFAULTS = dict(lr=8e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- 1. the C ABI against the host twins -----------------------------------------------------------------------------------
def _abi_case(poison, g_scale, steps=3):
    from beat_this_amd import _lib as L
    from beat_this_amd import optim as OP

    CH = L.OPTIM_CHUNK
    shapes = [(1,), (3,), (4,), (5,), (CH - 1,), (CH,), (CH + 1,), (2 * CH + 3,), (64, 192), (CH + 6,), (7,), (130,)]
    view_at = 9                                   # this parameter starts 4 bytes into its buffer: the one-element path
    sizes = [int(np.prod(s)) for s in shapes]
    groups = [i % 2 for i in range(len(sizes))]
    settings = [dict(DEFAULTS), dict(DEFAULTS, lr=2e-4, weight_decay=0.0)]
    rng = np.random.default_rng(11)
    d = dev()
    # host side: the twin's parameters and flat buffers
    h_bufs = [(rng.standard_normal(n + 4) * 0.05).astype(np.float32) for n in sizes]
    h_params = [b[1:1 + n] if i == view_at else b[:n] for i, (b, n) in enumerate(zip(h_bufs, sizes))]
    assert all(p.ctypes.data % 16 == (4 if i == view_at else 0) for i, p in enumerate(h_params))
    ht, hc, total, n_chunks = OP.plan([p.ctypes.data for p in h_params], sizes, groups, 2)
    offsets = [int(ht[i].offset) for i in range(len(sizes))]
    h_grad, h_m, h_v = (np.zeros(total, np.float32) for _ in range(3))
    # device side: every buffer guarded; the flat buffers start as zeros (their padding has to stay zero)
    g_params = [Guarded((n + 4,), torch.float32).fill(poison, data=torch.from_numpy(b).to(d)) for b, n in zip(h_bufs, sizes)]
    d_ptrs = [g.ptr() + (4 if i == view_at else 0) for i, g in enumerate(g_params)]
    dt, dc, d_total, d_chunks = OP.plan(d_ptrs, sizes, groups, 2)
    assert (d_total, d_chunks) == (total, n_chunks) and [int(dt[i].offset) for i in range(len(sizes))] == offsets
    flat = {k: Guarded((total,), torch.float32).fill(poison, data=torch.zeros(total, device=d)) for k in ("grad", "m", "v")}
    ws_bytes = L.lib().bt_grad_norm_workspace_bytes(total)
    ws = Guarded((ws_bytes,), torch.uint8).fill(poison)           # (poisoned payload: a slice read before it is written shows)
    record = Guarded((2,), torch.float32).fill(poison)
    t_dev = Guarded((len(sizes) * C.sizeof(L.OptimTensor),), torch.uint8).fill(poison, data=torch.frombuffer(bytearray(bytes(dt)), dtype=torch.uint8).to(d))
    c_dev = Guarded((n_chunks * C.sizeof(L.OptimChunk),), torch.uint8).fill(poison, data=torch.frombuffer(bytearray(bytes(dc))[:n_chunks * C.sizeof(L.OptimChunk)], dtype=torch.uint8).to(d))
    covered = np.zeros(total, bool)
    for o, n in zip(offsets, sizes):
        covered[o:o + n] = True
    stream = L.stream_ptr(d)
    out = []
    for t in range(1, steps + 1):
        grads = [(rng.standard_normal(n) * g_scale).astype(np.float32) for n in sizes]
        h_grad[:] = 0
        for o, g in zip(offsets, grads):
            h_grad[o:o + g.size] = g
        flat["grad"].t.copy_(torch.from_numpy(h_grad))
        truth = float(np.linalg.norm(h_grad.astype(np.float64)))
        max_norm = 0.25 * truth if (t == 1 and truth > 0) else 1.0   # half the scaled norm on the first step, then 1.0
        hyp = OP.hyper(settings, t, grad_scale=0.5, zero_grads=True)
        L.check(L.lib().bt_grad_norm(stream, flat["grad"].ptr(), total, hyp.grad_scale, max_norm, ws.ptr(), ws_bytes, record.ptr()))
        L.check(L.lib().bt_adamw_step(stream, t_dev.ptr(), len(sizes), c_dev.ptr(), n_chunks, flat["grad"].ptr(), flat["m"].ptr(),
                                      flat["v"].ptr(), total, C.byref(hyp), record.ptr() + 4))
        torch.cuda.synchronize()
        h_norm, h_coef = OP.grad_norm_host(h_grad, max_norm, 0.5)
        OP.adamw_step_host(ht, len(sizes), hc, n_chunks, h_grad, h_m, h_v, hyp, coef=h_coef)
        rec = record.t.cpu().numpy()
        assert bits(rec).tolist() == bits(np.array([h_norm, h_coef], np.float32)).tolist(), (t, rec, h_norm, h_coef)
        if truth > 0:
            assert abs(float(rec[0]) - 0.5 * truth) <= 1e-6 * 0.5 * truth
            assert (rec[1] < 1) == (max_norm < 0.5 * truth)
        for name, host in (("grad", h_grad), ("m", h_m), ("v", h_v)):
            got = flat[name].t.cpu().numpy()
            assert np.array_equal(bits(got), bits(host)), f"step {t}: flat {name} differs from the twin"
            assert not got[~covered].any(), f"step {t}: padding of {name} written"
        assert not flat["grad"].t.any()
        for i, (g, hb) in enumerate(zip(g_params, h_bufs)):
            assert np.array_equal(bits(g.t.cpu().numpy()), bits(hb)), f"step {t}: parameter {i} differs from the twin"
        out.append((rec.copy(), [g.t.cpu().numpy().copy() for g in g_params]))
    assert_intact(*[(f"parameter {i}", g) for i, g in enumerate(g_params)], *[(f"flat {k}", g) for k, g in flat.items()],
                  ("norm workspace", ws), ("norm record", record), ("tensor table", t_dev), ("chunk table", c_dev))
    return out


@pytest.mark.parametrize("regime,g_scale", [("typical", 1e-2), ("tiny", 1e-22), ("denormal_v", 1e-20), ("zero_gradients", 0.0)])
def test_device_equals_the_host_twin_bit_for_bit(regime, g_scale):
    res = [_abi_case(p, g_scale) for p in POISONS]
    for (rec_a, ps_a), (rec_b, ps_b) in zip(*res):
        assert np.array_equal(bits(rec_a), bits(rec_b)), "the norm record depends on the poison"
        for a, b in zip(ps_a, ps_b):
            assert np.array_equal(bits(a), bits(b)), "a parameter depends on the poison"
            assert np.isfinite(a).all()
    report("optim_twin", regime=regime, norm=float(res[0][-1][0][0]), coef=float(res[0][-1][0][1]))


# ---- 2. beat_this_amd.optim.AdamW on a small model ---------------------------------------------------------------------------
def make_model(seed=3):
    """a fresh D = 64, 2-layer, ff_mult 2 model on the GPU with the trunk and the heads trainable, and its state dict (CPU)"""
    import route_harness as H

    hp = dict(transformer_dim=64, ff_mult=2, n_layers=2)
    sd = dict(H.state_dict(hp, seed, "lively"))
    return H.make_model(hp, sd, freeze_freqs=True), sd


def model_loss(m, batch, rows=slice(None)):
    from beat_this_amd.model.loss import ShiftTolerantBCELoss

    out = m(batch["spect"][rows])
    fn = ShiftTolerantBCELoss().to(dev())
    return sum(fn(out[k], batch["truth_" + k][rows].float(), batch["padding_mask"][rows]) for k in ("beat", "downbeat"))


def trainable(m):
    return [(n, p) for n, p in m.named_parameters() if p.requires_grad]


def new_optimizer(m, **kw):
    from beat_this_amd import optim as OP

    return OP.AdamW(OP.param_groups_for(m, 0.01), lr=kw.pop("lr", 1e-3), **kw)


def host_twin_of(opt, params, grad_scale=1.0, max_norm=None):
    """one step of the host twin from the optimiser's present state -> (new parameters, norm, coef); nothing on the device moves"""
    from beat_this_amd import optim as OP

    st = opt.flat_state()
    hp = [p.detach().cpu().numpy().copy() for p in params]
    groups = [gi for gi, g in enumerate(opt.param_groups) for _ in g["params"]]
    ht, hc, total, n_chunks = OP.plan([p.ctypes.data for p in hp], [p.size for p in hp], groups, len(opt.param_groups))
    assert total == st["total"] and [int(ht[i].offset) for i in range(len(hp))] == st["offsets"]
    g, m, v = (st[k].cpu().numpy().copy() for k in ("grad", "exp_avg", "exp_avg_sq"))
    norm = coef = None
    if max_norm is not None:
        norm, coef = OP.grad_norm_host(g, max_norm, grad_scale)
    OP.adamw_step_host(ht, len(hp), hc, n_chunks, g, m, v, OP.hyper(opt.param_groups, st["step"] + 1, grad_scale), coef=coef)
    return hp, norm, coef


_RUNS = {}


def plain_run(steps=3):
    """``steps`` AdamW steps on one batch: losses, the gradients of every step, initial and final parameters, logits before"""
    if steps not in _RUNS:
        m, sd = make_model()
        batch = make_batch(2, 150, seed=61)
        with torch.no_grad():
            before = m(batch["spect"])
        opt = new_optimizer(m)
        names = [n for n, _ in trainable(m)]
        params = [p for g in opt.param_groups for p in g["params"]]
        order = {id(p): n for n, p in trainable(m)}
        p0 = {order[id(p)]: p.detach().cpu().numpy().copy() for p in params}
        losses, grads = [], []
        for _ in range(steps):
            loss = model_loss(m, batch)
            loss.backward()
            losses.append(float(loss.detach()))
            grads.append({order[id(p)]: p.grad.detach().cpu().numpy().copy() for p in params})
            opt.step()
        losses.append(float(model_loss(m, batch).detach()))
        opt.zero_grad()
        final = {order[id(p)]: p.detach().cpu().numpy().copy() for p in params}
        decay = {order[id(p)]: g["weight_decay"] for g in opt.param_groups for p in g["params"]}
        _RUNS[steps] = dict(model=m, sd=sd, batch=batch, before=before, opt=opt, names=names, p0=p0, losses=losses, grads=grads,
                            final=final, decay=decay)
    return _RUNS[steps]


def test_three_steps_against_the_yardstick_and_the_engine_repacks():
    r = plain_run()
    assert r["losses"][-1] < r["losses"][0], r["losses"]
    d_dev, d32, d64 = [], [], []
    for n in r["p0"]:
        p0, settings = r["p0"][n], dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=r["decay"][n])
        gs = [g[n] for g in r["grads"]]
        p = p0.astype(np.float64)
        m, v = np.zeros_like(p), np.zeros_like(p)
        for t, g32 in enumerate(gs, 1):
            g = g32.astype(np.float64)
            p = p * (1 - settings["lr"] * settings["weight_decay"])
            m = m + (g - m) * 0.1
            v = v * 0.999 + g * g * (1 - 0.999)
            p = p - settings["lr"] / (1 - 0.9 ** t) * (m / (np.sqrt(v) / np.sqrt(1 - 0.999 ** t) + 1e-8))
        tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
        topt = torch.optim.AdamW([tp], foreach=False, **settings)
        for g32 in gs:
            tp.grad = torch.from_numpy(g32.copy())
            topt.step()
        d64.append((p - p0).ravel())
        d32.append((tp.detach().numpy().astype(np.float64) - p0).ravel())
        d_dev.append((r["final"][n].astype(np.float64) - p0).ravel())
    d_dev, d32, d64 = (np.concatenate(x) for x in (d_dev, d32, d64))
    e_ref = float(np.linalg.norm(d32 - d64) / np.linalg.norm(d64))
    e_dev = float(np.linalg.norm(d_dev - d64) / np.linalg.norm(d64))
    print(f"three AdamW steps: e_ref {e_ref:.3e}, device {e_dev:.3e} = {e_dev / e_ref:.3f} e_ref; losses {r['losses']}")
    report("optim_model_steps", e_ref=e_ref, e_dev=e_dev, ratio=e_dev / e_ref, loss_first=r["losses"][0], loss_last=r["losses"][-1])
    assert e_dev <= 2 * e_ref, (e_dev, e_ref)
    # the inference engine packs again after the steps (the version bump), and computes what the oracle does on the new weights
    m, batch = r["model"], r["batch"]
    with torch.no_grad():
        after = m(batch["spect"])
    new_sd = dict(r["sd"])
    new_sd.update({n: torch.from_numpy(a) for n, a in r["final"].items()})
    ob, od = O.model_forward(new_sd, batch["spect"].cpu())
    err = max(float((after["beat"].cpu() - ob).abs().max()), float((after["downbeat"].cpu() - od).abs().max()))
    moved = float((after["beat"] - r["before"]["beat"]).abs().max())
    print(f"after training: max |logit - oracle(updated weights)| = {err:.3e}, moved by {moved:.3e}")
    report("optim_repack", err_after=err, moved=moved)
    assert err < 1e-3, err
    assert moved > 10 * err, (moved, err)


def test_two_runs_give_identical_bits():
    a = plain_run()
    m, _ = make_model()
    opt = new_optimizer(m)
    for _ in range(3):
        model_loss(m, a["batch"]).backward()
        opt.step()
    got = {n: p.detach().cpu().numpy() for n, p in trainable(m)}
    assert set(got) == set(a["final"]) and len(got) > 20
    for n in got:
        assert np.array_equal(bits(got[n]), bits(a["final"][n])), n
    st_a, st_b = a["opt"].flat_state(), opt.flat_state()
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(st_a[k].view(torch.int32), st_b[k].view(torch.int32)), k
    assert not st_b["grad"].any()   # (the step cleared what it consumed)


def test_max_grad_norm_below_the_actual_norm():
    r = plain_run()
    truth = float(np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in r["grads"][0].values())))
    m, _ = make_model()
    opt = new_optimizer(m, max_grad_norm=0.25 * truth)
    params = [p for g in opt.param_groups for p in g["params"]]
    model_loss(m, r["batch"]).backward()
    want, norm, coef = host_twin_of(opt, params, max_norm=0.25 * truth)
    opt.step()
    assert coef < 1 and abs(float(coef) - 0.25) < 1e-3
    for p, w in zip(params, want):
        assert np.array_equal(bits(p.detach().cpu().numpy()), bits(w))
    got = opt.last_grad_norm()
    assert got == float(norm) and abs(got - truth) <= 1e-6 * truth, (got, truth)
    report("optim_clip", norm=got, truth=truth, coef=float(coef))


def test_accumulate_two_half_batches():
    r = plain_run()
    m, _ = make_model()
    opt = new_optimizer(m, accumulate=2)
    params = [p for g in opt.param_groups for p in g["params"]]
    model_loss(m, r["batch"], slice(0, 1)).backward()
    first = opt.flat_state()["grad"].clone()
    model_loss(m, r["batch"], slice(1, 2)).backward()
    assert not torch.equal(first, opt.flat_state()["grad"])   # (autograd accumulated into the flat buffer in place)
    want, _, _ = host_twin_of(opt, params, grad_scale=0.5)
    opt.step()
    for p, w in zip(params, want):
        assert np.array_equal(bits(p.detach().cpu().numpy()), bits(w))
    # a remainder stepped with its own count
    model_loss(m, r["batch"], slice(0, 1)).backward()
    want, _, _ = host_twin_of(opt, params, grad_scale=1.0)
    opt.step(accumulated=1)
    for p, w in zip(params, want):
        assert np.array_equal(bits(p.detach().cpu().numpy()), bits(w))


def test_zero_grad_set_to_none_between_steps():
    r = plain_run()
    m, _ = make_model()
    opt = new_optimizer(m)
    params = [p for g in opt.param_groups for p in g["params"]]
    flat = opt.flat_state()["grad"]
    lo, hi = flat.data_ptr(), flat.data_ptr() + 4 * flat.numel()
    losses = []
    for _ in range(3):
        m.zero_grad(set_to_none=True)
        assert all(p.grad is None for p in params)
        loss = model_loss(m, r["batch"])
        loss.backward()
        assert all(p.grad is not None and not lo <= p.grad.data_ptr() < hi for p in params if p.ndim >= 2)   # foreign gradients
        losses.append(float(loss.detach()))
        opt.step()
        assert all(lo <= p.grad.data_ptr() < hi for p in params)   # the views are attached again
    losses.append(float(model_loss(m, r["batch"]).detach()))
    assert losses[-1] < losses[0], losses
    for n, p in trainable(m):
        assert np.array_equal(bits(p.detach().cpu().numpy()), bits(r["final"][n])), n
    # the optimiser's own zero_grad attaches cleared views, whatever set_to_none says
    m.zero_grad(set_to_none=True)
    opt.zero_grad(set_to_none=True)
    assert all(p.grad is not None and lo <= p.grad.data_ptr() < hi and not p.grad.any() for p in params)
    # a gradient that stays None counts as zero: m and v were zero for it, so the parameter only decays
    m2, _ = make_model()
    opt2 = new_optimizer(m2)
    w = m2.transformer_blocks.layers[0][0].to_qkv.weight
    start = w.detach().clone()
    m2.zero_grad(set_to_none=True)
    opt2.step()
    assert torch.equal(w.detach(), start * np.float32(1.0 - 1e-3 * 0.01)) and not opt2.flat_state()["exp_avg"].any()


def test_state_dict_layout_and_round_trip():
    r = plain_run()
    m, sd0 = make_model()
    opt = new_optimizer(m)
    for _ in range(2):
        model_loss(m, r["batch"]).backward()
        opt.step()
    state = opt.state_dict()
    params = [p for g in opt.param_groups for p in g["params"]]
    assert set(state) == {"state", "param_groups"} and len(state["state"]) == len(params)
    assert sorted(state["state"]) == list(range(len(params)))
    for i, p in enumerate(params):
        s = state["state"][i]
        assert set(s) == {"step", "exp_avg", "exp_avg_sq"} and float(s["step"]) == 2.0
        assert s["exp_avg"].shape == p.shape and s["exp_avg_sq"].shape == p.shape
    assert [g["params"] for g in state["param_groups"]] == [list(range(len(opt.param_groups[0]["params"]))),
                                                            list(range(len(opt.param_groups[0]["params"]), len(params)))]
    assert all({"lr", "betas", "eps", "weight_decay"} <= set(g) for g in state["param_groups"])
    # torch's own AdamW takes it
    twin = torch.optim.AdamW([{"params": g["params"], "weight_decay": g["weight_decay"]} for g in opt.param_groups], lr=1e-3)
    twin.load_state_dict(state)
    assert torch.equal(twin.state[params[0]]["exp_avg"], state["state"][0]["exp_avg"])
    weights = {n: p.detach().clone() for n, p in trainable(m)}
    # continue; then restart from the saved point in a fresh model and optimiser
    model_loss(m, r["batch"]).backward()
    opt.step()
    m2, _ = make_model()
    with torch.no_grad():
        for n, p in trainable(m2):
            p.copy_(weights[n])
    opt2 = new_optimizer(m2, lr=5e-4)
    opt2.load_state_dict(state)
    assert opt2.param_groups[0]["lr"] == 1e-3 and opt2.flat_state()["step"] == 2
    model_loss(m2, r["batch"]).backward()
    opt2.step()
    for (n, p), (_, q) in zip(trainable(m), trainable(m2)):
        assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32)), n
    for n, p in trainable(m):   # and three steps in a row are the plain run
        assert np.array_equal(bits(p.detach().cpu().numpy()), bits(r["final"][n])), n
    a, b = opt.flat_state(), opt2.flat_state()
    assert torch.equal(a["exp_avg"].view(torch.int32), b["exp_avg"].view(torch.int32))
    assert torch.equal(a["exp_avg_sq"].view(torch.int32), b["exp_avg_sq"].view(torch.int32))


def test_refusals():
    from beat_this_amd import optim as OP

    with pytest.raises(RuntimeError, match="ROCm GPUs only"):
        OP.AdamW([torch.nn.Parameter(torch.zeros(4))])
    with pytest.raises(TypeError, match="float32"):
        OP.AdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.float16, device=dev()))])
    with pytest.raises(ValueError, match="parameter groups"):
        OP.AdamW([{"params": [torch.nn.Parameter(torch.zeros(4, device=dev()))]} for _ in range(9)])
    opt = OP.AdamW([torch.nn.Parameter(torch.zeros(4, device=dev()))])
    with pytest.raises(RuntimeError, match="lays its parameters out once"):   # (a later group would silently never be updated)
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(4, device=dev()))]})
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        OP.AdamW([torch.nn.Parameter(torch.zeros(4, device=dev()))]).last_grad_norm()
