"""Weight averaging on the GPU (csrc/optim.hip: bt_adamw_ema_step, bt_ema_exchange; beat_this_amd/optim.py, train.py; DESIGN.md
section 22).

1. The C ABI against its host twin, bit for bit in p, m, v and the averages, over 3 steps of a plan whose tensor sizes sit on
   both sides of the chunk and of the 16-byte access width (one parameter is a view at a 4-byte offset), with and without a
   clip coefficient on the device; the same steps through bt_adamw_step give the same p, m, v.  Every buffer sits between guard
   bands and the padding between tensors is poisoned with 0xFF: neither is touched.  bt_ema_exchange is exact and its own inverse.
2. ``AdamW(ema_decay=0.9)`` on the D = 64, 2-layer model of tests/test_gpu_optim.py against the numpy restatement of
   tests/ema_reference.py fed the same gradients, a skipped step, the state dict, ``averaged_weights()``.
3. ``fit(ema_decay=0.5)`` on the synthetic data folder of tests/test_gpu_finetune.py: resume, checkpoint, the averaged model."""
import ctypes as C
import shutil

import numpy as np
import pytest
import torch

import ema_reference as R
from dataset_reference import build_data_folder
from gpu_util import Guarded, assert_intact, dev, report
from test_gpu_finetune import EPOCHS, new_datamodule, new_module
from test_gpu_optim import bits, make_batch, make_model, model_loss, new_optimizer

pytestmark = pytest.mark.gpu

DEFAULTS = dict(lr=8e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
SETTINGS = [dict(DEFAULTS), dict(DEFAULTS, lr=2e-4, weight_decay=0.0)]
POISON = 0xFF
DECAY = 0.9


def tbits(t):
    return t.detach().contiguous().view(torch.int32)


# ---- 1. the C ABI against the host twin --------------------------------------------------------------------------------------
class DevicePlan:
    """the plan of tests/test_ema_reference.py on the host and, guarded, on the device; the padding of the flat buffers is poisoned"""

    def __init__(self, with_ema=True):
        from beat_this_amd import _lib as L
        from beat_this_amd import optim as OP

        CH = L.OPTIM_CHUNK
        self.sizes = sizes = [0, 1, 3, 4, 5, 1023, CH - 1, CH, CH + 1, 2 * CH + 7, CH + 6]
        view_at = len(sizes) - 1
        self.groups = groups = [i % 2 for i in range(len(sizes))]
        rng = np.random.default_rng(11)
        d = dev()
        self.h_bufs = [(rng.standard_normal(n + 4) * 0.05).astype(np.float32) for n in sizes]
        self.h_params = [b[1:1 + n] if i == view_at else b[:n] for i, (b, n) in enumerate(zip(self.h_bufs, sizes))]
        self.ht, self.hc, self.total, self.n_chunks = OP.plan([p.ctypes.data for p in self.h_params], sizes, groups, 2)
        self.offsets = [int(self.ht[i].offset) for i in range(len(sizes))]
        self.covered = np.zeros(self.total, bool)
        for o, n in zip(self.offsets, sizes):
            self.covered[o:o + n] = True
        assert not self.covered.all()   # (there is padding to watch)
        names = ("grad", "m", "v", "ema") if with_ema else ("grad", "m", "v")
        self.host = {k: self.poisoned() for k in names}
        self.g_params = [Guarded((n + 4,), torch.float32).fill(POISON, data=torch.from_numpy(b).to(d)) for b, n in zip(self.h_bufs, sizes)]
        d_ptrs = [g.ptr() + (4 if i == view_at else 0) for i, g in enumerate(self.g_params)]
        assert d_ptrs[view_at] % 16 == 4
        dt, dc, d_total, d_chunks = OP.plan(d_ptrs, sizes, groups, 2)
        assert (d_total, d_chunks) == (self.total, self.n_chunks)
        self.flat = {k: Guarded((self.total,), torch.float32).fill(POISON, data=torch.from_numpy(self.host[k]).to(d)) for k in names}
        as_bytes = lambda table, n: torch.frombuffer(bytearray(bytes(table))[:n], dtype=torch.uint8).to(d)
        nt, nc = len(sizes) * C.sizeof(L.OptimTensor), self.n_chunks * C.sizeof(L.OptimChunk)
        self.t_dev = Guarded((nt,), torch.uint8).fill(POISON, data=as_bytes(dt, nt))
        self.c_dev = Guarded((nc,), torch.uint8).fill(POISON, data=as_bytes(dc, nc))
        self.coef = Guarded((1,), torch.float32).fill(POISON, data=torch.tensor([0.37], device=d))

    def poisoned(self):
        """zeros where a tensor lives, 0xFF bytes in the padding"""
        a = np.frombuffer(bytes([POISON]) * (4 * self.total), np.float32).copy()
        a[self.covered] = 0
        return a

    def set_grads(self, grads):
        for o, g in zip(self.offsets, grads):
            self.host["grad"][o:o + g.size] = g
        self.flat["grad"].t.copy_(torch.from_numpy(self.host["grad"]))

    def guards(self):
        return [*[(f"parameter {i}", g) for i, g in enumerate(self.g_params)], *[(f"flat {k}", g) for k, g in self.flat.items()],
                ("tensor table", self.t_dev), ("chunk table", self.c_dev), ("coefficient", self.coef)]

    def assert_equals_host(self, what):
        for k, g in self.flat.items():
            got = g.t.cpu().numpy()
            assert np.array_equal(bits(got), bits(self.host[k])), f"{what}: flat {k} differs from the twin (or its padding was written)"
            assert (got[~self.covered].view(np.uint8) == POISON).all(), f"{what}: padding of {k} written"
        for i, (g, hb) in enumerate(zip(self.g_params, self.h_bufs)):
            assert np.array_equal(bits(g.t.cpu().numpy()), bits(hb)), f"{what}: parameter {i} differs from the twin"


@pytest.mark.parametrize("with_coef", [False, True])
def test_device_equals_the_host_twin_and_the_plain_step_bit_for_bit(with_coef):
    from beat_this_amd import _lib as L
    from beat_this_amd import optim as OP

    ema, plain = DevicePlan(), DevicePlan(with_ema=False)
    lib, stream = L.lib(), L.stream_ptr(dev())
    rng = np.random.default_rng(12)
    n = len(ema.sizes)
    for t in (1, 2, 3):
        grads = [(rng.standard_normal(k) * 1e-2).astype(np.float32) for k in ema.sizes]
        hyp = OP.hyper(SETTINGS, t, grad_scale=0.5, zero_grads=True)
        ema.set_grads(grads)
        plain.set_grads(grads)
        L.check(lib.bt_adamw_ema_step(stream, ema.t_dev.ptr(), n, ema.c_dev.ptr(), ema.n_chunks, ema.flat["grad"].ptr(),
                                      ema.flat["m"].ptr(), ema.flat["v"].ptr(), ema.flat["ema"].ptr(), ema.total, C.byref(hyp),
                                      ema.coef.ptr() if with_coef else None, 1.0 - DECAY, int(t == 1)))
        L.check(lib.bt_adamw_step(stream, plain.t_dev.ptr(), n, plain.c_dev.ptr(), plain.n_chunks, plain.flat["grad"].ptr(),
                                  plain.flat["m"].ptr(), plain.flat["v"].ptr(), plain.total, C.byref(hyp),
                                  plain.coef.ptr() if with_coef else None))
        torch.cuda.synchronize()
        h = ema.host
        OP.adamw_ema_step_host(ema.ht, n, ema.hc, ema.n_chunks, h["grad"], h["m"], h["v"], h["ema"], hyp, 1.0 - DECAY, t == 1,
                               coef=np.float32(0.37) if with_coef else None)
        ema.assert_equals_host(f"step {t}")
        for k in ("grad", "m", "v"):
            assert torch.equal(tbits(ema.flat[k].t), tbits(plain.flat[k].t)), f"step {t}: {k} differs from bt_adamw_step's"
        for i, (a, b) in enumerate(zip(ema.g_params, plain.g_params)):
            assert torch.equal(tbits(a.t), tbits(b.t)), f"step {t}: parameter {i} differs from bt_adamw_step's"
    e = ema.flat["ema"].t.cpu().numpy()
    assert np.isfinite(e[ema.covered]).all() and e[ema.covered].any()
    assert_intact(*ema.guards(), *plain.guards())


def test_exchange_is_exact_and_its_own_inverse():
    from beat_this_amd import _lib as L

    plan = DevicePlan()
    lib, stream = L.lib(), L.stream_ptr(dev())
    rng = np.random.default_rng(13)
    avg = plan.poisoned()
    avg[plan.covered] = rng.standard_normal(int(plan.covered.sum())).astype(np.float32)
    avg[plan.offsets[3]] = np.float32("nan")   # (a move: any bit pattern travels)
    plan.flat["ema"].t.copy_(torch.from_numpy(avg))
    before_p = [g.t.cpu().numpy().copy() for g in plan.g_params]
    swap = lambda: L.check(lib.bt_ema_exchange(stream, plan.t_dev.ptr(), len(plan.sizes), plan.c_dev.ptr(), plan.n_chunks,
                                               plan.flat["ema"].ptr(), plan.total))
    swap()
    torch.cuda.synchronize()
    got_e = plan.flat["ema"].t.cpu().numpy()
    view_at = len(plan.sizes) - 1
    for i, (g, b, o, n) in enumerate(zip(plan.g_params, before_p, plan.offsets, plan.sizes)):
        lo = 1 if i == view_at else 0
        now = g.t.cpu().numpy()
        assert np.array_equal(bits(now[lo:lo + n]), bits(avg[o:o + n])), f"parameter {i} is not the average"
        assert np.array_equal(bits(got_e[o:o + n]), bits(b[lo:lo + n])), f"average {i} is not the parameter"
        rest = np.ones(n + 4, bool)
        rest[lo:lo + n] = False
        assert np.array_equal(bits(now[rest]), bits(b[rest])), f"the exchange wrote around parameter {i}"
    assert (got_e[~plan.covered].view(np.uint8) == POISON).all()
    swap()
    torch.cuda.synchronize()
    assert np.array_equal(bits(plan.flat["ema"].t.cpu().numpy()), bits(avg))
    for g, b in zip(plan.g_params, before_p):
        assert np.array_equal(bits(g.t.cpu().numpy()), bits(b))
    for k in ("grad", "m", "v"):
        assert np.array_equal(bits(plan.flat[k].t.cpu().numpy()), bits(plan.host[k]))
    assert_intact(*plan.guards())


# ---- 2. the optimiser on a small model ----------------------------------------------------------------------------------------
def params_of(opt):
    return [p for g in opt.param_groups for p in g["params"]]


def restatement_of(opt, decay):
    groups = [gi for gi, g in enumerate(opt.param_groups) for _ in g["params"]]
    settings = [dict(lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"]) for g in opt.param_groups]
    return R.EmaReference([p.detach().cpu().numpy() for p in params_of(opt)], groups, settings, decay)


def assert_matches(opt, ref, what):
    for i, (p, e) in enumerate(zip(params_of(opt), opt.ema_parameters())):
        assert e.shape == p.shape
        assert np.array_equal(bits(p.detach().cpu().numpy().ravel()), bits(ref.p[i])), f"{what}: parameter {i}"
        assert np.array_equal(bits(e.cpu().numpy().ravel()), bits(ref.e[i])), f"{what}: average {i}"
    assert opt.flat_state()["n_averaged"] == ref.n_averaged


_STEPS = {}


def three_steps():
    """three averaged steps on one batch, the restatement fed the same gradients alongside"""
    if not _STEPS:
        m, _ = make_model()
        batch = make_batch(2, 150, seed=61)
        opt = new_optimizer(m, ema_decay=DECAY)
        ref = restatement_of(opt, DECAY)
        assert opt.flat_state()["n_averaged"] == 0
        for _ in range(3):
            model_loss(m, batch).backward()
            ref.step([p.grad.detach().cpu().numpy() for p in params_of(opt)])
            opt.step()
        _STEPS.update(model=m, batch=batch, opt=opt, ref=ref)
    return _STEPS


def test_three_steps_equal_the_restatement_and_the_plain_optimiser():
    r = three_steps()
    assert_matches(r["opt"], r["ref"], "three steps")
    assert len(params_of(r["opt"])) > 20 and r["opt"].flat_state()["ema"].data_ptr() % 16 == 0
    m, _ = make_model()
    plain = new_optimizer(m)
    for _ in range(3):
        model_loss(m, r["batch"]).backward()
        plain.step()
    for p, q in zip(params_of(r["opt"]), params_of(plain)):
        assert torch.equal(tbits(p), tbits(q))
    assert set(plain.state_dict()) == {"state", "param_groups"} and set(plain.flat_state()) == {"grad", "exp_avg", "exp_avg_sq", "offsets", "total", "step"}
    for call in (plain.ema_parameters, lambda: plain.averaged_weights().__enter__()):
        with pytest.raises(RuntimeError, match="ema_decay"):
            call()
    e = torch.cat([x.reshape(-1) for x in r["opt"].ema_parameters()])
    p = torch.cat([x.detach().reshape(-1) for x in params_of(r["opt"])])
    report("ema_model_steps", distance=float((e - p).norm() / p.norm()))
    assert not torch.equal(e, p)


def test_a_skipped_step_leaves_the_average_alone():
    from beat_this_amd.optim import LossScaler

    r = three_steps()
    m, _ = make_model()
    opt = new_optimizer(m, ema_decay=DECAY)
    ref = restatement_of(opt, DECAY)
    scaler = LossScaler(init_scale=1024.0)
    for inject in (False, True, False):
        (model_loss(m, r["batch"]) * scaler.scale).backward()
        params = params_of(opt)
        if inject:
            params[1].grad.view(-1)[3] = float("inf")
        grads = [p.grad.detach().cpu().numpy() for p in params]
        scale = scaler.scale
        before = opt.flat_state()["ema"].clone(), [p.detach().clone() for p in params]
        opt.step(loss_scaler=scaler)
        assert opt.last_step_skipped == inject
        ref.step(grads, grad_scale=1.0 / scale, skipped=inject)
        if inject:
            assert torch.equal(tbits(before[0]), tbits(opt.flat_state()["ema"])) and opt.flat_state()["n_averaged"] == 1
            assert all(torch.equal(tbits(a), tbits(b)) for a, b in zip(before[1], params))
    assert scaler.skipped_steps == 1 and opt.flat_state()["step"] == 2
    assert_matches(opt, ref, "around a skipped step")


def test_state_dict_round_trip_continues_bit_for_bit():
    r = three_steps()
    m, _ = make_model()
    opt = new_optimizer(m, ema_decay=DECAY)
    for _ in range(2):
        model_loss(m, r["batch"]).backward()
        opt.step()
    state = opt.state_dict()
    n = len(params_of(opt))
    assert set(state) == {"state", "param_groups", "ema"} and set(state["ema"]) == {"decay", "n_averaged", "params"}
    assert state["ema"]["decay"] == DECAY and state["ema"]["n_averaged"] == 2 and sorted(state["ema"]["params"]) == list(range(n))
    assert all(state["ema"]["params"][i].shape == p.shape for i, p in enumerate(params_of(opt)))
    weights = [p.detach().clone() for p in params_of(opt)]
    model_loss(m, r["batch"]).backward()
    opt.step()
    assert_matches(opt, r["ref"], "two steps, a state dict, a third")
    m2, _ = make_model()
    opt2 = new_optimizer(m2, ema_decay=DECAY)
    with torch.no_grad():
        for p, w in zip(params_of(opt2), weights):
            p.copy_(w)
    opt2.load_state_dict(state)
    assert opt2.flat_state()["n_averaged"] == 2
    model_loss(m2, r["batch"]).backward()
    opt2.step()
    assert_matches(opt2, r["ref"], "a fresh optimiser continuing from the state dict")
    # averages that do not fit are refused before anything is written
    kept = {k: opt2.flat_state()[k].clone() for k in ("exp_avg", "exp_avg_sq", "ema")}
    broken = dict(state, state={}, ema=dict(state["ema"], params={i: e for i, e in state["ema"]["params"].items() if i != 5}))
    with pytest.raises(ValueError, match="average of parameter 5"):
        opt2.load_state_dict(broken)
    assert all(torch.equal(tbits(v), tbits(opt2.flat_state()[k])) for k, v in kept.items())
    assert opt2.flat_state()["n_averaged"] == 3 and opt2.flat_state()["step"] == 3
    # a state without an average starts one over: the next step copies; an optimiser without averaging ignores the entry
    opt2.load_state_dict({k: v for k, v in state.items() if k != "ema"})
    assert opt2.flat_state()["n_averaged"] == 0 and not opt2.flat_state()["ema"].any()
    with pytest.raises(RuntimeError, match="no average yet"):
        opt2.averaged_weights().__enter__()
    model_loss(m2, r["batch"]).backward()
    opt2.step()
    assert all(torch.equal(tbits(e), tbits(p)) for p, e in zip(params_of(opt2), opt2.ema_parameters()))
    assert new_optimizer(make_model()[0], ema_decay=np.float32(0.5)).ema_decay == 0.5   # (numpy's scalars are decays too)
    plain = new_optimizer(make_model()[0])
    plain.load_state_dict(state)
    assert set(plain.state_dict()) == {"state", "param_groups"} and plain.flat_state()["step"] == 2


def test_averaged_weights_exchanges_and_restores():
    r = three_steps()
    m, opt = r["model"], r["opt"]
    x = make_batch(1, 150, seed=7)["spect"]
    live = [p.detach().clone() for p in params_of(opt)]
    avg = [e.clone() for e in opt.ema_parameters()]
    with torch.no_grad():
        before = m(x)
        with opt.averaged_weights():
            assert all(torch.equal(tbits(p), tbits(a)) for p, a in zip(params_of(opt), avg))
            assert all(torch.equal(tbits(e), tbits(w)) for e, w in zip(opt.ema_parameters(), live))
            inside = m(x)
            with pytest.raises(RuntimeError, match="re-entrant"):
                opt.averaged_weights().__enter__()
            with pytest.raises(RuntimeError, match="inside averaged_weights"):
                opt.step()
            with pytest.raises(RuntimeError, match="inside averaged_weights"):
                opt.state_dict()
            with pytest.raises(RuntimeError, match="inside averaged_weights"):
                opt.load_state_dict({})
        after = m(x)
    assert all(torch.equal(tbits(p), tbits(w)) for p, w in zip(params_of(opt), live))
    assert all(torch.equal(tbits(e), tbits(a)) for e, a in zip(opt.ema_parameters(), avg))
    for k in ("beat", "downbeat"):
        assert torch.equal(tbits(before[k]), tbits(after[k])), k
        assert not torch.equal(before[k], inside[k]), f"{k}: the engine did not pack the averaged weights"
    assert_matches(opt, r["ref"], "after averaged_weights()")


# ---- 3. fit -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """fit() for two epochs with ema_decay 0.5 (the first epoch's checkpoint is kept), and the same run without averaging"""
    from beat_this_amd.train import fit

    tmp = tmp_path_factory.mktemp("ema")
    root = build_data_folder(str(tmp / "data"))
    out = {"tmp": tmp, "root": root}
    for name, kw in (("ema", dict(ema_decay=0.5)), ("plain", {})):
        ck, first, lines = str(tmp / f"{name}.ckpt"), str(tmp / f"{name}0.ckpt"), []

        def log(line, ck=ck, first=first, lines=lines):
            lines.append(line)
            if line.startswith("epoch 0:"):
                shutil.copy(ck, first)

        pl = new_module()
        np.random.seed(0)
        history = fit(pl, new_datamodule(root), EPOCHS, val_frequency=1, checkpoint_path=ck, log=log, **kw)
        out[name] = dict(ck=ck, first=first, pl=pl, history=history, lines=lines)
    return out


def same_tensors(a, b, what):
    assert set(a) == set(b), what
    for k, v in a.items():
        assert v.dtype == b[k].dtype and torch.equal(v, b[k]), (what, k)
        if v.dtype == torch.float32:
            assert torch.equal(tbits(v), tbits(b[k])), (what, k)


def test_fit_resumed_equals_uninterrupted_averages_included(runs):
    from beat_this_amd.inference import load_checkpoint
    from beat_this_amd.train import CHECKPOINT_KEYS, fit

    run = runs["ema"]
    print("\n".join(run["lines"]))
    assert all("validated on the averaged weights (decay 0.5)" in line for line in run["lines"])
    ck2, lines = str(runs["tmp"] / "resumed.ckpt"), []
    pl = new_module()
    np.random.seed(99)
    h = fit(pl, new_datamodule(runs["root"]), EPOCHS, val_frequency=1, checkpoint_path=ck2, resume=run["first"], log=lines.append,
            ema_decay=0.5)
    assert len(h["train_loss"]) == 1 and h["train_loss"][0] == run["history"]["train_loss"][1]
    a, b = load_checkpoint(run["ck"]), load_checkpoint(ck2)
    assert set(a) == set(CHECKPOINT_KEYS) | {"ema_state_dict"} == set(b)
    same_tensors(a["state_dict"], b["state_dict"], "weights")
    same_tensors(a["ema_state_dict"], b["ema_state_dict"], "averaged weights")
    sa, sb = a["optimizer_states"][0], b["optimizer_states"][0]
    assert set(sa) == {"state", "param_groups", "ema"} == set(sb) and sa["ema"]["n_averaged"] == 4 == sb["ema"]["n_averaged"]
    same_tensors(sa["ema"]["params"], sb["ema"]["params"], "the optimiser's averages")
    for i in sa["state"]:
        same_tensors(sa["state"][i], sb["state"][i], f"moments of parameter {i}")
    assert h["val"][0][1] == run["history"]["val"][1][1]
    # the averaged state dict: the optimised parameters are the averages, everything else is live
    opt = run["history"]["optimizer"]
    names = {id(p): n for n, p in run["pl"].named_parameters()}
    averaged = {names[id(p)]: e for p, e in zip(params_of(opt), opt.ema_parameters())}
    assert len(averaged) > 20 and set(a["ema_state_dict"]) == set(a["state_dict"])
    for k, v in a["ema_state_dict"].items():
        want = averaged[k].cpu() if k in averaged else a["state_dict"][k]
        assert torch.equal(v, want), k
    assert any(not torch.equal(a["ema_state_dict"][k], a["state_dict"][k]) for k in averaged)
    # a run with another setting: a checkpoint without an average starts one, an average is ignored without ema_decay
    h = fit(new_module(), new_datamodule(runs["root"]), EPOCHS, val_frequency=1, resume=runs["plain"]["first"], log=lines.append, ema_decay=0.5)
    assert h["optimizer"].flat_state()["n_averaged"] == 2
    h = fit(new_module(), new_datamodule(runs["root"]), EPOCHS, val_frequency=1, resume=run["first"], log=lines.append)
    assert "n_averaged" not in h["optimizer"].flat_state()


def test_the_averaged_checkpoint_is_the_model_inside_averaged_weights(runs):
    from beat_this_amd.inference import averaged_checkpoint, load_checkpoint, load_model

    run = runs["ema"]
    opt, model = run["history"]["optimizer"], run["pl"].model
    x = torch.log1p(torch.rand(1, 150, 128, generator=torch.Generator().manual_seed(5)) * 30).to(dev())
    ckpt = load_checkpoint(run["ck"])
    loaded = load_model(averaged_checkpoint(ckpt), dev())
    live_model = load_model(ckpt, dev())
    with torch.no_grad():
        before = model(x)
        with opt.averaged_weights():
            inside = model(x)
        after = model(x)
        want, live = loaded(x), live_model(x)
    for k in ("beat", "downbeat"):
        assert torch.equal(tbits(inside[k]), tbits(want[k])), k
        assert torch.equal(tbits(before[k]), tbits(after[k])) and torch.equal(tbits(after[k]), tbits(live[k])), k
        assert not torch.equal(inside[k], live[k]), k
    with pytest.raises(ValueError, match="ema_state_dict"):
        averaged_checkpoint(load_checkpoint(runs["plain"]["ck"]))


def test_without_ema_decay_the_run_is_the_one_it_was(runs):
    from beat_this_amd.inference import load_checkpoint
    from beat_this_amd.train import CHECKPOINT_KEYS, validate

    plain = runs["plain"]
    ckpt = load_checkpoint(plain["ck"])
    assert set(ckpt) == set(CHECKPOINT_KEYS) and set(ckpt["optimizer_states"][0]) == {"state", "param_groups"}
    assert not any("averaged" in line for line in plain["lines"])
    # the calls fit() made before there was averaging, made by hand: the same weights
    pl = new_module()
    np.random.seed(0)
    dm = new_datamodule(runs["root"])
    dm.setup("fit")
    loader = dm.train_dataloader()
    conf = pl.configure_optimizers(max(1, len(loader) * EPOCHS), max_grad_norm=None, accumulate=1)
    optimizer, scheduler = conf["optimizer"], conf["lr_scheduler"]["scheduler"]
    optimizer.zero_grad()
    for _ in range(EPOCHS):
        for i, batch in enumerate(loader):
            pl.training_step(batch, i).backward()
            optimizer.step(accumulated=1)
            scheduler.step()
        validate(pl, dm)
    for (n, p), (_, q) in zip(plain["pl"].named_parameters(), pl.named_parameters()):
        assert torch.equal(tbits(p), tbits(q)), n
    # and averaging does not move the weights: the averaged run trained the same ones
    for (n, p), (_, q) in zip(plain["pl"].named_parameters(), runs["ema"]["pl"].named_parameters()):
        assert torch.equal(tbits(p), tbits(q)), n
    assert plain["history"]["train_loss"] == runs["ema"]["history"]["train_loss"]
