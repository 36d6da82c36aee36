"""The 16-mixed training route on the GPU (csrc/train_mixed.inc): the fp16 MFMA GEMM exactly, the units,
the trunk with a loss and dropout against the fp64 truth with the yardstick of tests/route_reference.py -- every gradient within
2 x e_ref16, where e_ref16 is the reference's own 16-mixed error (the oracle under CPU fp16 autocast at loss scale 65536) and
the factor 2 covers that the device and autocast are different roundings of the same size (the contract alone sits at 0.3 .. 0.9
x e_ref16, tests/test_mixed_reference.py; a wrong tile index, a wrong transposition or a lost remainder moves a tensor by 1e-2
or more) -- then determinism and isolation, the loss scaler in the optimiser step, and ``fit(precision="16-mixed")``.

Every device entry is called on gpu_util.Guarded buffers: guard bands on both sides, both poison patterns."""
import ctypes as C

import numpy as np
import pytest
import torch

import route_cases as RC
import route_grads as RG
import route_harness as H
from gpu_util import POISONS, Guarded, assert_intact, dev, report
from route_harness import EDGES, EPOCHS, KS, MIXED_GATE as GATE, MixedUnit, Unit, new_datamodule, new_module, randn, same_bits

pytestmark = pytest.mark.gpu


def unscaled(res):
    """the gradients of a run whose upstream gradient carried the loss scale, divided by it in fp32"""
    return {k: (v if k in ("y", "save_o", "save_lse") else v / RG.SCALE) for k, v in res.items()}


def gate(name, got, truth, e_ref16, keys):
    return H.mixed_gate(name, got, truth, e_ref16, keys)


# ---- 1. exact products -------------------------------------------------------------------------------------------------------------
def matmul_exact(form, M, N, K, poison, seed):
    from beat_this_amd import _lib as L

    rng = np.random.default_rng(seed)
    a = rng.integers(-8, 9, size=(K, M) if form == 2 else (M, K))
    b = rng.integers(-8, 9, size=(N, K) if form == 0 else (K, N))
    want = (a.T if form == 2 else a).astype(np.int64) @ (b.T if form == 0 else b).astype(np.int64)
    ga = Guarded(a.shape, torch.float32).fill(poison, data=torch.from_numpy(a.astype(np.float32)).to(dev()))
    gb = Guarded(b.shape, torch.float32).fill(poison, data=torch.from_numpy(b.astype(np.float32)).to(dev()))
    gc = Guarded((M, N), torch.float32).fill(poison)
    L.check(L.lib().bt_train_matmul_mixed(L.stream_ptr(dev()), form, ga.ptr(), gb.ptr(), M, N, K, gc.ptr()))
    torch.cuda.synchronize()
    assert_intact(("A", ga), ("B", gb), ("C", gc))
    got = gc.t.cpu().numpy()
    assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32)), (form, M, N, K)


@pytest.mark.parametrize("form", [0, 1, 2])
def test_products_of_small_integers_are_exact(form):
    """operands in [-8, 8]: every partial sum is an integer below 2^24, exact in fp32 whatever the MFMA's internal order"""
    n = 0
    for i, M in enumerate(EDGES):
        for j in range(3):   # (three of the N per M, all of them over the M)
            N = EDGES[(i + 4 * j + form) % len(EDGES)]
            for K in KS:
                matmul_exact(form, M, N, K, POISONS[n % 2], 1000 * form + n)
                n += 1
    if form == 2:   # the summed rows on both sides of a BT_TRAIN_DW_ROWS chunk
        for K in (1023, 1024, 1025):
            for poison in POISONS:
                matmul_exact(2, 33, 129, K, poison, K)


# ---- 2. units ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", sorted(RC.UNIT_DIMS))
@pytest.mark.parametrize("kind", ["attn", "ff"])
def test_units_within_twice_e_ref16(kind, D):
    worst, away = (0.0, None), 0.0
    for i, (B, T) in enumerate(RC.UNIT_SIZES):
        sd, pfx, x, g, _, truth, _, e_ref16 = RC.unit_case(kind, D, B, T)
        got = unscaled(MixedUnit(kind, D, x, g * RG.SCALE, 0, poison=POISONS[i % 2], ff_mult=RC.UNIT_DIMS[D]).run(None))
        keys = RG.grad_keys(truth)
        ratio = gate(f"mixed {kind} D={D} B={B} T={T}", got, truth, e_ref16, keys)
        worst = max(worst, (ratio, (B, T)))
        # reported, not gated: how far the device is from the fp32 restatement of its own contract
        rest = RG.unit_grads(kind, sd, pfx, x, g, torch.float32, True, RG.SCALE)
        away = max(away, max(RG.rel(got[k], rest[k]) for k in keys))
        assert RG.rel(got["y"], truth["y"]) <= GATE * e_ref16
    print(f"mixed {kind} D={D}: worst {worst[0]:.2f} x e_ref16 at {worst[1]}, at most {away:.3e} from the restatement")
    report("mixed_unit", kind=kind, D=D, worst_ratio=worst[0], at=str(worst[1]), from_restatement=away)


# ---- 3. trunk and heads with a loss -------------------------------------------------------------------------------------------------
def trunk_device(m, h, beat, down, mask, scale):
    return H.loss_backward(lambda xd: m.task_heads(m.transformer_blocks(xd)), m, h, beat, down, mask, scale)


def test_trunk_and_heads_with_a_loss():
    c = RC.TRUNK
    hp = dict(transformer_dim=c["D"], ff_mult=c["ff_mult"], n_layers=c["L"])
    m = H.make_model(hp, H.state_dict(hp, 3, "lively"))
    sd = RC.trunk_state_dict(c["D"], c["ff_mult"], c["L"])
    for k, v in m.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k
    h, beat, down, mask = RC.trunk_batch()
    loss = RG.trunk_loss(beat, down, mask)
    truth = RG.trunk_grads(sd, h, torch.float64, c["L"], loss, None)
    auto = RG.trunk_grads(sd, h, torch.float32, c["L"], loss, None, RG.SCALE, autocast=True)
    keys = RG.grad_keys(truth)
    e_ref16 = RG.worst(auto, truth, keys)[0]
    assert np.isfinite(e_ref16)
    try:
        got = trunk_device(m.set_train_precision("16-mixed"), h, beat, down, mask, RG.SCALE)
    finally:
        m.set_train_precision("32-true")
    assert set(keys) <= set(got)
    ratio = gate("mixed trunk", got, truth, e_ref16, keys)
    for k in ("beat", "downbeat"):
        e16, e = RG.rel(auto[k], truth[k]), RG.rel(got[k], truth[k])
        print(f"mixed trunk {k} logits: autocast {e16:.3e}, device {e:.3e}")
        assert e <= GATE * e16, (k, e, e16)
    report("mixed_trunk", e_ref16=e_ref16, worst_ratio=ratio)


# ---- 4. dropout composes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["attn", "ff"])
def test_dropout_composes(kind):
    for i, (B, T) in enumerate(RC.DROP_SIZES):
        stream = 40 + i
        sd, pfx, x, g, masks, truth, _, e_ref16 = RC.unit_case(kind, 64, B, T, stream)
        got = unscaled(MixedUnit(kind, 64, x, g * RG.SCALE, 0, poison=POISONS[i % 2]).run((RC.DROP_P, RC.DROP_SEED, stream)))
        ratio = gate(f"mixed dropout {kind} T={T}", got, truth, e_ref16, RG.grad_keys(truth))
        assert RG.rel(got["y"], truth["y"]) <= GATE * e_ref16
        report("mixed_dropout", kind=kind, T=T, worst_ratio=ratio)


# ---- 5. determinism and isolation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["attn", "ff"])
def test_runs_are_bit_identical_whatever_the_poison(kind):
    D, B, T = 64, 3, 130
    x, g = randn(B, T, D, seed=51), randn(B, T, D, seed=52)
    word = int.from_bytes(bytes([POISONS[1]] * 4), "little")
    for drop in (None, (0.2, RC.DROP_SEED, 9)):
        res = [MixedUnit(kind, D, x, g, 1, poison=q).run(drop) for q in POISONS]
        again = MixedUnit(kind, D, x, g, 1).run(drop)
        for k in res[0]:
            assert same_bits(res[0][k], res[1][k]), f"{kind}: {k} depends on the poison"
            assert same_bits(res[0][k], again[k]), f"{kind}: {k} differs between two runs"
            assert torch.isfinite(res[0][k]).all(), f"{kind}: {k} keeps bytes of the 0xFF poison (or is not finite)"
            assert not (res[1][k].view(torch.int32) == word).any(), f"{kind}: {k} keeps words of the 0x7B poison"
        for b in range(B):   # a sequence's gx and y are the same alone and in the batch (without dropout: the masks follow the row)
            if drop is None:
                alone = MixedUnit(kind, D, x[b:b + 1], g[b:b + 1], 1).run(None)
                assert same_bits(alone["x"][0], again["x"][b]) and same_bits(alone["y"][0], again["y"][b]), (kind, b)
    # the route differs from the fp32 one, and one byte short of the workspace is refused before any launch
    plain = Unit(kind, D, x, g, 1).run(None, entry="plain")
    assert not same_bits(plain["x"], again["x"])
    u = MixedUnit(kind, D, x, g, 1)
    for backward in (0, 1):
        for drop in (None, (0.2, RC.DROP_SEED, 9)):
            assert u.call(backward, drop, ws_bytes=u.ws_bytes(backward, drop) - 1) == u.L.BT_ERR_WORKSPACE


def test_other_units_are_refused():
    from beat_this_amd import _lib as L

    a = L.TrainArgs()
    for unit in (L.UNIT_NORM, L.TRAIN_UNIT_HEAD, L.UNIT_STEM):
        assert L.lib().bt_train_workspace_bytes_mixed(unit, 1, 1, 8, 64, 128, 0) == 0
        assert L.lib().bt_train_forward_mixed(None, unit, C.byref(a), None) == L.BT_ERR_ARG
        assert L.lib().bt_train_backward_mixed(None, unit, C.byref(a), None) == L.BT_ERR_ARG
    assert L.lib().bt_train_matmul_mixed(None, 3, None, None, 1, 1, 1, None) == L.BT_ERR_ARG


def model_grads(m, spect, beat, down, mask):
    from beat_this_amd.model.loss import ShiftTolerantBCELoss

    m.zero_grad(set_to_none=True)
    out = m(spect)
    fn = ShiftTolerantBCELoss().to(dev())
    (fn(out["beat"], beat, mask) + fn(out["downbeat"], down, mask)).backward()
    res = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    return res


def fresh_model():
    """a D = 64, 2-layer model of its own (the tests below switch its precision and step its weights)"""
    hp = dict(transformer_dim=64, ff_mult=2, n_layers=2)
    return H.make_model(hp, H.state_dict(hp, 3, "lively"))


def small_batch(seed=61):
    gen = torch.Generator().manual_seed(seed)
    spect = torch.log1p(torch.rand(2, 150, 128, generator=gen) * 30).to(dev())
    beat = (torch.rand(2, 150, generator=gen) < 0.06).float().to(dev())
    return spect, beat, beat, torch.ones(2, 150, dtype=torch.bool, device=dev())


def test_switching_back_leaves_the_fp32_route_as_it_was():
    never, switched = fresh_model(), fresh_model()
    args = small_batch()
    assert never.train_precision == "32-true"
    want = model_grads(never, *args)
    assert switched.set_train_precision("16-mixed") is switched and switched.train_precision == "16-mixed"
    mixed = model_grads(switched, *args)
    assert len(mixed) == len(want) > 20 and any(not same_bits(mixed[k], want[k]) for k in want)
    for k in want:   # (another rounding of the same gradients, not other gradients)
        assert RG.rel(mixed[k], want[k]) < 5e-2, k
    with torch.no_grad():   # inference never looks at the switch
        a, b = never(args[0]), switched(args[0])
    assert same_bits(a["beat"], b["beat"]) and same_bits(a["downbeat"], b["downbeat"])
    switched.set_train_precision("32-true")
    back = model_grads(switched, *args)
    for k in want:
        assert same_bits(back[k], want[k]), k
    with pytest.raises(ValueError):
        switched.set_train_precision("bf16-mixed")


# ---- 6. loss scaling ---------------------------------------------------------------------------------------------------------------
def test_the_optimiser_skips_a_step_with_non_finite_gradients():
    from beat_this_amd.model.loss import ShiftTolerantBCELoss
    from beat_this_amd.optim import AdamW, LossScaler, param_groups_for

    m = fresh_model().set_train_precision("16-mixed")
    spect, beat, down, mask = small_batch()
    fn = ShiftTolerantBCELoss().to(dev())
    opt = AdamW(param_groups_for(m, 0.01), lr=1e-3, max_grad_norm=1.0)
    params = [p for g in opt.param_groups for p in g["params"]]

    def backward(scale):
        out = m(spect)
        ((fn(out["beat"], beat, mask) + fn(out["downbeat"], down, mask)) * scale).backward()

    def state():
        st = opt.flat_state()
        return [p.detach().clone() for p in params] + [st["exp_avg"].clone(), st["exp_avg_sq"].clone()], st["step"]

    backward(65536.0)
    opt.step(loss_scaler=LossScaler())   # (one finite step first, so that m, v and the step count are not their initial zeros)
    assert not opt.last_step_skipped
    before, step0 = state()
    scaler = LossScaler(init_scale=2.0 ** 40, growth_interval=2)
    backward(scaler.scale)               # at 2^40 the backward's fp16 operands overflow: the gradients are not finite
    assert not all(torch.isfinite(p.grad).all() for p in params)
    opt.step(loss_scaler=scaler)
    after, step1 = state()
    assert opt.last_step_skipped and step1 == step0
    for a, b in zip(before, after):
        assert same_bits(a, b)
    assert not opt.flat_state()["grad"].any() and all(not p.grad.any() for p in params)
    assert scaler.scale == 2.0 ** 39 and scaler.growth_tracker == 0 and scaler.skipped_steps == 1
    # the next steps at 65536 update the parameters; with growth interval 2 the scale doubles after two finite steps
    scaler.scale = 65536.0
    for n in (1, 2):
        backward(scaler.scale)
        opt.step(loss_scaler=scaler)
        assert not opt.last_step_skipped and opt.flat_state()["step"] == step0 + n
        assert scaler.scale == (65536.0 if n == 1 else 131072.0) and scaler.growth_tracker == n % 2
        assert np.isfinite(opt.last_grad_norm())
    moved = sum(not same_bits(p.detach(), b) for p, b in zip(params, before))
    assert moved > 20, moved   # (a parameter whose gradient is exactly zero and that is not decayed stays)
    # unscaling is exact (the scale is a power of two): an fp32 step from gradients scaled by 65536 is the unscaled step
    twins = []
    for scale in (None, 65536.0):
        gen = torch.Generator().manual_seed(71)
        ps = [torch.nn.Parameter(torch.randn(n, generator=gen).to(dev())) for n in (1000, 5000, 7)]
        o = AdamW(ps, lr=1e-2, max_grad_norm=1.0)
        (sum((p ** 2).sum() for p in ps) * 1e-3 * (scale or 1.0)).backward()
        o.step(**({} if scale is None else {"loss_scaler": LossScaler(init_scale=scale)}))
        twins.append(ps)
    for p, q in zip(*twins):
        assert same_bits(p.detach(), q.detach())


# ---- 7. the loop -------------------------------------------------------------------------------------------------------------------
def test_fit_in_16_mixed_resumes_bit_for_bit(tmp_path):
    from beat_this_amd.inference import load_checkpoint, load_model
    from beat_this_amd.train import CHECKPOINT_KEYS, fit

    r = H.fit_and_resume(tmp_path, precision="16-mixed")
    pl, h, h2, a, b, root = (r[k] for k in ("pl", "h", "h2", "a", "b", "root"))
    ck, ck32 = str(tmp_path / "run.ckpt"), str(tmp_path / "fp32.ckpt")
    assert pl.model.train_precision == "16-mixed" and h["loss_scaler"].scale == 65536.0 and h["loss_scaler"].growth_tracker == 4
    assert all(np.isfinite(v) and v < 10 for v in h["train_loss"])   # (reported unscaled)
    assert set(a) == set(CHECKPOINT_KEYS) | {"loss_scaler"} and a["loss_scaler"] == b["loss_scaler"] == h2["loss_scaler"].state_dict()
    assert r["first"]["loss_scaler"]["_growth_tracker"] == 2
    # the checkpoint is an ordinary one
    loaded = load_model(ck, dev())
    x = torch.log1p(torch.rand(1, 150, 128, generator=torch.Generator().manual_seed(5)) * 30).to(dev())
    with torch.no_grad():
        assert same_bits(loaded(x)["beat"], pl.model(x)["beat"])
    # a checkpoint written without the feature resumes in fp32, and a 16-mixed run resumes from it with a fresh scaler
    pl3 = new_module()
    np.random.seed(0)
    fit(pl3, new_datamodule(root), 1, val_frequency=1, checkpoint_path=ck32, log=lambda s: None)
    assert "loss_scaler" not in load_checkpoint(ck32)
    h4 = fit(new_module(), new_datamodule(root), EPOCHS, val_frequency=1, resume=ck32, log=lambda s: None)
    assert h4["loss_scaler"] is None and len(h4["train_loss"]) == 1
