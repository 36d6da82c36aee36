"""The yardstick of the 16-mixed route without a GPU (tests/route_reference.py).

1. The hand-written backward formulas of the restatement: with the rounding switched off, its fp64 gradients are the oracle's
   autograd to 1e-12 relative.
2. ``e_ref16``, the worst tensor of the oracle under CPU fp16 autocast at loss scale 65536 against the fp64 truth, is what the
   GPU tests gate on (2 x e_ref16).  That gate means something only if the contract ALONE stays inside it: for every case the
   GPU tests run, the restatement in fp32 at scale 65536 has to lie within 1.0 x e_ref16.  A case that does not gets another
   seed or size, never a wider condition.
3. The loss scaler's update rule against ``torch.amp.GradScaler("cpu")`` over a scripted run of finite and non-finite steps.
"""
import math

import pytest
import torch

import route_cases as RC
import route_grads as RG
import route_reference as REF

_TRUNK = {}


def trunk_truth():
    if not _TRUNK:
        c = RC.TRUNK
        sd = RC.trunk_state_dict(c["D"], c["ff_mult"], c["L"])
        h, beat, down, mask = RC.trunk_batch()
        loss = RG.trunk_loss(beat, down, mask)
        _TRUNK.update(sd=sd, h=h, loss=loss, truth=RG.trunk_grads(sd, h, torch.float64, c["L"], loss, None))
    return _TRUNK


# ---- 1. the backward formulas --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["attn", "ff"])
@pytest.mark.parametrize("D", sorted(RC.UNIT_DIMS))
def test_unrounded_restatement_is_the_oracle(kind, D):
    sd, pfx = RC.trunk_state_dict(D, RC.UNIT_DIMS[D]), RC.PFX[kind]
    for B, T in ((3, 33), (1, 65)):
        x, g = RC.unit_inputs(kind, D, B, T)
        want = RG.oracle_unit_grads(kind, sd, pfx, x, g, torch.float64, heads=D // 32)
        got = RG.unit_grads(kind, sd, pfx, x, g, torch.float64, False)
        assert set(want) <= set(got)
        for k in want:
            assert RG.rel(got[k], want[k]) <= 1e-12, (kind, D, B, T, k, RG.rel(got[k], want[k]))
    # with masks: route_reference's masked units
    B, T = RC.DROP_SIZES[0]
    masks = REF.unit_masks(kind, RC.DROP_P, RC.DROP_SEED, 3, B, T, D, RC.UNIT_DIMS[D] * D)
    x, g = RC.unit_inputs(kind, D, B, T)
    want = RG.unit_grads(kind, sd, pfx, x, g, torch.float64, None, masks=masks, p=RC.DROP_P)
    got = RG.unit_grads(kind, sd, pfx, x, g, torch.float64, False, masks=masks, p=RC.DROP_P)
    for k in want:
        assert RG.rel(got[k], want[k]) <= 1e-12, (kind, D, "dropout", k, RG.rel(got[k], want[k]))


def test_unrounded_trunk_is_the_oracle():
    t, c = trunk_truth(), RC.TRUNK
    want = RG.oracle_trunk_grads(t["sd"], t["h"], None, None, torch.float64, c["L"], loss_fn=t["loss"])
    got = RG.trunk_grads(t["sd"], t["h"], torch.float64, c["L"], t["loss"], False)
    for k in want:
        assert RG.rel(got[k], want[k]) <= 1e-12, (k, RG.rel(got[k], want[k]))
        assert RG.rel(t["truth"][k], want[k]) <= 1e-12, k


# ---- 2. the contract alone stays within e_ref16 ----------------------------------------------------------------------------------
def contract_ratio(name, kind, D, B, T, stream=None):
    sd, pfx, x, g, masks, truth, auto, e_ref16 = RC.unit_case(kind, D, B, T, stream)
    got = RG.unit_grads(kind, sd, pfx, x, g, torch.float32, True, RG.SCALE, masks, RC.DROP_P)
    err, key = RG.worst(got, truth, RG.grad_keys(truth))
    print(f"{name}: e_ref16 = {e_ref16:.3e}, contract = {err:.3e} ({err / e_ref16:.2f} x e_ref16, {key})")
    return err, e_ref16


@pytest.mark.parametrize("kind", ["attn", "ff"])
@pytest.mark.parametrize("D", sorted(RC.UNIT_DIMS))
def test_contract_within_e_ref16_units(kind, D):
    for B, T in RC.UNIT_SIZES:
        err, e_ref16 = contract_ratio(f"{kind} D={D} B={B} T={T}", kind, D, B, T)
        assert err <= 1.0 * e_ref16, (kind, D, B, T, err, e_ref16)


@pytest.mark.parametrize("kind", ["attn", "ff"])
def test_contract_within_e_ref16_dropout(kind):
    for i, (B, T) in enumerate(RC.DROP_SIZES):
        err, e_ref16 = contract_ratio(f"dropout {kind} T={T}", kind, 64, B, T, stream=40 + i)
        assert err <= 1.0 * e_ref16, (kind, B, T, err, e_ref16)


def test_contract_within_e_ref16_trunk():
    t, c = trunk_truth(), RC.TRUNK
    auto = RG.trunk_grads(t["sd"], t["h"], torch.float32, c["L"], t["loss"], None, RG.SCALE, autocast=True)
    got = RG.trunk_grads(t["sd"], t["h"], torch.float32, c["L"], t["loss"], True, RG.SCALE)
    keys = RG.grad_keys(t["truth"])
    e_ref16, err = RG.worst(auto, t["truth"], keys)[0], RG.worst(got, t["truth"], keys)
    print(f"trunk: e_ref16 = {e_ref16:.3e}, contract = {err[0]:.3e} ({err[0] / e_ref16:.2f} x e_ref16, {err[1]})")
    assert err[0] <= 1.0 * e_ref16
    # (reported only: the same arithmetic without the loss scale; on this batch the gradients are large enough not to lose
    # more to fp16's subnormals than to its rounding)
    bare = RG.trunk_grads(t["sd"], t["h"], torch.float32, c["L"], t["loss"], True, 1.0)
    print(f"trunk without a loss scale: {RG.worst(bare, t['truth'], keys)[0]:.3e}")


# ---- 3. the loss scaler ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interval", [2, 3])
def test_scale_update_is_grad_scalers(interval):
    from beat_this_amd.optim import LossScaler, scale_update

    script = [False, False, True, False, True, True, False, False, False, False, True, False, False]
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=0.0)
    ref = torch.amp.GradScaler("cpu", init_scale=65536.0, growth_interval=interval)
    mine = LossScaler(growth_interval=interval)
    scale, tracker = 65536.0, 0
    for bad in script:
        ref.scale(torch.ones(()))                     # (initialises the reference's scale tensor)
        p.grad = torch.full((1,), math.inf if bad else 1.0)
        ref.step(opt)
        ref.update()
        mine.update(bad)
        scale, tracker = scale_update(scale, tracker, bad, growth_interval=interval)
        assert mine.scale == scale == ref.get_scale(), (bad, mine.scale, scale, ref.get_scale())
        assert mine.growth_tracker == tracker == ref._get_growth_tracker()
    assert mine.skipped_steps == sum(script)
    # growth stops at fp32's range, as torch's does; the state dict round-trips
    big = LossScaler(init_scale=2.0 ** 127, growth_interval=1)
    big.update(False)
    assert big.scale == 2.0 ** 127
    other = LossScaler()
    other.load_state_dict(mine.state_dict())
    assert other.state_dict() == mine.state_dict() and set(mine.state_dict()) == set(ref.state_dict())
