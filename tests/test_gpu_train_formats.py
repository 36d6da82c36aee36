"""The operand formats of the training route beyond fp16, on the GPU (csrc/train_mixed.inc, csrc/train_front_mixed.inc): bfloat16
operands on the two 16-mixed routes and "32-high", fp32 products on three bfloat16 MFMAs over split
operands (section 25).

Every test here but the last runs once per format, over the reference modules of ``REFS`` (tests/bf16_reference.py,
tests/x3_reference.py: one shape, the cases one for one): the units, the trunk, the frontend's units and the whole model within the
format's gate of the fp64 truth -- 2 x e_ref_bf16, e_ref_bf16 the oracle's own error under CPU bfloat16 autocast at loss scale 1;
2 x e_x3 and e_ref_bf16 / 64, e_x3 the CPU contract twin's own error -- then bit identity and ``fit`` without a loss scale.  The
last refuses what no format knows.  What belongs to one format alone -- its exact arithmetic, its workspace, switching to it and
back -- is in tests/test_gpu_bf16.py and tests/test_gpu_train_high.py.  A new format: its reference module in ``REFS``.

Every device entry is called on gpu_util.Guarded buffers: guard bands on both sides, both poison patterns."""
import ctypes as C

import numpy as np
import pytest
import torch

import bf16_reference as BF
import route_cases as RC
import route_grads as RG
import route_harness as H
import x3_reference as X3
from gpu_util import POISONS, dev, report
from route_harness import MixedUnit, both_poisons, conv_dims, same_bits

pytestmark = pytest.mark.gpu
REFS = {R.FORMAT: R for R in (BF, X3)}
formats = pytest.mark.parametrize("fmt", list(REFS))
# keys gated at the cap e_ref_bf16 / 64 alone, by case name: findings recorded in DESIGN.md section 25 (none)
CAPPED = {}


def gate(R, name, got, case):
    return R.gate(name, got, case, report, CAPPED.get(case.get("name"), ()))


def abi_front(R, sd, unit, dims, B, T, x, gy, poison, batch=False):
    return H.abi_front_unit(sd, unit, dims, B, T, x, gy, poison, R.FORMAT, batch)


# ---- 1. the gate: units, trunk, frontend, whole model -----------------------------------------------------------------------------------
@formats
@pytest.mark.parametrize("D", sorted(RC.UNIT_DIMS))
@pytest.mark.parametrize("kind", ["attn", "ff"])
def test_units_within_the_gate(kind, D, fmt):
    R, worst = REFS[fmt], (0.0, None)
    for B, T in RC.UNIT_SIZES:
        case = R.unit_case(kind, D, B, T)
        name = f"{R.LABEL} {kind} D={D} B={B} T={T}"
        got = both_poisons(name, lambda q: MixedUnit(kind, D, case["x"], case["g"], 0, poison=q, ff_mult=RC.UNIT_DIMS[D], operand=fmt).run(None))
        worst = max(worst, (gate(R, name, got, case), (B, T)))
    print(f"{R.LABEL} {kind} D={D}: worst {worst[0]:.2f} x {R.E_NAME} at {worst[1]}")
    report(R.RECORD + "_unit", kind=kind, D=D, worst_ratio=worst[0], at=str(worst[1]))


@formats
@pytest.mark.parametrize("kind", ["attn", "ff"])
def test_units_with_dropout_within_the_gate(kind, fmt):
    """the masks of the truth are the host twin's (route_reference.unit_masks), the device evaluates its own"""
    R = REFS[fmt]
    for i, (B, T) in enumerate(RC.DROP_SIZES):
        stream = 40 + i
        case = R.unit_case(kind, 64, B, T, stream)
        name = f"{R.LABEL} dropout {kind} T={T}"
        got = both_poisons(name, lambda q: MixedUnit(kind, 64, case["x"], case["g"], 0, poison=q, operand=fmt).run((RC.DROP_P, RC.DROP_SEED, stream)))
        gate(R, name, got, case)


@formats
def test_trunk_and_heads_with_a_loss(fmt):
    R, c = REFS[fmt], RC.TRUNK
    case = R.trunk_case()
    hp = dict(transformer_dim=c["D"], ff_mult=c["ff_mult"], n_layers=c["L"])
    m = H.make_model(hp, H.state_dict(hp, 3, "lively"))
    for k, v in m.state_dict().items():
        assert torch.equal(v.cpu(), case["sd"][k]), k
    m.set_train_precision(*R.PRECISION)
    forward = lambda xd: m.task_heads(m.transformer_blocks(xd))
    got = H.loss_backward(forward, m, case["h"], case["beat"], case["down"], case["mask"])
    report(R.RECORD + "_trunk", **{R.E_NAME: case["e"]}, worst_ratio=gate(R, f"{R.LABEL} trunk", got, case))


@formats
@pytest.mark.parametrize("i,B,T", BF.CONV)
def test_conv_units_within_the_gate(i, B, T, fmt):
    R = REFS[fmt]
    case = R.conv_case(i, B, T)
    name = f"{R.LABEL} conv{i} B={B} T={T}"
    gate(R, name, both_poisons(name, lambda q: abi_front(R, case["sd"], "conv", conv_dims(i), B, T, case["x"], case["g"], q)), case)


@formats
@pytest.mark.parametrize("i,B,T", BF.CONV_BN)
def test_conv_units_with_batch_statistics(i, B, T, fmt):
    """the moved running buffers by the rule of section 19 (fp32 work on the conv's result): within 2 x max(e, 1e-7) of the fp64
    update, e the own distance of the format's yardstick run -- the bfloat16 autocast oracle, the split twin -- for that buffer"""
    R = REFS[fmt]
    case = R.conv_case(i, B, T, batch=True)
    name = f"{R.LABEL} conv{i} batch statistics B={B} T={T}"
    res, stats = both_poisons(name, lambda q: abi_front(R, dict(case["sd"]), "conv", conv_dims(i), B, T, case["x"], case["g"], q, batch=True))
    gate(R, name, res, case)
    for k, want in case["truth"]["stats"].items():
        if k.endswith("num_batches_tracked"):
            assert int(stats[k]) == int(want), k
            continue
        e = max(RG.rel(case["yard"]["stats"][k], want), 1e-7)
        err = RG.rel(stats[k], want)
        print(f"{name}: {k} yardstick {e:.3e}, device {err:.3e} ({err / e:.2f} x)")
        assert torch.isfinite(stats[k]).all() and err <= R.GATE * e, (name, k, err, e)


@formats
@pytest.mark.parametrize("i,leaf,B,T", BF.LEAVES)
def test_leaves_of_both_directions_within_the_gate(i, leaf, B, T, fmt):
    from beat_this_amd.model import backward as bw

    R = REFS[fmt]
    case = R.leaf_case(i, leaf, B, T)
    m = H.front_model(fmt)
    node, p = m.frontend.blocks[i].partial._modules[leaf], f"frontend.blocks.{i}.partial.{leaf}."

    def run():
        xd = case["x"].to(dev()).requires_grad_(True)
        if leaf.startswith("attn"):
            y = bw.attention(node, xd, *m._rope(xd.shape[1]), mixed=fmt, residual=True)
        else:
            y = bw.feedforward(node, xd, mixed=fmt, residual=True)
        params = [(p + n, q) for n, q in node.named_parameters() if not n.endswith("freqs")]
        grads = torch.autograd.grad([y], [xd] + [q for _, q in params], [case["g"].to(dev())])
        return dict(zip(["x"] + [n for n, _ in params], grads), y=y.detach())

    got, again = run(), run()
    assert len(got) == 7 and all(same_bits(got[k], again[k]) for k in got)
    gate(R, f"{R.LABEL} block {i} {leaf} B={B} T={T}", got, case)


@formats
@pytest.mark.parametrize("B,T", BF.LINEAR)
def test_projection_within_the_gate(B, T, fmt):
    R = REFS[fmt]
    case = R.linear_case(B, T)
    name = f"{R.LABEL} projection B={B} T={T}"
    gate(R, name, both_poisons(name, lambda q: abi_front(R, case["sd"], "linear", (4, 256, 64), B, T, case["x"], case["g"], q)), case)


@formats
def test_whole_model_with_both_parts_on_the_format(fmt):
    R = REFS[fmt]
    case = R.model_case()
    m = H.front_model(fmt)
    try:
        got = H.model_device(H.both_parts(m, *R.PRECISION), case["x"], case["beat"], case["down"], case["mask"])
    finally:
        H.both_parts(m, "32-true")
    keys = RG.grad_keys(case["truth"])
    assert set(keys) == set(got) - {"beat", "downbeat"} and len(keys) == 100
    report(R.RECORD + "_model", **{R.E_NAME: case["e"]}, worst_ratio=gate(R, f"{R.LABEL} whole model", got, case))


# ---- 2. bit identity ---------------------------------------------------------------------------------------------------------------
@formats
@pytest.mark.parametrize("kind", ["attn", "ff"])
def test_runs_are_bit_identical_and_a_sequence_alone_is_the_sequence_in_a_batch(kind, fmt):
    for drop in (None, (0.2, RC.DROP_SEED, 9)):
        name = f"{REFS[fmt].LABEL} {kind} drop={drop is not None}"
        first = both_poisons(name, lambda q: H.unit_run(kind, fmt, q, drop))
        again = H.unit_run(kind, fmt, drop=drop)
        assert all(same_bits(first[k], again[k]) for k in first), name
    plain = H.unit_run(kind, fmt)
    for b in range(3):   # (without dropout: the masks follow the row)
        alone = H.unit_run(kind, fmt, POISONS[b % 2], rows=slice(b, b + 1))
        assert same_bits(alone["x"][0], plain["x"][b]) and same_bits(alone["y"][0], plain["y"][b]), (kind, b)


@formats
def test_the_frontend_alone_and_in_a_batch(fmt):
    R, i = REFS[fmt], 0
    case = R.conv_case(i, 2, 65)
    both = abi_front(R, case["sd"], "conv", conv_dims(i), 2, 65, case["x"], case["g"], POISONS[0])
    alone = abi_front(R, case["sd"], "conv", conv_dims(i), 1, 65, case["x"][:1], case["g"][:1], POISONS[1])
    assert same_bits(alone["x"][0], both["x"][0]) and same_bits(alone["y"][0], both["y"][0])
    fp32 = H.abi_front_unit(case["sd"], "conv", conv_dims(i), 2, 65, case["x"], case["g"], POISONS[0])
    assert not same_bits(fp32["x"], both["x"])


# ---- 3. the loop -------------------------------------------------------------------------------------------------------------------
@formats
def test_fit_has_no_loss_scale_and_resumes_bit_for_bit(tmp_path, fmt):
    from beat_this_amd.train import CHECKPOINT_KEYS, fit
    from route_harness import new_datamodule, new_module

    precision, operand = REFS[fmt].PRECISION
    r = H.fit_and_resume(tmp_path, train_frontend=True, precision=precision, mixed_operand=operand, frontend_precision=precision,
                         frontend_mixed_operand=operand)
    m, h, root = r["pl"].model, r["h"], r["root"]
    assert (m.train_precision, m.frontend_precision) == (precision, precision) and not m.train_settings.needs_loss_scale()
    assert (m.train_operand, m.frontend_operand) == (operand or "fp16",) * 2
    assert h["loss_scaler"] is None and len(h["train_loss"]) == 2 and all(np.isfinite(v) and v < 10 for v in h["train_loss"])
    assert r["h2"]["loss_scaler"] is None and set(r["a"]) == set(r["b"]) == set(CHECKPOINT_KEYS) and "loss_scaler" not in r["first"]
    assert len(r["a"]["optimizer_states"][0]["state"]) == len(RG.all_keys(m.state_dict()))
    quiet = dict(train_frontend=True, log=lambda s: None)
    # beside a part on fp16 operands the loss is scaled ...
    h3 = fit(new_module(), new_datamodule(root), 0, precision=precision, mixed_operand=operand, frontend_precision="16-mixed", **quiet)
    assert h3["loss_scaler"] is not None
    # ... and beside none (bf16: the trunk alone) or beside bfloat16 ones (32-high: the trunk on bf16, the frontend on split operands) it is not
    if fmt == "bf16":
        h4 = fit(new_module(), new_datamodule(root), 0, precision="16-mixed", mixed_operand="bf16", log=lambda s: None)
    else:
        h4 = fit(new_module(), new_datamodule(root), 0, precision="16-mixed", mixed_operand="bf16", frontend_precision=precision, **quiet)
    assert h4["loss_scaler"] is None


# ---- 4. refusals before any launch ---------------------------------------------------------------------------------------------------
def test_refused_before_any_launch():
    """every pointer is null, so a launch would be seen; the shapes are valid, so the operand is what is refused"""
    from beat_this_amd import _lib as L

    lib, s = L.lib(), L.stream_ptr(dev())
    for operand in (2, 4, -1):
        for unit, hidden in ((L.UNIT_ATTN, 0), (L.UNIT_FF, 128)):
            a = L.TrainArgs(B=1, T=8, dim=64, hidden=hidden, operand=operand)
            for fn in (lib.bt_train_forward_mixed, lib.bt_train_backward_mixed):
                assert fn(s, unit, C.byref(a), None) == L.BT_ERR_ARG and b"operand" in lib.bt_last_error()
            for fn in (lib.bt_train_forward, lib.bt_train_backward):   # (never read there: the refusal is the null pointers')
                assert fn(s, unit, C.byref(a)) == L.BT_ERR_ARG and b"operand" not in lib.bt_last_error()
        for unit, (F_, C_, dim) in ((L.FRONT_CONV, (32, 32, 0)), (L.FRONT_LINEAR, (4, 256, 64))):
            a = L.FrontArgs(B=2, T=3, F=F_, C=C_, dim=dim, mixed=1, operand=operand)
            for fn in (lib.bt_front_forward, lib.bt_front_backward):
                assert fn(s, unit, C.byref(a)) == L.BT_ERR_ARG and b"operand" in lib.bt_last_error()
            a.mixed = 0                                                  # ignored with mixed = 0
            assert lib.bt_front_forward(s, unit, C.byref(a)) == L.BT_ERR_ARG and b"operand" not in lib.bt_last_error()
        b = L.FrontBnArgs(B=2, T=3, F=32, C=32, mixed=1, operand=operand)
        for fn in (lib.bt_front_bn_forward, lib.bt_front_bn_backward):
            assert fn(s, L.FRONT_CONV, C.byref(b)) == L.BT_ERR_ARG and b"operand" in lib.bt_last_error()
        b.mixed = 0
        assert lib.bt_front_bn_forward(s, L.FRONT_CONV, C.byref(b)) == L.BT_ERR_ARG and b"operand" not in lib.bt_last_error()
    for mixed in (3, 5, -1):
        assert lib.bt_train_matmul(s, mixed, 0, None, None, 1, 1, 1, None, None, None, 0, None, None, 0, 0, None, 0) == L.BT_ERR_ARG
        assert b"mixed" in lib.bt_last_error()
        assert lib.bt_train_attention(s, mixed, 0, 1, 8, 64, None, None, None, None, None, None, None) == L.BT_ERR_ARG
        assert b"mixed" in lib.bt_last_error()
    # the operand does not move a workspace size
    assert lib.bt_train_workspace_bytes_mixed(L.UNIT_ATTN, 1, 2, 33, 64, 0, 0) == lib.bt_train_workspace_bytes(L.UNIT_ATTN, 1, 2, 33, 64, 0)
    torch.cuda.synchronize()
