"""The yardstick of the bfloat16 operand format of the 16-mixed routes, next to tests/route_grads.py and
tests/route_reference.py, whose ``_run`` hard-codes fp16 autocast and whose ``r16`` hard-codes the fp16 rounding.  Two things are
restated here and put in their place for the length of a ``with bfloat16():`` block, so that every ``*_grads`` function of
route_grads.py serves unchanged:
  * the oracle under ``torch.autocast("cpu", dtype=torch.bfloat16)`` at loss scale 1 (``_run``: bfloat16 has fp32's exponent
    range, so the recipe has no scale and the yardstick takes none);
  * the contract twin: the fp32 oracle with both operands of every listed product rounded through ``torch.bfloat16`` (``rbf16``,
    round to nearest even) -- route_reference.py's restatement with one word changed.
``e_ref_bf16`` of a case is the worst relative distance of the autocast oracle's gradients from the fp64 oracle; the gate is the
project's ``MIXED_GATE`` = 2: the device within 2 x e_ref_bf16 on every gradient key, ``y`` and the logits.  The cases are
route_cases.py's, with its inputs; the fp64 truth does not depend on the operand format.

This module and tests/x3_reference.py have one shape, which tests/test_gpu_train_formats.py runs over: the constants below, the
case constructors, ``case["yard"]`` (the yardstick's own run) with ``case["e"]`` (its error), and ``gate``.
"""
import contextlib

import torch
import torch.nn.functional as F

import route_cases as RC
import route_grads as G
import route_reference as REF
from route_harness import MIXED_GATE as GATE

FORMAT = "bf16"                   # the name in _lib.OPERAND_FORMATS: ``mixed`` of model.backward, ``operand`` of the harness
PRECISION = ("16-mixed", "bf16")  # the arguments of set_train_precision / set_frontend_precision that put a part on it
LABEL, RECORD, E_NAME = "bf16", "bf16", "e_ref_bf16"   # in printed lines; the prefix of the report records; the field of case["e"] in them
_CASES = {}


def rbf16(t, on=True):
    """round to bfloat16 (to nearest even; NaN stays NaN, nothing overflows) and back"""
    return t.to(torch.bfloat16).to(t.dtype) if on else t


def training_batchnorm(stats):
    """``REF.training_batchnorm`` with bfloat16 inputs treated as it treats fp16 ones: the buffers stay fp32 under autocast"""
    def batchnorm(x, sd, pfx, ch_dim):
        assert ch_dim == 1
        dt = torch.float32 if x.dtype in (torch.float16, torch.bfloat16) else x.dtype
        mean = sd[pfx + "running_mean"].detach().to(dt).clone()
        var = sd[pfx + "running_var"].detach().to(dt).clone()
        y = F.batch_norm(x, mean, var, sd[pfx + "weight"], sd[pfx + "bias"], training=True, momentum=0.1, eps=1e-5)
        stats[pfx + "running_mean"], stats[pfx + "running_var"] = mean, var
        if pfx + "num_batches_tracked" in sd:
            stats[pfx + "num_batches_tracked"] = sd[pfx + "num_batches_tracked"].detach().clone() + 1
        return REF._PlainGrad.apply(y)
    return batchnorm


def _run(sd, x, keys, dtype, forward, scale=1.0, autocast=False, batch=False):
    """``G._run`` with ``autocast`` meaning CPU bfloat16 autocast"""
    leaf, xl = G._leaves(sd, x, dtype)
    stats = {}
    batchnorm = training_batchnorm if batch is True else batch
    with (REF.swapped(batchnorm(stats)) if batch else contextlib.nullcontext()):
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            outs, loss = forward(leaf, xl)
            (loss * scale).backward()
    res = {k: v / scale for k, v in G._collect(leaf, xl, keys).items()}
    res.update({k: v.detach() for k, v in outs.items()})
    if batch:
        res["stats"] = stats
    return res


@contextlib.contextmanager
def bfloat16():
    """inside the block route_reference.py's restatement rounds through bfloat16 and route_grads.py's autocast is bfloat16's"""
    real = REF.r16, G._run
    REF.r16, G._run = rbf16, _run
    try:
        yield
    finally:
        REF.r16, G._run = real


def yardstick(run):
    """run(dtype, on, autocast) -> a ``*_grads`` result at loss scale 1.  -> dict(truth (fp64 oracle), yard (the oracle under
    bfloat16 autocast), twin (the contract in fp32), e = e_ref_bf16)"""
    truth = run(torch.float64, None, False)
    with bfloat16():
        auto = run(torch.float32, None, True)
        twin = run(torch.float32, True, False)
    return dict(truth=truth, yard=auto, twin=twin, e=G.worst(auto, truth)[0])


def _case(key, make):
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


# ---- the trunk's units and the trunk (the cases of section 16) ----------------------------------------------------------------------
def unit_case(kind, D, B, T, drop_stream=None):
    """-> dict(sd, pfx, x, g, masks or None, truth, yard, twin, e): ``RC.unit_case``'s inputs under the bfloat16 yardstick"""
    def make():
        sd, pfx = RC.trunk_state_dict(D, RC.UNIT_DIMS[D]), RC.PFX[kind]
        x, g = RC.unit_inputs(kind, D, B, T)
        masks = None if drop_stream is None else REF.unit_masks(kind, RC.DROP_P, RC.DROP_SEED, drop_stream, B, T, D, RC.UNIT_DIMS[D] * D)
        run = lambda dt, on, ac: G.unit_grads(kind, sd, pfx, x, g, dt, on, 1.0, masks, RC.DROP_P, autocast=ac)
        return dict(yardstick(run), sd=sd, pfx=pfx, x=x, g=g, masks=masks)
    return _case(("unit", kind, D, B, T, drop_stream), make)


def trunk_case():
    """``RC.TRUNK`` with ``RC.trunk_batch`` and the shift-tolerant loss -> dict(sd, h, beat, down, mask, truth, yard, twin, e)"""
    def make():
        c = RC.TRUNK
        sd = RC.trunk_state_dict(c["D"], c["ff_mult"], c["L"])
        h, beat, down, mask = RC.trunk_batch()
        loss = G.trunk_loss(beat, down, mask)
        run = lambda dt, on, ac: G.trunk_grads(sd, h, dt, c["L"], loss, on, autocast=ac)
        return dict(yardstick(run), sd=sd, h=h, beat=beat, down=down, mask=mask)
    return _case("trunk", make)


# ---- the frontend (the smallest cases of section 19 that cross a tile) and the whole model ------------------------------------------
CONV = ((0, 2, 65), (2, 2, 3))      # (unit, B, T): 2080 rows -- three BT_TRAIN_DW_ROWS chunks, the last of 32 rows -- and 24 rows
CONV_BN = ((1, 2, 3),)              # 48 rows of 128 channels on batch statistics
LEAVES = ((0, "attnF", 2, 3), (0, "ffT", 2, 3))   # (block, leaf, B, T): 6 sequences of 32 tokens; 64 sequences of 3 tokens
LINEAR = ((2, 3),)
MODEL = (2, 33)                     # RC.model_inputs(2, 33, True), both parts on bfloat16


def conv_case(i, B, T, batch=False):
    def make():
        sd = RC.model_state_dict()
        x, g = RC.conv_inputs(i, B, T)
        run = lambda dt, on, ac: G.conv_grads(sd, i, x, g, dt, on, 1.0, autocast=ac, batch=batch)
        return dict(yardstick(run), sd=sd, x=x, g=g)
    return _case(("conv", i, B, T, batch), make)


def leaf_case(i, leaf, B, T):
    """one leaf of block i as the unit call with its residual runs it, on the rows of a (B, T) batch: x, g (B', T', C)"""
    def make():
        sd = RC.model_state_dict()
        shape = REF.leaf_shape(i, leaf, B, T)
        gen = torch.Generator().manual_seed(7000 + 100 * i + 10 * T + B + len(leaf))
        x, g = torch.randn(*shape, generator=gen), torch.randn(*shape, generator=gen) * 2.0 ** -14
        run = lambda dt, on, ac: G.leaf_grads(sd, i, leaf, x, g, dt, None, on, 1.0, autocast=ac)
        return dict(yardstick(run), sd=sd, x=x, g=g)
    return _case(("leaf", i, leaf, B, T), make)


def linear_case(B, T):
    def make():
        sd = RC.model_state_dict()
        x, g = RC.linear_inputs(B, T)
        run = lambda dt, on, ac: G.linear_grads(sd, x, g, dt, on, 1.0, autocast=ac)
        return dict(yardstick(run), sd=sd, x=x, g=g)
    return _case(("linear", B, T), make)


def model_case():
    def make():
        sd = RC.model_state_dict("lively", True)
        x, beat, down, mask = RC.model_inputs(*MODEL, True)
        loss_fn = G.trunk_loss(beat, down, mask)
        run = lambda dt, on, ac: G.model_grads(sd, x, loss_fn, dt, on, 1.0, autocast=ac)
        return dict(yardstick(run), sd=sd, x=x, beat=beat, down=down, mask=mask)
    return _case("model", make)


# ---- the gate ---------------------------------------------------------------------------------------------------------------------
def outputs_of(truth):
    return [k for k in ("y", "beat", "downbeat") if k in truth]


def gate(name, got, case, report=None, capped=()):
    """every gradient key of the truth, ``y`` and the logits within GATE x e_ref_bf16 of the fp64 truth and finite (``capped``:
    x3_reference.gate's; this format has no cap, so no key can be gated at it alone).  Prints every figure before it asserts ->
    the worst distance in e_ref_bf16"""
    truth, e_ref = case["truth"], case["e"]
    assert not capped, f"{name}: bfloat16 has no cap to gate {capped} at"
    keys = G.grad_keys(truth) + outputs_of(truth)
    assert e_ref > 0 and e_ref < float("inf"), f"{name}: e_ref_bf16 = {e_ref}"
    missing = [k for k in keys if k not in got]
    assert not missing, f"{name}: no value for {missing}"
    errs = {k: G.rel(got[k], truth[k]) for k in keys}
    k = max(errs, key=errs.get)
    print(f"{name}: e_ref_bf16 = {e_ref:.3e}, worst error = {errs[k]:.3e} ({errs[k] / e_ref:.2f} x e_ref_bf16, {k})")
    for key in outputs_of(truth):
        print(f"{name}: {key} {errs[key]:.3e} ({errs[key] / e_ref:.2f} x e_ref_bf16)")
    if report is not None:
        report("bf16", case=name, e_ref_bf16=e_ref, worst_ratio=errs[k] / e_ref, worst_tensor=k)
    for key, e in errs.items():
        assert torch.isfinite(got[key]).all(), f"{name}: {key} is not finite"
        assert e <= GATE * e_ref, f"{name}: {key} is {e:.3e} from the fp64 truth, the gate is 2 x e_ref_bf16 = {GATE * e_ref:.3e}"
    return errs[k] / e_ref
