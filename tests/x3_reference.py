"""The contract twin of the "32-high" training precision, next to tests/route_reference.py and
tests/bf16_reference.py.  Every fp32 operand of a listed matrix product is the sum of two bfloat16 numbers,
    hi = bf16(a) (to nearest even),  lo = bf16(a - hi),  lo = 0 where hi is not finite,
and a product is A_lo B_hi + A_hi B_lo + A_hi B_hi, added in that order; the lo lo term is dropped.  ``_MatMul``, ``_AttnCore``
and ``_Conv`` below are route_reference.py's autograd functions with that product in place of ``r16(a) @ r16(b)``, in fp32 torch;
``high()`` puts them in its place for the length of a ``with`` block, the way ``bf16_reference.bfloat16()`` swaps ``r16``, so that
every ``*_grads`` function of route_grads.py serves unchanged.

``yardstick`` gives the fp64 truth, the twin, ``e_x3`` -- the twin's worst relative distance from the truth over every gradient
key -- and ``e_ref_bf16``, bf16_reference.py's (the oracle under CPU bfloat16 autocast).  The gate of the device is
``MIXED_GATE`` = 2 x e_x3 and the cap ``e_ref_bf16 / CAP`` on every gradient key, ``y`` and the logits.  The cases are
bf16_reference.py's, truth and e_ref_bf16 computed once and shared with it.  The module has bf16_reference.py's shape (see there).
"""
import contextlib

import torch
import torch.nn.functional as F

import bf16_reference as BF
import route_cases as RC
import route_grads as G
import route_reference as REF
from route_harness import MIXED_GATE as GATE

CAP = 64.0           # e_x3 and the device within e_ref_bf16 / 64: the halves keep 2^-17 of an operand where bfloat16 keeps 2^-9
CAP_EXEMPT = ()      # names of the cases that miss the cap on the CPU (test_x3_reference.py prints their ratios); never the gate
FORMAT = "bf16x3"
PRECISION = ("32-high", None)
LABEL, RECORD, E_NAME = "32-high", "high", "e_x3"
_CASES = {}


def split(t):
    """-> (hi, lo) in t's dtype"""
    hi = t.to(torch.bfloat16).to(t.dtype)
    lo = torch.where(torch.isfinite(hi), (t - hi).to(torch.bfloat16).to(t.dtype), torch.zeros_like(t))
    return hi, lo


def product(op, a, b, on=True):
    """op(a_lo, b_hi) + op(a_hi, b_lo) + op(a_hi, b_hi) for a bilinear ``op``; ``on`` False: op(a, b)"""
    if not on:
        return op(a, b)
    (ah, al), (bh, bl) = split(a), split(b)
    return op(al, bh) + op(ah, bl) + op(ah, bh)


def mm(a, b, on=True):
    return product(torch.matmul, a, b, on)


class _MatMul(torch.autograd.Function):
    """C = A B; dA = dC B^T, dB = A^T dC, each on split operands"""

    @staticmethod
    def forward(ctx, a, b, on):
        ctx.save_for_backward(a, b)
        ctx.on = on
        return mm(a, b, on)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        return mm(g, b.transpose(-1, -2), ctx.on), mm(a.transpose(-1, -2), g, ctx.on), None


class _AttnCore(torch.autograd.Function):
    """route_reference._AttnCore with every one of its six products on split operands: P m c, dS and the own side's q, k, v, dO
    are split like everything else"""

    @staticmethod
    def forward(ctx, q, k, v, mc, on):
        scale = q.shape[-1] ** -0.5
        p = torch.softmax(mm(q, k.transpose(-1, -2), on) * scale, dim=-1)
        pm = p if mc is None else p * mc
        o = mm(pm, v, on)
        ctx.save_for_backward(q, k, v, p, o, mc)
        ctx.on = on
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, p, o, mc = ctx.saved_tensors
        on, scale = ctx.on, q.shape[-1] ** -0.5
        pm = p if mc is None else p * mc
        delta = (do * o).sum(-1, keepdim=True)
        dp = mm(do, v.transpose(-1, -2), on)
        if mc is not None:
            dp = dp * mc
        ds = p * (dp - delta)
        dv = mm(pm.transpose(-1, -2), do, on)
        return mm(ds, k, on) * scale, mm(ds.transpose(-1, -2), q, on) * scale, dv, None, None


class _Conv(torch.autograd.Function):
    """route_reference._Conv with its three products on split operands; g is the gradient at the convolution's output"""

    @staticmethod
    def forward(ctx, x, w, on):
        ctx.save_for_backward(x, w)
        ctx.on = on
        return product(lambda a, b: F.conv2d(a, b, stride=(2, 1), padding=(0, 1)), x, w, on)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gx = product(lambda a, b: torch.nn.grad.conv2d_input(x.shape, a, b, stride=(2, 1), padding=(0, 1)), w, g, ctx.on)
        gw = product(lambda a, b: torch.nn.grad.conv2d_weight(a, w.shape, b, stride=(2, 1), padding=(0, 1)), x, g, ctx.on)
        return gx, gw, None


@contextlib.contextmanager
def high():
    """inside the block route_reference.py's restatement (``on`` = True) multiplies split operands"""
    real = REF._MatMul, REF._AttnCore, REF._Conv
    REF._MatMul, REF._AttnCore, REF._Conv = _MatMul, _AttnCore, _Conv
    try:
        yield
    finally:
        REF._MatMul, REF._AttnCore, REF._Conv = real


def yardstick(run, bf_case):
    """run(dtype, on, autocast) -> a ``*_grads`` result at loss scale 1; ``bf_case``: bf16_reference.py's case of the same inputs.
    -> dict(truth (fp64 oracle), yard (the twin: the contract in fp32), e = e_x3, e_ref_bf16)"""
    truth = bf_case["truth"]
    with high():
        twin = run(torch.float32, True, False)
    return dict(truth=truth, yard=twin, e=G.worst(twin, truth)[0], e_ref_bf16=bf_case["e"])


def _case(key, bf_case, run):
    if key not in _CASES:
        _CASES[key] = dict({k: v for k, v in bf_case.items() if k not in ("yard", "twin", "e")}, **yardstick(run, bf_case), name=key)
    return _CASES[key]


# ---- the cases: bf16_reference.py's, one for one --------------------------------------------------------------------------------------
def unit_case(kind, D, B, T, drop_stream=None):
    c = BF.unit_case(kind, D, B, T, drop_stream)
    run = lambda dt, on, ac: G.unit_grads(kind, c["sd"], c["pfx"], c["x"], c["g"], dt, on, 1.0, c["masks"], RC.DROP_P, autocast=ac)
    name = f"{kind} D={D} B={B} T={T}" + ("" if drop_stream is None else " dropout")
    return _case(name, c, run)


def trunk_case():
    c = BF.trunk_case()
    loss = G.trunk_loss(c["beat"], c["down"], c["mask"])
    return _case("trunk", c, lambda dt, on, ac: G.trunk_grads(c["sd"], c["h"], dt, RC.TRUNK["L"], loss, on, autocast=ac))


def conv_case(i, B, T, batch=False):
    c = BF.conv_case(i, B, T, batch)
    run = lambda dt, on, ac: G.conv_grads(c["sd"], i, c["x"], c["g"], dt, on, 1.0, autocast=ac, batch=batch)
    return _case(f"conv{i} B={B} T={T}" + (" batch statistics" if batch else ""), c, run)


def leaf_case(i, leaf, B, T):
    c = BF.leaf_case(i, leaf, B, T)
    return _case(f"block {i} {leaf} B={B} T={T}", c, lambda dt, on, ac: G.leaf_grads(c["sd"], i, leaf, c["x"], c["g"], dt, None, on, 1.0, autocast=ac))


def linear_case(B, T):
    c = BF.linear_case(B, T)
    return _case(f"projection B={B} T={T}", c, lambda dt, on, ac: G.linear_grads(c["sd"], c["x"], c["g"], dt, on, 1.0, autocast=ac))


def model_case():
    c = BF.model_case()
    loss_fn = G.trunk_loss(c["beat"], c["down"], c["mask"])
    return _case("whole model", c, lambda dt, on, ac: G.model_grads(c["sd"], c["x"], loss_fn, dt, on, 1.0, autocast=ac))


def gpu_cases():
    """(name, thunk) of every case the GPU gate uses, in its order"""
    out = []
    for kind in ("attn", "ff"):
        for D in sorted(RC.UNIT_DIMS):
            out += [(f"{kind} D={D} B={B} T={T}", lambda a=(kind, D, B, T): unit_case(*a)) for B, T in RC.UNIT_SIZES]
        out += [(f"{kind} D=64 B={B} T={T} dropout", lambda a=(kind, 64, B, T, 40 + i): unit_case(*a)) for i, (B, T) in enumerate(RC.DROP_SIZES)]
    out.append(("trunk", trunk_case))
    out += [(f"conv{i} B={B} T={T}", lambda a=(i, B, T): conv_case(*a)) for i, B, T in BF.CONV]
    out += [(f"conv{i} B={B} T={T} batch statistics", lambda a=(i, B, T): conv_case(*a, batch=True)) for i, B, T in BF.CONV_BN]
    out += [(f"block {i} {leaf} B={B} T={T}", lambda a=(i, leaf, B, T): leaf_case(*a)) for i, leaf, B, T in BF.LEAVES]
    out += [(f"projection B={B} T={T}", lambda a=(B, T): linear_case(*a)) for B, T in BF.LINEAR]
    out.append(("whole model", model_case))
    return out


# ---- the gate ---------------------------------------------------------------------------------------------------------------------
def gate(name, got, case, report=None, capped=()):
    """every gradient key of the truth, ``y`` and the logits finite, within GATE x e_x3 of the fp64 truth and within e_ref_bf16 /
    CAP (unless the case is in CAP_EXEMPT).  ``capped``: keys gated at the cap alone (a finding recorded in DESIGN.md section
    25).  Prints every figure before it asserts -> the worst distance in e_x3"""
    truth, e_x3, e_bf = case["truth"], case["e"], case["e_ref_bf16"]
    keys = G.grad_keys(truth) + BF.outputs_of(truth)
    assert 0 < e_x3 < float("inf") and 0 < e_bf < float("inf"), f"{name}: e_x3 = {e_x3}, e_ref_bf16 = {e_bf}"
    missing = [k for k in keys if k not in got]
    assert not missing, f"{name}: no value for {missing}"
    errs = {k: G.rel(got[k], truth[k]) for k in keys}
    k = max(errs, key=errs.get)
    print(f"{name}: e_x3 = {e_x3:.3e}, e_ref_bf16 = {e_bf:.3e} ({e_bf / e_x3:.0f} x), worst error = {errs[k]:.3e} "
          f"({errs[k] / e_x3:.2f} x e_x3, {k}; the twin's own {G.rel(case['yard'][k], truth[k]):.3e})")
    for key in BF.outputs_of(truth):
        print(f"{name}: {key} {errs[key]:.3e} ({errs[key] / e_x3:.2f} x e_x3)")
    if report is not None:
        report("high", case=name, e_x3=e_x3, e_ref_bf16=e_bf, worst_ratio=errs[k] / e_x3, worst_tensor=k)
    for key, e in errs.items():
        assert torch.isfinite(got[key]).all(), f"{name}: {key} is not finite"
        if key not in capped:
            assert e <= GATE * e_x3, f"{name}: {key} is {e:.3e} from the fp64 truth, the gate is 2 x e_x3 = {GATE * e_x3:.3e}"
        if case["name"] not in CAP_EXEMPT:
            assert e <= e_bf / CAP, f"{name}: {key} is {e:.3e} from the fp64 truth, the cap is e_ref_bf16 / 64 = {e_bf / CAP:.3e}"
    return errs[k] / e_x3
