""""32-high" on the GPU (csrc/train_mixed.inc, csrc/train_front_mixed.inc with Operand<bf16x3>): fp32
products on three bfloat16 MFMAs over split operands.  The GEMM exactly -- a split operand against an 8-bit one, two split
operands minus their lo lo term in int64, inf and NaN rows -- then the units, the trunk, the frontend's units and the whole model
within 2 x e_x3 of the fp64 truth and within e_ref_bf16 / 64 (tests/x3_reference.py: e_x3 is the CPU contract twin's own error),
bit identity, no bleed into the other precisions, refusals, and ``fit`` without a loss scale.

Every device entry is called on gpu_util.Guarded buffers: guard bands on both sides, both poison patterns."""
import contextlib
import ctypes as C
import shutil

import numpy as np
import pytest
import torch

import bf16_reference as BF
import route_cases as RC
import route_grads as RG
import route_harness as H
import x3_reference as X3
from dataset_reference import build_data_folder
from gpu_util import POISONS, assert_intact, dev, report
from route_harness import both_poisons, same_bits
from test_gpu_bf16 import conv_dims, matmul
from test_gpu_mixed import EDGES, KS, MixedUnit

pytestmark = pytest.mark.gpu
X3M, BF16M = 4, 2        # `mixed` of bt_train_matmul / bt_train_attention: 1 + BT_OPERAND_*
OPERAND_X3 = 3
HIGH = "32-high"


# ---- 1. exact products -------------------------------------------------------------------------------------------------------------
def odd_ints(rng, shape, lo_bits, hi_bits):
    """odd integers of lo_bits .. hi_bits significant bits, either sign"""
    bits = rng.integers(lo_bits, hi_bits + 1, size=shape)
    v = (1 << (bits - 1)) | rng.integers(0, 1 << 62, size=shape) % (1 << (bits - 1)) | 1
    return v * rng.choice([-1, 1], size=shape)


def halves(v):
    hi, lo = X3.split(torch.from_numpy(np.asarray(v, dtype=np.float32)))
    return hi.numpy().astype(np.int64), lo.numpy().astype(np.int64)


def shapes(form, M, N, K):
    return ((K, M) if form == 2 else (M, K)), ((N, K) if form == 0 else (K, N))


def as_mk_kn(form, a, b):
    """the operands as A [M, K] and B [K, N] whatever the form stores"""
    return (a.T if form == 2 else a), (b.T if form == 0 else b)


def split_against_eight_bits(form, M, N, K, seed, also_bf16=False):
    """(a): A needs 9 to 12 significant bits, B at most 8 and so small that every partial sum of |a b| stays below 2^24: A = hi +
    lo exactly, B has no lo half, the three terms are sums of integers"""
    rng = np.random.default_rng(seed)
    sa, sb = shapes(form, M, N, K)
    bmax = max(1, min(255, (1 << 24) // (4200 * K)))
    a, b = odd_ints(rng, sa, 9, 12), rng.integers(-bmax, bmax + 1, size=sb)
    A, B = as_mk_kn(form, a, b)
    want = A.astype(np.int64) @ B.astype(np.int64)
    assert (np.abs(A).astype(np.int64) @ np.abs(B).astype(np.int64)).max() < 1 << 24
    for poison in POISONS:
        got = matmul(X3M, form, a, b, M, N, K, poison)
        assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32)), (form, M, N, K, poison)
    if also_bf16:   # which route ran: plain bfloat16 keeps 8 bits of A
        assert np.abs(want).max() > 0 and not np.array_equal(matmul(BF16M, form, a, b, M, N, K, POISONS[0]), want.astype(np.float32))


def both_split(form, M, N, K, seed):
    """(b): both operands need a lo half: 9-bit odd integers, B non-zero on at most 60 of the k (60 x 515^2 < 2^24).  The result is
    A B - A_lo B_lo in int64, exactly"""
    rng = np.random.default_rng(seed)
    sa, sb = shapes(form, M, N, K)
    a, b = odd_ints(rng, sa, 9, 9), odd_ints(rng, sb, 9, 9)
    if K > 60:
        dead = rng.permutation(K)[60:]
        if form == 0:
            b[:, dead] = 0
        else:
            b[dead, :] = 0
    A, B = as_mk_kn(form, a, b)
    (_, al), (_, bl) = halves(A), halves(B)
    assert np.abs(al).max() > 0 and np.abs(bl).max() > 0
    want = A.astype(np.int64) @ B.astype(np.int64) - al @ bl
    got = matmul(X3M, form, a, b, M, N, K, POISONS[seed % 2])
    assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32)), (form, M, N, K)


def walk(form):
    n = 0
    for i, M in enumerate(EDGES):
        for j in range(3):   # (three of the N per M, all of them over the M: the walk of test_gpu_bf16.py)
            N = EDGES[(i + 4 * j + form) % len(EDGES)]
            for K in KS:
                yield M, N, K, 3000 * form + n
                n += 1
    if form == 2:   # the summed rows on both sides of a BT_TRAIN_DW_ROWS chunk
        for K in (1023, 1024, 1025):
            yield 33, 129, K, K


@pytest.mark.parametrize("form", [0, 1, 2])
def test_a_split_operand_against_an_eight_bit_one_is_exact(form):
    for M, N, K, seed in walk(form):
        split_against_eight_bits(form, M, N, K, seed)
    split_against_eight_bits(form, 33, 65, 17, 7, also_bf16=True)


@pytest.mark.parametrize("form", [0, 1, 2])
def test_two_split_operands_lose_the_lo_lo_term_and_nothing_else(form):
    for M, N, K, seed in walk(form):
        both_split(form, M, N, K, seed)


@pytest.mark.parametrize("form", [0, 1, 2])
def test_an_overflow_stays_an_overflow_and_a_nan_stays_in_its_row(form):
    """(c): row 0 of A holds +inf, row 1 holds 3.4e38 (hi = inf, lo = 0 by the rule), row 2 a NaN; B is positive with positive lo
    halves (integer + 2^-10).  Rows 0 and 1 are +inf, row 2 NaN, the rest exact."""
    inf = float("inf")
    for M, N, K in ((5, 7, 9), (33, 65, 17), (65, 33, 100)):
        rng = np.random.default_rng(M + K)
        A = rng.integers(0, 9, size=(M, K)).astype(np.float64)
        B = rng.integers(1, 9, size=(K, N)) + 2.0 ** -10
        assert bool((X3.split(torch.from_numpy(B.astype(np.float32)))[1] > 0).all())
        want = A @ B
        A[0, K // 2], A[1, K - 1], A[2, 0] = inf, 3.4e38, float("nan")
        a, b = (A.T if form == 2 else A), (B.T if form == 0 else B)
        got = matmul(X3M, form, a, b, M, N, K, POISONS[K % 2])
        assert (got[:2] == inf).all() and np.isnan(got[2]).all(), (form, M, N, K, got[:3])
        assert np.array_equal(got[3:], want[3:].astype(np.float32)), (form, M, N, K)


# ---- 2. the gate --------------------------------------------------------------------------------------------------------------------
# keys gated at the cap e_ref_bf16 / 64 alone, by case name: findings recorded in DESIGN.md section 25 (none)
CAPPED = {}


class HighUnit(MixedUnit):
    """test_gpu_mixed.MixedUnit with bt_train_args.operand = BT_OPERAND_BF16X3 (unless told otherwise)"""

    def __init__(self, *args, operand=OPERAND_X3, **kw):
        super().__init__(*args, **kw)
        self.a.operand = operand


def gate(name, got, case):
    return X3.gate(name, got, case, report, CAPPED.get(case["name"], ()))


@pytest.mark.parametrize("D", sorted(RC.UNIT_DIMS))
@pytest.mark.parametrize("kind", ["attn", "ff"])
def test_units_within_twice_e_x3(kind, D):
    worst = (0.0, None)
    for B, T in RC.UNIT_SIZES:
        case = X3.unit_case(kind, D, B, T)
        name = f"32-high {kind} D={D} B={B} T={T}"
        got = both_poisons(name, lambda q: HighUnit(kind, D, case["x"], case["g"], 0, poison=q, ff_mult=RC.UNIT_DIMS[D]).run(None))
        worst = max(worst, (gate(name, got, case), (B, T)))
    print(f"32-high {kind} D={D}: worst {worst[0]:.2f} x e_x3 at {worst[1]}")
    report("high_unit", kind=kind, D=D, worst_ratio=worst[0], at=str(worst[1]))


@pytest.mark.parametrize("kind", ["attn", "ff"])
def test_units_with_dropout_within_twice_e_x3(kind):
    """the masks of the truth are the host twin's (route_reference.unit_masks), the device evaluates its own"""
    for i, (B, T) in enumerate(RC.DROP_SIZES):
        stream = 40 + i
        case = X3.unit_case(kind, 64, B, T, stream)
        name = f"32-high dropout {kind} T={T}"
        got = both_poisons(name, lambda q: HighUnit(kind, 64, case["x"], case["g"], 0, poison=q).run((RC.DROP_P, RC.DROP_SEED, stream)))
        gate(name, got, case)


def test_trunk_and_heads_with_a_loss():
    c = RC.TRUNK
    case = X3.trunk_case()
    hp = dict(transformer_dim=c["D"], ff_mult=c["ff_mult"], n_layers=c["L"])
    m = H.make_model(hp, H.state_dict(hp, 3, "lively"))
    for k, v in m.state_dict().items():
        assert torch.equal(v.cpu(), case["sd"][k]), k
    m.set_train_precision(HIGH)
    forward = lambda xd: m.task_heads(m.transformer_blocks(xd))
    got = H.loss_backward(forward, m, case["h"], case["beat"], case["down"], case["mask"])
    report("high_trunk", e_x3=case["e_x3"], worst_ratio=gate("32-high trunk", got, case))


class _X3Queries:
    """the library with the *_x3 workspace queries where route_harness.abi_front_unit asks the *_mixed ones"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        swap = {"bt_front_workspace_bytes_mixed": "bt_front_workspace_bytes_x3",
                "bt_front_bn_workspace_bytes_mixed": "bt_front_bn_workspace_bytes_x3"}
        return getattr(self._lib, swap.get(name, name))


@contextlib.contextmanager
def x3_front_structs():
    """inside the block the frontend's argument structs are born with operand = BT_OPERAND_BF16X3 and the workspace is sized by
    the *_x3 queries: route_harness.abi_front_unit builds the structs itself, sets ``mixed`` alone and asks the *_mixed queries"""
    from beat_this_amd import _lib as L

    real = L.FrontArgs, L.FrontBnArgs, L.lib
    L.FrontArgs = lambda **kw: real[0](operand=OPERAND_X3, **kw)
    L.FrontBnArgs = lambda **kw: real[1](operand=OPERAND_X3, **kw)
    L.lib = lambda: _X3Queries(real[2]())
    try:
        yield
    finally:
        L.FrontArgs, L.FrontBnArgs, L.lib = real


def abi_front(sd, unit, dims, B, T, x, gy, poison, batch=False):
    with x3_front_structs():
        return H.abi_front_unit(sd, unit, dims, B, T, x, gy, poison, True, batch)


@pytest.mark.parametrize("i,B,T", BF.CONV)
def test_conv_units_within_twice_e_x3(i, B, T):
    case = X3.conv_case(i, B, T)
    name = f"32-high conv{i} B={B} T={T}"
    gate(name, both_poisons(name, lambda q: abi_front(case["sd"], "conv", conv_dims(i), B, T, case["x"], case["g"], q)), case)


@pytest.mark.parametrize("i,B,T", BF.CONV_BN)
def test_conv_units_with_batch_statistics(i, B, T):
    """the moved running buffers are fp32 work on the conv's result: within 2 x max(e, 1e-7) of the fp64 update, e the twin's own
    distance for that buffer"""
    case = X3.conv_case(i, B, T, batch=True)
    name = f"32-high conv{i} batch statistics B={B} T={T}"
    res, stats = both_poisons(name, lambda q: abi_front(dict(case["sd"]), "conv", conv_dims(i), B, T, case["x"], case["g"], q, batch=True))
    gate(name, res, case)
    for k, want in case["truth"]["stats"].items():
        if k.endswith("num_batches_tracked"):
            assert int(stats[k]) == int(want), k
            continue
        e = max(RG.rel(case["twin"]["stats"][k], want), 1e-7)
        err = RG.rel(stats[k], want)
        print(f"{name}: {k} twin {e:.3e}, device {err:.3e} ({err / e:.2f} x)")
        assert torch.isfinite(stats[k]).all() and err <= X3.GATE * e, (name, k, err, e)


def front_model(cache="x3"):
    """the D = 64 model of route_cases.model_state_dict on the GPU, everything trainable"""
    return H.make_model(RC.HP, RC.model_state_dict("lively", True), frontend=True, freeze_freqs=True, cache=cache)


@pytest.mark.parametrize("i,leaf,B,T", BF.LEAVES)
def test_leaves_of_both_directions_within_twice_e_x3(i, leaf, B, T):
    from beat_this_amd.model import backward as bw

    case = X3.leaf_case(i, leaf, B, T)
    m = front_model()
    node, p = m.frontend.blocks[i].partial._modules[leaf], f"frontend.blocks.{i}.partial.{leaf}."

    def run():
        xd = case["x"].to(dev()).requires_grad_(True)
        if leaf.startswith("attn"):
            y = bw.attention(node, xd, *m._rope(xd.shape[1]), mixed="bf16x3", residual=True)
        else:
            y = bw.feedforward(node, xd, mixed="bf16x3", residual=True)
        params = [(p + n, q) for n, q in node.named_parameters() if not n.endswith("freqs")]
        grads = torch.autograd.grad([y], [xd] + [q for _, q in params], [case["g"].to(dev())])
        return dict(zip(["x"] + [n for n, _ in params], grads), y=y.detach())

    got, again = run(), run()
    assert len(got) == 7 and all(same_bits(got[k], again[k]) for k in got)
    gate(f"32-high block {i} {leaf} B={B} T={T}", got, case)


@pytest.mark.parametrize("B,T", BF.LINEAR)
def test_projection_within_twice_e_x3(B, T):
    case = X3.linear_case(B, T)
    name = f"32-high projection B={B} T={T}"
    gate(name, both_poisons(name, lambda q: abi_front(case["sd"], "linear", (4, 256, 64), B, T, case["x"], case["g"], q)), case)


def test_whole_model_with_both_parts_on_32_high():
    case = X3.model_case()
    m = front_model()
    try:
        m.set_frontend_precision(HIGH).set_train_precision(HIGH)
        got = H.model_device(m, case["x"], case["beat"], case["down"], case["mask"])
    finally:
        m.set_frontend_precision("32-true").set_train_precision("32-true")
    keys = RG.grad_keys(case["truth"])
    assert set(keys) == set(got) - {"beat", "downbeat"} and len(keys) == 100
    report("high_model", e_x3=case["e_x3"], worst_ratio=gate("32-high whole model", got, case))


# ---- 3. reproducibility --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["attn", "ff"])
def test_runs_are_bit_identical_and_a_sequence_alone_is_the_sequence_in_a_batch(kind):
    D, B, T = 64, 3, 130
    x, g = H.randn(B, T, D, seed=51), H.randn(B, T, D, seed=52)
    for drop in (None, (0.2, RC.DROP_SEED, 9)):
        name = f"32-high {kind} drop={drop is not None}"
        first = both_poisons(name, lambda q: HighUnit(kind, D, x, g, 1, poison=q).run(drop))
        again = HighUnit(kind, D, x, g, 1).run(drop)
        assert all(same_bits(first[k], again[k]) for k in first), name
    plain = HighUnit(kind, D, x, g, 1).run(None)
    for b in range(B):   # (without dropout: the masks follow the row)
        alone = HighUnit(kind, D, x[b:b + 1], g[b:b + 1], 1, poison=POISONS[b % 2]).run(None)
        assert same_bits(alone["x"][0], plain["x"][b]) and same_bits(alone["y"][0], plain["y"][b]), (kind, b)
    # another arithmetic for the same gradients: neither the bfloat16 call's bits nor far from them
    bf = HighUnit(kind, D, x, g, 1, operand=1).run(None)
    assert not same_bits(plain["x"], bf["x"]) and RG.rel(plain["x"], bf["x"]) < 5e-2


def test_the_frontend_alone_and_in_a_batch():
    i = 0
    case = X3.conv_case(i, 2, 65)
    both = abi_front(case["sd"], "conv", conv_dims(i), 2, 65, case["x"], case["g"], POISONS[0])
    alone = abi_front(case["sd"], "conv", conv_dims(i), 1, 65, case["x"][:1], case["g"][:1], POISONS[1])
    assert same_bits(alone["x"][0], both["x"][0]) and same_bits(alone["y"][0], both["y"][0])
    fp32 = H.abi_front_unit(case["sd"], "conv", conv_dims(i), 2, 65, case["x"], case["g"], POISONS[0])
    assert not same_bits(fp32["x"], both["x"]) and RG.rel(both["x"], fp32["x"]) < 1e-3


# ---- 4. no bleed ----------------------------------------------------------------------------------------------------------------------
def test_switching_to_32_high_and_back_leaves_the_other_routes_as_they_were():
    fresh = lambda: H.make_model(RC.HP, RC.model_state_dict("init0"), frontend=True, freeze_freqs=True)
    never, switched = fresh(), fresh()
    x, beat, down, mask = RC.model_inputs(2, 33, True)
    run = lambda m: H.model_device(m, x, beat, down, mask, 1024.0)
    want32 = run(never)
    want16 = run(never.set_train_precision("16-mixed").set_frontend_precision("16-mixed"))
    wantbf = run(never.set_train_precision("16-mixed", "bf16").set_frontend_precision("16-mixed", "bf16"))
    high = run(switched.set_train_precision(HIGH).set_frontend_precision(HIGH))
    moved = [k for k in want32 if not same_bits(high[k], want32[k])]
    assert len(high) == len(want32) == 102 and len(moved) > 90, len(moved)
    for k in want32:   # (the same gradients, 2^-17 of an operand away, not bfloat16's)
        assert RG.rel(high[k], want32[k]) < 1e-2, k
    assert sum(not same_bits(high[k], wantbf[k]) for k in wantbf) > 90
    with torch.no_grad():   # inference never looks at the switch
        a, b = never(x.to(dev())), switched(x.to(dev()))
    assert same_bits(a["beat"], b["beat"]) and same_bits(a["downbeat"], b["downbeat"])
    back32 = run(switched.set_train_precision("32-true").set_frontend_precision("32-true"))
    assert all(same_bits(back32[k], want32[k]) for k in want32)
    switched.set_train_precision(HIGH).set_frontend_precision(HIGH)
    back16 = run(switched.set_train_precision("16-mixed").set_frontend_precision("16-mixed"))
    assert all(same_bits(back16[k], want16[k]) for k in want16)
    switched.set_train_precision(HIGH).set_frontend_precision(HIGH)
    backbf = run(switched.set_train_precision("16-mixed", "bf16").set_frontend_precision("16-mixed", "bf16"))
    assert all(same_bits(backbf[k], wantbf[k]) for k in wantbf)
    # one part alone: the trunk on 32-high leaves the frontend's own launches on fp32
    half = run(switched.set_frontend_precision("32-true").set_train_precision(HIGH))
    assert not same_bits(half["beat"], want32["beat"]) and not same_bits(half["x"], want32["x"]) and not same_bits(half["x"], high["x"])
    switched.set_train_precision("32-true")


# ---- 5. refusals before any launch ---------------------------------------------------------------------------------------------------
def test_refused_before_any_launch():
    """every pointer is null, so a launch would be seen; the shapes are valid, so the operand is what is refused"""
    from beat_this_amd import _lib as L

    lib, s = L.lib(), L.stream_ptr(dev())
    for operand in (2, 4, -1):
        for unit, hidden in ((L.UNIT_ATTN, 0), (L.UNIT_FF, 128)):
            a = L.TrainArgs(B=1, T=8, dim=64, hidden=hidden, operand=operand)
            for fn in (lib.bt_train_forward_mixed, lib.bt_train_backward_mixed):
                assert fn(s, unit, C.byref(a), None) == L.BT_ERR_ARG and b"operand" in lib.bt_last_error()
        for unit, (F_, C_, dim) in ((L.FRONT_CONV, (32, 32, 0)), (L.FRONT_LINEAR, (4, 256, 64))):
            a = L.FrontArgs(B=2, T=3, F=F_, C=C_, dim=dim, mixed=1, operand=operand)
            for fn in (lib.bt_front_forward, lib.bt_front_backward):
                assert fn(s, unit, C.byref(a)) == L.BT_ERR_ARG and b"operand" in lib.bt_last_error()
        b = L.FrontBnArgs(B=2, T=3, F=32, C=32, mixed=1, operand=operand)
        for fn in (lib.bt_front_bn_forward, lib.bt_front_bn_backward):
            assert fn(s, L.FRONT_CONV, C.byref(b)) == L.BT_ERR_ARG and b"operand" in lib.bt_last_error()
    # operand 3 is known: what is refused then is the null pointers, and on the units without a mixed form `mixed` itself
    a = L.TrainArgs(B=1, T=8, dim=64, hidden=0, operand=OPERAND_X3)
    assert lib.bt_train_forward_mixed(s, L.UNIT_ATTN, C.byref(a), None) == L.BT_ERR_ARG and b"operand" not in lib.bt_last_error()
    a = L.FrontArgs(B=2, T=3, F=128, C=32, dim=0, mixed=1, operand=OPERAND_X3)
    assert lib.bt_front_forward(s, L.FRONT_STEM, C.byref(a)) == L.BT_ERR_ARG and b"mixed" in lib.bt_last_error()
    for mixed in (3, 5, -1):
        assert lib.bt_train_matmul(s, mixed, 0, None, None, 1, 1, 1, None, None, None, 0, None, None, 0, 0, None, 0) == L.BT_ERR_ARG
        assert b"mixed" in lib.bt_last_error()
        assert lib.bt_train_attention(s, mixed, 0, 1, 8, 64, None, None, None, None, None, None, None) == L.BT_ERR_ARG
        assert b"mixed" in lib.bt_last_error()
    assert lib.bt_train_matmul(s, X3M, 0, None, None, 1, 1, 1, None, None, None, 0, None, None, 0, 0, None, 0) == L.BT_ERR_ARG
    assert b"mixed" not in lib.bt_last_error()
    # the new queries: the fp32 size plus both images; 0 for unsupported shapes and for units without a mixed form
    for backward in (0, 1):
        plain, one = lib.bt_front_workspace_bytes(L.FRONT_CONV, backward, 2, 3, 32, 32, 0), lib.bt_front_workspace_bytes_mixed(L.FRONT_CONV, backward, 2, 3, 32, 32, 0)
        assert lib.bt_front_workspace_bytes_x3(L.FRONT_CONV, backward, 2, 3, 32, 32, 0) == plain + 2 * (one - plain) > one > plain
        plain, one = lib.bt_front_bn_workspace_bytes(L.FRONT_CONV, backward, 2, 3, 32, 32), lib.bt_front_bn_workspace_bytes_mixed(L.FRONT_CONV, backward, 2, 3, 32, 32)
        assert lib.bt_front_bn_workspace_bytes_x3(L.FRONT_CONV, backward, 2, 3, 32, 32) == plain + 2 * (one - plain) > one
        assert lib.bt_front_workspace_bytes_x3(L.FRONT_LINEAR, backward, 2, 3, 4, 256, 64) == lib.bt_front_workspace_bytes_mixed(L.FRONT_LINEAR, backward, 2, 3, 4, 256, 64) > 0
        assert lib.bt_front_workspace_bytes_x3(L.FRONT_STEM, backward, 2, 3, 128, 32, 0) == 0
        assert lib.bt_front_workspace_bytes_x3(L.FRONT_SWAP, backward, 2, 3, 4, 32, 0) == 0
        assert lib.bt_front_workspace_bytes_x3(L.FRONT_CONV, backward, 2, 3, 33, 32, 0) == 0
        assert lib.bt_front_workspace_bytes_x3(L.FRONT_CONV, backward, 2, 3, 32, 48, 0) == 0
        assert lib.bt_front_bn_workspace_bytes_x3(L.FRONT_LINEAR, backward, 2, 3, 4, 256) == 0
        assert lib.bt_front_bn_workspace_bytes_x3(L.FRONT_CONV, backward, 1, 1, 2, 32) == 0
    assert lib.bt_train_workspace_bytes_mixed(L.UNIT_ATTN, 1, 2, 33, 64, 0, 0) == lib.bt_train_workspace_bytes(L.UNIT_ATTN, 1, 2, 33, 64, 0)
    torch.cuda.synchronize()


def test_a_workspace_of_the_mixed_size_is_too_small():
    """a conv call on split operands with the one-image workspace: BT_ERR_WORKSPACE, nothing launched, nothing written"""
    from beat_this_amd import _lib as L
    from gpu_util import Guarded

    lib, s = L.lib(), L.stream_ptr(dev())
    for struct, query, fn in ((L.FrontArgs, lambda: lib.bt_front_workspace_bytes_mixed(L.FRONT_CONV, 0, 2, 3, 32, 32, 0), lib.bt_front_forward),
                              (L.FrontBnArgs, lambda: lib.bt_front_bn_workspace_bytes_mixed(L.FRONT_CONV, 0, 2, 3, 32, 32), lib.bt_front_bn_forward)):
        n = query()
        bufs = [Guarded((2, 3, 32, 32), torch.float32).fill(POISONS[0]) for _ in range(3)] + \
               [Guarded((64,), torch.float32).fill(POISONS[0]) for _ in range(6)] + [Guarded((64, 32, 2, 3), torch.float32).fill(POISONS[0])]
        ws = Guarded((n,), torch.uint8).fill(POISONS[0])
        a = struct(B=2, T=3, F=32, C=32, mixed=1, operand=OPERAND_X3)
        a.x, a.y, a.save_pre = (b.ptr() for b in bufs[:3])
        a.bn_w, a.bn_b, a.bn_mean, a.bn_var = (b.ptr() for b in bufs[3:7])
        if struct is L.FrontBnArgs:
            a.save_mean, a.save_rstd = bufs[7].ptr(), bufs[8].ptr()
        a.w = bufs[9].ptr()
        a.ws, a.ws_bytes = ws.ptr(), n
        before = [b.t.clone() for b in bufs]
        assert fn(s, L.FRONT_CONV, C.byref(a)) == L.BT_ERR_WORKSPACE, lib.bt_last_error()
        torch.cuda.synchronize()
        assert all(same_bits(b.t, t) for b, t in zip(bufs, before))
        assert_intact(*[(f"buffer {i}", b) for i, b in enumerate(bufs)], ("workspace", ws))


# ---- 6. the loop -------------------------------------------------------------------------------------------------------------------
def test_fit_on_32_high_has_no_loss_scale_and_resumes_bit_for_bit(tmp_path):
    from beat_this_amd.inference import load_checkpoint
    from beat_this_amd.train import CHECKPOINT_KEYS, fit
    from test_gpu_finetune import new_datamodule, new_module

    root = build_data_folder(str(tmp_path / "data"))
    ck, first, ck2 = (str(tmp_path / n) for n in ("run.ckpt", "epoch0.ckpt", "resumed.ckpt"))

    def log(line):
        if line.startswith("epoch 0:"):
            shutil.copy(ck, first)

    kw = dict(val_frequency=1, train_frontend=True, precision=HIGH, frontend_precision=HIGH)
    pl = new_module()
    np.random.seed(0)
    h = fit(pl, new_datamodule(root), 2, checkpoint_path=ck, log=log, **kw)
    m = pl.model
    assert (m.train_precision, m.frontend_precision) == (HIGH, HIGH) and not m.train_settings.needs_loss_scale()
    assert h["loss_scaler"] is None and len(h["train_loss"]) == 2 and all(np.isfinite(v) and v < 10 for v in h["train_loss"])
    pl2 = new_module()
    np.random.seed(99)
    h2 = fit(pl2, new_datamodule(root), 2, checkpoint_path=ck2, resume=first, log=lambda s: None, **kw)
    a, b = load_checkpoint(ck), load_checkpoint(ck2)
    assert h2["loss_scaler"] is None and set(a) == set(b) == set(CHECKPOINT_KEYS) and "loss_scaler" not in load_checkpoint(first)
    for k, v in a["state_dict"].items():
        assert torch.equal(v, b["state_dict"][k]), k
    sa, sb = a["optimizer_states"][0], b["optimizer_states"][0]
    assert len(sa["state"]) == len(sb["state"]) == len(RG.all_keys(pl.model.state_dict()))
    for i in sa["state"]:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert same_bits(torch.as_tensor(sa["state"][i][k]), torch.as_tensor(sb["state"][i][k])), (i, k)
    fresh = new_module()
    assert sum(not torch.equal(p.detach(), q.detach()) for p, q in zip(fresh.parameters(), pl.parameters())) > 20
    # beside a part on fp16 operands the loss is scaled; beside bfloat16 ones it is not
    h3 = fit(new_module(), new_datamodule(root), 0, train_frontend=True, precision=HIGH, frontend_precision="16-mixed", log=lambda s: None)
    assert h3["loss_scaler"] is not None
    h4 = fit(new_module(), new_datamodule(root), 0, train_frontend=True, precision="16-mixed", mixed_operand="bf16",
             frontend_precision=HIGH, log=lambda s: None)
    assert h4["loss_scaler"] is None
