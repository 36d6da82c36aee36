"""bfloat16 operands on the two 16-mixed routes on the GPU (csrc/train_mixed.inc, csrc/train_front_mixed.inc, DESIGN.md section
24): the bf16 MFMA GEMM exactly -- on values the fp16 route cannot hold, and on a tie that shows round to nearest even -- then
the units, the trunk, the frontend's units and the whole model within 2 x e_ref_bf16 of the fp64 truth (tests/bf16_reference.py:
e_ref_bf16 is the oracle's own error under CPU bfloat16 autocast at loss scale 1), bit identity, refusals, and ``fit`` without a
loss scale.

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
from dataset_reference import build_data_folder
from gpu_util import POISONS, Guarded, assert_intact, dev, report
from route_harness import both_poisons, same_bits
from test_gpu_mixed import EDGES, KS, MixedUnit

pytestmark = pytest.mark.gpu
BF16, F16 = 2, 1        # `mixed` of bt_train_matmul / bt_train_attention: 1 + BT_OPERAND_*


# ---- 1. exact products -------------------------------------------------------------------------------------------------------------
def guarded(arr, poison):
    t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32))
    return Guarded(t.shape, torch.float32).fill(poison, data=t.to(dev()))


def matmul(mixed, form, a, b, M, N, K, poison):
    """bt_train_matmul on guarded buffers (form 2 with its workspace) -> C as numpy"""
    from beat_this_amd import _lib as L

    lib = L.lib()
    ga, gb, gc = guarded(a, poison), guarded(b, poison), Guarded((M, N), torch.float32).fill(poison)
    n = lib.bt_train_matmul_workspace_bytes(form, M, N, K)
    ws = Guarded((max(n, 1),), torch.uint8).fill(poison)
    L.check(lib.bt_train_matmul(L.stream_ptr(dev()), mixed, form, ga.ptr(), gb.ptr(), M, N, K, gc.ptr(), None, None, 0, None, None, 0, 0,
                                ws.ptr() if n else None, n))
    torch.cuda.synchronize()
    assert_intact(("A", ga), ("B", gb), ("C", gc), ("workspace", ws))
    return gc.t.cpu().numpy()


def matmul_exact(form, M, N, K, seed):
    """integers in [-8, 8], A times 2^17 and B times 2^-17: every operand is exact in bfloat16 (four significant bits, fp32's
    exponents), every partial sum an integer below 2^24; in fp16 A is inf and the product inf or NaN"""
    rng = np.random.default_rng(seed)
    a = rng.integers(-8, 9, size=(K, M) if form == 2 else (M, K))
    b = rng.integers(-8, 9, size=(N, K) if form == 0 else (K, N))
    want = (a.T if form == 2 else a).astype(np.int64) @ (b.T if form == 0 else b).astype(np.int64)
    for poison in POISONS:
        got = matmul(BF16, form, a * 2.0 ** 17, b * 2.0 ** -17, M, N, K, poison)
        assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32)), (form, M, N, K, poison)
    return a, b, want


@pytest.mark.parametrize("form", [0, 1, 2])
def test_products_beyond_the_range_of_fp16_are_exact(form):
    n = 0
    for i, M in enumerate(EDGES):
        for j in range(3):   # (three of the N per M, all of them over the M)
            N = EDGES[(i + 4 * j + form) % len(EDGES)]
            for K in KS:
                matmul_exact(form, M, N, K, 2000 * form + n)
                n += 1
    if form == 2:   # the summed rows on both sides of a BT_TRAIN_DW_ROWS chunk
        for K in (1023, 1024, 1025):
            matmul_exact(2, 33, 129, K, K)
    # which route ran: the fp16 one turns the same operands into inf or NaN
    a, b, want = matmul_exact(form, 33, 65, 17, 7)
    assert np.abs(want).max() > 0 and not np.isfinite(matmul(F16, form, a * 2.0 ** 17, b * 2.0 ** -17, 33, 65, 17, POISONS[0])).all()


def test_ties_round_to_even():
    """257 lies half way between bfloat16's 256 and 258, 259 between 258 and 260: the even significands are 256 and 260"""
    eye = np.eye(2)
    for form, a in ((0, [[257.0, 259.0]]), (1, [[257.0, 259.0]]), (2, [[257.0], [259.0]])):
        for poison in POISONS:
            got = matmul(BF16, form, np.array(a), eye, 1, 2, 2, poison)
            assert got.tolist() == [[256.0, 260.0]], (form, got)
    for form in (0, 1):   # the other operand is rounded too; a NaN stays one (in its own row: NaN x 0 is NaN), 3e38 stays finite
        got = matmul(BF16, form, eye, np.array([[257.0, 0.0], [0.0, 259.0]]), 2, 2, 2, POISONS[0])
        assert got.tolist() == [[256.0, 0.0], [0.0, 260.0]], (form, got)
    got = matmul(BF16, 0, np.array([[float("nan"), 1.0], [3.0e38, 1.0]]), eye, 2, 2, 2, POISONS[1])
    assert np.isnan(got[0]).all() and np.isfinite(got[1, 0]) and got[1, 0] > 2.9e38 and got[1, 1] == 1.0


# ---- 2. units ----------------------------------------------------------------------------------------------------------------------
class Bf16Unit(MixedUnit):
    """test_gpu_mixed.MixedUnit with ``operand`` of bt_train_args set (BT_OPERAND_BF16 unless told otherwise)"""

    def __init__(self, *args, operand=1, **kw):
        super().__init__(*args, **kw)
        self.a.operand = operand


def gate(name, got, case):
    return BF.gate(name, got, case, report)


@pytest.mark.parametrize("D", sorted(RC.UNIT_DIMS))
@pytest.mark.parametrize("kind", ["attn", "ff"])
def test_units_within_twice_e_ref_bf16(kind, D):
    worst = (0.0, None)
    for B, T in RC.UNIT_SIZES:
        case = BF.unit_case(kind, D, B, T)
        name = f"bf16 {kind} D={D} B={B} T={T}"
        got = both_poisons(name, lambda q: Bf16Unit(kind, D, case["x"], case["g"], 0, poison=q, ff_mult=RC.UNIT_DIMS[D]).run(None))
        worst = max(worst, (gate(name, got, case), (B, T)))
    print(f"bf16 {kind} D={D}: worst {worst[0]:.2f} x e_ref_bf16 at {worst[1]}")
    report("bf16_unit", kind=kind, D=D, worst_ratio=worst[0], at=str(worst[1]))


@pytest.mark.parametrize("kind", ["attn", "ff"])
def test_units_with_dropout_within_twice_e_ref_bf16(kind):
    """the masks of the truth are the host twin's (route_reference.unit_masks), the device evaluates its own"""
    for i, (B, T) in enumerate(RC.DROP_SIZES):
        stream = 40 + i
        case = BF.unit_case(kind, 64, B, T, stream)
        name = f"bf16 dropout {kind} T={T}"
        got = both_poisons(name, lambda q: Bf16Unit(kind, 64, case["x"], case["g"], 0, poison=q).run((RC.DROP_P, RC.DROP_SEED, stream)))
        gate(name, got, case)


# ---- 3. trunk and heads with a loss -------------------------------------------------------------------------------------------------
def test_trunk_and_heads_with_a_loss():
    c = RC.TRUNK
    case = BF.trunk_case()
    hp = dict(transformer_dim=c["D"], ff_mult=c["ff_mult"], n_layers=c["L"])
    m = H.make_model(hp, H.state_dict(hp, 3, "lively"))
    for k, v in m.state_dict().items():
        assert torch.equal(v.cpu(), case["sd"][k]), k
    m.set_train_precision("16-mixed", operand="bf16")
    forward = lambda xd: m.task_heads(m.transformer_blocks(xd))
    got = H.loss_backward(forward, m, case["h"], case["beat"], case["down"], case["mask"])
    report("bf16_trunk", e_ref_bf16=case["e_ref"], worst_ratio=gate("bf16 trunk", got, case))


# ---- 4. the frontend ----------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def bf16_front_structs():
    """inside the block the frontend's argument structs are born with operand = BT_OPERAND_BF16: route_harness.abi_front_unit
    builds them itself and sets ``mixed`` alone"""
    from beat_this_amd import _lib as L

    real = L.FrontArgs, L.FrontBnArgs
    L.FrontArgs = lambda **kw: real[0](operand=L.OPERAND_BF16, **kw)
    L.FrontBnArgs = lambda **kw: real[1](operand=L.OPERAND_BF16, **kw)
    try:
        yield
    finally:
        L.FrontArgs, L.FrontBnArgs = real


def abi_front(sd, unit, dims, B, T, x, gy, poison, batch=False, bf16=True, mixed=True):
    with (bf16_front_structs() if bf16 else contextlib.nullcontext()):
        return H.abi_front_unit(sd, unit, dims, B, T, x, gy, poison, mixed, batch)


def conv_dims(i):
    return f"frontend.blocks.{i}.", 32 >> i, 32 << i


@pytest.mark.parametrize("i,B,T", BF.CONV)
def test_conv_units_within_twice_e_ref_bf16(i, B, T):
    case = BF.conv_case(i, B, T)
    name = f"bf16 conv{i} B={B} T={T}"
    gate(name, both_poisons(name, lambda q: abi_front(case["sd"], "conv", conv_dims(i), B, T, case["x"], case["g"], q)), case)


@pytest.mark.parametrize("i,B,T", BF.CONV_BN)
def test_conv_units_with_batch_statistics(i, B, T):
    """the moved running buffers by the rule of section 19: within 2 x max(e, 1e-7) of the fp64 update, e the bfloat16 autocast
    oracle's own distance for that buffer"""
    case = BF.conv_case(i, B, T, batch=True)
    name = f"bf16 conv{i} batch statistics B={B} T={T}"
    sd = dict(case["sd"])
    res, stats = both_poisons(name, lambda q: abi_front(sd, "conv", conv_dims(i), B, T, case["x"], case["g"], q, batch=True))
    gate(name, res, case)
    for k, want in case["truth"]["stats"].items():
        if k.endswith("num_batches_tracked"):
            assert int(stats[k]) == int(want), k
            continue
        e = max(RG.rel(case["auto"]["stats"][k], want), 1e-7)
        err = RG.rel(stats[k], want)
        print(f"{name}: {k} autocast {e:.3e}, device {err:.3e} ({err / e:.2f} x)")
        assert torch.isfinite(stats[k]).all() and err <= BF.GATE * e, (name, k, err, e)


def front_model(cache="bf16"):
    """the D = 64 model of route_cases.model_state_dict on the GPU, everything trainable"""
    return H.make_model(RC.HP, RC.model_state_dict("lively", True), frontend=True, freeze_freqs=True, cache=cache)


@pytest.mark.parametrize("i,leaf,B,T", BF.LEAVES)
def test_leaves_of_both_directions_within_twice_e_ref_bf16(i, leaf, B, T):
    from beat_this_amd.model import backward as bw

    case = BF.leaf_case(i, leaf, B, T)
    m = front_model()
    node, p = m.frontend.blocks[i].partial._modules[leaf], f"frontend.blocks.{i}.partial.{leaf}."

    def run():
        xd = case["x"].to(dev()).requires_grad_(True)
        if leaf.startswith("attn"):
            y = bw.attention(node, xd, *m._rope(xd.shape[1]), mixed="bf16", residual=True)
        else:
            y = bw.feedforward(node, xd, mixed="bf16", residual=True)
        params = [(p + n, q) for n, q in node.named_parameters() if not n.endswith("freqs")]
        grads = torch.autograd.grad([y], [xd] + [q for _, q in params], [case["g"].to(dev())])
        return dict(zip(["x"] + [n for n, _ in params], grads), y=y.detach())

    got, again = run(), run()
    assert len(got) == 7 and all(same_bits(got[k], again[k]) for k in got)
    gate(f"bf16 block {i} {leaf} B={B} T={T}", got, case)


@pytest.mark.parametrize("B,T", BF.LINEAR)
def test_projection_within_twice_e_ref_bf16(B, T):
    case = BF.linear_case(B, T)
    name = f"bf16 projection B={B} T={T}"
    gate(name, both_poisons(name, lambda q: abi_front(case["sd"], "linear", (4, 256, 64), B, T, case["x"], case["g"], q)), case)


def test_whole_model_with_both_parts_on_bf16():
    case = BF.model_case()
    m = front_model()
    try:
        m.set_frontend_precision("16-mixed", operand="bf16").set_train_precision("16-mixed", operand="bf16")
        got = H.model_device(m, case["x"], case["beat"], case["down"], case["mask"])
    finally:
        m.set_frontend_precision("32-true").set_train_precision("32-true")
    keys = RG.grad_keys(case["truth"])
    assert set(keys) == set(got) - {"beat", "downbeat"} and len(keys) == 100
    report("bf16_model", e_ref_bf16=case["e_ref"], worst_ratio=gate("bf16 whole model", got, case))


# ---- 5. bit identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["attn", "ff"])
def test_runs_are_bit_identical_and_a_sequence_alone_is_the_sequence_in_a_batch(kind):
    D, B, T = 64, 3, 130
    x, g = H.randn(B, T, D, seed=51), H.randn(B, T, D, seed=52)
    for drop in (None, (0.2, RC.DROP_SEED, 9)):
        name = f"bf16 {kind} drop={drop is not None}"
        first = both_poisons(name, lambda q: Bf16Unit(kind, D, x, g, 1, poison=q).run(drop))
        again = Bf16Unit(kind, D, x, g, 1).run(drop)
        assert all(same_bits(first[k], again[k]) for k in first), name
    plain = Bf16Unit(kind, D, x, g, 1).run(None)
    for b in range(B):   # (without dropout: the masks follow the row)
        alone = Bf16Unit(kind, D, x[b:b + 1], g[b:b + 1], 1, poison=POISONS[b % 2]).run(None)
        assert same_bits(alone["x"][0], plain["x"][b]) and same_bits(alone["y"][0], plain["y"][b]), (kind, b)
    # operand = 0 is the *_mixed call of before, and bfloat16 is another rounding of the same gradients
    f16 = MixedUnit(kind, D, x, g, 1).run(None)
    zero = Bf16Unit(kind, D, x, g, 1, operand=0, poison=POISONS[0]).run(None)
    assert all(same_bits(zero[k], f16[k]) for k in f16)
    assert not same_bits(plain["x"], f16["x"]) and RG.rel(plain["x"], f16["x"]) < 5e-2


def test_the_frontend_alone_and_in_a_batch_and_operand_zero():
    i = 0
    case = BF.conv_case(i, 2, 65)
    both = abi_front(case["sd"], "conv", conv_dims(i), 2, 65, case["x"], case["g"], POISONS[0])
    alone = abi_front(case["sd"], "conv", conv_dims(i), 1, 65, case["x"][:1], case["g"][:1], POISONS[1])
    assert same_bits(alone["x"][0], both["x"][0]) and same_bits(alone["y"][0], both["y"][0])
    # operand = 0 (what the harness leaves) is the fp16 call; with mixed = 0 the operand is not read
    from beat_this_amd import _lib as L

    f16 = abi_front(case["sd"], "conv", conv_dims(i), 2, 65, case["x"], case["g"], POISONS[0], bf16=False)
    assert not same_bits(f16["x"], both["x"]) and not same_bits(f16["save_pre"], both["save_pre"])
    fp32 = abi_front(case["sd"], "conv", conv_dims(i), 2, 65, case["x"], case["g"], POISONS[0], bf16=False, mixed=False)
    ignored = abi_front(case["sd"], "conv", conv_dims(i), 2, 65, case["x"], case["g"], POISONS[1], bf16=True, mixed=False)
    assert all(same_bits(fp32[k], ignored[k]) for k in fp32) and not same_bits(fp32["x"], both["x"])
    # the raw GEMM: mixed = 1 of bt_train_matmul is bt_train_matmul_mixed
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal((65, 100)), rng.standard_normal((33, 100))
    ga, gb, gc = guarded(a, POISONS[0]), guarded(b, POISONS[0]), Guarded((65, 33), torch.float32).fill(POISONS[0])
    L.check(L.lib().bt_train_matmul_mixed(L.stream_ptr(dev()), 0, ga.ptr(), gb.ptr(), 65, 33, 100, gc.ptr()))
    torch.cuda.synchronize()
    assert_intact(("A", ga), ("B", gb), ("C", gc))
    assert np.array_equal(gc.t.cpu().numpy(), matmul(F16, 0, a, b, 65, 33, 100, POISONS[1]))


def test_switching_to_bf16_and_back_leaves_the_other_routes_as_they_were():
    fresh = lambda: H.make_model(RC.HP, RC.model_state_dict("init0"), frontend=True, freeze_freqs=True)
    never, switched = fresh(), fresh()
    x, beat, down, mask = RC.model_inputs(2, 33, True)
    run = lambda m: H.model_device(m, x, beat, down, mask, 1024.0)
    want32 = run(never)
    want16 = run(never.set_train_precision("16-mixed").set_frontend_precision("16-mixed"))
    switched.set_train_precision("16-mixed", operand="bf16").set_frontend_precision("16-mixed", operand="bf16")
    bf = run(switched)
    moved = [k for k in want16 if not same_bits(bf[k], want16[k])]
    assert len(bf) == len(want16) == 102 and len(moved) > 90, len(moved)
    for k in want32:   # (another rounding of the same gradients, not other gradients)
        assert RG.rel(bf[k], want32[k]) < 0.2, k
    with torch.no_grad():   # inference never looks at the switch
        a, b = never(x.to(dev())), switched(x.to(dev()))
    assert same_bits(a["beat"], b["beat"]) and same_bits(a["downbeat"], b["downbeat"])
    back16 = run(switched.set_train_precision("16-mixed", "fp16").set_frontend_precision("16-mixed", "fp16"))
    assert all(same_bits(back16[k], want16[k]) for k in want16)
    back32 = run(switched.set_train_precision("32-true").set_frontend_precision("32-true"))
    assert all(same_bits(back32[k], want32[k]) for k in want32)
    # one part alone: the trunk on bfloat16 leaves the frontend's own launches on fp32 (its gradients move with what flows back)
    half = run(switched.set_train_precision("16-mixed", "bf16"))
    assert not same_bits(half["beat"], want32["beat"]) and not same_bits(half["x"], want32["x"])
    stem = "frontend.stem.conv2d.weight"
    assert RG.rel(half[stem], want32[stem]) < 0.2
    switched.set_train_precision("32-true")


# ---- 6. refusals before any launch ---------------------------------------------------------------------------------------------------
def test_refused_before_any_launch():
    """every pointer is null, so a launch would be seen; the shapes are valid, so the operand is what is refused"""
    from beat_this_amd import _lib as L

    lib, s = L.lib(), L.stream_ptr(dev())
    for operand in (2, -1):
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
    for mixed in (3, -1):
        assert lib.bt_train_matmul(s, mixed, 0, None, None, 1, 1, 1, None, None, None, 0, None, None, 0, 0, None, 0) == L.BT_ERR_ARG
        assert b"mixed" in lib.bt_last_error()
        assert lib.bt_train_attention(s, mixed, 0, 1, 8, 64, None, None, None, None, None, None, None) == L.BT_ERR_ARG
        assert b"mixed" in lib.bt_last_error()
    # the operand does not move a workspace size
    assert lib.bt_train_workspace_bytes_mixed(L.UNIT_ATTN, 1, 2, 33, 64, 0, 0) == lib.bt_train_workspace_bytes(L.UNIT_ATTN, 1, 2, 33, 64, 0)
    torch.cuda.synchronize()


# ---- 7. the loop -------------------------------------------------------------------------------------------------------------------
def test_fit_on_bf16_has_no_loss_scale_and_resumes_bit_for_bit(tmp_path):
    from beat_this_amd.inference import load_checkpoint
    from beat_this_amd.train import CHECKPOINT_KEYS, fit
    from test_gpu_finetune import new_datamodule, new_module

    root = build_data_folder(str(tmp_path / "data"))
    ck, first, ck2 = (str(tmp_path / n) for n in ("run.ckpt", "epoch0.ckpt", "resumed.ckpt"))

    def log(line):
        if line.startswith("epoch 0:"):
            shutil.copy(ck, first)

    kw = dict(val_frequency=1, train_frontend=True, precision="16-mixed", mixed_operand="bf16", frontend_precision="16-mixed",
              frontend_mixed_operand="bf16")
    pl = new_module()
    np.random.seed(0)
    h = fit(pl, new_datamodule(root), 2, checkpoint_path=ck, log=log, **kw)
    m = pl.model
    assert (m.train_precision, m.train_operand, m.frontend_precision, m.frontend_operand) == ("16-mixed", "bf16", "16-mixed", "bf16")
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
    # a mixed run -- the trunk on bfloat16, the frontend on fp16 -- does scale its loss
    h3 = fit(new_module(), new_datamodule(root), 0, train_frontend=True, precision="16-mixed", mixed_operand="bf16",
             frontend_precision="16-mixed", log=lambda s: None)
    assert h3["loss_scaler"] is not None
    h4 = fit(new_module(), new_datamodule(root), 0, precision="16-mixed", mixed_operand="bf16", log=lambda s: None)
    assert h4["loss_scaler"] is None
