"""What belongs to the bfloat16 operand format alone, on the GPU (the tests it shares with the other formats
are in tests/test_gpu_train_formats.py): the bf16 MFMA GEMM exactly -- on values the fp16 route cannot hold, and on a tie that
shows round to nearest even -- operand 0 as the fp16 call of before, and switching to bfloat16 and back.

Every device entry is called on gpu_util.Guarded buffers: guard bands on both sides, both poison patterns."""
import numpy as np
import pytest
import torch

import bf16_reference as BF
import route_grads as RG
import route_harness as H
from gpu_util import POISONS, Guarded, assert_intact, dev
from route_harness import conv_dims, guarded, matmul, same_bits, walk

pytestmark = pytest.mark.gpu
F16M, BF16M = 1, 2        # `mixed` of bt_train_matmul / bt_train_attention: 1 + BT_OPERAND_*


def matmul_exact(form, M, N, K, seed):
    """integers in [-8, 8], A times 2^17 and B times 2^-17: every operand is exact in bfloat16 (four significant bits, fp32's
    exponents), every partial sum an integer below 2^24; in fp16 A is inf and the product inf or NaN"""
    rng = np.random.default_rng(seed)
    a = rng.integers(-8, 9, size=(K, M) if form == 2 else (M, K))
    b = rng.integers(-8, 9, size=(N, K) if form == 0 else (K, N))
    want = (a.T if form == 2 else a).astype(np.int64) @ (b.T if form == 0 else b).astype(np.int64)
    for poison in POISONS:
        got = matmul(BF16M, form, a * 2.0 ** 17, b * 2.0 ** -17, M, N, K, poison)
        assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32)), (form, M, N, K, poison)
    return a, b, want


@pytest.mark.parametrize("form", [0, 1, 2])
def test_products_beyond_the_range_of_fp16_are_exact(form):
    for M, N, K, seed in walk(form, 2000):
        matmul_exact(form, M, N, K, seed)
    # which route ran: the fp16 one turns the same operands into inf or NaN
    a, b, want = matmul_exact(form, 33, 65, 17, 7)
    assert np.abs(want).max() > 0 and not np.isfinite(matmul(F16M, form, a * 2.0 ** 17, b * 2.0 ** -17, 33, 65, 17, POISONS[0])).all()


def test_ties_round_to_even():
    """257 lies half way between bfloat16's 256 and 258, 259 between 258 and 260: the even significands are 256 and 260"""
    eye = np.eye(2)
    for form, a in ((0, [[257.0, 259.0]]), (1, [[257.0, 259.0]]), (2, [[257.0], [259.0]])):
        for poison in POISONS:
            got = matmul(BF16M, form, np.array(a), eye, 1, 2, 2, poison)
            assert got.tolist() == [[256.0, 260.0]], (form, got)
    for form in (0, 1):   # the other operand is rounded too; a NaN stays one (in its own row: NaN x 0 is NaN), 3e38 stays finite
        got = matmul(BF16M, form, eye, np.array([[257.0, 0.0], [0.0, 259.0]]), 2, 2, 2, POISONS[0])
        assert got.tolist() == [[256.0, 0.0], [0.0, 260.0]], (form, got)
    got = matmul(BF16M, 0, np.array([[float("nan"), 1.0], [3.0e38, 1.0]]), eye, 2, 2, 2, POISONS[1])
    assert np.isnan(got[0]).all() and np.isfinite(got[1, 0]) and got[1, 0] > 2.9e38 and got[1, 1] == 1.0


@pytest.mark.parametrize("kind", ["attn", "ff"])
def test_operand_zero_is_the_mixed_call_of_before(kind):
    """... and bfloat16 is another rounding of the same gradients"""
    plain, f16 = H.unit_run(kind, "bf16"), H.unit_run(kind, None)
    zero = H.unit_run(kind, "fp16", POISONS[0])
    assert all(same_bits(zero[k], f16[k]) for k in f16)
    assert not same_bits(plain["x"], f16["x"]) and RG.rel(plain["x"], f16["x"]) < 5e-2


def test_the_frontend_on_operand_zero_and_the_raw_gemm():
    from beat_this_amd import _lib as L

    case = BF.conv_case(0, 2, 65)
    run = lambda poison, operand, **kw: H.abi_front_unit(case["sd"], "conv", conv_dims(0), 2, 65, case["x"], case["g"], poison, operand, **kw)
    both = run(POISONS[0], "bf16")
    # operand = 0 is the fp16 call; with mixed = 0 the operand is not read
    f16 = run(POISONS[0], "fp16")
    assert not same_bits(f16["x"], both["x"]) and not same_bits(f16["save_pre"], both["save_pre"])
    fp32, ignored = run(POISONS[0], None), run(POISONS[1], "bf16", mixed=False)
    assert all(same_bits(fp32[k], ignored[k]) for k in fp32) and not same_bits(fp32["x"], both["x"])
    # the raw GEMM: mixed = 1 of bt_train_matmul is bt_train_matmul_mixed
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal((65, 100)), rng.standard_normal((33, 100))
    ga, gb, gc = guarded(a, POISONS[0]), guarded(b, POISONS[0]), Guarded((65, 33), torch.float32).fill(POISONS[0])
    L.check(L.lib().bt_train_matmul_mixed(L.stream_ptr(dev()), 0, ga.ptr(), gb.ptr(), 65, 33, 100, gc.ptr()))
    torch.cuda.synchronize()
    assert_intact(("A", ga), ("B", gb), ("C", gc))
    assert np.array_equal(gc.t.cpu().numpy(), matmul(F16M, 0, a, b, 65, 33, 100, POISONS[1]))


def test_switching_to_bf16_and_back_leaves_the_other_routes_as_they_were():
    never, switched, run, x, want32, want16 = H.switching()
    bf = run(H.both_parts(switched, "16-mixed", "bf16"))
    moved = [k for k in want16 if not same_bits(bf[k], want16[k])]
    assert len(bf) == len(want16) == 102 and len(moved) > 90, len(moved)
    for k in want32:   # (another rounding of the same gradients, not other gradients)
        assert RG.rel(bf[k], want32[k]) < 0.2, k
    H.inference_never_looks_at_the_switch(never, switched, x)
    back16 = run(H.both_parts(switched, "16-mixed", "fp16"))
    assert all(same_bits(back16[k], want16[k]) for k in want16)
    back32 = run(H.both_parts(switched, "32-true"))
    assert all(same_bits(back32[k], want32[k]) for k in want32)
    # one part alone: the trunk on bfloat16 leaves the frontend's own launches on fp32 (its gradients move with what flows back)
    half = run(switched.set_train_precision("16-mixed", "bf16"))
    assert not same_bits(half["beat"], want32["beat"]) and not same_bits(half["x"], want32["x"])
    stem = "frontend.stem.conv2d.weight"
    assert RG.rel(half[stem], want32[stem]) < 0.2
    switched.set_train_precision("32-true")
