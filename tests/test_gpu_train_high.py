"""What belongs to "32-high" alone, on the GPU (csrc/train_mixed.inc, csrc/train_front_mixed.inc with Operand<bf16x3>, DESIGN.md
section 25; the tests it shares with the other formats are in tests/test_gpu_train_formats.py): the GEMM exactly -- a split operand
against an 8-bit one, two split operands minus their lo lo term in int64, inf and NaN rows -- another arithmetic than bfloat16's
and close to fp32's, no bleed into the other precisions, a known operand, the ``*_x3`` workspace queries and a workspace of the
mixed size.

Every device entry is called on gpu_util.Guarded buffers: guard bands on both sides, both poison patterns."""
import ctypes as C

import numpy as np
import pytest
import torch

import route_grads as RG
import route_harness as H
import x3_reference as X3
from gpu_util import POISONS, Guarded, assert_intact, dev
from route_harness import conv_dims, matmul, same_bits, walk

pytestmark = pytest.mark.gpu
X3M, BF16M = 4, 2        # `mixed` of bt_train_matmul / bt_train_attention: 1 + BT_OPERAND_*
OPERAND_X3 = 3


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


@pytest.mark.parametrize("form", [0, 1, 2])
def test_a_split_operand_against_an_eight_bit_one_is_exact(form):
    for M, N, K, seed in walk(form, 3000):
        split_against_eight_bits(form, M, N, K, seed)
    split_against_eight_bits(form, 33, 65, 17, 7, also_bf16=True)


@pytest.mark.parametrize("form", [0, 1, 2])
def test_two_split_operands_lose_the_lo_lo_term_and_nothing_else(form):
    for M, N, K, seed in walk(form, 3000):
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


@pytest.mark.parametrize("kind", ["attn", "ff"])
def test_split_operands_are_another_arithmetic_for_the_same_gradients(kind):
    """neither the bfloat16 call's bits nor far from them"""
    plain, bf = H.unit_run(kind, "bf16x3"), H.unit_run(kind, "bf16")
    assert not same_bits(plain["x"], bf["x"]) and RG.rel(plain["x"], bf["x"]) < 5e-2


def test_the_frontend_on_split_operands_stays_close_to_fp32():
    case = X3.conv_case(0, 2, 65)
    both, fp32 = (H.abi_front_unit(case["sd"], "conv", conv_dims(0), 2, 65, case["x"], case["g"], POISONS[0], operand) for operand in ("bf16x3", None))
    assert not same_bits(fp32["x"], both["x"]) and RG.rel(both["x"], fp32["x"]) < 1e-3


def test_switching_to_32_high_and_back_leaves_the_other_routes_as_they_were():
    HIGH = "32-high"
    never, switched, run, x, want32, want16 = H.switching()
    wantbf = run(H.both_parts(never, "16-mixed", "bf16"))
    high = run(H.both_parts(switched, HIGH))
    moved = [k for k in want32 if not same_bits(high[k], want32[k])]
    assert len(high) == len(want32) == 102 and len(moved) > 90, len(moved)
    for k in want32:   # (the same gradients, 2^-17 of an operand away, not bfloat16's)
        assert RG.rel(high[k], want32[k]) < 1e-2, k
    assert sum(not same_bits(high[k], wantbf[k]) for k in wantbf) > 90
    H.inference_never_looks_at_the_switch(never, switched, x)
    back32 = run(H.both_parts(switched, "32-true"))
    assert all(same_bits(back32[k], want32[k]) for k in want32)
    H.both_parts(switched, HIGH)
    back16 = run(H.both_parts(switched, "16-mixed"))
    assert all(same_bits(back16[k], want16[k]) for k in want16)
    H.both_parts(switched, HIGH)
    backbf = run(H.both_parts(switched, "16-mixed", "bf16"))
    assert all(same_bits(backbf[k], wantbf[k]) for k in wantbf)
    # one part alone: the trunk on 32-high leaves the frontend's own launches on fp32
    half = run(switched.set_frontend_precision("32-true").set_train_precision(HIGH))
    assert not same_bits(half["beat"], want32["beat"]) and not same_bits(half["x"], want32["x"]) and not same_bits(half["x"], high["x"])
    switched.set_train_precision("32-true")


def test_a_known_operand_is_not_what_is_refused():
    """operand 3 is known: what is refused then is the null pointers, and on the units without a mixed form `mixed` itself"""
    from beat_this_amd import _lib as L

    lib, s = L.lib(), L.stream_ptr(dev())
    a = L.TrainArgs(B=1, T=8, dim=64, hidden=0, operand=OPERAND_X3)
    assert lib.bt_train_forward_mixed(s, L.UNIT_ATTN, C.byref(a), None) == L.BT_ERR_ARG and b"operand" not in lib.bt_last_error()
    a = L.FrontArgs(B=2, T=3, F=128, C=32, dim=0, mixed=1, operand=OPERAND_X3)
    assert lib.bt_front_forward(s, L.FRONT_STEM, C.byref(a)) == L.BT_ERR_ARG and b"mixed" in lib.bt_last_error()
    assert lib.bt_train_matmul(s, X3M, 0, None, None, 1, 1, 1, None, None, None, 0, None, None, 0, 0, None, 0) == L.BT_ERR_ARG
    assert b"mixed" not in lib.bt_last_error()
    torch.cuda.synchronize()


def test_the_x3_queries_are_the_fp32_size_plus_both_images():
    """... and 0 for unsupported shapes and for units without a mixed form"""
    from beat_this_amd import _lib as L

    lib = L.lib()
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


def test_a_workspace_of_the_mixed_size_is_too_small():
    """a conv call on split operands with the one-image workspace: BT_ERR_WORKSPACE, nothing launched, nothing written"""
    from beat_this_amd import _lib as L

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
