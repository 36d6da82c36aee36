"""The "selection attention" cases of tests/train_exact_reference.py without a GPU: for every case the GPU test runs, plain and
under a p = 0.5 mask, the generator's preconditions hold and the two numpy emulations of the device's orders of operation
(sequential keys in fp32; tiles of 32 with fp16 rounding of P and dS, in both directions) give the fp64 expectation bit for
bit -- so a mismatch on the device means a kernel error, not a property of the inputs -- and three mutants of the tiled order
each change at least one output tensor of every case with T >= 33."""
import numpy as np
import pytest

import train_exact_reference as X

VARIANTS = [None] + list(X.DROPS)


@pytest.fixture(scope="module", autouse=True)
def library():
    """the masks come from the library's host twin (bt_dropout_mask_host)"""
    from beat_this_amd import _lib

    _lib.build()
    return _lib
NAMES = ("O", "lse", "dq", "dk", "dv")


def check(case, got, what):
    want = X.expectation(case)
    for n in NAMES:
        g, w = (got[n][..., None], want[n][..., None]) if n == "lse" else (got[n], want[n])
        assert X.same_bits(got[n], want[n]), f"{what}: " + case.describe(n, g, w)


@pytest.mark.parametrize("B,T,dim", X.CASES)
def test_both_orders_give_the_expectation_bit_for_bit(B, T, dim):
    for drop in VARIANTS:
        case = X.make_case(B, T, dim, drop)
        # the preconditions: the scores' levels, P a power of two, everything the MFMAs read exact in fp16
        assert np.isin(case.P, (0.0, 0.25, 0.5, 1.0)).all() and np.array_equal(case.P.sum(-1), np.ones((B, dim // 32, T)))
        for x in (case.q, case.k, case.v, case.dO, case.Pm, case.dS):
            assert np.array_equal(x.astype(np.float16).astype(np.float64), x)
        assert np.abs(case.dk).max() < 2.0 ** 24 and case.qkv().shape == (B * T, 3 * dim)
        if T > 4:   # a token's query does not simply select its own key
            assert (case.kc != case.qc).any()
        check(case, X.emulate_sequential(case), f"sequential order, {(B, T, dim)}, dropout {drop}")
        check(case, X.emulate_tiled(case), f"tiled order, {(B, T, dim)}, dropout {drop}")


@pytest.mark.parametrize("B,T,dim", [c for c in X.CASES if c[1] >= 33])
def test_mutants_miss_the_expectation(B, T, dim):
    case = X.make_case(B, T, dim, X.DROPS[0])
    want = X.expectation(case)
    for mutant in X.MUTANTS:
        got = X.emulate_tiled(case, mutant)
        changed = [n for n in NAMES if not X.same_bits(got[n], want[n])]
        print(f"{(B, T, dim)} {mutant}: changes {changed}")
        assert changed, (mutant, B, T, dim)
    with pytest.raises(ValueError):
        X.emulate_tiled(case, "no such mutant")


def test_layouts_round_trip():
    case = X.make_case(2, 97, 192)
    qkv = case.qkv()
    for s, x in enumerate((case.q, case.k, case.v)):
        assert np.array_equal(case.unrows(qkv[:, s * 192:(s + 1) * 192]), x)
    assert qkv[97 + 5, 192 + 2 * 32 + 7] == case.k[1, 2, 5, 7]            # row b T + t, section, head h in columns 32 h
    assert np.array_equal(case.unrows(case.per_row(case.lse), 1)[..., 0], case.lse)


def test_the_raw_entries_refuse_bad_arguments_before_any_launch(library):
    L, lib = library, library.lib()
    assert lib.bt_train_matmul(None, 0, 3, None, None, 1, 1, 1, None, None, None, 0, None, None, 0, 0, None, 0) == L.BT_ERR_ARG
    assert b"bt_train_matmul" in lib.bt_last_error()
    assert lib.bt_train_attention(None, 1, 0, 1, 8, 64, None, None, None, None, None, None, None) == L.BT_ERR_ARG
    assert b"bt_train_attention" in lib.bt_last_error()
    for K, chunks in ((1, 1), (1024, 1), (1025, 2), (4100, 5), (12000, 12)):
        assert lib.bt_train_matmul_workspace_bytes(2, 33, 129, K) == chunks * 33 * 129 * 4
        assert lib.bt_train_matmul_workspace_bytes(0, 33, 129, K) == lib.bt_train_matmul_workspace_bytes(1, 33, 129, K) == 0
    assert lib.bt_train_matmul_workspace_bytes(2, 0, 129, 5) == 0
