"""The training route's GEMMs and attention sweeps element by element, on the fp32 route and the 16-mixed one (csrc/train.hip,
csrc/train_mixed.inc), through the raw diagnostic entries bt_train_matmul and bt_train_attention -- which launch through the
host helpers the unit calls use (linear_fwd, linear_bwd_input, linear_bwd_weight, attn_fwd_sweep, attn_bwd_sweeps, each with the
call's Launch context), and whose GEMMs share one epilogue (gemm_epilogue of csrc/train_common.h).

1. Products of integers in [-8, 8]: every partial sum is an integer below 2^24, so C has to be the int64 product bit for bit
   whatever the order, on the fp32 MFMA as on the fp16 one -- the three forms at the edges of the 64-wide, 128-wide and 32-wide
   tiles, the weight gradient through the real split path (partials per BT_TRAIN_DW_ROWS chunk in the workspace, one to five
   chunks), the epilogue (bias, residual, +=, GELU into act) and its two dropout forms at p = 0.5 against bt_dropout_mask_host.
2. "Selection attention" (tests/train_exact_reference.py): inputs whose softmax is exact, so O, lse and dQ | dK | dV have to
   equal the fp64 expectation bit for bit (but for the sign of a zero), plain and under a p = 0.5 mask; the backward is given the
   host's lse and delta.  tests/test_train_exact_reference.py shows on the CPU that both routes' orders of operation reproduce
   that expectation, so a mismatch here is a kernel error.

Every call runs on gpu_util.Guarded buffers: guard bands on both sides, both poison patterns."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import train_exact_reference as X
from gpu_util import POISONS, Guarded, assert_intact, dev

pytestmark = pytest.mark.gpu
EDGES = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)   # the 64-wide fp32 tile, the 128-wide mixed tile, the 32-wide MFMA tile
KS = (1, 15, 16, 17, 33, 64, 100)
SPLIT_ROWS = (1023, 1024, 1025, 2047, 2049, 3073, 4100)   # one to five chunks, a last chunk of 1, 1023 and 4 rows
SPLIT_SHAPES = ((33, 129), (65, 64), (6, 192))            # (6, 192): to_gates
EPI_SHAPES = ((65, 132), (130, 260))                      # N a multiple of 4; across a tile both ways on both routes
EPI_K = 33


def guarded(arr, poison):
    t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32))
    return Guarded(t.shape, torch.float32).fill(poison, data=t.to(dev()))


def matmul(mixed, form, a, b, M, N, K, poison, bias=None, resid=None, c_old=None, act=False, drop=None, ws_bytes=None):
    """bt_train_matmul on guarded buffers -> (rc, C, act or None).  c_old: C's contents before the call (accum); drop: (seed,
    stream, site, drop_act) at p = 0.5"""
    from beat_this_amd import _lib as L

    lib = L.lib()
    named = [("A", guarded(a, poison)), ("B", guarded(b, poison))]
    gc = Guarded((M, N), torch.float32).fill(poison) if c_old is None else guarded(c_old, poison)
    named.append(("C", gc))
    opt = {}
    for name, arr in (("bias", bias), ("resid", resid)):
        if arr is not None:
            opt[name] = guarded(arr, poison)
            named.append((name, opt[name]))
    if act:
        opt["act"] = Guarded((M, N), torch.float32).fill(poison)
        named.append(("act", opt["act"]))
    need = lib.bt_train_matmul_workspace_bytes(form, M, N, K)
    n = need if ws_bytes is None else ws_bytes
    ws = Guarded((max(n, 1),), torch.uint8).fill(poison)
    named.append(("workspace", ws))
    d, site, drop_act = None, 0, 0
    if drop is not None:
        d, site, drop_act = C.byref(L.TrainDropout(p=0.5, seed=drop[0], stream=drop[1])), drop[2], drop[3]
    ptr = lambda k: opt[k].ptr() if k in opt else None
    rc = lib.bt_train_matmul(L.stream_ptr(dev()), mixed, form, named[0][1].ptr(), named[1][1].ptr(), M, N, K, gc.ptr(), ptr("bias"),
                             ptr("resid"), int(c_old is not None), ptr("act"), d, site, drop_act, ws.ptr() if n else None, n)
    torch.cuda.synchronize()
    assert_intact(*named)
    return rc, gc.t.cpu().numpy(), opt["act"].t.cpu().numpy() if act else None


def operands(form, M, N, K, seed):
    """integer operands of a form and their int64 product [M, N]"""
    rng = np.random.default_rng(seed)
    a = rng.integers(-8, 9, size=(K, M) if form == 2 else (M, K))
    b = rng.integers(-8, 9, size=(N, K) if form == 0 else (K, N))
    return a, b, (a.T if form == 2 else a).astype(np.int64) @ (b.T if form == 0 else b).astype(np.int64), rng


def first_difference(got, want):
    bad = np.argwhere(got != want)
    r, c = (int(i) for i in bad[0])
    return f"{len(bad)} of {got.size} elements differ, the first at (row, column) = {(r, c)}: got {got[r, c]!r}, want {want[r, c]!r}"


def assert_exact(got, want, what):
    want32 = want.astype(np.float32)
    assert np.array_equal(want32.astype(np.int64), want), "the expectation is not exact in fp32"
    assert np.array_equal(got, want32), f"{what}: " + first_difference(got, want32)


# ---- 1. the GEMMs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [0, 1])
@pytest.mark.parametrize("form", [0, 1, 2])
def test_products_of_small_integers_are_exact(form, mixed):
    from beat_this_amd import _lib as L

    n = 0
    for i, M in enumerate(EDGES):
        for j in range(3):   # (three of the N per M, all of them over the M)
            N = EDGES[(i + 4 * j + form) % len(EDGES)]
            for K in KS:
                a, b, want, _ = operands(form, M, N, K, 5000 * mixed + 1000 * form + n)
                rc, got, _ = matmul(mixed, form, a, b, M, N, K, POISONS[n % 2])
                L.check(rc)
                assert_exact(got, want, f"mixed={mixed} form={form} M={M} N={N} K={K}")
                n += 1


@pytest.mark.parametrize("mixed", [0, 1])
@pytest.mark.parametrize("M,N", SPLIT_SHAPES)
def test_the_split_weight_gradient_is_exact(M, N, mixed):
    """form 2 through linear_bwd_weight: blockIdx.z = the chunk, partials at C + z M N in the workspace, reduce_parts_kernel.
    The workspace is exactly the query's size between its guard bands; the largest sum is 4100 * 64 = 262 400."""
    from beat_this_amd import _lib as L

    for K in SPLIT_ROWS:
        chunks = (K + L.TRAIN_DW_ROWS - 1) // L.TRAIN_DW_ROWS
        assert L.lib().bt_train_matmul_workspace_bytes(2, M, N, K) == chunks * M * N * 4
        a, b, want, _ = operands(2, M, N, K, 100 * K + M + mixed)
        for poison in POISONS:
            rc, got, _ = matmul(mixed, 2, a, b, M, N, K, poison)
            L.check(rc)
            assert_exact(got, want, f"mixed={mixed} split dW M={M} N={N} rows={K} ({chunks} chunks)")


def gelu64(v):
    return np.array([0.5 * x * (1.0 + math.erf(x / math.sqrt(2.0))) for x in v.reshape(-1).astype(np.float64)]).reshape(v.shape)


def assert_act(act, value, factor, what):
    """act against factor * the fp64 GELU of the exact value, element by element within 1e-6 max(1, |v|): erff at 4 ulp of a
    value of at most 1 is 2.4e-7, halved and times |v|, plus three roundings; a value taken from another row, column or mask
    group is off by order 1"""
    want = factor * gelu64(value)
    err = np.abs(act.astype(np.float64) - want)
    tol = 1e-6 * np.maximum(1.0, np.abs(value.astype(np.float64)))
    worst = np.unravel_index(np.argmax(err / tol), err.shape)
    print(f"{what}: act is at most {err[worst] / tol[worst]:.3f} of its tolerance away (at {worst}, value {value[worst]})")
    assert np.isfinite(act).all() and (err <= tol).all(), \
        f"{what}: act{tuple(int(i) for i in worst)} = {act[worst]!r}, want {want[worst]!r} (value {value[worst]})"


def epilogue_inputs(M, N, seed):
    """integer A, B, their product, bias, resid and old C.  (The tests then choose the residual of half of the elements so that
    the value lands in [-6, 6], where the GELU is neither 0 nor the identity.)"""
    a, b, prod, rng = operands(0, M, N, EPI_K, seed)
    bias = rng.integers(-8, 9, size=N)
    c_old = rng.integers(-8, 9, size=(M, N))
    resid = rng.integers(-8, 9, size=(M, N))
    return a, b, prod, bias, resid, c_old, rng


@pytest.mark.parametrize("mixed", [0, 1])
@pytest.mark.parametrize("M,N", EPI_SHAPES)
def test_the_epilogue_is_exact(M, N, mixed):
    from beat_this_amd import _lib as L

    for i, poison in enumerate(POISONS):
        a, b, prod, bias, resid, c_old, rng = epilogue_inputs(M, N, 31 * M + mixed + i)
        small = rng.random((M, N)) < 0.5
        resid = np.where(small, rng.integers(-6, 7, size=(M, N)) - prod - bias[None, :] - c_old, resid)
        want = prod + bias[None, :] + resid + c_old
        rc, got, act = matmul(mixed, 0, a, b, M, N, EPI_K, poison, bias=bias, resid=resid, c_old=c_old, act=True)
        L.check(rc)
        what = f"mixed={mixed} epilogue M={M} N={N}"
        assert_exact(got, want, what)
        assert_act(act, got, 1.0, what)
        # each optional input on its own
        for kw, w in ((dict(bias=bias), prod + bias[None, :]), (dict(resid=resid), prod + resid), (dict(c_old=c_old), prod + c_old)):
            rc, got, _ = matmul(mixed, 0, a, b, M, N, EPI_K, poison, **kw)
            L.check(rc)
            assert_exact(got, w, f"{what} {list(kw)}")


@pytest.mark.parametrize("mixed", [0, 1])
@pytest.mark.parametrize("M,N", EPI_SHAPES)
def test_the_two_dropout_forms_are_exact(M, N, mixed):
    """p = 0.5: 1 / (1 - p) is exactly 2 and kept values stay integers.  drop_act = 0: C = resid + m 2 (A B^T + bias);
    drop_act = 1: C as without dropout, act = m 2 gelu(C).  The mask is bt_dropout_mask_host's, per element."""
    from beat_this_amd import _lib as L

    for i, (seed, stream) in enumerate(X.DROPS):
        keep = np.zeros((M, N), dtype=np.uint8)
        d = L.TrainDropout(p=0.5, seed=seed, stream=stream)
        L.check(L.lib().bt_dropout_mask_host(C.byref(d), L.DROP_FF_HIDDEN, 1, M, 32, N, keep.ctypes.data))
        assert 0.4 < keep.mean() < 0.6
        keep = keep.astype(np.int64)
        a, b, prod, bias, resid, _, rng = epilogue_inputs(M, N, 77 * M + 2 * i + mixed)
        poison = POISONS[i % 2]
        for drop_act in (0, 1):
            what = f"mixed={mixed} dropout drop_act={drop_act} M={M} N={N} seed={seed:#x} stream={stream:#x}"
            base = 2 * keep * (prod + bias[None, :]) if drop_act == 0 else prod + bias[None, :]
            small = rng.random((M, N)) < 0.5
            res = np.where(small, rng.integers(-6, 7, size=(M, N)) - base, resid)
            want = base + res
            rc, got, act = matmul(mixed, 0, a, b, M, N, EPI_K, poison, bias=bias, resid=res, act=True,
                                  drop=(seed, stream, L.DROP_FF_HIDDEN, drop_act))
            L.check(rc)
            assert_exact(got, want, what)
            if drop_act == 0:
                assert_act(act, got, 1.0, what)
            else:
                dropped = keep == 0
                assert (act[dropped] == 0).all(), f"{what}: act is not zero on {int((act[dropped] != 0).sum())} dropped elements"
                assert_act(act, got, 2.0 * keep, what)


def test_matmul_refuses_bad_arguments():
    from beat_this_amd import _lib as L

    lib, z = L.lib(), np.zeros((4, 4), dtype=np.int64)
    assert lib.bt_train_matmul(None, 0, 3, None, None, 1, 1, 1, None, None, None, 0, None, None, 0, 0, None, 0) == L.BT_ERR_ARG
    for mixed in (0, 1):
        assert matmul(mixed, 3, z, z, 4, 4, 4, POISONS[0])[0] == L.BT_ERR_ARG
        assert matmul(mixed, -1, z, z, 4, 4, 4, POISONS[0])[0] == L.BT_ERR_ARG
        assert matmul(mixed, 1, z, z, 4, 4, 4, POISONS[0], bias=np.zeros(4))[0] == L.BT_ERR_ARG
        assert matmul(mixed, 2, z, z, 4, 4, 4, POISONS[0], c_old=z)[0] == L.BT_ERR_ARG
        assert matmul(mixed, 0, np.zeros((4, 4)), np.zeros((6, 4)), 4, 6, 4, POISONS[0], drop=(1, 1, L.DROP_FF_OUT, 0))[0] == L.BT_ERR_ARG
        assert matmul(mixed, 0, z, z, 4, 4, 4, POISONS[0], drop=(1, 1, L.DROP_ATTN_P, 0))[0] == L.BT_ERR_ARG
        assert matmul(mixed, 0, z, z, 4, 4, 4, POISONS[0], drop=(1, 1, L.DROP_FF_OUT, 1))[0] == L.BT_ERR_ARG   # (no act to mask)
        # one byte short of the partials is refused before any launch (the poisoned C stays as it was)
        K = 2 * L.TRAIN_DW_ROWS + 1
        need = lib.bt_train_matmul_workspace_bytes(2, 4, 4, K)
        assert need == 3 * 4 * 4 * 4 and lib.bt_train_matmul_workspace_bytes(0, 4, 4, K) == 0
        zk = np.zeros((K, 4))
        rc, got, _ = matmul(mixed, 2, zk, zk, 4, 4, K, POISONS[1], ws_bytes=need - 1)
        assert rc == L.BT_ERR_WORKSPACE and (got.view(np.uint32) == 0x7B7B7B7B).all()
        assert matmul(mixed, 2, zk, zk, 4, 4, K, POISONS[1], ws_bytes=0)[0] == L.BT_ERR_ARG


# ---- 2. selection attention ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_of(B, T, dim, drop):
    return X.make_case(B, T, dim, drop)


def attention(mixed, case, drop, poison):
    """bt_train_attention forward, then backward from the HOST's lse and delta -> dict O, lse, dq, dk, dv shaped like the
    expectation's"""
    from beat_this_amd import _lib as L

    lib, B, T, dim, H = L.lib(), case.B, case.T, case.dim, case.H
    d = None if drop is None else C.byref(L.TrainDropout(p=X.DROP_P, seed=drop[0], stream=drop[1]))
    qkv, dO = guarded(case.qkv(), poison), guarded(case.rows(case.dO), poison)
    lse_in, delta = guarded(case.per_row(case.lse), poison), guarded(case.per_row(case.delta), poison)
    O, lse, dqkv = (Guarded(s, torch.float32).fill(poison) for s in ((B * T, dim), (B * T, H), (B * T, 3 * dim)))
    named = [("qkv", qkv), ("dO", dO), ("lse (host)", lse_in), ("delta", delta), ("O", O), ("lse", lse), ("dqkv", dqkv)]
    L.check(lib.bt_train_attention(L.stream_ptr(dev()), mixed, 0, B, T, dim, qkv.ptr(), d, O.ptr(), lse.ptr(), None, None, None))
    L.check(lib.bt_train_attention(L.stream_ptr(dev()), mixed, 1, B, T, dim, qkv.ptr(), d, None, lse_in.ptr(), dO.ptr(), delta.ptr(),
                                   dqkv.ptr()))
    torch.cuda.synchronize()
    assert_intact(*named)
    g = dqkv.t.cpu().numpy()
    return dict(O=case.unrows(O.t.cpu().numpy()), lse=case.unrows(lse.t.cpu().numpy(), 1)[..., 0], dq=case.unrows(g[:, :dim]),
                dk=case.unrows(g[:, dim:2 * dim]), dv=case.unrows(g[:, 2 * dim:]))


@pytest.mark.parametrize("mixed", [0, 1])
@pytest.mark.parametrize("B,T,dim", X.CASES)
def test_selection_attention_is_exact(B, T, dim, mixed):
    n = 0
    for drop in (None,) + X.DROPS:
        case = case_of(B, T, dim, drop)
        want = X.expectation(case)
        for poison in POISONS if drop is None else (POISONS[n % 2],):
            got = attention(mixed, case, drop, poison)
            what = f"mixed={mixed} {(B, T, dim)} dropout {drop} poison {poison:#x}"
            for name in ("O", "lse", "dq", "dk", "dv"):
                g, w = (got[name][..., None], want[name][..., None]) if name == "lse" else (got[name], want[name])
                assert np.isfinite(g).all(), f"{what}: {name} is not finite"
                assert X.same_bits(g, w), f"{what}: " + case.describe(name, g, w)
        n += 1


def test_attention_refuses_bad_arguments():
    from beat_this_amd import _lib as L

    lib = L.lib()
    buf = Guarded((8, 192), torch.float32).fill(POISONS[0])
    p, s = buf.ptr(), L.stream_ptr(dev())
    assert lib.bt_train_attention(s, 0, 0, 1, 8, 64, None, None, p, p, None, None, None) == L.BT_ERR_ARG
    assert lib.bt_train_attention(s, 0, 0, 1, 8, 64, p, None, None, p, None, None, None) == L.BT_ERR_ARG
    assert lib.bt_train_attention(s, 1, 1, 1, 8, 64, p, None, None, p, p, None, p) == L.BT_ERR_ARG
    assert lib.bt_train_attention(s, 1, 0, 1, 8, 48, p, None, p, p, None, None, None) == L.BT_ERR_ARG
    assert lib.bt_train_attention(s, 1, 0, 0, 8, 64, p, None, p, p, None, None, None) == L.BT_ERR_ARG
    assert lib.bt_train_attention(s, 0, 0, 1, 8, 64, p + 4, None, p, p, None, None, None) == L.BT_ERR_ARG
    d = L.TrainDropout(p=1.0, seed=1, stream=1)
    assert lib.bt_train_attention(s, 0, 0, 1, 8, 64, p, C.byref(d), p, p, None, None, None) == L.BT_ERR_ARG
    torch.cuda.synchronize()
    assert_intact(("buffer", buf))
