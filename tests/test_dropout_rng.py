"""The generator and the mask contract of the training route's dropout, without a GPU: bt_philox4x32_10_host against the
Random123 known answers, bt_dropout_mask_host against the numpy restatement of the header's mapping (route_reference.py),
the kept fraction, the independence of sites / streams / seeds, and the argument checks."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import route_reference as REF
from conftest import ROOT

SITES = (REF.ATTN_P, REF.ATTN_OUT, REF.FF_HIDDEN, REF.FF_OUT)
SIGMAS = 5.0


def L():
    from beat_this_amd import _lib

    _lib.build()
    return _lib


def host_mask(p, seed, stream, site, B, T, dim, hidden):
    lib = L()
    d = lib.TrainDropout(p=p, seed=seed, stream=stream)
    n = B * (dim // 32) * T * T if site == REF.ATTN_P else B * T * (hidden if site == REF.FF_HIDDEN else dim)
    out = np.full(n, 7, dtype=np.uint8)
    lib.check(lib.lib().bt_dropout_mask_host(C.byref(d), site, B, T, dim, hidden, out.ctypes.data))
    assert set(np.unique(out)) <= {0, 1}            # every byte was written
    return out


def test_binding_of_the_dropout_entry_points():
    lib = L()
    header = open(os.path.join(ROOT, "include", "beat_this_amd.h")).read()
    assert re.search(r"#define BT_ABI_VERSION 600\b", header) and lib.lib().bt_version() == 600
    for name in ("bt_train_forward_dropout", "bt_train_backward_dropout", "bt_train_workspace_bytes_dropout",
                 "bt_train_dropout_struct_sizes", "bt_philox4x32_10_host", "bt_dropout_mask_host"):
        assert hasattr(lib.lib(), name) and name in lib.EXPORTS and re.search(r"\b%s\(" % name, header), name
    for name, value in (("BT_DROP_ATTN_P", lib.DROP_ATTN_P), ("BT_DROP_ATTN_OUT", lib.DROP_ATTN_OUT),
                        ("BT_DROP_FF_HIDDEN", lib.DROP_FF_HIDDEN), ("BT_DROP_FF_OUT", lib.DROP_FF_OUT)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert (lib.DROP_ATTN_P, lib.DROP_ATTN_OUT, lib.DROP_FF_HIDDEN, lib.DROP_FF_OUT) == SITES
    out = (C.c_int32 * 4)()
    lib.lib().bt_train_dropout_struct_sizes(out)
    D = lib.TrainDropout
    assert list(out) == [C.sizeof(D), D.p.offset, D.seed.offset, D.stream.offset] == [24, 0, 8, 16]
    # the second workspace query: the forward's is the old one, the backward of the two units with dropout grows by [B T, dim]
    for unit in (lib.UNIT_ATTN, lib.UNIT_FF, lib.UNIT_NORM, lib.TRAIN_UNIT_HEAD):
        for B, T, D_, hid in ((1, 1, 64, 128), (2, 65, 96, 192), (8, 1500, 512, 2048)):
            old = [lib.lib().bt_train_workspace_bytes(unit, b, B, T, D_, hid) for b in (0, 1)]
            new = [lib.lib().bt_train_workspace_bytes_dropout(unit, b, B, T, D_, hid) for b in (0, 1)]
            assert new[0] == old[0] and new[1] % 256 == 0
            grows = unit in (lib.UNIT_ATTN, lib.UNIT_FF)
            assert new[1] - old[1] == ((B * T * D_ * 4 + 255) // 256 * 256 if grows else 0), (unit, B, T)
    assert lib.lib().bt_train_workspace_bytes_dropout(lib.UNIT_FF, 1, 1, 8, 48, 96) == 0


KNOWN_ANSWERS = [   # Random123's kat_vectors for philox4x32 with 10 rounds
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KNOWN_ANSWERS)
def test_philox_known_answers(ctr, key, want):
    lib = L()
    c, k, out = (C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), (C.c_uint32 * 4)()
    lib.lib().bt_philox4x32_10_host(c, k, out)
    assert tuple(out) == want, [hex(v) for v in out]
    assert tuple(int(v) for v in REF.philox4x32_10(ctr, key)) == want       # (the restatement stands on the same answers)


@pytest.mark.parametrize("dim", [32, 96])
@pytest.mark.parametrize("T", [1, 3, 4, 5, 63, 65])
def test_host_twin_equals_the_numpy_restatement(T, dim):
    B, hidden = 2, 2 * dim
    for p in (0.0, 0.2, 0.5):
        for site in SITES:
            seed, stream = 0x1234_5678_9ABC_DEF0 + site, (1 << 40) + 3 * T
            got = host_mask(p, seed, stream, site, B, T, dim, hidden)
            want = REF.mask(p, seed, stream, site, B, T, dim, hidden)
            assert np.array_equal(got, want.reshape(-1)), (p, site)
            if p == 0.0:
                assert got.all()


def _within(kept, n, q):
    """|kept - n q| within SIGMAS binomial standard deviations"""
    return abs(kept - n * q) <= SIGMAS * math.sqrt(n * q * (1 - q))


@pytest.mark.parametrize("p", [0.2, 0.5])
def test_kept_fraction(p):
    B, T, dim, hidden = 2, 50, 160, 320            # 16000 elements at the dim sites, 32000 hidden, 50000 probabilities
    for site in SITES:
        for seed in (0, 1, 2 ** 63 + 5):
            m = host_mask(p, seed, 11, site, B, T, dim, hidden)
            assert _within(int(m.sum()), m.size, 1 - p), (site, seed, m.mean())


def test_sites_streams_and_seeds_are_independent():
    B, T, dim, hidden, p = 2, 50, 160, 160, 0.2    # (hidden = dim: the three row sites have one shape)
    base = dict(seed=5, stream=9)
    m = {s: host_mask(p, base["seed"], base["stream"], s, B, T, dim, hidden) for s in SITES}
    for s in SITES:
        assert np.array_equal(m[s], host_mask(p, base["seed"], base["stream"], s, B, T, dim, hidden))   # same arguments, same mask
        others = [host_mask(p, base["seed"], base["stream"] + 1, s, B, T, dim, hidden),
                  host_mask(p, base["seed"], base["stream"] + (1 << 32), s, B, T, dim, hidden),
                  host_mask(p, base["seed"] + 1, base["stream"], s, B, T, dim, hidden),
                  host_mask(p, base["seed"] + (1 << 32), base["stream"], s, B, T, dim, hidden)]
        others += [m[o] for o in (REF.ATTN_OUT, REF.FF_HIDDEN, REF.FF_OUT) if o != s and s != REF.ATTN_P]
        for other in others:
            diff = int((m[s] != other).sum())
            assert _within(diff, m[s].size, 2 * p * (1 - p)), (s, diff / m[s].size)


def test_argument_checks():
    lib = L()
    out = np.zeros(4 * 32, dtype=np.uint8)
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        d = lib.TrainDropout(p=bad, seed=0, stream=0)
        assert lib.lib().bt_dropout_mask_host(C.byref(d), REF.ATTN_OUT, 1, 4, 32, 64, out.ctypes.data) == lib.BT_ERR_ARG, bad
        with pytest.raises(ValueError):
            lib.check(lib.BT_ERR_ARG)
        a = lib.TrainArgs()
        a.B, a.T, a.dim, a.hidden, a.rope_len = 1, 8, 64, 128, 1536
        for fn in (lib.lib().bt_train_forward_dropout, lib.lib().bt_train_backward_dropout):
            for unit in (lib.UNIT_ATTN, lib.UNIT_FF):
                assert fn(None, unit, C.byref(a), C.byref(d)) == lib.BT_ERR_ARG
                assert b"0 <= p < 1" in lib.lib().bt_last_error()
    d = lib.TrainDropout(p=0.2, seed=0, stream=0)
    assert lib.lib().bt_dropout_mask_host(C.byref(d), 4, 1, 4, 32, 64, out.ctypes.data) == lib.BT_ERR_ARG
    assert lib.lib().bt_dropout_mask_host(C.byref(d), REF.ATTN_OUT, 1, 4, 48, 64, out.ctypes.data) == lib.BT_ERR_ARG
    assert lib.lib().bt_dropout_mask_host(None, REF.ATTN_OUT, 1, 4, 32, 64, out.ctypes.data) == lib.BT_ERR_ARG
    # the norm and the head take no dropout; p = 0 there is no dropout and passes on to the usual checks
    a = lib.TrainArgs()
    a.B, a.T, a.dim, a.hidden, a.rope_len = 1, 8, 64, 128, 1536
    for fn in (lib.lib().bt_train_forward_dropout, lib.lib().bt_train_backward_dropout):
        for unit in (lib.UNIT_NORM, lib.TRAIN_UNIT_HEAD):
            assert fn(None, unit, C.byref(a), C.byref(d)) == lib.BT_ERR_ARG
            assert b"BT_UNIT_ATTN and BT_UNIT_FF only" in lib.lib().bt_last_error()
            zero = lib.TrainDropout(p=0.0)
            assert fn(None, unit, C.byref(a), C.byref(zero)) == lib.BT_ERR_ARG
            assert b"null" in lib.lib().bt_last_error()


def test_the_model_refuses_bad_rates():
    from beat_this_amd.model import BeatThis

    for bad in (-0.1, 1.0, float("nan")):
        m = BeatThis(transformer_dim=64, n_layers=1, ff_mult=2, dropout={"frontend": 0.1, "transformer": bad})
        with pytest.raises(ValueError, match="0 <= p < 1"):
            m.enable_dropout(seed=1)
    m = BeatThis(transformer_dim=64, n_layers=1, ff_mult=2)
    assert m.dropout == {"frontend": 0.1, "transformer": 0.2} and m.dropout_state() is None
    m.enable_dropout(seed=7)
    assert m.dropout_state() == {"seed": 7, "calls": 0}
    m.set_dropout_state({"seed": 9, "calls": 12})
    assert m.dropout_state() == {"seed": 9, "calls": 12}
    m.disable_dropout()
    assert m.dropout_state() is None
