"""No-GPU checks of the forward's workspace layout (bt_workspace_regions, BT_OPT_WS_GUARD): bt_engine_create and the sizing
entry points make no HIP call, so a description with only the shape fields filled in is enough."""
import ctypes as C
import json
import os

import pytest

from conftest import GOLDEN

# transformer_dim, ff_mult, n_layers, partial_transformers, sum_head: small0 / final0 and the ablation variants of
# test_gpu_model.py::test_ablation_variants_against_oracle
VARIANTS = {"small0": (128, 4, 6, 1, 1), "final0": (512, 4, 6, 1, 1), "no_sum_head": (128, 4, 6, 1, 0),
            "no_partial": (128, 4, 6, 0, 1), "three_layers_d256": (256, 4, 3, 1, 1), "d64_ffmult2": (64, 2, 2, 1, 1),
            "d192": (192, 4, 2, 1, 1)}
BATCHES = (1, 2, 11, 33, 96, 175, 350)
LENGTHS = (1, 37, 1012, 1500, 1536)   # (1536 = rope_len of a PackedModel)
PRECS = (0, 1, 3)


def _engine(name):
    from beat_this_amd import _lib as L

    L.build()
    D, mult, n_layers, partial, sum_head = VARIANTS[name]
    d = L.ModelDesc()
    d.transformer_dim, d.ff_mult, d.n_layers, d.rope_len = D, mult, n_layers, 1536
    d.partial_transformers, d.sum_head = partial, sum_head
    h = C.c_void_p()
    L.check(L.lib().bt_engine_create(C.byref(d), C.byref(h)))
    return L, h


def regions(L, h, B, T, prec):
    n = L.lib().bt_workspace_regions(h, B, T, prec, None, 0)
    assert n > 0, L.lib().bt_last_error()
    buf = (C.c_int64 * (2 * n))()
    assert L.lib().bt_workspace_regions(h, B, T, prec, buf, n) == n
    return [(buf[2 * i], buf[2 * i + 1]) for i in range(n)]


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_workspace_regions_are_ordered_aligned_disjoint_and_sum_to_the_size(name):
    """Every (B, T, precision) of the grid: region 0 is the 256-byte status block at offset 0, regions are 256-aligned and in
    address order, none overlaps the next one even before alignment, the last ends within bt_workspace_bytes and the aligned
    regions tile it exactly.  With the option at 0 the size equals what the library computed before bt_workspace_regions and
    BT_OPT_WS_GUARD existed (tests/golden/workspace_bytes.json, recorded from the previous build)."""
    L, h = _engine(name)
    lib = L.lib()
    before = json.load(open(os.path.join(GOLDEN, "workspace_bytes.json")))
    D, mult = VARIANTS[name][:2]
    try:
        for prec in PRECS:
            for B in BATCHES:
                for T in LENGTHS:
                    total = lib.bt_workspace_bytes(h, B, T, prec)
                    assert total == before[f"{D},{mult},{prec},{B},{T}"], (prec, B, T)
                    r = regions(L, h, B, T, prec)
                    assert r[0] == (0, 256)
                    assert len(r) == (9 if prec == 0 else 16 if prec == 3 else 15)
                    for (b0, e0), (b1, _) in zip(r, r[1:]):
                        assert b0 % 256 == 0 and b0 < e0 <= b1 and b1 == (e0 + 255) // 256 * 256, (prec, B, T, b0, e0, b1)
                    assert r[-1][0] % 256 == 0 and (r[-1][1] + 255) // 256 * 256 == total
    finally:
        lib.bt_engine_destroy(h)


@pytest.mark.parametrize("name", ["small0", "final0", "d64_ffmult2", "d192"])
def test_workspace_guard_inserts_exactly_the_requested_gap(name):
    """BT_OPT_WS_GUARD = g: every region keeps its requested size, the gap after each (alignment slack excluded) is exactly g,
    bt_workspace_bytes grows by g per region, bt_audio2beats_plan's forward_bytes follows, and back at 0 the packed layout
    returns.  Values that are not multiples of 256 are refused."""
    L, h = _engine(name)
    lib = L.lib()
    try:
        v = C.c_int(-1)
        L.check(lib.bt_engine_get_option(h, L.OPT_WS_GUARD, C.byref(v)))
        assert v.value == 0
        assert lib.bt_engine_set_option(h, L.OPT_WS_GUARD, 100) == L.BT_ERR_ARG
        assert lib.bt_engine_set_option(h, L.OPT_WS_GUARD, -256) == L.BT_ERR_ARG
        for g in (256, 1 << 21):
            for prec in PRECS:
                for B, T in ((1, 1), (2, 37), (11, 1500), (33, 1012), (175, 1500)):
                    L.check(lib.bt_engine_set_option(h, L.OPT_WS_GUARD, 0))
                    plain, n0 = regions(L, h, B, T, prec), lib.bt_workspace_bytes(h, B, T, prec)
                    L.check(lib.bt_engine_set_option(h, L.OPT_WS_GUARD, g))
                    L.check(lib.bt_engine_get_option(h, L.OPT_WS_GUARD, C.byref(v)))
                    assert v.value == g
                    r, n1 = regions(L, h, B, T, prec), lib.bt_workspace_bytes(h, B, T, prec)
                    assert [e - b for b, e in r] == [e - b for b, e in plain]
                    assert n1 == n0 + g * len(r)
                    for (b0, e0), (b1, _) in zip(r, r[1:]):
                        assert b1 - (e0 + 255) // 256 * 256 == g
                    assert n1 - (r[-1][1] + 255) // 256 * 256 == g
            plan = L.A2BPlan()
            L.check(lib.bt_audio2beats_plan(h, 22050 * 40, 1, 1, 3, C.byref(plan)))
            assert plan.forward_bytes == lib.bt_workspace_bytes(h, plan.B, plan.T, 3)
        L.check(lib.bt_engine_set_option(h, L.OPT_WS_GUARD, 0))
        assert lib.bt_workspace_bytes(h, 11, 1500, 3) == sum((e - b + 255) // 256 * 256 for b, e in regions(L, h, 11, 1500, 3))
        assert lib.bt_workspace_regions(h, 0, 1500, 3, None, 0) == L.BT_ERR_ARG
        assert lib.bt_workspace_regions(h, 1, 1500, 2, None, 0) == L.BT_ERR_ARG
    finally:
        lib.bt_engine_destroy(h)
