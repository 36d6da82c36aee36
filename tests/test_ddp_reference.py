"""No-GPU checks of data-parallel training: the host twin of the rank-ordered gradient sum against a
sequential numpy sum, its refusals, the ABI additions, the sharded loader on the synthetic data folder, fit's grouping
arithmetic and the command line's new switches."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dataset_reference as R
from conftest import ROOT
from ddp_util import bits, sequential_sum, spread_parts

WORLDS = (1, 2, 3, 8, 16)
SIZES = (0, 1, 3, 4, 4095, 4097)


def _lib():
    from beat_this_amd import _lib as L

    L.build()
    return L


@pytest.mark.parametrize("world", WORLDS)
def test_host_twin_equals_the_sequential_float32_sum(world):
    from beat_this_amd.parallel import grad_rank_sum_host

    _lib()
    differs = 0
    for n in SIZES:
        for stride in (n, n + 5, (n + 3) // 4 * 4 + 8):
            flat = spread_parts(world, n, stride, seed=1000 * world + n)
            want = sequential_sum(flat, world, n, stride)
            keep = flat.copy()
            got = grad_rank_sum_host(flat, world, n, stride)
            assert got.shape == (n,) and np.array_equal(bits(got), bits(want)), (world, n, stride)
            assert np.array_equal(bits(flat), bits(keep))   # (the parts are only read)
            if world > 2 and n >= 4095:
                differs += int((bits(sequential_sum(flat, world, n, stride, list(range(world))[::-1])) != bits(want)).sum())
    if world > 2:   # the data makes the order matter: the reversed-rank sum has other bits somewhere
        assert differs > 0


def test_the_order_of_the_ranks_matters_in_these_data():
    """the premise of the comparisons above, on its own: with three or more ranks the reversed-rank sum differs in at least one
    element (two ranks commute)"""
    for world in (3, 8, 16):
        flat = spread_parts(world, 4097, 4097, seed=1000 * world + 4097)
        a = sequential_sum(flat, world, 4097, 4097)
        b = sequential_sum(flat, world, 4097, 4097, list(range(world))[::-1])
        assert (bits(a) != bits(b)).any(), world


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_a_non_finite_gradient_of_one_rank_reaches_the_sum(bad):
    from beat_this_amd.parallel import grad_rank_sum_host

    _lib()
    for world, where in ((2, 0), (3, 1), (8, 7)):
        n = 9
        flat = spread_parts(world, n, n, seed=5)
        flat[where * n + 4] = bad
        got = grad_rank_sum_host(flat, world, n)
        assert np.isnan(got[4]) if np.isnan(bad) else got[4] == bad
        assert np.isfinite(np.delete(got, 4)).all()
    two = np.array([np.inf, -np.inf], np.float32)   # inf - inf: a NaN, which the loss scaler's skip rule sees as well
    assert np.isnan(grad_rank_sum_host(two, 2, 1)[0])


def test_in_place_over_rank_zero_and_the_refusals():
    from beat_this_amd.parallel import grad_rank_sum_host

    L = _lib()
    fn = L.lib().bt_grad_rank_sum_host
    for world, n, stride in ((1, 7, 7), (2, 4097, 4100), (3, 10, 11), (16, 4095, 4095)):
        flat = spread_parts(world, n, stride, seed=77)
        want = grad_rank_sum_host(flat, world, n, stride)
        work = flat.copy()
        assert grad_rank_sum_host(work, world, n, stride, out=work) is work
        assert np.array_equal(bits(work[:n]), bits(want)) and np.array_equal(bits(work[n:]), bits(flat[n:]))
    a, out = np.ones(64, np.float32), np.zeros(64, np.float32)
    ok = lambda *args: fn(*args) == L.BT_OK
    refused = lambda *args: fn(*args) == L.BT_ERR_ARG
    assert ok(a.ctypes.data, 16, 4, 16, out.ctypes.data) and out[:16].tolist() == [4.0] * 16
    assert ok(a.ctypes.data, 4, L.REDUCE_MAX_WORLD, 4, out.ctypes.data) and out[:4].tolist() == [16.0] * 4
    assert refused(a.ctypes.data, 16, 0, 16, out.ctypes.data)
    assert refused(a.ctypes.data, 1, L.REDUCE_MAX_WORLD + 1, 1, out.ctypes.data)
    assert refused(a.ctypes.data, 16, 2, -1, out.ctypes.data)
    assert refused(a.ctypes.data, 15, 2, 16, out.ctypes.data)          # stride < n, world > 1
    assert ok(a.ctypes.data, 0, 1, 16, out.ctypes.data)                # (world 1: the stride plays no part)
    assert refused(None, 16, 2, 16, out.ctypes.data) and refused(a.ctypes.data, 16, 2, 16, None)
    assert refused(a.ctypes.data, 16, 2, 16, a.ctypes.data + 4)        # overlaps rank 0's part, but is not it
    assert refused(a.ctypes.data, 16, 2, 16, a.ctypes.data + 4 * 16)   # rank 1's part
    assert refused(a.ctypes.data, 16, 2, 16, a.ctypes.data + 4 * 31)   # the last element of the parts
    assert ok(a.ctypes.data, 16, 2, 16, a.ctypes.data + 4 * 32)        # right behind them
    assert ok(a.ctypes.data, 16, 2, 0, out.ctypes.data)                # n = 0: nothing to do
    with pytest.raises(ValueError, match="bt_grad_rank_sum_host"):
        L.check(fn(a.ctypes.data, 16, 0, 16, out.ctypes.data))
    # the device entry point refuses the same arguments before it touches a GPU
    dfn = L.lib().bt_grad_rank_sum
    assert dfn(None, a.ctypes.data, 16, 0, 16, out.ctypes.data) == L.BT_ERR_ARG
    assert dfn(None, a.ctypes.data, 15, 2, 16, out.ctypes.data) == L.BT_ERR_ARG
    assert dfn(None, None, 16, 2, 16, out.ctypes.data) == L.BT_ERR_ARG
    assert dfn(None, a.ctypes.data, 16, 2, 16, a.ctypes.data + 4) == L.BT_ERR_ARG
    assert dfn(None, a.ctypes.data, 16, 2, 0, out.ctypes.data) == L.BT_OK   # n = 0 launches nothing


def test_header_binding_and_library_agree_on_the_additions():
    L = _lib()
    header = open(os.path.join(ROOT, "include", "beat_this_amd.h")).read()
    declared = set(re.findall(r"\b(bt_[a-z_0-9]+)\s*\(", header))
    new = {"bt_grad_rank_sum", "bt_grad_rank_sum_host"}
    assert new <= declared and new <= set(L.EXPORTS) and set(L.EXPORTS) == declared
    for name in new:
        assert hasattr(L.lib(), name)
    assert L.EXPORTS["bt_grad_rank_sum"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p])
    assert L.EXPORTS["bt_grad_rank_sum_host"] == (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p])
    defines = {k: int(v) for k, v in re.findall(r"^#define (BT_REDUCE_\w+) (\d+)\s*$", header, re.M)}
    assert defines == {"BT_REDUCE_MAX_WORLD": L.REDUCE_MAX_WORLD, "BT_REDUCE_CHUNK": L.REDUCE_CHUNK} and L.REDUCE_MAX_WORLD == 16
    assert re.search(r"#define BT_ABI_VERSION 600\b", header) and L.lib().bt_version() == L.ABI_VERSION == 600
    assert "reduce.hip" in L.SOURCES and "-ffp-contract=off" in L.FLAGS_BY_SOURCE["reduce.hip"]
    assert L.FLAGS_BY_SOURCE["reduce.hip"] == L.FLAGS_BY_SOURCE["optim.hip"]


# ---- the sharded loader ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return R.build_data_folder(str(tmp_path_factory.mktemp("ddp_dataset")))


def _train_loader(folder, batch_size):
    from beat_this_amd.dataset import BeatDataModule

    dm = BeatDataModule(folder, batch_size=batch_size, train_length=R.TRAIN_LENGTH, spect_fps=R.FPS,
                        augmentations={"tempo": R.TEMPO, "pitch": R.PITCH, "mask": R.MASK_SHORT}, device="cpu")
    dm.setup("fit")
    return dm.train_dataloader()


def _plain(planned):
    """a batch's plan as plain data: (member path, start, frames, mask ops, tempo percentage) per item"""
    return [(path, int(start), int(n), repr(ops), int(percentage)) for _, path, start, n, ops, percentage in planned]


def _state():
    kind, keys, pos, has_gauss, cached = np.random.get_state()
    return kind, keys.tolist(), pos, has_gauss, cached


@pytest.mark.parametrize("batch_size", [1, 2])
def test_the_shards_of_a_loader_are_the_unsharded_sequence(folder, batch_size):
    loader = _train_loader(folder, batch_size)
    n = len(loader)
    assert n == 5 // batch_size
    ds = loader.dataset
    # the unsharded sequence, as BatchLoader.__iter__ draws it: the permutation, then every batch's plan
    np.random.seed(11)
    order = np.random.permutation(len(ds))
    want = [_plain(ds.plan_batch(order[i * batch_size:(i + 1) * batch_size])) for i in range(n)]
    after = _state()
    assert len({repr(w) for w in want}) == n   # (random excerpts: the batches differ)
    for world in (1, 2, 3):
        union = {}
        for rank in range(world):
            np.random.seed(11)
            shard = loader.shard(rank, world)
            assert len(shard) == n and (shard.rank, shard.world) == (rank, world)
            seen = list(shard.iter_plans())
            assert _state() == after, (world, rank)   # numpy's generator is where the unsharded loader leaves it
            assert [j for j, _, _ in seen] == list(range(n)) and [o for _, o, _ in seen] == [j % world for j in range(n)]
            assert [_plain(p) for _, _, p in seen] == want   # (every rank draws every plan)
            for j, owner, planned in seen:
                if owner == rank:
                    assert j not in union
                    union[j] = _plain(planned)
        assert [union[j] for j in range(n)] == want, world
    # a second epoch goes on from the generator's state, as the unsharded loader's would
    second = [_plain(p) for _, _, p in loader.shard(1, 2).iter_plans()]
    assert second != want
    with pytest.raises(ValueError):
        loader.shard(2, 2)
    with pytest.raises(ValueError):
        loader.shard(0, 0)


def test_plan_batch_is_what_batch_draws(folder):
    """``plan_batch`` holds the draws of ``batch``: a batch built from a plan consumes nothing more (checked on the host: the
    plans of two consecutive calls equal the plans of one pass that draws item by item)"""
    loader = _train_loader(folder, 2)
    ds = loader.dataset
    np.random.seed(3)
    a = _plain(ds.plan_batch([0, 1])) + _plain(ds.plan_batch([2]))
    np.random.seed(3)
    b = _plain([ds._plan(i) for i in (0, 1, 2)])
    assert a == b


# ---- fit's grouping ----------------------------------------------------------------------------------------------------------------
def _restated_groups(batches, accumulate, world):
    """plain Python: walk the global batches, close a group after accumulate * world of them and at the end"""
    groups, first, count = [], 0, 0
    for j in range(batches):
        count += 1
        if count == accumulate * world:
            groups.append((first, count))
            first, count = j + 1, 0
    if count:
        groups.append((first, count))
    return groups


@pytest.mark.parametrize("batches,world,accumulate,want", [(5, 2, 1, [(0, 2), (2, 2), (4, 1)]), (5, 2, 2, [(0, 4), (4, 1)]),
                                                           (5, 3, 1, [(0, 3), (3, 2)])])
def test_step_groups_of_five_batches(batches, world, accumulate, want):
    import math

    from beat_this_amd.train import step_groups

    groups = step_groups(batches, accumulate, world)
    assert groups == want == _restated_groups(batches, accumulate, world)
    assert len(groups) == math.ceil(batches / (accumulate * world))   # steps_per_epoch
    assert sum(c for _, c in groups) == batches
    owners = [[j % world for j in range(first, first + count)] for first, count in groups]
    if (batches, world, accumulate) == (5, 2, 1):
        assert owners[-1] == [0]        # the remainder: rank 1 owns nothing and still steps, with the global count 1
    if (batches, world, accumulate) == (5, 2, 2):
        assert owners == [[0, 1, 0, 1], [0]]
    if (batches, world, accumulate) == (5, 3, 1):
        assert owners[-1] == [0, 1]     # rank 2 owns nothing of the remainder


def test_step_groups_in_general():
    from beat_this_amd.train import step_groups

    for batches in range(0, 14):
        for world in (1, 2, 3, 4):
            for accumulate in (1, 2, 3):
                assert step_groups(batches, accumulate, world) == _restated_groups(batches, accumulate, world)
    assert step_groups(7, 2) == step_groups(7, 2, 1) == [(0, 2), (2, 2), (4, 2), (6, 1)]   # (a single process: fit's old arithmetic)
    with pytest.raises(ValueError):
        step_groups(5, 0, 2)


def test_segment_length():
    from beat_this_amd.parallel import segment_length

    assert [segment_length(t, w) for t, w in ((16, 2), (17, 2), (18946658, 8), (4, 16), (0, 3))] == [8, 12, 2368336, 4, 0]
    for total in (1, 5, 4096, 18946658):
        for world in (1, 2, 3, 8, 16):
            per = segment_length(total, world)
            assert per % 4 == 0 and per * world >= total and (per - 4) * world < total + 4 * world


# ---- the command line ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,message", [(["--gpus", "0"], "--gpus"), (["--share-gpu"], "--share-gpu"),
                                           (["--gpus", "1", "--share-gpu"], "--share-gpu"), (["--gpus", "-2"], "--gpus")])
def test_the_new_switches_end_in_parser_errors(flags, message, capsys):
    from beat_this_amd import train

    with pytest.raises(SystemExit) as e:
        train.main(["--data-dir", "/nowhere/at/all", "--output", "/nowhere/at/all/o"] + flags)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "error:" in err and message in err


def test_the_parser_knows_gpus_and_defaults_to_one():
    from beat_this_amd.train import get_parser

    args = get_parser().parse_args(["--data-dir", "d", "--output", "o"])
    assert args.gpus == 1 and args.share_gpu is False
    args = get_parser().parse_args(["--data-dir", "d", "--output", "o", "--gpus", "8", "--share-gpu"])
    assert args.gpus == 8 and args.share_gpu is True
