"""The rank-ordered gradient sum on the device (csrc/reduce.hip), in one process: bt_grad_rank_sum against
its host twin bit for bit through the C ABI on guarded, poisoned buffers, and ``AdamW(process_group=...)`` on an RCCL group
of one rank against the optimiser without a group."""
import os
import socket

import numpy as np
import pytest
import torch

import route_harness as H
from gpu_util import POISONS, Guarded, assert_intact, dev
from ddp_util import bits, spread_parts

pytestmark = pytest.mark.gpu

WORLDS = (1, 2, 3, 8, 16)
SIZES = (1, 3, 4, 4095, 4096, 4097, 3 * 4096 + 5)


def layouts(n):
    """(name, stride, element offset of d_parts, in place): a 16-byte aligned stride, an odd one and a pointer that is only 4-byte
    aligned (both take the one-element-per-lane path), and the sum in place over rank 0's part on the wide and the narrow path"""
    aligned, odd = (n + 3) // 4 * 4 + 8, (n | 1) + 2
    return (("aligned", aligned, 0, False), ("odd stride", odd, 0, False), ("offset pointer", aligned, 1, False),
            ("in place", aligned, 0, True), ("in place, odd stride", odd, 0, True), ("packed", n, 0, False))


def host_sum(flat, world, n, stride):
    """the host twin's result, computed once per (data, layout) and shared by both poisons"""
    from beat_this_amd.parallel import grad_rank_sum_host

    return grad_rank_sum_host(flat, world, n, stride)


@pytest.mark.parametrize("world", WORLDS)
def test_device_equals_the_host_twin_bit_for_bit(world):
    from beat_this_amd import _lib as L

    lib, d = L.lib(), dev()
    for n in SIZES:
        for name, stride, offset, in_place in layouts(n):
            size = (world - 1) * stride + n
            flat = spread_parts(world, n, stride, seed=31 * world + n)
            want = host_sum(flat, world, n, stride)
            assert np.isfinite(want).all()
            for poison in POISONS:
                parts = Guarded((offset + size,), torch.float32).fill(poison)
                parts.t[offset:].copy_(torch.from_numpy(flat))
                # (the gaps between the parts keep spread_parts' 7e37: a sum that read them would overflow or show it)
                before = parts.t.clone()
                out = parts if in_place else Guarded((offset + n,), torch.float32).fill(poison)
                rc = lib.bt_grad_rank_sum(L.stream_ptr(d), parts.ptr() + 4 * offset, stride, world, n, out.ptr() + 4 * offset)
                L.check(rc)
                torch.cuda.synchronize()
                what = (world, n, name, hex(poison))
                assert_intact((f"parts {what}", parts), (f"out {what}", out))
                got = out.t[offset:offset + n].cpu().numpy()
                assert np.array_equal(bits(got), bits(want)), what
                keep = slice(n, None) if in_place else slice(None)   # the parts are only read (rank 0's aside, in place)
                assert torch.equal(parts.t[offset:][keep].view(torch.int32), before[offset:][keep].view(torch.int32)), what
                assert bool((out.t[:offset].view(torch.uint8) == poison).all()), what   # (nothing in front of d_out is written)


def test_non_finite_values_propagate_and_the_refusals_launch_nothing():
    from beat_this_amd import _lib as L

    lib, d = L.lib(), dev()
    n, world = 4097, 3
    flat = spread_parts(world, n, n + 3, seed=9)
    flat[(n + 3) + 5], flat[2 * (n + 3) + 4096] = np.inf, np.nan
    want = host_sum(flat, world, n, n + 3)
    assert want[5] == np.inf and np.isnan(want[4096])
    parts = Guarded(flat.shape, torch.float32).fill(POISONS[0], data=torch.from_numpy(flat))
    out = Guarded((n,), torch.float32).fill(POISONS[0])
    L.check(lib.bt_grad_rank_sum(L.stream_ptr(d), parts.ptr(), n + 3, world, n, out.ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.t.cpu().numpy()), bits(want))
    # refused before any launch: the output stays poisoned
    out.fill(POISONS[1])
    for args in ((parts.ptr(), n + 3, 0, n, out.ptr()), (parts.ptr(), n + 3, 17, n, out.ptr()), (parts.ptr(), n - 1, 2, n, out.ptr()),
                 (parts.ptr(), n + 3, 2, -1, out.ptr()), (None, n + 3, 2, n, out.ptr()), (parts.ptr(), n + 3, 2, n, None),
                 (parts.ptr(), n + 3, 2, n, parts.ptr() + 4), (parts.ptr(), n + 3, 2, n, parts.ptr() + 4 * (n + 3))):
        assert lib.bt_grad_rank_sum(L.stream_ptr(d), *args) == L.BT_ERR_ARG, args
    assert lib.bt_grad_rank_sum(L.stream_ptr(d), parts.ptr(), n + 3, 2, 0, out.ptr()) == L.BT_OK
    torch.cuda.synchronize()
    assert bool((out.t.view(torch.uint8) == POISONS[1]).all())
    assert_intact(("parts", parts), ("out", out))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _three_steps(batch, max_grad_norm, **kw):
    """three clipped AdamW steps on the D = 64, 2-layer model of test_gpu_optim's real-gradient case -> what the run leaves"""
    from beat_this_amd import optim as OP

    hp = dict(transformer_dim=64, ff_mult=2, n_layers=2)
    m = H.make_model(hp, dict(H.state_dict(hp, 3, "lively")), freeze_freqs=True)
    opt = OP.AdamW(OP.param_groups_for(m, 0.01), lr=1e-3, max_grad_norm=max_grad_norm, **kw)
    norms = []
    for _ in range(3):
        H.model_loss(m, batch)[0].backward()
        opt.step()
        norms.append(opt.last_grad_norm())
    st = opt.flat_state()
    res = {"grad": st["grad"].clone(), "exp_avg": st["exp_avg"].clone(), "exp_avg_sq": st["exp_avg_sq"].clone()}
    res.update({n: p.detach().clone() for n, p in m.named_parameters() if p.requires_grad})
    return res, norms, opt


@pytest.mark.timeout(180)
def test_adamw_on_a_one_rank_rccl_group_has_the_bits_of_the_optimiser_without_a_group():
    import torch.distributed as dist

    batch = H.make_batch(2, 150, seed=61)
    _, free, _ = _three_steps(batch, 1e9)
    limit = 0.5 * free[0]   # (the first step clips, whatever the later ones do)
    want, norms, plain = _three_steps(batch, limit)
    assert any(n + 1e-6 > limit for n in norms) and plain._reducer is None
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(_free_port())
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev())
    try:
        got, got_norms, opt = _three_steps(batch, limit, process_group=dist.group.WORLD)
        ex = opt._reducer
        assert ex is not None and ex.world == 1 and ex.per % 4 == 0 and ex.per >= ex.total
        assert opt.flat_state()["grad"].data_ptr() == ex.store.data_ptr()   # (the gradient buffer heads the exchange's store)
        assert not bool(ex.store[ex.total:].any())                            # the tail padding stays zero
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    assert got_norms == norms
    assert set(got) == set(want) and len(got) > 20
    for k in want:
        assert H.same_bits(got[k], want[k]), k
    assert not bool(got["grad"].any())   # (the step cleared what it consumed)


@pytest.mark.timeout(180)
def test_fit_on_a_one_rank_rccl_group_repeats_the_run_without_a_group(tmp_path):
    """the collectives on the device (no staging): ``fit(process_group=...)`` in a world of one -- the broadcast, the exchange, the
    gathered losses, the sharded validation, the fingerprint, the barrier -- leaves the bits of ``fit`` without a group, case B's
    settings (dropout, clipping, 16-mixed with a live loss scale, weight averaging)"""
    import torch.distributed as dist

    import ddp_worker as DW
    from dataset_reference import build_data_folder
    from test_gpu_ddp_fit import checkpoint, differences

    root = build_data_folder(str(tmp_path / "data"))
    outs = {name: str(tmp_path / name) for name in ("plain", "group")}
    for out in outs.values():
        os.makedirs(out)
    want, _ = DW.run_fit("B", root, outs["plain"])
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(_free_port())
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev())
    try:
        got, _ = DW.run_fit("B", root, outs["group"], process_group=dist.group.WORLD, staged=False)
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    assert want["global_step"] == 10 and [s["accumulated"] for s in want["steps"]] == [1] * 10
    diffs = differences(got, want, "result")
    assert not diffs, diffs[:8]
    for name in ("epoch0.ckpt", "run.ckpt"):
        diffs = differences(checkpoint(dict(out=outs["group"]), name), checkpoint(dict(out=outs["plain"]), name), name)
        assert not diffs, diffs[:8]
