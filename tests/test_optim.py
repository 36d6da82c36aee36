"""No-GPU checks of the optimiser step (csrc/optim.hip through its host twins, beat_this_amd/optim.py).

Yardstick of the AdamW arithmetic: the truth is an fp64 numpy AdamW over the same fp32 gradients; e_ref is the relative L2
distance of ``torch.optim.AdamW(foreach=False)`` on CPU fp32 from that truth, measured on p_final - p_initial; the twin has to
be within 2 e_ref.  (An elementwise fp32 restatement without FMA measures 0.99 .. 1.01 e_ref over 1 .. 100 steps in the four
regimes below, the last of which has a denormal v, eps dominating and e_ref = 3.5e-3; an error in a bias correction, the decay
or the placement of eps misses 2 e_ref by orders of magnitude.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT


def _L():
    from beat_this_amd import _lib as L

    L.build()
    return L


def _optim():
    _L()
    from beat_this_amd import optim

    return optim


CHUNK = 4096   # (checked against the library in test_header_exports_and_struct_sizes)
SIZES = [1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]
DEFAULTS = dict(lr=8e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)


class HostProblem:
    """parameters as separate numpy arrays, the flat buffers and the planner's tables"""

    def __init__(self, sizes, groups, n_groups, seed=0, p_scale=0.05):
        O = _optim()
        rng = np.random.default_rng(seed)
        self.params = [(rng.standard_normal(n) * p_scale).astype(np.float32) for n in sizes]
        self.groups = list(groups)
        self.tensors, self.chunks, self.total, self.n_chunks = O.plan([p.ctypes.data for p in self.params], sizes, groups, n_groups)
        self.offsets = [int(self.tensors[i].offset) for i in range(len(sizes))]
        self.grad, self.m, self.v = (np.zeros(self.total, np.float32) for _ in range(3))

    def set_grads(self, grads):
        self.grad[:] = 0
        for o, g in zip(self.offsets, grads):
            self.grad[o:o + g.size] = g

    def step(self, group_settings, t, grad_scale=1.0, coef=None, zero=True):
        O = _optim()
        O.adamw_step_host(self.tensors, len(self.params), self.chunks, self.n_chunks, self.grad, self.m, self.v,
                          O.hyper(group_settings, t, grad_scale, zero), coef)

    def moment(self, buf, i):
        return buf[self.offsets[i]:self.offsets[i] + self.params[i].size]


def adamw64(p0, grads, settings, grad_scale=1.0):
    """fp64 AdamW (torch.optim.AdamW's defaults) over the fp32 gradients of every step -> (p, m, v)"""
    lr, (b1, b2), eps, wd = settings["lr"], settings["betas"], settings["eps"], settings["weight_decay"]
    p = p0.astype(np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for t, g32 in enumerate(grads, 1):
        g = g32.astype(np.float64) * grad_scale
        p = p * (1 - lr * wd)
        m = m + (g - m) * (1 - b1)
        v = v * b2 + g * g * (1 - b2)
        p = p - lr / (1 - b1 ** t) * (m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps))
    return p, m, v


def torch_adamw32(p0, grads, settings):
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.AdamW([p], foreach=False, **settings)
    for g in grads:
        p.grad = torch.from_numpy(g.copy())
        opt.step()
    return p.detach().numpy()


def rel(a, truth):
    return float(np.linalg.norm(a.astype(np.float64) - truth) / np.linalg.norm(truth))


REGIMES = {"typical": (dict(DEFAULTS), 1e-3), "no_decay_unit_grads": (dict(DEFAULTS, weight_decay=0.0), 1.0),
           "small_lr_tiny_grads": (dict(DEFAULTS, lr=1e-5), 1e-6), "denormal_v": (dict(DEFAULTS), 1e-22)}


@pytest.mark.parametrize("steps", [3, 20])
@pytest.mark.parametrize("regime", list(REGIMES))
def test_twin_against_the_fp64_yardstick(regime, steps):
    settings, g_scale = REGIMES[regime]
    n = CHUNK + 1000
    hp = HostProblem([n], [0], 1, seed=1)
    p0 = hp.params[0].copy()
    rng = np.random.default_rng(2)
    grads = [(rng.standard_normal(n) * g_scale).astype(np.float32) for _ in range(steps)]
    for t, g in enumerate(grads, 1):
        hp.set_grads([g])
        hp.step([settings], t)
        assert not hp.grad.any()   # (the consumed gradients are cleared)
    truth, m64, v64 = adamw64(p0, grads, settings)
    d64 = truth - p0.astype(np.float64)
    e_ref = rel(torch_adamw32(p0, grads, settings).astype(np.float64) - p0.astype(np.float64), d64)
    e_twin = rel(hp.params[0].astype(np.float64) - p0.astype(np.float64), d64)
    print(f"{regime}, {steps} steps: e_ref {e_ref:.3e}, twin {e_twin:.3e} = {e_twin / e_ref:.3f} e_ref")
    assert e_twin <= 2 * e_ref, (e_twin, e_ref)
    assert rel(hp.m[:n], m64) < 1e-5
    if regime != "denormal_v":   # (there v holds a few denormal bits)
        assert rel(hp.v[:n], v64) < 1e-5


def test_zero_gradients_only_decay():
    hp = HostProblem([CHUNK + 5, 7], [0, 1], 2, seed=3)
    p0 = [p.copy() for p in hp.params]
    groups = [dict(DEFAULTS), dict(DEFAULTS, weight_decay=0.0)]
    for t in (1, 2, 3):
        hp.step(groups, t)
    assert not hp.m.any() and not hp.v.any() and not hp.grad.any()
    decay = np.float32(1.0 - DEFAULTS["lr"] * DEFAULTS["weight_decay"])
    want = p0[0]
    for _ in range(3):
        want = want * decay
    assert np.array_equal(hp.params[0], want)
    assert np.array_equal(hp.params[1], p0[1])


def test_two_groups_grad_scale_and_coef():
    sizes = [CHUNK + 3, 50, 5]
    groups = [dict(DEFAULTS), dict(DEFAULTS, lr=2e-4, weight_decay=0.0)]
    rng = np.random.default_rng(4)
    grads = [[(rng.standard_normal(n) * 1e-2).astype(np.float32) for n in sizes] for _ in range(3)]
    assign = [0, 1, 0]
    # grad_scale 0.5; a coefficient of 0.25 on top; both at once equal one scale of 0.125 (powers of two commute exactly)
    runs = {}
    for name, gs, coef in (("scale", 0.5, None), ("coef", 1.0, 0.25), ("both", 0.5, 0.25), ("one", 0.125, None)):
        hp = HostProblem(sizes, assign, 2, seed=5)
        p0 = [p.copy() for p in hp.params]
        for t, g in enumerate(grads, 1):
            hp.set_grads(g)
            hp.step(groups, t, grad_scale=gs, coef=coef)
        runs[name] = hp
        eff = gs * (coef or 1.0)
        for i, n in enumerate(sizes):
            truth, _, _ = adamw64(p0[i], [g[i] for g in grads], groups[assign[i]], grad_scale=eff)
            d64 = truth - p0[i].astype(np.float64)
            scaled = [(g[i] * np.float32(eff)) for g in grads]   # (exact: a power of two)
            e_ref = rel(torch_adamw32(p0[i], scaled, groups[assign[i]]).astype(np.float64) - p0[i], d64)
            e_twin = rel(hp.params[i].astype(np.float64) - p0[i], d64)
            assert e_twin <= 2 * e_ref, (name, i, e_twin, e_ref)
    for i in range(len(sizes)):
        assert np.array_equal(runs["both"].params[i], runs["one"].params[i])
    assert not np.array_equal(runs["scale"].params[0], runs["coef"].params[0])
    # the groups really differ: tensor 1 under group 0's settings moves elsewhere
    hp = HostProblem(sizes, [0, 0, 0], 2, seed=5)
    for t, g in enumerate(grads, 1):
        hp.set_grads(g)
        hp.step(groups, t, grad_scale=0.5)
    assert np.array_equal(hp.params[0], runs["scale"].params[0]) and not np.array_equal(hp.params[1], runs["scale"].params[1])


def test_scalar_path_parameter_is_the_same_arithmetic():
    """a parameter at a 4-byte offset (a view) and the same values in an aligned array end with the same bits"""
    O = _optim()
    n = CHUNK + 6
    rng = np.random.default_rng(6)
    base = (rng.standard_normal(n + 1) * 0.05).astype(np.float32)
    view, own = base[1:], base[1:].copy()
    g = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    out = []
    for arr in (view, own):
        tensors, chunks, total, n_chunks = O.plan([arr.ctypes.data], [n], [0], 1)
        grad, m, v = (np.zeros(total, np.float32) for _ in range(3))
        grad[:n] = g
        O.adamw_step_host(tensors, 1, chunks, n_chunks, grad, m, v, O.hyper([DEFAULTS], 1))
        out.append(arr.copy())
    assert np.array_equal(out[0], out[1])


def test_grad_norm_host():
    O = _optim()
    rng = np.random.default_rng(7)
    for n in (4, 8, CHUNK - 4, CHUNK, CHUNK + 4, 3 * CHUNK + 8):
        g = (rng.standard_normal(n) * 0.3).astype(np.float32)
        truth = float(np.linalg.norm(g.astype(np.float64)))
        for scale in (1.0, 0.5):
            for max_norm in (truth * scale * 0.5, truth * scale * 2.0):
                norm, coef = O.grad_norm_host(g, max_norm, scale)
                assert abs(float(norm) - truth * scale) <= 1e-6 * truth * scale
                want = min(np.float32(1.0), np.float32(max_norm) / (norm + np.float32(1e-6)))   # clip_grad_norm_'s formula, fp32
                assert coef == np.float32(want), (n, max_norm, coef, want)
                assert (coef < 1) == (max_norm < truth * scale)
    t = torch.from_numpy(g.copy()).requires_grad_(True)
    t.grad = torch.from_numpy(g.copy())
    total = float(torch.nn.utils.clip_grad_norm_([t], max_norm=truth * 0.5))
    norm, coef = O.grad_norm_host(g, truth * 0.5)
    assert abs(total - float(norm)) <= 1e-6 * truth
    assert np.allclose(t.grad.numpy(), g * coef, rtol=1e-6, atol=0)
    # zeros: norm 0, nothing clipped; a non-finite gradient propagates as in torch
    norm, coef = O.grad_norm_host(np.zeros(8, np.float32), 1.0)
    assert norm == 0 and coef == 1
    bad = g.copy()
    bad[5] = np.nan
    norm, coef = O.grad_norm_host(bad, 1.0)
    assert np.isnan(norm) and np.isnan(coef)
    bad[5] = np.inf
    norm, coef = O.grad_norm_host(bad, 1.0)
    assert np.isinf(norm) and coef == 0


def test_planner_tables_cover_every_element_once():
    O = _optim()
    L = _L()
    assert CHUNK == L.OPTIM_CHUNK
    sizes = SIZES + [0, 64 * 192]
    bufs = [np.zeros(max(n, 1), np.float32) for n in sizes]
    groups = [i % 2 for i in range(len(sizes))]
    tensors, chunks, total, n_chunks = O.plan([b.ctypes.data for b in bufs], sizes, groups, 2)
    assert n_chunks == sum((n + CHUNK - 1) // CHUNK for n in sizes)
    flat = np.zeros(total, np.int32)
    seen = [np.zeros(n, np.int32) for n in sizes]
    end = 0
    for i, n in enumerate(sizes):
        t = tensors[i]
        assert t.offset % 4 == 0 and t.offset >= end and t.numel == n and t.group == groups[i] and t.param == (bufs[i].ctypes.data)
        assert t.offset - end < 4   # (no more padding than the alignment needs)
        end = t.offset + n
    assert total % 4 == 0 and 0 <= total - end < 4
    for c in range(n_chunks):
        i, k = chunks[c].tensor, chunks[c].chunk
        lo, hi = k * CHUNK, min(sizes[i], (k + 1) * CHUNK)
        assert 0 <= lo < hi
        seen[i][lo:hi] += 1
        flat[tensors[i].offset + lo:tensors[i].offset + hi] += 1
    assert all((s == 1).all() for s in seen)
    assert int(flat.sum()) == sum(sizes) and flat.max() == 1
    # and the twin writes exactly there: padding stays zero under a step with non-zero everything
    hp = HostProblem(SIZES, [0] * len(SIZES), 1, seed=8)
    hp.set_grads([np.full(n, 1e-3, np.float32) for n in SIZES])
    hp.step([DEFAULTS], 1, zero=False)
    covered = np.zeros(hp.total, bool)
    for o, n in zip(hp.offsets, SIZES):
        covered[o:o + n] = True
    assert hp.m[covered].all() and hp.v[covered].all() and hp.grad[covered].all()   # (zero=False keeps the gradients)
    assert not hp.m[~covered].any() and not hp.v[~covered].any() and not hp.grad[~covered].any()


def test_argument_errors():
    L = _L()
    O = _optim()
    lib = L.lib()
    ARG = L.BT_ERR_ARG
    buf = np.zeros(64, np.float32)
    ptrs = (C.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data + 128)
    numel = (C.c_int64 * 2)(8, 8)
    groups = (C.c_int32 * 2)(0, 1)
    tensors = (L.OptimTensor * 2)()
    total, n_chunks = C.c_int64(), C.c_int64()

    def plan(n=2, p=ptrs, ne=numel, g=groups, ng=2, t=tensors, tot=C.byref(total), nc=C.byref(n_chunks), chunks=None, cap=0):
        return lib.bt_optim_plan(n, p, ne, g, ng, t, tot, chunks, cap, nc)

    assert plan() == L.BT_OK and total.value == 16 and n_chunks.value == 2
    assert plan(p=None) == ARG and plan(ne=None) == ARG and plan(g=None) == ARG and plan(t=None) == ARG
    assert plan(tot=None) == ARG and plan(nc=None) == ARG
    assert plan(ne=(C.c_int64 * 2)(8, -1)) == ARG and b"numel" in lib.bt_last_error()
    assert plan(g=(C.c_int32 * 2)(0, 2)) == ARG and b"group" in lib.bt_last_error()
    assert plan(g=(C.c_int32 * 2)(-1, 0)) == ARG
    assert plan(ng=0) == ARG and plan(ng=L.OPTIM_MAX_GROUPS + 1) == ARG
    assert plan(p=(C.c_void_p * 2)(buf.ctypes.data, None)) == ARG and b"null" in lib.bt_last_error()
    assert plan(chunks=(L.OptimChunk * 1)(), cap=1) == ARG and b"chunk table" in lib.bt_last_error()
    with pytest.raises(ValueError):
        O.plan([buf.ctypes.data], [-3], [0], 1)

    # the device entry points refuse their arguments before anything is launched
    h = O.hyper([DEFAULTS, DEFAULTS], 1)
    a = buf.ctypes.data
    assert a % 16 == 0
    chunks = (L.OptimChunk * 2)()
    assert plan(chunks=chunks, cap=2) == L.BT_OK
    step = lambda *args: lib.bt_adamw_step(None, *args)
    good = [C.addressof(tensors), 2, C.addressof(chunks), 2, a, a, a, 16, C.byref(h), None]
    for i in (0, 2, 4, 5, 6, 8):
        bad = list(good)
        bad[i] = None
        assert step(*bad) == ARG, i
    for i in (4, 5, 6):
        bad = list(good)
        bad[i] = a + 4
        assert step(*bad) == ARG and b"16-byte" in lib.bt_last_error(), i
    bad_h = O.hyper([DEFAULTS], 1)
    bad_h.n_groups = 9
    assert step(*(good[:8] + [C.byref(bad_h), None])) == ARG
    assert step(*(good[:7] + [15, C.byref(h), None])) == ARG
    need = lib.bt_grad_norm_workspace_bytes(3 * L.OPTIM_NORM_SLICE + 4)
    assert need == 4 * 8 and lib.bt_grad_norm_workspace_bytes(-1) == 0
    norm = lambda *args: lib.bt_grad_norm(None, *args)
    n = 3 * L.OPTIM_NORM_SLICE + 4
    assert norm(a, n, 1.0, 1.0, a, need - 1, a) == ARG and b"workspace too small" in lib.bt_last_error()
    assert norm(None, n, 1.0, 1.0, a, need, a) == ARG and norm(a, n, 1.0, 1.0, None, need, a) == ARG
    assert norm(a, n, 1.0, 1.0, a, need, None) == ARG
    assert norm(a + 4, n, 1.0, 1.0, a, need, a) == ARG and norm(a, -4, 1.0, 1.0, a, need, a) == ARG
    assert norm(a, 6, 1.0, 1.0, a, need, a) == ARG
    # the twins
    rec = np.zeros(2, np.float32)
    assert lib.bt_grad_norm_host(None, 8, 1.0, 1.0, rec.ctypes.data) == ARG
    assert lib.bt_grad_norm_host(a, 8, 1.0, 1.0, None) == ARG and lib.bt_grad_norm_host(a, -4, 1.0, 1.0, rec.ctypes.data) == ARG
    twin = lib.bt_adamw_step_host
    for i in (0, 2, 4, 5, 6, 8):
        bad = list(good)
        bad[i] = None
        assert twin(*bad) == ARG, i
    assert twin(*(good[:4] + [a + 4] + good[5:])) == ARG
    t_bad = (L.OptimTensor * 2)()
    C.memmove(t_bad, tensors, C.sizeof(t_bad))
    t_bad[1].group = 3
    assert twin(C.addressof(t_bad), *good[1:]) == ARG and b"group" in lib.bt_last_error()
    t_bad[1].group, t_bad[1].numel = 0, -1
    assert twin(C.addressof(t_bad), *good[1:]) == ARG
    t_bad[1].numel, t_bad[1].offset = 8, 12
    assert twin(C.addressof(t_bad), *good[1:]) == ARG   # (past the end of the flat buffers)
    c_bad = (L.OptimChunk * 2)()
    c_bad[1].tensor = 2
    assert twin(good[0], 2, C.addressof(c_bad), *good[3:]) == ARG
    one_group = O.hyper([DEFAULTS], 1)   # (the tables use group 1)
    assert twin(*(good[:8] + [C.byref(one_group), None])) == ARG and b"group" in lib.bt_last_error()
    assert twin(*good) == L.BT_OK


def test_cosine_warmup_scheduler():
    O = _optim()

    def factor(step, warmup, n, raise_to=0.5):
        if step < n:
            f = 0.5 * (1 + np.cos(np.pi * step / n))
            return f * step / warmup if step <= warmup else f
        return raise_to * min((step - n) / warmup, 1)

    for raise_last, raise_to in ((0, 0.5), (0.2, 0.5), (0.2, 0.25)):
        warmup, max_iters, base = 5, 40, [0.1, 0.02]
        n = int((1 - raise_last) * max_iters)
        ps = [torch.nn.Parameter(torch.zeros(2)), torch.nn.Parameter(torch.zeros(3))]
        opt = torch.optim.SGD([{"params": [ps[0]], "lr": base[0]}, {"params": [ps[1]], "lr": base[1]}], lr=1.0)
        sched = O.CosineWarmupScheduler(opt, warmup, max_iters, raise_last=raise_last, raise_to=raise_to)
        assert isinstance(sched, torch.optim.lr_scheduler.LRScheduler)
        got = []
        for step in range(max_iters + 10):
            got.append([g["lr"] for g in opt.param_groups])
            opt.step()
            sched.step()
        for step in (0, 1, warmup, warmup + 1, n - 1, n, n + 1, n + warmup, max_iters - 1, max_iters, max_iters + 5):
            want = [b * factor(step, warmup, n, raise_to) for b in base]
            assert np.allclose(got[step], want, rtol=1e-12, atol=1e-18), (raise_last, step, got[step], want)
        assert got[0] == [0.0, 0.0] and all(type(v) is float for v in got[3])
        if raise_last == 0:
            assert got[max_iters + 5] == [b * raise_to for b in base]       # beyond max_iters: raise_to of the base rate
            assert np.allclose(got[warmup], [b * 0.5 * (1 + np.cos(np.pi * warmup / n)) for b in base])
        state = sched.state_dict()
        assert state["last_epoch"] == max_iters + 10


def test_param_groups_for():
    O = _optim()
    net = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.LayerNorm(3), torch.nn.Conv1d(3, 2, 3), torch.nn.Linear(3, 1))
    net[3].weight.requires_grad_(False)
    net.register_parameter("scalar", torch.nn.Parameter(torch.zeros(())))
    groups = O.param_groups_for(net, 0.03)
    assert [g["weight_decay"] for g in groups] == [0.03, 0]
    decayed, plain = ({id(p) for p in g["params"]} for g in groups)
    assert decayed == {id(net[0].weight), id(net[2].weight)}
    assert plain == {id(net[0].bias), id(net[1].weight), id(net[1].bias), id(net[2].bias), id(net[3].bias), id(net.scalar)}
    opt = torch.optim.AdamW(groups, lr=1e-3)   # (usable as torch's param_groups)
    assert len(opt.param_groups) == 2


def test_header_exports_and_struct_sizes():
    L = _L()
    header = open(os.path.join(ROOT, "include", "beat_this_amd.h")).read()
    declared = set(re.findall(r"\b(bt_[a-z_0-9]+)\s*\(", header))
    new = {"bt_optim_struct_sizes", "bt_optim_plan", "bt_grad_norm_workspace_bytes", "bt_grad_norm", "bt_adamw_step",
           "bt_grad_norm_host", "bt_adamw_step_host"}
    assert new <= declared and new <= set(L.EXPORTS) and set(L.EXPORTS) == declared
    for name in new:
        assert hasattr(L.lib(), name)
    assert re.search(r"#define BT_ABI_VERSION 600\b", header) and L.lib().bt_version() == 600 == L.ABI_VERSION
    sizes = (C.c_int32 * 10)()
    L.lib().bt_optim_struct_sizes(sizes)
    assert list(sizes) == [C.sizeof(L.OptimTensor), C.sizeof(L.OptimChunk), C.sizeof(L.OptimGroup), C.sizeof(L.OptimHyper),
                           L.OptimTensor.offset.offset, L.OptimTensor.group.offset, L.OptimHyper.g.offset, L.OPTIM_CHUNK,
                           L.OPTIM_NORM_SLICE, L.OPTIM_MAX_GROUPS]
    for macro, value in (("BT_OPTIM_CHUNK", L.OPTIM_CHUNK), ("BT_OPTIM_NORM_SLICE", L.OPTIM_NORM_SLICE),
                         ("BT_OPTIM_MAX_GROUPS", L.OPTIM_MAX_GROUPS)):
        assert re.search(rf"#define {macro} {value}\b", header)
    assert 2048 <= L.OPTIM_CHUNK <= 8192 and L.OPTIM_MAX_GROUPS == 8
    assert "optim.hip" in L.SOURCES and "-ffp-contract=off" in L.FLAGS_BY_SOURCE["optim.hip"]


def test_optimizer_refuses_cpu_parameters():
    O = _optim()
    with pytest.raises(RuntimeError, match="ROCm GPUs only"):
        O.AdamW([torch.nn.Parameter(torch.zeros(4))])
