"""The device side of the training route's GPU tests (test_gpu_backward, _dropout, _mixed, _train_formats, _bf16, _train_high,
_frontend_backward, _batch_stats, _front_mixed, _front_dropout, _train_route, _finetune*, _ema, _optim): random inputs, the bit
comparison, the run under both poison bytes, the model factory, the whole-model backward, one frontend unit and one trunk unit
through the C ABI on any operand format, the raw GEMM, the fit-and-resume run and the 16-mixed gate.  Where the tests' own copies
differed in strength, this is the strongest of them.  The comparisons work on CPU tensors too (tests/test_route_harness.py)."""
import ctypes as C

import numpy as np
import torch

import route_grads as RG
from gpu_util import POISONS, Guarded, assert_intact, dev

MODEL_KEYS = ("spect_dim", "transformer_dim", "ff_mult", "n_layers", "head_dim", "stem_dim", "sum_head", "partial_transformers")
MIXED_GATE = 2.0
POISON_WORD = int.from_bytes(bytes([POISONS[1]] * 4), "little")
_CACHE = {}


def randn(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def same_bits(a, b):
    """the same shape, the same dtype and the same bytes, whatever the dtype"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().reshape(-1).view(torch.uint8),
                                                                     b.contiguous().reshape(-1).view(torch.uint8))


def _words(t):
    """the payload as 32-bit words (a trailing part of less than a word is left out)"""
    raw = t.contiguous().reshape(-1).view(torch.uint8)
    return raw[:raw.numel() // 4 * 4].view(torch.int32)


def both_poisons(name, run):
    """run(poison) under both poison bytes -> the first result.  A result is a dict of tensors or a tuple of such dicts.  The two
    runs have to be bit-identical; a float tensor has to be finite (0xFF is a NaN in every float format) and free of the 0x7B
    word; an integer tensor is compared exactly and may hold any value."""
    res = [run(p) for p in POISONS]
    parts = [r if isinstance(r, (tuple, list)) else (r,) for r in res]
    assert len(parts[0]) == len(parts[1]), name
    for first, second in zip(*parts):
        assert set(first) == set(second), f"{name}: the two runs return different tensors"
        for k in first:
            a, b = first[k], second[k]
            assert same_bits(a, b), f"{name}: {k} differs between two runs (or depends on the poison)"
            if a.is_floating_point():
                assert torch.isfinite(a).all(), f"{name}: {k} keeps bytes of the 0xFF poison (or is not finite)"
                assert not (_words(b) == POISON_WORD).any(), f"{name}: {k} keeps words of the 0x7B poison"
    return res[0]


# ---- models -----------------------------------------------------------------------------------------------------------------------
def state_dict(hp, seed, style, counters=0):
    """``weights.random_state_dict`` of the resolved ``hp``, one object per configuration; ``counters``: added to every
    num_batches_tracked (an update that overwrites instead of blending shows)"""
    from beat_this_amd import weights as W

    key = ("sd", tuple(sorted(hp.items())), seed, style, counters)
    if key not in _CACHE:
        sd = W.random_state_dict(W.resolve_hparams(hp), seed=seed, style=style)
        for k in sd:
            if counters and k.endswith("num_batches_tracked"):
                sd[k] = sd[k] + counters
        _CACHE[key] = sd
    return _CACHE[key]


def make_model(hp, sd, *, frontend=False, trunk=True, freeze_freqs=False, dropout=None, cache=None):
    """``BeatThis(hp)`` with the weights ``sd`` on the GPU, the trunk and the heads trainable (``trunk``); ``frontend``: the frontend
    too, behind its opt-in; ``freeze_freqs``: the rotary tables stay fixed; ``dropout``: the constructor's rates.  ``cache``: None = a model of
    the caller's own, else a hashable key under which the tests that leave its state as they found it share one model."""
    from beat_this_amd import weights as W
    from beat_this_amd.model import BeatThis

    if cache is not None and ("model", cache) in _CACHE:
        return _CACHE["model", cache]
    hp = W.resolve_hparams(hp)
    m = BeatThis(**{k: hp[k] for k in MODEL_KEYS}, **({} if dropout is None else {"dropout": dropout}))
    m.load_state_dict(sd)
    m = m.to(dev())
    if frontend:
        m.set_frontend_trainable()
    if trunk:
        m.transformer_blocks.requires_grad_(True)
        m.task_heads.requires_grad_(True)
    if freeze_freqs:
        for n, p in m.named_parameters():
            if n.endswith("rotary_embed.freqs"):
                p.requires_grad_(False)
    if cache is not None:
        _CACHE["model", cache] = m
    return m


def make_batch(B, T, seed):
    """the device entries of a ``ds.batch(...)`` result"""
    gen = torch.Generator().manual_seed(seed)
    spect = torch.log1p(torch.rand(B, T, 128, generator=gen) * 30)
    beat = torch.rand(B, T, generator=gen) < 0.06
    down = beat & (torch.rand(B, T, generator=gen) < 0.3)
    mask = torch.ones(B, T, dtype=torch.bool)
    mask[-1, T - 20:] = False
    d = dev()
    return dict(spect=spect.to(d), truth_beat=beat.to(d), truth_downbeat=down.to(d), padding_mask=mask.to(d))


# ---- the whole model's backward ---------------------------------------------------------------------------------------------------
def weighted_backward(m, x, g_b, g_d):
    """gradients of sum(beat g_b) + sum(downbeat g_d) -> (gradients by name and "x", beat, downbeat, the buffers after the call)"""
    m.zero_grad(set_to_none=True)
    xd = x.to(dev()).requires_grad_(True)
    out = m(xd)
    (out["beat"] * g_b.to(dev())).sum().add((out["downbeat"] * g_d.to(dev())).sum()).backward()
    got = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    got["x"] = xd.grad.clone()
    m.zero_grad(set_to_none=True)
    return got, out["beat"].detach(), out["downbeat"].detach(), {n: b.detach().clone() for n, b in m.named_buffers()}


def loss_backward(forward, m, x, beat, down, mask, scale=1.0):
    """gradients of the shift-tolerant loss of ``forward(x on the device)`` = {"beat", "downbeat"}, taken of loss * scale and
    divided by scale -> {<parameter name>, "x", "beat", "downbeat"}"""
    from beat_this_amd.model.loss import ShiftTolerantBCELoss

    m.zero_grad(set_to_none=True)
    xd = x.to(dev()).requires_grad_(True)
    out = forward(xd)
    fn = ShiftTolerantBCELoss().to(dev())
    loss = fn(out["beat"], beat.to(dev()), mask.to(dev()).bool()) + fn(out["downbeat"], down.to(dev()), mask.to(dev()).bool())
    (loss * scale).backward()
    res = {n: p.grad / scale for n, p in m.named_parameters() if p.grad is not None}
    res.update(x=xd.grad / scale, beat=out["beat"].detach(), downbeat=out["downbeat"].detach())
    m.zero_grad(set_to_none=True)
    return res


def model_device(m, x, beat, down, mask, scale=1.0):
    return loss_backward(m, m, x, beat, down, mask, scale)


# ---- one frontend unit through the C ABI ----------------------------------------------------------------------------------------------
def abi_front_unit(sd, unit, dims, B, T, x, gy, poison, operand=None, batch=False, *, mixed=None):
    """Forward + backward of one frontend unit through bt_front_* (running statistics) or, with ``batch``, bt_front_bn_* (batch
    statistics).  ``operand``: None = fp32, else a format name of _lib.OPERAND_FORMATS: the struct's ``mixed`` and ``operand`` and
    the workspace query follow from it (``mixed`` = False beside a format: the call that has to ignore its operand).
    unit, dims: "stem", None; "conv", (key prefix, F, C); "linear", (F, C, dim); "swap", (F, C).
    Every input, parameter, running buffer, saved tensor, output, gradient and the workspaces are ``Guarded`` buffers filled with
    ``poison``; their bands are checked once, after the backward.
    -> {"y", "save_pre" (conv), "x" (= gx), <state dict key>: gradient}; with ``batch`` a pair of that and {<key>: running
    buffer after the forward} (the backward must leave them alone)."""
    from beat_this_amd import _lib as L

    d, keep, bias = dev(), [], None
    if unit == "stem":
        code, F_, C_, dim, xs, ys = L.FRONT_STEM, 128, 32, 0, (B, T, 128), (B, T, 32, 32)
        wkey, bns = "frontend.stem.conv2d.weight", {"bn1": "frontend.stem.bn1d.", "bn": "frontend.stem.bn2d."}
    elif unit == "conv":
        p, F_, C_ = dims
        code, dim, xs, ys = L.FRONT_CONV, 0, (B, T, F_, C_), (B, T, F_ // 2, 2 * C_)
        wkey, bns = p + "conv2d.weight", {"bn": p + "norm."}
    elif unit == "linear":
        F_, C_, dim = dims
        code, xs, ys = L.FRONT_LINEAR, (B, T, F_, C_), (B, T, dim)
        wkey, bns, bias = "frontend.linear.weight", {}, "frontend.linear.bias"
    else:
        F_, C_ = dims
        code, dim, xs, ys, wkey, bns = L.FRONT_SWAP, 0, (B, T, F_, C_), (B, F_, T, C_), None, {}
    assert not batch or unit in ("stem", "conv")

    def guarded(shape, data=None, dtype=torch.float32):
        g = Guarded(shape, dtype).fill(poison, data=None if data is None else data.to(d))
        keep.append(g)
        return g

    a = L.FrontBnArgs(B=B, T=T, F=F_, C=C_) if batch else L.FrontArgs()
    if not batch:
        a.B, a.T, a.F, a.C, a.dim = B, T, F_, C_, dim
    mixed = operand is not None if mixed is None else mixed
    a.mixed = int(mixed)
    value, suffix = L.OPERAND_FORMATS[operand] if operand is not None else (0, "")
    a.operand = value
    a.x, a.gy = guarded(xs, x).ptr(), guarded(ys, gy).ptr()
    outs = {"y": guarded(ys), "x": guarded(xs)}
    a.y, a.gx = outs["y"].ptr(), outs["x"].ptr()
    if unit == "conv":
        outs["save_pre"] = guarded(ys)
        a.save_pre = outs["save_pre"].ptr()
    for field, key in (("w", wkey), ("b", bias)):
        if key is not None:
            setattr(a, field, guarded(sd[key].shape, sd[key]).ptr())
            outs[key] = guarded(sd[key].shape)
            setattr(a, "g_" + field, outs[key].ptr())
    stats = {}
    for f, p in bns.items():
        n = sd[p + "weight"].shape
        for leaf, field in (("weight", "_w"), ("bias", "_b")):
            setattr(a, f + field, guarded(n, sd[p + leaf]).ptr())
            outs[p + leaf] = guarded(n)
            setattr(a, f"g_{f}{field}", outs[p + leaf].ptr())
        stats[p + "running_mean"], stats[p + "running_var"] = guarded(n, sd[p + "running_mean"]), guarded(n, sd[p + "running_var"])
        setattr(a, f + "_mean", stats[p + "running_mean"].ptr())
        setattr(a, f + "_var", stats[p + "running_var"].ptr())
        if batch:
            stats[p + "num_batches_tracked"] = guarded((1,), sd[p + "num_batches_tracked"].reshape(1), torch.int64)
            setattr(a, f + "_tracked", stats[p + "num_batches_tracked"].ptr())
            save = "save1" if f == "bn1" else "save"
            setattr(a, save + "_mean", guarded(n).ptr())
            setattr(a, save + "_rstd", guarded(n).ptr())
    lib, family = L.lib(), "bt_front_bn" if batch else "bt_front"
    size = lambda query, backward: query(code, backward, B, T, F_, C_, *(() if batch else (dim,)))
    query = getattr(lib, f"{family}_workspace_bytes{suffix if mixed else ''}")
    plain = lib.bt_front_workspace_bytes if mixed and not batch else None
    calls = (getattr(lib, family + "_forward"), getattr(lib, family + "_backward"))
    after = None
    for backward, fn in enumerate(calls):
        n = size(query, backward)
        assert n > 0 and (plain is None or n >= size(plain, backward))
        ws = guarded((n,), dtype=torch.uint8)
        a.ws, a.ws_bytes = ws.ptr(), n
        L.check(fn(L.stream_ptr(d), code, C.byref(a)))
        torch.cuda.synchronize()
        if batch and not backward:
            after = {k: g.t.clone().reshape(sd[k].shape) for k, g in stats.items()}
    for k in after or ():
        assert same_bits(stats[k].t.reshape(sd[k].shape), after[k]), f"{unit}: the backward touched {k}"
    assert_intact(*[(f"{unit} buffer {i}", g) for i, g in enumerate(keep)])
    res = {k: g.t.clone() for k, g in outs.items()}
    return (res, after) if batch else res


# ---- one unit of the trunk through the C ABI ----------------------------------------------------------------------------------------
FIELDS = dict(attn=dict(gamma="norm.gamma", w1="to_qkv.weight", w2="to_gates.weight", b2="to_gates.bias", w3="to_out.0.weight"),
              ff=dict(gamma="net.0.gamma", w1="net.1.weight", b1="net.1.bias", w2="net.4.weight", b2="net.4.bias"))


def unit_state_dict(D, ff_mult=2):
    """the ``lively`` weights of a 2-layer trunk of width D and hidden width ff_mult D (a state dict only: the engine's frontend
    cannot be built at D = 96, ff_mult 2, and the unit calls need nothing of it but the rotary table, which does not depend on the
    width)"""
    return state_dict(dict(transformer_dim=D, ff_mult=ff_mult, n_layers=2), 3, "lively")


class Plain:
    def __init__(self, shape, dtype, data=None):
        self.t = torch.empty(shape, dtype=dtype, device=dev()) if data is None else data.to(dev(), dtype).contiguous()

    def ptr(self):
        return self.t.data_ptr()


class Unit:
    """The operands of one attention / feed-forward call (layer 1 of unit_state_dict), optionally in guarded buffers filled
    with ``poison``; ``run`` does the forward and the backward and returns the outputs by state-dict key"""

    def __init__(self, kind, D, x, gy, residual, poison=None, ff_mult=2):
        from beat_this_amd import _lib as L

        self.L, self.kind, self.poison, self.keep = L, kind, poison, []
        hp = dict(transformer_dim=64, ff_mult=2, n_layers=2)   # (the model that lends its rotary table: test_gpu_dropout's D = 64 one)
        m, sd = make_model(hp, state_dict(hp, 3, "lively"), cache=("dropout", 64, 2, 3)), unit_state_dict(D, ff_mult)
        self.sd, self.pfx = sd, f"transformer_blocks.layers.1.{0 if kind == 'attn' else 1}."
        self.unit = L.UNIT_ATTN if kind == "attn" else L.UNIT_FF
        Bn, T = x.shape[:2]
        self.shape, self.hidden = (Bn, T, D), ff_mult * D
        eng = m.engine()
        eng.ensure_positions(T)
        self.rope = eng.packed._rope_t
        a = self.a = L.TrainArgs()
        a.B, a.T, a.dim, a.hidden, a.rope_len, a.residual = Bn, T, D, self.hidden, eng.packed.desc.rope_len, int(residual)
        a.rope = self.rope.data_ptr()
        self.x, self.gy = self.buf((Bn, T, D), x), self.buf((Bn, T, D), gy)
        a.x, a.gy = self.x.ptr(), self.gy.ptr()
        self.params = {f: self.buf(sd[self.pfx + n].shape, sd[self.pfx + n]) for f, n in FIELDS[kind].items()}
        self.outs = {"y": self.buf((Bn, T, D))}
        if kind == "attn":
            self.outs["save_o"], self.outs["save_lse"] = self.buf((Bn, T, D)), self.buf((Bn, T, D // 32))
        self.grads = {"gx": self.buf((Bn, T, D))}
        for f, g in self.params.items():
            self.grads["g_" + f] = self.buf(g.t.shape)
        for f, g in list(self.params.items()) + list(self.outs.items()) + list(self.grads.items()):
            setattr(a, f, g.ptr())

    def buf(self, shape, data=None, dtype=torch.float32):
        if self.poison is None:
            b = Plain(shape, dtype, data)
        else:
            b = Guarded(shape, dtype).fill(self.poison, data=None if data is None else data.to(dev()))
        self.keep.append(b)
        return b

    def ws_bytes(self, backward, drop):
        lib = self.L.lib()
        query = lib.bt_train_workspace_bytes_dropout if drop is not None and drop[0] > 0 else lib.bt_train_workspace_bytes
        return query(self.unit, backward, *self.shape, self.hidden)

    def call(self, backward, drop, entry, ws_bytes=None):
        """one entry point -> its return code.  entry "plain": bt_train_forward / _backward (drop must be None); "dropout": the
        *_dropout ones with NULL (drop None) or (p, seed, stream)"""
        L, lib = self.L, self.L.lib()
        n = self.ws_bytes(backward, drop) if ws_bytes is None else ws_bytes
        ws = self.buf((max(n, 1),), dtype=torch.uint8)
        self.a.ws, self.a.ws_bytes = ws.ptr(), n
        if entry == "plain":
            assert drop is None
            return (lib.bt_train_backward if backward else lib.bt_train_forward)(L.stream_ptr(dev()), self.unit, C.byref(self.a))
        d = None if drop is None else C.byref(L.TrainDropout(p=drop[0], seed=drop[1], stream=drop[2]))
        fn = lib.bt_train_backward_dropout if backward else lib.bt_train_forward_dropout
        return fn(L.stream_ptr(dev()), self.unit, C.byref(self.a), d)

    def run(self, drop, entry="dropout"):
        for backward in (0, 1):
            self.L.check(self.call(backward, drop, entry))
        torch.cuda.synchronize()
        if self.poison is not None:
            assert_intact(*[(f"{self.kind} buffer {i}", g) for i, g in enumerate(self.keep)])
        res = {"y": self.outs["y"].t.clone(), "x": self.grads["gx"].t.clone()}
        for f, n in FIELDS[self.kind].items():
            res[self.pfx + n] = self.grads["g_" + f].t.clone()
        for k in ("save_o", "save_lse"):
            if k in self.outs:
                res[k] = self.outs[k].t.clone()
        return res


class MixedUnit(Unit):
    """Unit on the *_mixed entry points (drop: None or (p, seed, stream)); ``operand``: a format name of _lib.OPERAND_FORMATS for
    bt_train_args.operand, None leaves the field as the struct is born (0: fp16)"""

    def __init__(self, *args, operand=None, **kw):
        super().__init__(*args, **kw)
        if operand is not None:
            self.a.operand = self.L.OPERAND_FORMATS[operand][0]

    def ws_bytes(self, backward, drop):
        return self.L.lib().bt_train_workspace_bytes_mixed(self.unit, backward, *self.shape, self.hidden, int(drop is not None))

    def call(self, backward, drop, entry="mixed", ws_bytes=None):
        L, lib = self.L, self.L.lib()
        n = self.ws_bytes(backward, drop) if ws_bytes is None else ws_bytes
        ws = self.buf((max(n, 1),), dtype=torch.uint8)
        self.a.ws, self.a.ws_bytes = ws.ptr(), n
        d = None if drop is None else C.byref(L.TrainDropout(p=drop[0], seed=drop[1], stream=drop[2]))
        fn = lib.bt_train_backward_mixed if backward else lib.bt_train_forward_mixed
        return fn(L.stream_ptr(dev()), self.unit, C.byref(self.a), d)


# ---- the raw GEMM on guarded buffers, and the shapes the exact-product tests walk -------------------------------------------------------
EDGES = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)   # the issue's sizes and the wave's 64-wide share of the 128-wide tile
KS = (1, 15, 16, 17, 33, 64, 100)


def guarded(arr, poison):
    t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32))
    return Guarded(t.shape, torch.float32).fill(poison, data=t.to(dev()))


def matmul(mixed, form, a, b, M, N, K, poison):
    """bt_train_matmul (``mixed``: 0, or 1 + BT_OPERAND_*) on guarded buffers (form 2 with its workspace) -> C as numpy"""
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


# ---- the frontend's shapes and the whole model of route_cases ------------------------------------------------------------------------------
def conv_dims(i):
    """conv unit i of the frontend -> (key prefix, F, C), the ``dims`` of abi_front_unit"""
    return f"frontend.blocks.{i}.", 32 >> i, 32 << i


def front_model(cache):
    """the D = 64 model of route_cases.model_state_dict on the GPU, everything trainable"""
    import route_cases as RC

    return make_model(RC.HP, RC.model_state_dict("lively", True), frontend=True, freeze_freqs=True, cache=cache)


def model_loss(m, batch, which=("beat", "downbeat")):
    from beat_this_amd.model.loss import ShiftTolerantBCELoss

    out = m(batch["spect"])
    fn = ShiftTolerantBCELoss().to(dev())
    return sum(fn(out[k], batch["truth_" + k].float(), batch["padding_mask"]) for k in which), out


# ---- what the tests of the operand formats share (test_gpu_train_formats, test_gpu_bf16, test_gpu_train_high) ---------------------------
def walk(form, seed0):
    """(M, N, K, seed) over the tile edges: three of the N per M, all of them over the M; form 2 also with the summed rows on both
    sides of a BT_TRAIN_DW_ROWS chunk"""
    n = 0
    for i, M in enumerate(EDGES):
        for j in range(3):
            N = EDGES[(i + 4 * j + form) % len(EDGES)]
            for K in KS:
                yield M, N, K, seed0 * form + n
                n += 1
    if form == 2:
        for K in (1023, 1024, 1025):
            yield 33, 129, K, K


def unit_run(kind, operand, poison=None, drop=None, rows=slice(None)):
    """the D = 64 unit with its residual on the (3, 130) inputs of the bit-identity tests (or ``rows`` of them), on ``operand``"""
    x, g = randn(3, 130, 64, seed=51), randn(3, 130, 64, seed=52)
    return MixedUnit(kind, 64, x[rows], g[rows], 1, poison=poison, operand=operand).run(drop)


def both_parts(m, precision, operand=None):
    """the trunk and the frontend of ``m`` on one precision (and operand)"""
    return m.set_train_precision(precision, operand).set_frontend_precision(precision, operand)


def switching():
    """two models of the same weights, one never switched; -> (never, switched, run, x, the fp32 and the fp16 16-mixed results)"""
    import route_cases as RC

    fresh = lambda: make_model(RC.HP, RC.model_state_dict("init0"), frontend=True, freeze_freqs=True)
    never, switched = fresh(), fresh()
    x, beat, down, mask = RC.model_inputs(2, 33, True)
    run = lambda m: model_device(m, x, beat, down, mask, 1024.0)
    want32 = run(never)
    want16 = run(both_parts(never, "16-mixed"))
    return never, switched, run, x, want32, want16


def inference_never_looks_at_the_switch(never, switched, x):
    with torch.no_grad():
        a, b = never(x.to(dev())), switched(x.to(dev()))
    assert same_bits(a["beat"], b["beat"]) and same_bits(a["downbeat"], b["downbeat"])


# ---- fit ------------------------------------------------------------------------------------------------------------------------------
LR, WARMUP, EPOCHS = 2e-3, 2, 2


def new_module():
    from beat_this_amd import weights as W
    from beat_this_amd.model.pl_module import PLBeatThis

    pl = PLBeatThis(transformer_dim=64, n_layers=2, ff_mult=2, lr=LR, warmup_steps=WARMUP, max_epochs=EPOCHS, eval_trim_beats=0)
    sd = W.random_state_dict(W.resolve_hparams(dict(transformer_dim=64, ff_mult=2, n_layers=2)), seed=3, style="lively")
    pl.load_state_dict({"model." + k: v for k, v in sd.items()})
    return pl.to(dev())


def new_datamodule(root):
    from beat_this_amd.dataset import BeatDataModule

    return BeatDataModule(root, batch_size=2, train_length=150, augmentations={}, device=dev())


def fit_and_resume(tmp_path, **kw):
    """``fit`` for EPOCHS epochs on the seeded data folder, keeping the checkpoint of epoch 0, then a second module under another numpy
    seed that resumes from it: the two final checkpoints hold the same weights and the same optimiser state, bit for bit.
    -> dict(root, pl, h (the first run's history), h2 (the resumed one's), a, b (the two final checkpoints), first (epoch 0's))"""
    import shutil

    from beat_this_amd.inference import load_checkpoint
    from beat_this_amd.train import fit
    from dataset_reference import build_data_folder

    root = build_data_folder(str(tmp_path / "data"))
    ck, first, ck2 = (str(tmp_path / n) for n in ("run.ckpt", "epoch0.ckpt", "resumed.ckpt"))

    def log(line):
        if line.startswith("epoch 0:"):
            shutil.copy(ck, first)

    pl = new_module()
    np.random.seed(0)
    h = fit(pl, new_datamodule(root), EPOCHS, val_frequency=1, checkpoint_path=ck, log=log, **kw)
    pl2 = new_module()
    np.random.seed(99)
    h2 = fit(pl2, new_datamodule(root), EPOCHS, val_frequency=1, checkpoint_path=ck2, resume=first, log=lambda s: None, **kw)
    a, b = load_checkpoint(ck), load_checkpoint(ck2)
    assert set(a) == set(b)
    for k, v in a["state_dict"].items():
        assert torch.equal(v, b["state_dict"][k]), k
    sa, sb = a["optimizer_states"][0], b["optimizer_states"][0]
    assert len(sa["state"]) == len(sb["state"]) > 0
    for i in sa["state"]:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert same_bits(torch.as_tensor(sa["state"][i][k]), torch.as_tensor(sb["state"][i][k])), (i, k)
    # the run moved the weights
    assert sum(not torch.equal(p.detach(), q.detach()) for p, q in zip(new_module().parameters(), pl.parameters())) > 20
    return dict(root=root, pl=pl, h=h, h2=h2, a=a, b=b, first=load_checkpoint(first))


# ---- the 16-mixed gate --------------------------------------------------------------------------------------------------------------
def mixed_gate(name, got, truth, e_ref16, keys=None, extra=(), scale=None, report=None):
    """every gradient of ``keys`` (the truth's gradients) and every tensor of ``extra`` within 2 x e_ref16 of the fp64 truth and
    finite; prints the figures first -> the worst gradient's distance in e_ref16"""
    keys = RG.grad_keys(truth) if keys is None else list(keys)
    assert np.isfinite(e_ref16) and e_ref16 > 0 and set(keys) <= set(got), name
    errs = {k: RG.rel(got[k], truth[k]) for k in keys}
    k = max(errs, key=errs.get)
    at = "" if scale is None else f" (scale {scale:g})"
    print(f"{name}: e_ref16 = {e_ref16:.3e}{at}, worst device error = {errs[k]:.3e} ({errs[k] / e_ref16:.2f} x e_ref16, {k})")
    for key in extra:
        errs[key] = RG.rel(got[key], truth[key])
        print(f"{name}: {key} {errs[key]:.3e} ({errs[key] / e_ref16:.2f} x e_ref16)")
    if report is not None:
        report("front_mixed", case=name, e_ref16=e_ref16, worst_ratio=errs[k] / e_ref16, worst_tensor=k)
    for key, e in errs.items():
        assert torch.isfinite(got[key]).all(), f"{name}: {key} is not finite"
        assert e <= MIXED_GATE * e_ref16, f"{name}: {key} is {e:.3e} from the fp64 truth, the gate is 2 x e_ref16 = {MIXED_GATE * e_ref16:.3e}"
    return errs[k] / e_ref16
