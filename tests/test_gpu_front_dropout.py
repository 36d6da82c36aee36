"""Frontend dropout on the GPU: the dropout kernels of the training route at the shapes of the frontend's
leaves -- width 32 with a single head, sequences of 8, 16 and 32 tokens (under the 64-query block of the fp32 sweeps and the 32-wide
tile of the mixed ones), 130 sequences per call -- then the partial transformers, the whole model, the opt-in's bookkeeping, ``fit``
and the command line, against route_reference.py: fp64 torch on the CPU with the masks of the host twin's contract.

Gates: fp32 -- the outputs and every gradient within route_grads.GATE (10) x e_ref, e_ref the same computation in fp32; 16-mixed
-- within 2 x e_ref16, the distance the CPU fp16-autocast run with the same masks, at the loss scale the helper finds, keeps from
fp64 (tests/test_gpu_mixed.py's gate).  B = 2; T = 3 (a ragged last key group inside one block) and T = 65 (a second 64-query block
on the fp32 route, a third 32-wide tile on the mixed one).

Worst ratios measured on an MI355X are recorded in DESIGN.md section 21."""
import copy
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import route_cases as RC
import route_grads as RG
import route_harness as H
import route_reference as REF
from conftest import ROOT
from dataset_reference import build_data_folder
from gpu_util import Guarded, assert_intact, dev, report
from route_harness import MIXED_GATE, both_poisons, model_device, randn, same_bits

pytestmark = pytest.mark.gpu

B = 2
SEED = 0x5EED_0000_0000_0021          # (beyond 32 bits: both key words are in use)
P_FRONT, P_TRUNK = 0.1, 0.2           # the reference's rates
N_LAYERS = RC.HP["n_layers"]
_MODELS = {}


def new_model(partial=True, dropout=None):
    """the D = 64, two-layer model of route_cases.model_state_dict on the GPU, everything trainable"""
    return H.make_model(dict(RC.HP, partial_transformers=partial), RC.model_state_dict("lively", partial), frontend=True, freeze_freqs=True,
                        dropout=dropout or {"frontend": P_FRONT, "transformer": P_TRUNK})


def shared_model():
    """one model for the tests that leave its state as they found it"""
    if "shared" not in _MODELS:
        _MODELS["shared"] = new_model()
    return _MODELS["shared"]


# ---- 1. the leaves through the C ABI at the frontend's shapes ------------------------------------------------------------------------
class Leaf:
    """The operands of one leaf call -- BT_UNIT_ATTN / BT_UNIT_FF with residual = 1 on (B', T', C) with the weights of
    ``frontend.blocks.i.partial.<leaf>`` -- in guarded buffers filled with ``poison`` (tests/test_gpu_dropout.py's ``Unit``, on
    either route); ``run`` does the forward and the backward and returns the outputs by state-dict key"""

    def __init__(self, i, leaf, x, gy, poison, mixed):
        from beat_this_amd import _lib as L

        self.L, self.poison, self.mixed, self.keep = L, poison, mixed, []
        sd, m = RC.model_state_dict(), shared_model()
        kind = "attn" if leaf.startswith("attn") else "ff"
        self.keys = RG.leaf_keys(i, leaf)
        self.unit = L.UNIT_ATTN if kind == "attn" else L.UNIT_FF
        Bn, T, D = x.shape
        self.hidden = int(sd[f"frontend.blocks.{i}.partial.ff{leaf[-1]}.net.1.weight"].shape[0])
        self.shape = (Bn, T, D)
        rope, rope_len = m._rope(T)
        a = self.a = L.TrainArgs()
        a.B, a.T, a.dim, a.hidden, a.rope_len, a.residual = Bn, T, D, self.hidden, rope_len, 1
        a.rope = rope.data_ptr()
        self.rope = rope
        a.x, a.gy = self.buf((Bn, T, D), x).ptr(), self.buf((Bn, T, D), gy).ptr()
        fields = ("gamma", "w1", "w2", "b2", "w3") if kind == "attn" else ("gamma", "w1", "b1", "w2", "b2")
        self.outs = {"y": self.buf((Bn, T, D)), "x": self.buf((Bn, T, D))}
        a.y, a.gx = self.outs["y"].ptr(), self.outs["x"].ptr()
        if kind == "attn":
            self.outs["save_o"], self.outs["save_lse"] = self.buf((Bn, T, D)), self.buf((Bn, T, D // 32))
            a.save_o, a.save_lse = self.outs["save_o"].ptr(), self.outs["save_lse"].ptr()
        for f, k in zip(fields, self.keys):
            setattr(a, f, self.buf(sd[k].shape, sd[k]).ptr())
            self.outs[k] = self.buf(sd[k].shape)
            setattr(a, "g_" + f, self.outs[k].ptr())

    def buf(self, shape, data=None, dtype=torch.float32):
        b = Guarded(shape, dtype).fill(self.poison, data=None if data is None else data.to(dev()))
        self.keep.append(b)
        return b

    def run(self, drop):
        L, lib = self.L, self.L.lib()
        d = C.byref(L.TrainDropout(p=drop[0], seed=drop[1], stream=drop[2]))
        for backward in (0, 1):
            if self.mixed:
                n = lib.bt_train_workspace_bytes_mixed(self.unit, backward, *self.shape, self.hidden, 1)
                fn = lib.bt_train_backward_mixed if backward else lib.bt_train_forward_mixed
            else:
                n = lib.bt_train_workspace_bytes_dropout(self.unit, backward, *self.shape, self.hidden)
                fn = lib.bt_train_backward_dropout if backward else lib.bt_train_forward_dropout
            assert n > 0
            ws = self.buf((n,), dtype=torch.uint8)
            self.a.ws, self.a.ws_bytes = ws.ptr(), n
            L.check(fn(L.stream_ptr(dev()), self.unit, C.byref(self.a), d))
        torch.cuda.synchronize()
        assert_intact(*[(f"leaf buffer {j}", g) for j, g in enumerate(self.keep)])
        return {k: g.t.clone() for k, g in self.outs.items()}


def mixed_gate(name, got, truth, e_ref16, scale, extra=("y",)):
    """every gradient (and ``extra``) within 2 x e_ref16 of the fp64 truth -> the worst gradient's distance in e_ref16"""
    return H.mixed_gate(name, got, truth, e_ref16, None, extra, scale)


def without_stats(res):
    return {k: v for k, v in res.items() if k != "stats"}


# (block, direction): (B', T', dim) = (130, 32, 32), (130, 16, 64), (130, 8, 128) in the frequency direction of a (2, 65) batch and
# (64, 65, 32), (32, 65, 64), (16, 65, 128) in its time direction
LEAF_CASES = [(i, d) for d in "FT" for i in (0, 1, 2)]
RATES = (0.1, 0.5)


@pytest.mark.parametrize("mixed", [False, True], ids=["fp32", "mixed"])
@pytest.mark.parametrize("kind", ["attn", "ff"])
@pytest.mark.parametrize("i,direction", LEAF_CASES)
def test_leaves_at_the_frontends_shapes(i, direction, kind, mixed):
    leaf = kind + direction
    Bp, Tp, C_ = REF.leaf_shape(i, leaf, B, 65)
    assert (Bp, Tp, C_) == {"F": ((130, 32, 32), (130, 16, 64), (130, 8, 128)), "T": ((64, 65, 32), (32, 65, 64), (16, 65, 128))}[direction][i]
    sd = RC.model_state_dict()
    seed = 3000 + 100 * i + 10 * "FT".index(direction) + (5 if kind == "ff" else 0)
    x, g = randn(Bp, Tp, C_, seed=seed), randn(Bp, Tp, C_, seed=seed + 1) * 2.0 ** -14
    worst = 0.0
    for p in RATES:
        drop = (p, SEED, 7000 + seed + int(10 * p))
        name = f"front dropout leaf {leaf}{i} {'mixed' if mixed else 'fp32'} ({Bp}, {Tp}, {C_}) p={p}"
        if not mixed:
            got = both_poisons(name, lambda q: Leaf(i, leaf, x, g, q, False).run(drop))
            g32, g64 = (without_stats(RG.leaf_grads(sd, i, leaf, x, g, dt, drop)) for dt in (torch.float32, torch.float64))
            ratio = RG.check(name, got, g32, g64)[1]
        else:
            truth, _, scale, e_ref16 = RG.mixed_yardstick(
                lambda dt, s, auto: without_stats(RG.leaf_grads(sd, i, leaf, x, g, dt, drop, None, s, auto)))
            got = both_poisons(name, lambda q: Leaf(i, leaf, x, g * scale, q, True).run(drop))
            got = {k: (v if k in ("y", "save_o", "save_lse") else v / scale) for k, v in got.items()}
            ratio = mixed_gate(name, got, truth, e_ref16, scale)
        worst = max(worst, ratio)
    report("front_dropout_leaf", leaf=leaf, block=i, mixed=mixed, shape=str((Bp, Tp, C_)), worst_ratio=worst)


# ---- 2. each partial transformer through backward.partial_ft ------------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [False, True], ids=["fp32", "mixed"])
@pytest.mark.parametrize("T", [3, 65])
@pytest.mark.parametrize("i", [0, 1, 2])
def test_partial_transformers_with_drops(i, T, mixed):
    from beat_this_amd.model import backward as bw

    m, sd = shared_model(), RC.model_state_dict()
    node, pfx = m.frontend.blocks[i].partial, f"frontend.blocks.{i}.partial."
    x, g = RC.partial_inputs(i, B, T)
    drops = {leaf: (P_FRONT, SEED, 50 + 4 * i + j) for j, leaf in enumerate(REF.LEAVES)}
    name = f"front dropout partial{i} {'mixed' if mixed else 'fp32'} B={B} T={T}"

    def run(scale, how):
        xd = x.to(dev()).requires_grad_(True)
        y = bw.partial_ft(node, xd, m._rope, mixed, how)
        params = [(pfx + n, q) for n, q in node.named_parameters() if not n.endswith("freqs")]
        grads = torch.autograd.grad([y], [xd] + [q for _, q in params], [(g * scale).to(dev())])
        res = {k: v / scale for k, v in zip(["x"] + [n for n, _ in params], grads)}
        res["y"] = y.detach()
        return res

    four = [drops[leaf] for leaf in REF.LEAVES]
    if not mixed:
        got, again = run(1.0, four), run(1.0, iter(four).__next__)          # four values, or a callable that yields them
        g32, g64 = (without_stats(RG.partial_grads(sd, i, x, g, dt, drops=drops)) for dt in (torch.float32, torch.float64))
        ratio = RG.check(name, got, g32, g64)[1]
    else:
        truth, _, scale, e_ref16 = RG.mixed_yardstick(
            lambda dt, s, auto: without_stats(RG.partial_grads(sd, i, x, g, dt, None, s, auto, drops=drops)))
        got, again = run(scale, four), run(scale, iter(four).__next__)
        ratio = mixed_gate(name, got, truth, e_ref16, scale)
    assert len(got) == 22 and all(same_bits(got[k], again[k]) for k in got)
    plain, default = run(1.0, None), run(1.0, [None] * 4)                   # no dropout: the calls as ever
    assert all(same_bits(plain[k], default[k]) for k in plain) and not same_bits(plain["y"], got["y"])
    with pytest.raises(ValueError, match="four leaves"):
        run(1.0, four[:3])
    report("front_dropout_partial", block=i, T=T, mixed=mixed, worst_ratio=ratio)


# ---- 3. the whole model ------------------------------------------------------------------------------------------------------------
def model_inputs(T=65):
    x, beat, down, mask = RC.model_inputs(B, T, True)
    return x, beat, down, mask, RG.trunk_loss(beat, down, mask)


@pytest.mark.parametrize("variant", ["fp32", "batch_statistics", "mixed"])
def test_the_whole_model_with_both_opt_ins(variant):
    sd = RC.model_state_dict()
    x, beat, down, mask, loss_fn = model_inputs()
    m = new_model().train()
    m.enable_dropout(seed=SEED, frontend=True)
    first = 3                                                               # (not 0: the streams follow the counter)
    m.set_dropout_state({"seed": SEED, "calls": first})
    plan, trunk, used = REF.model_plan(sd, P_FRONT, P_TRUNK, SEED, first)
    assert used == 12 + 2 * N_LAYERS and trunk == (P_TRUNK, SEED, first + 12)
    batch = variant == "batch_statistics"
    name = f"front dropout whole model {variant} B={B} T=65"
    if batch:
        m.set_batch_statistics()
    if variant == "mixed":
        m.set_frontend_precision("16-mixed").set_train_precision("16-mixed")
        truth, auto, scale, e_ref16 = RG.mixed_yardstick(
            lambda dt, s, a: without_stats(RG.model_grads(sd, x, loss_fn, dt, None, s, a, plan_=plan, trunk_drop=trunk)), start=RG.SCALE)
        got = model_device(m, x, beat, down, mask, scale)
        assert set(RG.grad_keys(truth)) == set(got) - {"beat", "downbeat"} and len(got) == 102
        ratio = mixed_gate(name, got, truth, e_ref16, scale, extra=())
        for k in ("beat", "downbeat"):
            e16, e = RG.rel(auto[k], truth[k]), RG.rel(got[k], truth[k])
            print(f"{name} {k} logits: autocast {e16:.3e}, device {e:.3e}")
            assert e <= MIXED_GATE * e16, (k, e, e16)
    else:
        r32, r64 = (RG.model_grads(sd, x, loss_fn, dt, plan_=plan, trunk_drop=trunk, batch=batch) for dt in (torch.float32, torch.float64))
        got = model_device(m, x, beat, down, mask)
        assert set(RG.grad_keys(r64)) == set(got) - {"beat", "downbeat"} and len(got) == 102
        if batch:
            stats = {k: v.detach().cpu() for k, v in m.state_dict().items() if k in r64["stats"]}
            as_bu = lambda r: {"grads": without_stats(r), "stats": r["stats"]}
            ratio = RG.check_batch(name, got, stats, as_bu(r32), as_bu(r64), report)[1]
        else:
            ratio = RG.check(name, got, without_stats(r32), without_stats(r64), report)[1]
    assert m.dropout_state() == {"seed": SEED, "calls": first + 12 + 2 * N_LAYERS, "frontend": True}
    report("front_dropout_model", variant=variant, worst_ratio=ratio)


def test_the_counter_advances_by_the_calls_that_drop():
    x = model_inputs()[0].to(dev())
    for partial, rates, want in ((True, None, 12 + 2 * N_LAYERS), (False, None, 2 * N_LAYERS),
                                 (True, {"frontend": 0.0, "transformer": P_TRUNK}, 2 * N_LAYERS),
                                 (True, {"frontend": P_FRONT, "transformer": 0.0}, 12)):
        m = new_model(partial, rates).train()
        m.enable_dropout(seed=SEED, frontend=True)
        for n in (1, 2):
            out = m(x)
            assert m.dropout_state()["calls"] == n * want, (partial, rates, n)
            assert torch.isfinite(out["beat"]).all()
        m.frontend(x)                                                      # the stage alone: its leaves only
        assert m.dropout_state()["calls"] == 2 * want + (12 if partial and m.dropout["frontend"] > 0 else 0)


# ---- 4. nothing existing moved ----------------------------------------------------------------------------------------------------
def test_without_the_frontend_opt_in_the_bits_are_the_parents():
    from beat_this_amd.model import backward as bw

    x, beat, down, mask, _ = model_inputs()
    never = new_model().train()                                             # dropout never enabled: hands out nothing
    m = new_model().train().enable_dropout(seed=SEED)
    assert m.dropout_state() == {"seed": SEED, "calls": 0} and not m.frontend_dropout
    got = model_device(m, x, beat, down, mask)
    assert m.dropout_state() == {"seed": SEED, "calls": 2 * N_LAYERS}       # no third key, 2 L numbers
    # the parent's semantics from the pieces: the frontend without dropout, then the trunk's units with streams 0 .. 2 L - 1
    from beat_this_amd.model.loss import ShiftTolerantBCELoss

    xd = x.to(dev()).requires_grad_(True)
    h = bw.frontend_train(never, xd, False, False)
    for l, (attn, ff) in enumerate(never.transformer_blocks.layers):
        h = bw.attention(attn, h, *never._rope(h.shape[1]), (P_TRUNK, SEED, 2 * l)) + h
        h = bw.feedforward(ff, h, (P_TRUNK, SEED, 2 * l + 1)) + h
    ob, od = bw.head(never.task_heads, bw.final_norm(never.transformer_blocks.norm, h), True)
    fn = ShiftTolerantBCELoss().to(dev())
    (fn(ob, beat.to(dev()), mask.to(dev()).bool()) + fn(od, down.to(dev()), mask.to(dev()).bool())).backward()
    want = {n: p.grad for n, p in never.named_parameters() if p.grad is not None}
    want.update(x=xd.grad, beat=ob.detach(), downbeat=od.detach())
    assert set(want) == set(got) and len(got) == 102
    for k in want:
        assert same_bits(got[k], want[k]), f"{k} moved"


def test_eval_no_grad_rewind_and_capture():
    x, beat, down, mask, _ = model_inputs()
    never = new_model()
    want = model_device(never, x, beat, down, mask)                         # eval(), dropout never enabled
    m = new_model().enable_dropout(seed=SEED, frontend=True)
    got = model_device(m, x, beat, down, mask)                              # opted in, but in eval()
    assert m.dropout_state() == {"seed": SEED, "calls": 0, "frontend": True}
    assert set(got) == set(want)
    for k in want:
        assert same_bits(got[k], want[k]), f"eval(): {k} moved"
    m.train()
    with torch.no_grad():                                                   # the inference path never drops
        quiet = m(x.to(dev()))
    assert m.dropout_state()["calls"] == 0 and torch.isfinite(quiet["beat"]).all()
    first, second = model_device(m, x, beat, down, mask), model_device(m, x, beat, down, mask)
    per = 12 + 2 * N_LAYERS
    assert m.dropout_state()["calls"] == 2 * per
    m.set_dropout_state({"seed": SEED, "calls": 0})                         # (no key: the opt-in stays)
    again, second_again = model_device(m, x, beat, down, mask), model_device(m, x, beat, down, mask)
    assert m.dropout_state() == {"seed": SEED, "calls": 2 * per, "frontend": True}
    for k in first:
        assert same_bits(first[k], again[k]) and same_bits(second[k], second_again[k]), k
    assert not same_bits(first["beat"], second["beat"]) and not same_bits(first["beat"], want["beat"])
    trunk_only = model_device(new_model().train().enable_dropout(seed=SEED), x, beat, down, mask)
    assert not same_bits(first["beat"], trunk_only["beat"])
    # a capture with frontend dropout active is refused, and takes no number
    xd = x.to(dev()).requires_grad_(True)
    m.frontend(xd)                                                          # (warm: the rotary tables and the allocator have seen the shapes)
    torch.cuda.synchronize()
    calls = m.dropout_state()["calls"]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        xd * 2.0                                                            # (something to capture)
        with pytest.raises(RuntimeError, match="graph capture"):
            m.frontend(xd)
    torch.cuda.synchronize()
    assert m.dropout_state()["calls"] == calls


# ---- 5. the loop and the command line -----------------------------------------------------------------------------------------------
LR, WARMUP, EPOCHS = 2e-3, 2, 2


def new_module(frontend_dropout, seed=11):
    from beat_this_amd.model.pl_module import PLBeatThis

    pl = PLBeatThis(transformer_dim=64, n_layers=2, ff_mult=2, lr=LR, warmup_steps=WARMUP, max_epochs=EPOCHS, eval_trim_beats=0,
                    apply_dropout=True, dropout_seed=seed, train_frontend=True, apply_frontend_dropout=frontend_dropout)
    pl.load_state_dict({"model." + k: v for k, v in RC.model_state_dict().items()})
    return pl.to(dev())


def new_datamodule(root):
    from beat_this_amd.dataset import BeatDataModule

    return BeatDataModule(root, batch_size=2, train_length=150, augmentations={}, device=dev())


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from beat_this_amd.train import fit

    tmp = tmp_path_factory.mktemp("front_dropout")
    root = build_data_folder(str(tmp / "data"))
    ck, first = str(tmp / "run.ckpt"), str(tmp / "epoch0.ckpt")

    def log(line):   # (called after the epoch's checkpoint is written)
        if line.startswith("epoch 0:"):
            shutil.copy(ck, first)

    pl = new_module(False)                                                  # fit() sets the opt-in
    np.random.seed(0)
    history = fit(pl, new_datamodule(root), EPOCHS, val_frequency=2, checkpoint_path=ck, log=log, train_frontend=True,
                  frontend_dropout=True)
    return dict(tmp=tmp, root=root, ck=ck, first=first, pl=pl, history=history)


def test_fit_with_frontend_dropout_differs_resumes_and_loads(run):
    from beat_this_amd.inference import load_checkpoint, load_model
    from beat_this_amd.train import CHECKPOINT_KEYS, fit

    h = run["history"]
    assert run["pl"].model.training and run["pl"].model.frontend_dropout
    assert len(h["train_loss"]) == EPOCHS and all(np.isfinite(h["train_loss"]))
    plain = new_module(False)
    np.random.seed(0)
    h0 = fit(plain, new_datamodule(run["root"]), EPOCHS, val_frequency=2, log=lambda line: None, train_frontend=True)
    assert plain.model.dropout_state() is not None and not plain.model.frontend_dropout
    print("train losses: with frontend dropout", h["train_loss"], "trunk dropout only", h0["train_loss"])
    assert h0["train_loss"][0] != h["train_loss"][0] and h0["train_loss"][1] != h["train_loss"][1]
    # the checkpoint: the usual keys, the opt-in inside rng["dropout"], readable by load_model
    a = load_checkpoint(run["ck"])
    assert set(a) == set(CHECKPOINT_KEYS)
    calls = a["rng"]["dropout"]["calls"]
    assert a["rng"]["dropout"] == {"seed": 11, "calls": calls, "frontend": True}
    assert calls > 0 and calls % (12 + 2 * 2) == 0                          # 12 + 2 L per training forward
    assert load_checkpoint(run["first"])["rng"]["dropout"]["calls"] == calls // 2
    assert set(load_checkpoint(str(run["ck"]))["hyper_parameters"]) == set(plain.hyper_parameters)
    loaded = load_model(run["ck"], dev())
    x = torch.log1p(torch.rand(2, 150, 128, generator=torch.Generator().manual_seed(5)) * 30).to(dev())
    with torch.no_grad():
        want, got = run["pl"].model(x), loaded(x)
    for k in ("beat", "downbeat"):
        assert same_bits(got[k], want[k]), k
    # one epoch plus a resumed second one: the bits of the uninterrupted run; the checkpoint's state brings the opt-in back
    ck2 = str(run["tmp"] / "resumed.ckpt")
    pl = new_module(False, seed=999)                                        # (whatever seed, no opt-in: the checkpoint's state replaces both)
    np.random.seed(1234)
    h2 = fit(pl, new_datamodule(run["root"]), EPOCHS, val_frequency=2, checkpoint_path=ck2, resume=run["first"], log=lambda line: None,
             train_frontend=True)
    assert pl.model.frontend_dropout and h2["train_loss"] == h["train_loss"][1:]
    b = load_checkpoint(ck2)
    assert b["rng"]["dropout"] == a["rng"]["dropout"]
    for k, v in a["state_dict"].items():
        assert torch.equal(v, b["state_dict"][k]) and (not v.is_floating_point() or same_bits(v, b["state_dict"][k])), k
    for i, st in a["optimizer_states"][0]["state"].items():
        for k in ("exp_avg", "exp_avg_sq"):
            assert same_bits(st[k], b["optimizer_states"][0]["state"][i][k]), (i, k)
    # the switch needs its prerequisites
    from beat_this_amd.model.pl_module import PLBeatThis

    with pytest.raises(ValueError, match="dropout enabled"):
        fit(PLBeatThis(transformer_dim=64, n_layers=2, ff_mult=2).to(dev()), new_datamodule(run["root"]), 0, train_frontend=True,
            frontend_dropout=True, log=lambda line: None)
    with pytest.raises(ValueError, match="trainable frontend"):
        fit(PLBeatThis(transformer_dim=64, n_layers=2, ff_mult=2, apply_dropout=True).to(dev()), new_datamodule(run["root"]), 0,
            frontend_dropout=True, log=lambda line: None)
    off = new_module(True)
    fit(off, new_datamodule(run["root"]), 0, frontend_dropout=False, log=lambda line: None)
    assert off.model.dropout_state() == {"seed": 11, "calls": 0}


def test_cli_trains_with_frontend_dropout(run):
    from beat_this_amd.inference import load_checkpoint

    start, out = str(run["tmp"] / "start.ckpt"), str(run["tmp"] / "cli" / "out.ckpt")
    fresh = new_module(False)
    torch.save({"state_dict": {k: v.cpu() for k, v in fresh.state_dict().items()}, "hyper_parameters": fresh.hyper_parameters}, start)
    r = subprocess.run([sys.executable, "-m", "beat_this_amd.train", "--data-dir", run["root"], "--checkpoint", start, "--output", out,
                        "--max-epochs", "1", "--batch-size", "2", "--train-length", "150", "--accumulate-grad-batches", "1",
                        "--warmup-steps", "2", "--val-frequency", "1", "--eval-trim-beats", "0", "--no-mask-augmentation",
                        "--train-frontend", "--dropout", "--apply-frontend-dropout", "--frontend-dropout", "0.3", "--seed", "3"],
                       cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "epoch 0: train_loss" in r.stdout
    ckpt = load_checkpoint(out)
    d = ckpt["rng"]["dropout"]
    assert d["seed"] == 3 and d["frontend"] is True and d["calls"] > 0 and d["calls"] % 16 == 0
    assert ckpt["hyper_parameters"]["dropout"] == {"frontend": 0.3, "transformer": 0.2}
