"""The mapping from the model's training settings to the arguments of each unit call, on the GPU: for every combination of
frontend (frozen / trainable / trainable with batch statistics), trunk precision, frontend precision, dropout (off / trunk /
trunk and frontend) and train() / eval() that the model admits, one forward and backward through the public API on one copy of a
model must be, bit for bit, the composition spelled out by hand from backward.py's functions on a second copy whose settings
are never touched: ``frontend_train(model, x, batch_statistics, mixed, drops)`` or the engine's frontend under ``no_grad``, the
layer loop, the final norm and the head, with the (p, seed, stream) tuples counted here in the documented order (block 0
``attnF``, ``ffF``, ``attnT``, ``ffT``, blocks 1 and 2, then the trunk's units).  Compared: the logits, every gradient, every buffer
(running statistics and ``num_batches_tracked``) and ``dropout_state()["calls"]``.  No tolerance: the route is deterministic and
has no atomics; the kernels themselves are pinned elsewhere.

D = 64, two layers, B = 2, T = 48: a ragged last block of 32 frames, and batch x time >= 2 for batch statistics."""
import copy
import itertools

import pytest
import torch

from gpu_util import dev
from route_harness import same_bits
from beat_this_amd import weights as W

pytestmark = pytest.mark.gpu

SMALL = dict(transformer_dim=64, n_layers=2, ff_mult=2)
B, T = 2, 48
SEED = 0x5EED_0000_0000_0022
P_FRONT, P_TRUNK = 0.1, 0.2
_BASE = {}


def base():
    """The model every copy is taken from (trunk and heads trainable), the input and the two weightings of the loss"""
    if not _BASE:
        from beat_this_amd.model import BeatThis

        m = BeatThis(**SMALL, dropout={"frontend": P_FRONT, "transformer": P_TRUNK})
        m.load_state_dict(W.random_state_dict(W.resolve_hparams(SMALL), seed=3, style="lively"))
        m = m.to(dev())
        for n, p in m.named_parameters():
            p.requires_grad_(not n.startswith("frontend.") and not n.endswith("rotary_embed.freqs"))
        g = torch.Generator().manual_seed(22)
        _BASE.update(model=m, x=torch.log1p(torch.rand(B, T, 128, generator=g) * 30).to(dev()),
                     wb=torch.randn(B, T, generator=g).to(dev()), wd=torch.randn(B, T, generator=g).to(dev()))
    return _BASE


def finish(m, x, beat, down):
    """backward of a fixed weighting of the logits -> everything that is compared"""
    (beat * base()["wb"]).sum().add((down * base()["wd"]).sum()).backward()
    out = {"beat": beat.detach(), "downbeat": down.detach(), "x.grad": x.grad}
    out.update({"grad " + n: p.grad for n, p in m.named_parameters()})
    out.update({"buffer " + n: b for n, b in m.named_buffers()})
    return out


def through_the_api(front, trunk16, front16, drop, training):
    m = copy.deepcopy(base()["model"])
    if front != "frozen":
        m.set_frontend_trainable()
    if front == "batch":
        m.set_batch_statistics()
    m.set_train_precision("16-mixed" if trunk16 else "32-true").set_frontend_precision("16-mixed" if front16 else "32-true")
    if drop != "off":
        m.enable_dropout(seed=SEED, frontend=drop == "both")
    m.train(training)
    x = base()["x"].clone().requires_grad_(True)
    out = m(x)
    state = m.dropout_state()
    return finish(m, x, out["beat"], out["downbeat"]), None if state is None else state["calls"]


def by_hand(front, trunk16, front16, drop, training):
    from beat_this_amd.model import backward as bw

    m = copy.deepcopy(base()["model"]).train(training)      # (its settings stay the defaults: every argument is explicit)
    x = base()["x"].clone().requires_grad_(True)
    streams = itertools.count()
    if front == "frozen":
        with torch.no_grad():
            h = m.engine(frontend_only=True).forward_stages(x, m._precision(), 0, 0)
    else:
        for n, p in m.frontend.named_parameters():
            p.requires_grad_(not n.endswith("rotary_embed.freqs"))
        drops = (lambda: (P_FRONT, SEED, next(streams))) if drop == "both" and training else None
        h = bw.frontend_train(m, x, front == "batch" and training, front16, drops)
    trunk_drop = (lambda: (P_TRUNK, SEED, next(streams))) if drop != "off" and training else (lambda: None)
    for attn, ff in m.transformer_blocks.layers:
        h = bw.attention(attn, h, *m._rope(T), trunk_drop(), trunk16) + h
        h = bw.feedforward(ff, h, trunk_drop(), trunk16) + h
    beat, down = bw.head(m.task_heads, bw.final_norm(m.transformer_blocks.norm, h), True)
    return finish(m, x, beat, down), None if drop == "off" else next(streams)


@pytest.mark.parametrize("front", ["frozen", "trainable", "batch"])
def test_the_api_takes_the_route_spelled_out_by_hand(front):
    for trunk16, front16, drop, training in itertools.product((False, True), (False, True), ("off", "trunk", "both"), (True, False)):
        case = (front, trunk16, front16, drop, training)
        got, calls = through_the_api(*case)
        want, streams = by_hand(*case)
        assert calls == streams, case
        if training and drop != "off":
            assert calls == 2 * SMALL["n_layers"] + (12 if drop == "both" and front != "frozen" else 0), case
        assert set(got) == set(want), case
        for k in want:
            assert (got[k] is None) == (want[k] is None), (case, k)
            assert want[k] is None or same_bits(got[k], want[k]), (case, k)
        assert (got["x.grad"] is None) == (front == "frozen") and got["grad task_heads.beat_downbeat_lin.weight"] is not None, case
        tracked = "frontend.stem.bn1d.num_batches_tracked"
        moved = int(got["buffer " + tracked]) != int(base()["model"].state_dict()[tracked])
        assert moved == (front == "batch" and training), case
