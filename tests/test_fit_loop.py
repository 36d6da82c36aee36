"""``fit()``'s epoch loop on the CPU, with fakes in the place of the module, the optimiser, the schedule and the loader: the exact
sequence of training, optimiser and scheduler calls for a single process (written out below, not derived from ``step_groups``),
the epoch's mean loss bit for bit, what ``configure_optimizers`` is handed, that a run without a process group does not import
``torch.distributed``, the refusal of a loader that yields another number of batches than its ``len()`` -- and the same fakes
on two gloo ranks: who runs which batch, the groups' counts, the same mean loss as the single process, rank 0 alone logging.

The losses come from a table of fp32 values whose sums depend on the association: an epoch's mean is right only if the five
values are added one after the other, in batch order, in fp32, from zero."""
import os
import queue
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

BATCHES, EPOCHS = 5, 2
# 2^24 swallows what is added to it in fp32: (0.1 + 2^24) + 1 - 2^24 + 0.7 is 0.7 left to right, 1.8 exactly, 1.7 or 1.0 in
# other orders; the second epoch does the same around 2^25, where 2.5 is rounded up to 4: 4.6 left to right, 3.4 exactly
LOSSES = np.array([[0.1, 16777216.0, 1.0, -16777216.0, 0.7], [0.3, 33554432.0, 2.5, -33554432.0, 0.6]], dtype=np.float32)
# accumulate -> one epoch's calls: bJ = training_step of batch J (then its backward), sN = optimizer.step(accumulated=N),
# each followed by scheduler.step(); and the run's optimiser steps after both epochs
SEQUENCE = {
    1: ("b0 s1 b1 s1 b2 s1 b3 s1 b4 s1", 10),
    2: ("b0 b1 s2 b2 b3 s2 b4 s1", 6),
    3: ("b0 b1 b2 s3 b3 b4 s2", 4),
    5: ("b0 b1 b2 b3 b4 s5", 2),
    7: ("b0 b1 b2 b3 b4 s5", 2),
}


def calls(text):
    out = []
    for word in text.split():
        out += [("batch", int(word[1:]))] if word[0] == "b" else [("step", int(word[1:])), ("sched",)]
    return out


def expected_means():
    means = []
    for row in LOSSES:
        total = np.float32(0.0)
        for value in row:
            total = np.float32(total + value)
        means.append(float(total) / BATCHES)
    return means


class FakeModel:
    batch_statistics = False

    def __init__(self):
        from beat_this_amd.model.settings import TrainSettings

        self.train_settings = TrainSettings()

    def dropout_state(self):
        return None


class FakeOptimizer:
    device = torch.device("cpu")

    def __init__(self, events, params):
        self.events, self.param_groups = events, [{"params": params, "lr": 0.0}]

    def zero_grad(self):
        pass

    def step(self, accumulated=None, loss_scaler=None):
        assert loss_scaler is None
        self.events.append(("step", accumulated))

    def flat_state(self):
        return {"exp_avg": torch.zeros(4), "n_averaged": 0}

    def state_dict(self):
        return {"state": {}, "param_groups": []}


class FakeScheduler:
    def __init__(self, events):
        self.events = events

    def step(self):
        self.events.append(("sched",))

    def get_last_lr(self):
        return [0.0]

    def state_dict(self):
        return {}


class FakeModule(torch.nn.Module):
    """``training_step`` of batch j, the e-th time it comes: LOSSES[e][j] as a 0-dim fp32 tensor that requires grad"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))
        self.model, self.events, self.configured, self.times = FakeModel(), [], [], {}

    def training_step(self, batch, batch_idx):
        assert batch == {"j": batch_idx}
        epoch = self.times.get(batch_idx, 0)
        self.times[batch_idx] = epoch + 1
        self.events.append(("batch", batch_idx))
        loss = self.w.sum() * 0.0 + torch.tensor(LOSSES[epoch][batch_idx])
        assert loss.dtype == torch.float32 and loss.ndim == 0 and loss.requires_grad
        return loss

    def configure_optimizers(self, total_steps, **kw):
        self.configured.append(dict(total_steps=total_steps, **kw))
        return {"optimizer": FakeOptimizer(self.events, [self.w]), "lr_scheduler": {"scheduler": FakeScheduler(self.events)}}


class FakeLoader:
    """a sized list-like of ``BATCHES`` batches; ``yields``: how many it really hands out"""

    def __init__(self, yields=BATCHES):
        self.yields = yields

    def __len__(self):
        return BATCHES

    def __iter__(self):
        return iter([{"j": j} for j in range(self.yields)])

    def shard(self, rank, world):
        return ((j, {"j": j}) for j in range(BATCHES) if j % world == rank)


class FakeData:
    def __init__(self, loader):
        self.loader = loader

    def setup(self, stage):
        assert stage == "fit"

    def train_dataloader(self):
        return self.loader


def run_fit(accumulate, loader=None, **kw):
    from beat_this_amd.train import fit

    pl, lines = FakeModule(), []
    history = fit(pl, FakeData(loader or FakeLoader()), EPOCHS, accumulate_grad_batches=accumulate, val_frequency=EPOCHS + 1,
                  log=lines.append, **kw)
    return pl, history, lines


def test_the_loss_table_shows_the_association():
    means = expected_means()
    assert means[0] == float(np.float32(0.7)) / BATCHES
    for row, mean in zip(LOSSES, means):
        assert float(row.astype(np.float64).sum()) / BATCHES != mean       # not a sum in fp64
        assert float(np.float32(row[::-1].sum())) / BATCHES != mean and float((row[:3].sum() + row[3:].sum())) / BATCHES != mean


@pytest.mark.parametrize("accumulate", sorted(SEQUENCE))
def test_single_process_calls_and_mean_loss(accumulate):
    pl, history, lines = run_fit(accumulate)
    text, steps = SEQUENCE[accumulate]
    assert pl.events == calls(text) * EPOCHS
    assert history["global_step"] == steps and history["epoch"] == EPOCHS - 1
    got, want = history["train_loss"], expected_means()
    assert [np.float64(v).tobytes() for v in got] == [np.float64(v).tobytes() for v in want], (got, want)
    assert pl.configured == [dict(total_steps=steps, max_grad_norm=None, accumulate=accumulate)]   # no process_group, staged, ema_decay
    assert history["val"] == [] and history["loss_scaler"] is None
    assert len(lines) == EPOCHS and all(line.startswith(f"epoch {e}: train_loss ") for e, line in enumerate(lines))
    assert f"{steps} steps" in lines[-1] and "ranks" not in lines[-1]


@pytest.mark.parametrize("yields, told, ran", [(4, "ended after 4", "b0 b1 s2 b2 b3"), (6, "yielded batch 5", "b0 b1 s2 b2 b3 s2 b4")])
def test_a_loader_that_lies_about_its_length_is_refused(yields, told, ran):
    """both counts are named, and no step with a wrong count was taken on the way"""
    from beat_this_amd.train import fit

    pl = FakeModule()
    with pytest.raises(RuntimeError) as e:
        fit(pl, FakeData(FakeLoader(yields)), EPOCHS, accumulate_grad_batches=2, val_frequency=EPOCHS + 1, log=lambda line: None)
    assert f"{BATCHES} batches" in str(e.value) and told in str(e.value)
    assert pl.events == calls(ran)


CHILD = r"""
import builtins, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import torch
import test_fit_loop as T
import beat_this_amd.train, beat_this_amd.optim, beat_this_amd.model.settings
asked, real = [], builtins.__import__
def recording(name, globals=None, locals=None, fromlist=(), level=0):
    if level == 0 and str((globals or {}).get("__name__", "")).startswith("beat_this_amd"):
        asked.extend([name] + [f"{name}.{leaf}" for leaf in fromlist or ()])
    return real(name, globals, locals, fromlist, level)
builtins.__import__ = recording
exec("import torch.distributed as dist", {"__name__": "beat_this_amd.probe"})
assert asked == ["torch.distributed"], asked   # (the recorder sees what it is there to see)
del asked[:]
before = set(sys.modules)
pl, history, lines = T.run_fit(2)
builtins.__import__ = real
assert pl.events == T.calls(T.SEQUENCE[2][0]) * T.EPOCHS
new = [m for m in set(sys.modules) - before if m.startswith("torch.distributed")]
named = [m for m in asked if m.startswith("torch.distributed")]
assert not new and not named, (new, named)
print("fit imported nothing of torch.distributed")
"""


def test_a_single_process_does_not_import_torch_distributed():
    """in a fresh process: ``import torch`` may load torch.distributed by itself, so besides ``sys.modules`` before and after the
    call, every import statement the package executes during it is recorded"""
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, os.path.join(ROOT, "tests")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "fit imported nothing of torch.distributed" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank(rank, world, port, q, accumulate):
    import torch.distributed as dist

    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    np.random.seed(0)   # (fit's rule: the ranks share numpy's seed, and compare the generator at every epoch's end)
    pl, history, lines = run_fit(accumulate, process_group=dist.group.WORLD, staged=True)
    q.put((rank, dict(events=pl.events, train_loss=history["train_loss"], global_step=history["global_step"], lines=lines,
                      configured=[{k: v for k, v in c.items() if k != "process_group"} for c in pl.configured],
                      grouped=["process_group" in c for c in pl.configured])))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("accumulate, counts", [(1, [2, 2, 1]), (2, [4, 1])])
def test_two_ranks_run_the_same_loop(accumulate, counts):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q, accumulate)) for r in range(2)]
    for p in procs:
        p.start()
    got, waited = {}, 0
    try:
        while len(got) < 2:
            try:
                got.update([q.get(timeout=1)])
            except queue.Empty:   # (a rank that raised will never answer: do not wait for it)
                waited += 1
                assert waited < 100 and all(p.exitcode in (None, 0) for p in procs), [p.exitcode for p in procs]
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:   # (nothing is left running, whatever happened)
            if p.is_alive():
                p.kill()
    want = expected_means()
    for rank, mine in ((0, [0, 2, 4]), (1, [1, 3])):
        res = got[rank]
        assert [e[1] for e in res["events"] if e[0] == "batch"] == mine * EPOCHS
        assert [e[1] for e in res["events"] if e[0] == "step"] == counts * EPOCHS
        assert sum(e == ("sched",) for e in res["events"]) == len(counts) * EPOCHS == res["global_step"]
        assert [np.float64(v).tobytes() for v in res["train_loss"]] == [np.float64(v).tobytes() for v in want], (rank, res["train_loss"], want)
        assert res["configured"] == [dict(total_steps=len(counts) * EPOCHS, max_grad_norm=None, accumulate=accumulate * 2, staged=True)]
        assert res["grouped"] == [True]
    assert got[1]["lines"] == [] and len(got[0]["lines"]) == EPOCHS and all(", 2 ranks" in line for line in got[0]["lines"])
