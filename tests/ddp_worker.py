"""One rank of the two-rank runs of tests/test_gpu_ddp_fit.py (a helper, not a test file): started by torch.distributed.run, all
ranks on cuda:0, a gloo group with staged collectives.  The cases and what a run leaves are defined here, so that the test
process builds its single-process twins from the same settings.

    python -m torch.distributed.run --nproc-per-node=2 tests/ddp_worker.py --case B --root DATA --out DIR [--resume CKPT]
                                                                           [--seed N] [--fail-rank R --fail-step S]

Rank r writes DIR/rank<r>.pt (``outcome``); rank 0's ``fit`` writes DIR/run.ckpt and keeps every epoch's as DIR/epoch<e>.ckpt."""
import argparse
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for path in (HERE, os.path.dirname(HERE)):
    if path not in sys.path:
        sys.path.insert(0, path)

import numpy as np   # noqa: E402
import torch   # noqa: E402

DROPOUT_SEED = 0x5EED_0000_0000_0001   # (beyond 32 bits)
# the settings of a case: ``fit``'s keywords (accumulate: per rank, world 2), and what is done to the module before
FULL = dict(max_grad_norm=0.68, precision="16-mixed", mixed_operand="fp16", ema_decay=0.5)
CASES = {
    "A": dict(accumulate=1, fit={}, dropout=False),
    "B": dict(accumulate=1, fit=FULL, dropout=True),
    "D": dict(accumulate=1, fit=dict(train_frontend=True, batch_statistics=True), dropout=False),
    "E": dict(accumulate=2, fit={}, dropout=False),
}
WORLD = 2


def new_module(case):
    import route_harness as H

    pl = H.new_module()
    if CASES[case]["dropout"]:
        pl.model.enable_dropout(DROPOUT_SEED)
    return pl


def new_datamodule(root):
    """batch size 1: an epoch of five global batches, two full groups and a remainder in which rank 1 owns nothing"""
    import route_harness as H
    from beat_this_amd.dataset import BeatDataModule

    return BeatDataModule(root, batch_size=1, train_length=150, augmentations={}, device=H.dev())


def observe_steps(pl, steps, fail_step=None, configured=None):
    """every optimiser step leaves its groups' rates (as they are BEFORE the step), its count and, with clipping, its norm in
    ``steps``; ``fail_step``: the step with that number raises instead; ``configured``: a list that receives the arguments of
    every ``configure_optimizers`` call.  (Shared with tests/test_gpu_finetune_trajectory.py, like the loader below.)"""
    configure = pl.configure_optimizers

    def configure_optimizers(total_steps, **kw):
        conf = configure(total_steps, **kw)
        if configured is not None:
            configured.append(dict(total_steps=total_steps, **kw))
        opt = conf["optimizer"]
        step = opt.step

        def recording_step(*args, **kwargs):
            if fail_step is not None and len(steps) == fail_step:
                raise RuntimeError(f"ddp_worker: told to fail in optimiser step {fail_step}")
            lrs = [g["lr"] for g in opt.param_groups]
            result = step(*args, **kwargs)
            steps.append(dict(lrs=lrs, accumulated=kwargs.get("accumulated"), skipped=bool(opt.last_step_skipped),
                              norm=opt.last_grad_norm() if opt.max_grad_norm is not None else None))
            return result

        recording_step._wrapped_by_lr_sched = True   # (the scheduler's own wrapper is inside: it still sees every step)
        opt.step = recording_step
        return conf

    pl.configure_optimizers = configure_optimizers


TENSORS = ("spect", "truth_beat", "truth_downbeat", "padding_mask", "downbeat_mask")


class RecordingLoader:
    """the training loader, every batch it yields cloned to the CPU on the way"""

    def __init__(self, loader, seen):
        self.loader, self.seen = loader, seen

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            self.seen.append({k: batch[k].detach().cpu().clone() for k in TENSORS})
            yield batch


def run_fit(case, root, out, seed=0, resume=None, accumulate=None, process_group=None, fail_step=None, keep_epochs=True, record=None,
            staged=True):
    """one ``fit`` of ``case`` for route_harness.EPOCHS epochs -> (``outcome``, the module); ``accumulate``: overrides the case's
    (the single-process twins); the epochs' checkpoints are kept beside ``out``/run.ckpt; ``record``: a list that receives the
    training batches of a single-process run; ``staged``: the collectives of a run with a group go through host copies"""
    import route_harness as H
    from beat_this_amd.train import fit

    c = CASES[case]
    pl, dm, steps = new_module(case), new_datamodule(root), []
    observe_steps(pl, steps, fail_step)
    if record is not None:
        dm.setup("fit")
        train_dataloader = dm.train_dataloader
        dm.train_dataloader = lambda: RecordingLoader(train_dataloader(), record)
    ck = os.path.join(out, "run.ckpt")

    def log(line):   # (called after the epoch's checkpoint is written; in a group, on rank 0 only)
        if keep_epochs and line.startswith("epoch "):
            shutil.copy(ck, os.path.join(out, f"epoch{int(line.split()[1].rstrip(':'))}.ckpt"))

    extra = {} if process_group is None else dict(process_group=process_group, staged=staged)
    np.random.seed(seed)
    history = fit(pl, dm, H.EPOCHS, accumulate_grad_batches=c["accumulate"] if accumulate is None else accumulate, val_frequency=1,
                  checkpoint_path=ck, resume=resume, log=log, **c["fit"], **extra)
    return outcome(pl, history, steps), pl


def outcome(pl, history, steps):
    opt, scaler = history["optimizer"], history["loss_scaler"]
    return {"train_loss": list(history["train_loss"]), "val": list(history["val"]), "epoch": history["epoch"],
            "global_step": history["global_step"], "last_epoch": history["scheduler"].last_epoch, "steps": steps,
            "loss_scaler": None if scaler is None else scaler.state_dict(), "dropout": pl.model.dropout_state(),
            "numpy_pos": int(np.random.get_state()[2]),
            "state_dict": {k: v.detach().cpu() for k, v in pl.state_dict().items()},
            "optimizer": _cpu(opt.state_dict())}


def _cpu(obj):
    if isinstance(obj, torch.Tensor):
        return obj.detach().cpu()
    if isinstance(obj, dict):
        return {k: _cpu(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_cpu(v) for v in obj)
    return obj


def main():
    from datetime import timedelta

    import torch.distributed as dist
    from beat_this_amd.train import run_rank

    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True, choices=sorted(CASES))
    ap.add_argument("--root", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--resume", default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--fail-rank", type=int, default=-1)
    ap.add_argument("--fail-step", type=int, default=0)
    args = ap.parse_args()

    def body():
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", timeout=timedelta(seconds=120))
        rank = dist.get_rank()
        assert dist.get_world_size() == WORLD
        result, _ = run_fit(args.case, args.root, args.out, seed=args.seed, resume=args.resume, process_group=dist.group.WORLD,
                            fail_step=args.fail_step if rank == args.fail_rank else None)
        torch.save(result, os.path.join(args.out, f"rank{rank}.pt"))
        dist.barrier()
        dist.destroy_process_group()
        return 0

    return run_rank(body)   # (a rank that raises takes the job down at once: beat_this_amd.train's rule)


if __name__ == "__main__":
    sys.exit(main())
