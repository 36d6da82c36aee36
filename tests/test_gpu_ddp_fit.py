"""Data-parallel ``fit`` on two ranks that share the GPU (gloo, staged collectives) against the
single-process run it has to repeat: ``python -m torch.distributed.run --nproc-per-node=2 tests/ddp_worker.py`` per case, the
twin in this process.  The D = 64, 2-layer module and the settings of tests/route_harness.py on the seeded data folder at batch
size 1: an epoch has five global batches -- two full groups and a remainder in which rank 1 owns nothing.

  A  fp32, accumulate 1 x world 2 == one process with accumulate 2, bit for bit
  B  A with dropout (seed beyond 32 bits), clipping between the run's norms, 16-mixed on fp16 operands (a live loss scale) and
     weight averaging
  C  B resumed in world 2 from its epoch-0 checkpoint == the uninterrupted world-2 run
  D  batch statistics with a trainable frontend: everything but the BatchNorms' running buffers as the twin's
  E  accumulate 2 x world 2 against one process with accumulate 4: another association, within 10 e_ref
  F  a rank that raises takes the job down
One launch per case, shared by its checks; no launch is repeated."""
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import ddp_worker as DW
import route_grads as RG
import route_harness as H
from conftest import ROOT
from dataset_reference import build_data_folder
from gpu_util import dev, report

pytestmark = pytest.mark.gpu

LAUNCH_TIMEOUT = 240
_RUNS = {}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch(case, root, out, *extra):
    """the two-rank run of ``case`` -> (return code, seconds, output); started once, never again"""
    os.makedirs(out, exist_ok=True)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={DW.WORLD}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "ddp_worker.py"), "--case", case, "--root", root,
           "--out", out, *extra]
    t0 = time.monotonic()
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=LAUNCH_TIMEOUT)
    return r.returncode, time.monotonic() - t0, r.stdout[-4000:] + r.stderr[-8000:]


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return build_data_folder(str(tmp_path_factory.mktemp("ddp_fit") / "data"))


@pytest.fixture(scope="module")
def runs(folder, tmp_path_factory):
    root = folder
    base = tmp_path_factory.mktemp("ddp_fit_runs")

    def get(name):
        """name: "A", "B", "C", "D", "E" = the world-2 launch {rc, out, ranks, ...}; "twin A" ... = the single-process run"""
        if name in _RUNS:
            if isinstance(_RUNS[name], str):
                pytest.fail(_RUNS[name])
            return _RUNS[name]
        out = str(base / name.replace(" ", "_"))
        os.makedirs(out, exist_ok=True)
        if name.startswith("twin "):
            case, record = name[5:], []
            result, pl = DW.run_fit(case, root, out, accumulate=DW.CASES[case]["accumulate"] * DW.WORLD, record=record)
            _RUNS[name] = dict(out=out, result=result, pl=pl, batches=record, root=root)
            return _RUNS[name]
        extra = ()
        if name == "C":   # B's epoch-0 checkpoint, under another numpy seed: the generator comes from the checkpoint
            extra = ("--resume", os.path.join(get("B")["out"], "epoch0.ckpt"), "--seed", "99")
        _RUNS[name] = f"the launch of case {name} failed earlier in this session"
        rc, seconds, text = launch("B" if name == "C" else name, root, out, *extra)
        assert rc == 0, f"case {name}: the two-rank run ended with status {rc} after {seconds:.0f} s\n{text}"
        ranks = [torch.load(os.path.join(out, f"rank{r}.pt"), weights_only=False) for r in range(DW.WORLD)]
        _RUNS[name] = dict(out=out, ranks=ranks, seconds=seconds, root=root)
        print(f"case {name}: two ranks, {seconds:.1f} s")
        return _RUNS[name]

    yield get
    _RUNS.clear()


def differences(a, b, path="", skip=lambda path: False):
    """the paths at which two nested results differ in a bit: tensors by their bytes, floats by their bits"""
    if skip(path):
        return []
    if isinstance(a, dict) and isinstance(b, dict):
        if set(a) != set(b):
            return [f"{path}: keys {sorted(map(str, set(a) ^ set(b)))}"]
        return [d for k in a for d in differences(a[k], b[k], f"{path}/{k}", skip)]
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        if len(a) != len(b):
            return [f"{path}: {len(a)} against {len(b)} entries"]
        return [d for i, (x, y) in enumerate(zip(a, b)) for d in differences(x, y, f"{path}/{i}", skip)]
    if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor):
        return [] if H.same_bits(a.cpu(), b.cpu()) else [f"{path}: tensors differ"]
    if isinstance(a, float) and isinstance(b, float):
        return [] if np.float64(a).tobytes() == np.float64(b).tobytes() else [f"{path}: {a!r} against {b!r}"]
    return [] if type(a) is type(b) and a == b else [f"{path}: {a!r} against {b!r}"]


def checkpoint(run, name="run.ckpt"):
    from beat_this_amd.inference import load_checkpoint

    return load_checkpoint(os.path.join(run["out"], name), "cpu")


def is_running_buffer(path):
    return path.rsplit("/", 1)[-1].endswith(RG.STAT_LEAVES) and "/state_dict/" in path


def identical_to_twin(runs, case, twin=None, skip=lambda path: False):
    """the identities of cases A and B: both ranks' results and every checkpoint against the single-process run's"""
    from beat_this_amd.train import CHECKPOINT_KEYS

    got, want = runs(case), runs(twin or f"twin {case}")
    ref = want["ranks"][0] if "ranks" in want else want["result"]
    assert len(ref["steps"]) == ref["global_step"] == ref["last_epoch"] == 6 and [s["accumulated"] for s in ref["steps"]] == [2, 2, 1] * 2
    assert len(ref["train_loss"]) == H.EPOCHS and [e for e, _ in ref["val"]] == list(range(H.EPOCHS)) and len(ref["val"][0][1]) == 7
    for rank, res in enumerate(got["ranks"]):
        diffs = differences(res, ref, f"rank {rank}", skip)
        assert not diffs, diffs[:8]
    for name in ("epoch0.ckpt", "run.ckpt"):
        a, b = checkpoint(got, name), checkpoint(want, name)
        assert set(a) == set(b) and set(CHECKPOINT_KEYS) <= set(a)
        diffs = differences(a, b, name, skip)
        assert not diffs, diffs[:8]
    return got, ref


def test_case_a_two_ranks_repeat_the_single_process_run_with_accumulate_two(runs):
    from beat_this_amd.train import CHECKPOINT_KEYS

    got, ref = identical_to_twin(runs, "A")
    final = checkpoint(got)
    assert set(final) == set(CHECKPOINT_KEYS)   # today's keys exactly
    assert final["epoch"] == H.EPOCHS - 1 and final["global_step"] == 6
    assert len(final["optimizer_states"][0]["state"]) > 20
    moved = sum(not torch.equal(v, runs("twin A")["pl"].state_dict()[k].cpu()) for k, v in checkpoint(got, "epoch0.ckpt")["state_dict"].items())
    assert moved > 20   # (the run moved the weights between the epochs)
    assert ref["numpy_pos"] == got["ranks"][1]["numpy_pos"]   # numpy's generator, on the rank that owns fewer batches too


def test_case_b_dropout_clipping_loss_scale_and_averages(runs):
    got, ref = identical_to_twin(runs, "B")
    final = checkpoint(got)
    assert {"loss_scaler", "ema_state_dict"} <= set(final) and "dropout" in final["rng"]
    assert final["rng"]["dropout"] == {"seed": DW.DROPOUT_SEED, "calls": 2 * 2 * 5 * H.EPOCHS}   # 2 L per forward, 10 forwards
    assert ref["loss_scaler"] is not None and ref["dropout"] == final["rng"]["dropout"]
    norms = [s["norm"] for s in ref["steps"] if not s["skipped"]]
    print("case B: gradient norms", [s["norm"] for s in ref["steps"]], "skipped", [s["skipped"] for s in ref["steps"]],
          "loss scale", ref["loss_scaler"]["scale"])
    limit = DW.FULL["max_grad_norm"]
    assert len(norms) >= 3 and any(n + 1e-6 > limit for n in norms) and not all(n + 1e-6 > limit for n in norms), norms
    a, b = final["ema_state_dict"], final["state_dict"]
    assert sum(not torch.equal(a[k], b[k]) for k in a) > 20   # (the averages are not the live weights)


def test_case_c_a_resumed_two_rank_run_ends_like_the_uninterrupted_one(runs):
    whole, resumed = runs("B"), runs("C")
    diffs = differences(checkpoint(resumed), checkpoint(whole), "run.ckpt")
    assert not diffs, diffs[:8]
    for rank in range(DW.WORLD):
        a, b = resumed["ranks"][rank], whole["ranks"][rank]
        assert a["train_loss"] == b["train_loss"][1:] and a["global_step"] == 6
        assert differences(a["steps"], b["steps"][3:], "steps") == []
        for key in ("state_dict", "optimizer", "loss_scaler", "dropout", "numpy_pos", "last_epoch"):
            diffs = differences(a[key], b[key], f"rank {rank}/{key}")
            assert not diffs, diffs[:8]
        assert differences(a["val"], b["val"][1:], "val") == []


def test_case_d_batch_statistics_leave_only_the_running_buffers_to_differ(runs):
    skip = lambda path: is_running_buffer(path) or "/val" in path   # (validation reads the running buffers)
    got, ref = identical_to_twin(runs, "D", skip=skip)
    r0, r1 = got["ranks"]
    diffs = differences(r0["state_dict"], r1["state_dict"], "ranks")   # after the epoch-end broadcast: the same buffers
    assert not diffs, diffs[:8]
    assert differences(r0["val"], r1["val"], "val") == []
    stats = [k for k in r0["state_dict"] if k.endswith(RG.STAT_LEAVES)]
    assert len(stats) == 15   # five BatchNorms
    twin = runs("twin D")["result"]["state_dict"]
    assert any(not torch.equal(r0["state_dict"][k], twin[k]) for k in stats)   # the stated exception is real
    trained = [k for k in r0["state_dict"] if k.startswith("model.frontend.") and not k.endswith(RG.STAT_LEAVES)]
    start = H.new_module().state_dict()
    assert sum(not torch.equal(r0["state_dict"][k], start[k].cpu()) for k in trained) > 20   # (the frontend was trained)


def test_case_e_accumulation_on_two_ranks_stays_within_the_gate_of_the_fp64_loop(runs):
    """world 2 x accumulate 2 against accumulate 4: the same steps, counts and rates exactly; the weights within 10 e_ref of the fp64
    loop over the batches the single-process run drew (e_ref: the fp32 loop against it); DESIGN.md section 26 has the figures."""
    got, twin = runs("E"), runs("twin E")
    ref = twin["result"]
    assert len(ref["steps"]) == 4 and [s["accumulated"] for s in ref["steps"]] == [4, 1] * 2
    for rank, res in enumerate(got["ranks"]):
        assert res["global_step"] == ref["global_step"] == res["last_epoch"] == 4
        assert [(s["lrs"], s["accumulated"]) for s in res["steps"]] == [(s["lrs"], s["accumulated"]) for s in ref["steps"]], rank
    assert differences(got["ranks"][0], got["ranks"][1], "ranks") == []
    assert got["ranks"][0]["numpy_pos"] == ref["numpy_pos"]
    batches, pl = twin["batches"], twin["pl"]
    assert len(batches) == 5 * H.EPOCHS
    with torch.no_grad():
        for b in batches:
            b["h"] = pl.model.frontend(b["spect"].to(dev())).cpu()
    sd = {k[len("model."):]: v.cpu() for k, v in H.new_module().state_dict().items()}
    settings = dict(n_layers=2, lr=H.LR, weight_decay=0.01, warmup=H.WARMUP, total_steps=4, accumulate=4, max_grad_norm=None,
                    pos_weights={"beat": 1, "downbeat": 1}, epochs=H.EPOCHS, batches_per_epoch=5)
    truth, yard = (RG.run(sd, batches, dt, **settings) for dt in (torch.float64, torch.float32))
    keys = RG.trainable_keys(sd)
    for e in range(H.EPOCHS):
        name = "run.ckpt" if e == H.EPOCHS - 1 else f"epoch{e}.ckpt"
        for label, run in (("two ranks x accumulate 2", got), ("one process, accumulate 4", twin)):
            params = {k: checkpoint(run, name)["state_dict"]["model." + k] for k in keys}
            RG.check(f"ddp E epoch {e}, {label}: p - p_initial", RG.displacement(params, sd),
                     RG.displacement(yard["epochs"][e]["params"], sd), RG.displacement(truth["epochs"][e]["params"], sd), report)
    a, b = checkpoint(got)["state_dict"], checkpoint(twin)["state_dict"]
    print("case E: tensors with other bits than the accumulate-4 run:", sum(not torch.equal(a[k], b[k]) for k in a), "of", len(a))


def test_case_f_a_rank_that_raises_takes_the_job_down(folder, tmp_path):
    root = folder
    out = str(tmp_path / "F")
    rc, seconds, text = launch("A", root, out, "--fail-rank", "1", "--fail-step", "1")
    print(f"case F: status {rc} after {seconds:.1f} s")
    assert rc != 0, text
    assert "told to fail in optimiser step 1" in text
    assert seconds < LAUNCH_TIMEOUT / 2, f"the job took {seconds:.0f} s to come down"
    assert not os.path.exists(os.path.join(out, "run.ckpt")) and not os.path.exists(os.path.join(out, "rank0.pt"))


def test_the_command_line_on_two_ranks_writes_the_single_process_checkpoint(folder, tmp_path):
    """``python -m beat_this_amd.train --gpus 2 --share-gpu`` launches itself under torch.distributed.run and leaves, bit for bit, the
    checkpoint of ``--gpus 1 --accumulate-grad-batches 2``; only rank 0 prints the run's lines"""
    from beat_this_amd.inference import load_checkpoint

    root = folder
    base = [sys.executable, "-m", "beat_this_amd.train", "--data-dir", root, "--max-epochs", "1", "--batch-size", "1", "--train-length", "150",
            "--n-layers", "2", "--transformer-dim", "64", "--warmup-steps", "2", "--no-tempo-augmentation", "--no-pitch-augmentation",
            "--no-mask-augmentation", "--val-frequency", "1", "--dropout", "--seed", "7"]
    outs = {}
    for name, flags in (("two", ["--gpus", "2", "--share-gpu", "--accumulate-grad-batches", "1"]), ("one", ["--accumulate-grad-batches", "2"])):
        path = str(tmp_path / f"{name}.ckpt")
        r = subprocess.run(base + ["--output", path] + flags, cwd=ROOT, capture_output=True, text=True, timeout=LAUNCH_TIMEOUT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
        outs[name] = (load_checkpoint(path, "cpu"), r.stdout)
    diffs = differences(outs["two"][0], outs["one"][0], "checkpoint")
    assert not diffs, diffs[:8]
    for text in (outs["two"][1], outs["one"][1]):
        assert text.count("Starting a run with:") == 1 and text.count("epoch 0: train_loss") == 1 and text.count("wrote ") == 1
    assert "3 steps" in outs["two"][1] and "2 ranks" in outs["two"][1]
