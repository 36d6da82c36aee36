"""Training batches on the MI355X (csrc/data.hip): bt_train_batch against its host twin bit for bit -- frame counts on either
side of the kernel's 64-frame block, batches of 1 / 3 / 8, float16 and float32 on both sides, the resident and the staged
store -- with the outputs poisoned and guarded; the block-boundary cases against the numpy restatement; ``augment_mask_`` on a
CUDA tensor; a whole piece; and one batch through the model and the losses."""
import json
import os

import numpy as np
import pytest
import torch

import dataset_reference as R
from gpu_util import Guarded, assert_intact, dev

pytestmark = pytest.mark.gpu

LENGTHS = (1, 63, 64, 65, 100, 1500)   # BT_TRAIN_FRAME_BLOCK = 64
BATCHES = (1, 3, 8)
PIECES = {"p1701": 1701, "p1500": 1500, "p1501": 1501, "p97": 97, "p640": 640, "p64": 64, "p65": 65, "p2000": 2000}


def test_the_frame_block_is_64():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "beat_this_amd.h")).read()
    assert "#define BT_TRAIN_FRAME_BLOCK 64" in header


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """two datasets of seeded spectrograms with their row number in column 0: "h" a float16 bundle, "s" float32 files"""
    root = str(tmp_path_factory.mktemp("gpu_dataset"))
    rng = np.random.default_rng(77)
    bundle = {}
    for dataset, dtype in (("h", np.float16), ("s", np.float32)):
        ann = os.path.join(root, "annotations", dataset)
        os.makedirs(os.path.join(ann, "annotations", "beats"))
        json.dump({"has_downbeats": True}, open(os.path.join(ann, "info.json"), "w"))
        for piece, frames in PIECES.items():
            times = np.cumsum(rng.uniform(0.2, 0.7, frames // 15 + 3)) - 0.15
            with open(os.path.join(ann, "annotations", "beats", piece + ".beats"), "w") as f:
                f.write("".join(f"{t:.5f}\t{i % 3 + 1}\n" for i, t in enumerate(times[times > 0])))
            a = R.spectrogram(rng, frames).astype(dtype)
            if dtype == np.float32:
                a[:, 1:] += rng.standard_normal((frames, 127)).astype(np.float32) * 1e-3   # (not float16 values)
                os.makedirs(os.path.join(root, "audio", "spectrograms", dataset, piece))
                np.save(os.path.join(root, "audio", "spectrograms", dataset, piece, "track.npy"), a)
            else:
                bundle[f"{piece}/track"] = a
    np.savez(os.path.join(root, "audio", "spectrograms", "h.npz"), **bundle)
    return root


def mask_for(L):
    """the train.py mask augmentation, its lengths cut to what fits an excerpt of L frames and the shortest piece (64)"""
    longest = min(2.0, max(min(L, 64) - 2, 0) / R.FPS)
    return dict(R.MASK_PERMUTE, min_len=min(0.1, longest), max_len=longest)


def make(folder, dataset, L, resident):
    from beat_this_amd.dataset import BeatTrackingDataset

    aug = {"mask": mask_for(L)} if L is not None else {}
    return BeatTrackingDataset([f"{dataset}/{p}" for p in PIECES], folder, spect_fps=R.FPS, train_length=L, augmentations=aug,
                               device=dev(), resident=resident)


def host_batch(ds, indices, seed):
    np.random.seed(seed)
    return [ds[i] for i in indices]


def assert_batch_equals_items(batch, items, out_dtype):
    torch.cuda.synchronize()
    for k in ("truth_beat", "truth_downbeat", "padding_mask", "downbeat_mask"):
        assert batch[k].dtype == torch.bool
        want = np.stack([np.asarray(it[k]) for it in items])
        assert np.array_equal(batch[k].cpu().numpy(), want), k
    with np.errstate(over="ignore"):
        want = np.stack([it["spect"] for it in items]).astype(out_dtype)   # (float16 -> float32 is exact; the other way
    got = batch["spect"].cpu().numpy()                                      # rounds as numpy does: tests/test_dataset.py)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    for k in ("spect_path", "dataset", "start_frame", "truth_orig_beat", "truth_orig_downbeat"):
        assert isinstance(batch[k], list) and batch[k] == [it[k] for it in items], k


@pytest.mark.parametrize("L", LENGTHS)
def test_batches_equal_the_host_twin(folder, L):
    """ds.batch against [ds[i]] under the same seed: every batch size, both stores, both output types, resident and staged"""
    rng = np.random.default_rng(L)
    for dataset in ("h", "s"):
        for resident in (True, False):
            ds = make(folder, dataset, L, resident)
            for B in BATCHES:
                indices = rng.integers(0, len(ds), B).tolist()
                for out_dtype in (torch.float32, torch.float16):
                    seed = int(rng.integers(0, 1 << 30))
                    items = host_batch(ds, indices, seed)
                    np.random.seed(seed)
                    batch = ds.batch(indices, spect_dtype=out_dtype)
                    assert batch["spect"].shape == (B, L, 128) and ds.is_resident == resident
                    assert_batch_equals_items(batch, items, np.float32 if out_dtype == torch.float32 else np.float16)


def random_plans(rng, B, L, rows, n_ann):
    from beat_this_amd.dataset import plan as P

    plans, times, values = [], [], []
    for b in range(B):
        n = L if rng.random() < 0.4 else int(rng.integers(0, L + 1))
        start = int(rng.integers(0, rows - n + 1))
        ops = [P.MaskOp(*op) for op in R.random_ops(rng, n)] if n > 1 else []
        t = np.sort(rng.uniform((start - 20) / R.FPS, (start + n + 20) / R.FPS, int(rng.integers(0, n_ann))))
        first = sum(len(x) for x in times)
        plans.append(P.ItemPlan(start, n, start, ops, first, first + t.size, bool(b % 2)))
        times.append(t)
        values.append(rng.integers(1, 4, t.size).astype(np.int32))
    return plans, np.concatenate(times), np.concatenate(values)


def device_run(store, plans, L, time, value, spect_dtype):
    """bt_train_batch into guarded buffers poisoned with 0xFF -> numpy dict of the five outputs"""
    from beat_this_amd.dataset import plan as P

    B, d = len(plans), dev()
    shapes = {"spect": ((B, L, 128), spect_dtype), "truth_beat": ((B, L), torch.uint8), "truth_downbeat": ((B, L), torch.uint8),
              "padding_mask": ((B, L), torch.uint8), "downbeat_mask": ((B,), torch.uint8)}
    bufs = {k: Guarded(shape, dtype).fill(0xFF) for k, (shape, dtype) in shapes.items()}
    d_store = torch.from_numpy(store).to(d)
    d_time, d_value = torch.from_numpy(time).to(d), torch.from_numpy(value).to(d)
    P.run_device(d, d_store, store.shape[0], P.F16 if store.dtype == np.float16 else P.F32, plans, L, d_time, d_value, time.size,
                 R.FPS, {k: g.t for k, g in bufs.items()})
    torch.cuda.synchronize()
    assert_intact(*bufs.items())
    return {k: g.t.cpu().numpy() for k, g in bufs.items()}


def assert_equal_host(got, store, plans, L, time, value, spect_np_dtype):
    from beat_this_amd.dataset import plan as P

    want = P.run_host(store, plans, L, time, value, R.FPS, spect_dtype=spect_np_dtype)
    for k, w in want.items():
        assert got[k].tobytes() == w.tobytes(), k   # (0 / 1 bytes: the poison 0xFF is gone from every byte)
    return want


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("L", LENGTHS)
def test_random_plans_guarded_and_poisoned(L, B):
    """overlapping zero / permute operations, excerpts shorter than the batch (also empty ones), annotations around both ends:
    every byte of the poisoned outputs is written, none outside them, the bits are the host twin's"""
    rng = np.random.default_rng(1000 * L + B)
    for store_dtype, spect_dtype in ((np.float16, torch.float32), (np.float16, torch.float16), (np.float32, torch.float32),
                                     (np.float32, torch.float16)):
        rows = 1700
        store = (rng.standard_normal((rows, 128)) * 3).astype(store_dtype)
        store[:, 0] = np.arange(rows)
        plans, time, value = random_plans(rng, B, L, rows, 40)
        got = device_run(store, plans, L, time, value, spect_dtype)
        assert_equal_host(got, store, plans, L, time, value, np.float32 if spect_dtype == torch.float32 else np.float16)


def test_block_boundaries_against_the_restatement():
    """L = 200 (blocks 0-63, 64-127, 128-191, 192-199): padding that begins inside a block, an operation and a part boundary
    that straddle a block boundary, annotations on the first and last frame of a block, an item without operations, an item
    without annotations; each item alone has the bits it has inside the batch"""
    from beat_this_amd.dataset import plan as P

    rng = np.random.default_rng(3)
    store = rng.standard_normal((900, 128)).astype(np.float16)
    store[:, 0] = np.arange(900)
    L = 200
    straddle = [(50, 40, 1, ((0, 26, 14), (14, 0, 26))),        # frames 50-89: the parts meet at frame 64
                (60, 8, 1, ((0, 5, 3), (3, 0, 5))),             # 60-67 across the boundary, over the first one
                (120, 16, 0, ()),                               # zeros over 120-135
                (100, 60, 1, ((0, 30, 30), (30, 0, 30)))]       # maps 100-159 through the zeroed stretch
    frames = [0, 63, 64, 127, 128, 191, 192, 199]
    items = [  # (first row, n, ops, annotated frames relative to the excerpt)
        (100, 200, straddle, frames),
        (300, 70, [], frames),                                  # padding begins at 70, inside block 1
        (0, 200, straddle[:1], []),                             # no annotations
        (650, 129, [(0, 129, 1, ((0, 128, 1), (1, 0, 128)))], [127, 128, 129, 130]),   # 129, 130: outside the excerpt
        (10, 64, [(0, 64, 0, ())], [63, 64]),                   # a whole block zeroed, padding from the boundary on
    ]
    plans, times, values = [], [], []
    for row, n, ops, fr in items:
        t = np.array([(row + f) / R.FPS for f in fr])
        first = sum(len(x) for x in times)
        plans.append(P.ItemPlan(row, n, row, [P.MaskOp(*op) for op in ops], first, first + t.size, True))
        times.append(t)
        values.append(np.array([1, 2] * 4, np.int32)[:t.size])
    time, value = np.concatenate(times), np.concatenate(values)
    got = device_run(store, plans, L, time, value, torch.float16)
    assert_equal_host(got, store, plans, L, time, value, np.float16)
    for b, (row, n, ops, fr) in enumerate(items):
        spect, beat, down, pad = R.item(store, row, n, L, ops, times[b], values[b])
        assert got["spect"][b].tobytes() == spect.tobytes(), b
        assert np.array_equal(got["truth_beat"][b], beat) and np.array_equal(got["truth_downbeat"][b], down), b
        assert np.array_equal(got["padding_mask"][b], pad) and np.flatnonzero(beat).tolist() == [f for f in fr if f < n], b
        alone = device_run(store, [plans[b]], L, time, value, torch.float16)
        for k in got:
            assert alone[k][0].tobytes() == got[k][b].tobytes(), (b, k)
    assert got["spect"][2][63, 0] == 50 + 26 + 13 and got["spect"][2][64, 0] == 50   # the parts' seam, by hand


def test_optional_outputs_and_given_buffers(folder):
    """only the outputs that are given are written; ds.batch fills the tensors passed as ``out``"""
    from beat_this_amd.dataset import plan as P

    rng = np.random.default_rng(8)
    store = rng.standard_normal((300, 128)).astype(np.float16)
    plans, time, value = random_plans(rng, 3, 100, 300, 20)
    d = dev()
    want = P.run_host(store, plans, 100, time, value, R.FPS)
    for keep in ("spect", "truth_downbeat", "padding_mask"):
        g = Guarded((3, 100, 128) if keep == "spect" else (3, 100), torch.float16 if keep == "spect" else torch.uint8).fill(0xFF)
        P.run_device(d, torch.from_numpy(store).to(d), 300, P.F16, plans, 100, torch.from_numpy(time).to(d),
                     torch.from_numpy(value).to(d), time.size, R.FPS, {keep: g.t})
        torch.cuda.synchronize()
        assert_intact((keep, g))
        assert g.t.cpu().numpy().tobytes() == want[keep].tobytes()
    ds = make(folder, "h", 100, True)
    out = {"spect": torch.empty((2, 100, 128), dtype=torch.float16, device=d),
           "truth_beat": torch.empty((2, 100), dtype=torch.bool, device=d)}
    items = host_batch(ds, [0, 3], 5)
    np.random.seed(5)
    batch = ds.batch([0, 3], out=out)
    assert batch["spect"] is out["spect"] and batch["truth_beat"] is out["truth_beat"]
    assert_batch_equals_items(batch, items, np.float16)
    with pytest.raises(ValueError):
        ds.batch([0, 3], out={"spect": torch.empty((2, 99, 128), dtype=torch.float16, device=d)})


def test_augment_mask_on_a_cuda_tensor_equals_the_numpy_call():
    from beat_this_amd.dataset.augment import augment_mask_

    rng = np.random.default_rng(4)
    for seed, (dtype, params) in enumerate(((np.float16, R.MASK_PERMUTE), (np.float32, R.MASK_PERMUTE), (np.float16, R.MASK_ZERO),
                                            (np.float32, R.MASK_TINY))):
        x = rng.standard_normal((1500 if seed < 2 else 333, 128)).astype(dtype)
        np.random.seed(seed)
        want = augment_mask_(x.copy(), {"mask": params}, R.FPS)
        t = torch.from_numpy(x).to(dev())
        np.random.seed(seed)
        assert augment_mask_(t, {"mask": params}, R.FPS) is t
        assert t.cpu().numpy().tobytes() == want.tobytes() and not np.array_equal(want, x)


def test_a_whole_piece_of_1701_frames(folder):
    for resident in (True, False):
        ds = make(folder, "h", None, resident)
        assert ds.get_frame_count(0) == 1701
        items = host_batch(ds, [0], 0)
        batch = ds.batch([0])
        assert batch["spect"].shape == (1, 1701, 128) and bool(batch["padding_mask"].all())
        assert_batch_equals_items(batch, items, np.float32)
        assert np.array_equal(batch["spect"][0, :, 0].cpu().numpy(), np.arange(1701))
    with pytest.raises(ValueError, match="same number of frames"):
        ds.batch([0, 1])


def test_a_batch_through_the_model_and_the_losses(folder):
    """B = 2, T = 1500, small0 with random weights: batch -> BeatThis -> the shift-tolerant losses with the reference's masks;
    finite, and the same bits as the same computation fed from the host twin's items"""
    from beat_this_amd import weights as W
    from beat_this_amd.model import BeatThis
    from beat_this_amd.model.loss import ShiftTolerantBCELoss

    hp = W.resolve_hparams("small0")
    model = BeatThis(**{k: hp[k] for k in ("spect_dim", "transformer_dim", "ff_mult", "n_layers", "head_dim", "stem_dim")})
    model.load_state_dict(W.random_state_dict("small0", seed=2, style="lively"))
    model = model.to(dev())
    ds = make(folder, "h", 1500, True)
    loss = ShiftTolerantBCELoss(pos_weight=4).to(dev())

    def losses(batch):
        with torch.no_grad():
            out = model(batch["spect"])
        pad = batch["padding_mask"]
        return (float(loss(out["beat"], batch["truth_beat"].float(), pad)),
                float(loss(out["downbeat"], batch["truth_downbeat"].float(), pad * batch["downbeat_mask"][:, None])))

    items = host_batch(ds, [3, 7], 12)   # (97 frames: mostly padding; 2000 frames: a random excerpt)
    np.random.seed(12)
    got = losses(ds.batch([3, 7]))
    collated = torch.utils.data.default_collate(items)
    host = {k: (v.to(dev()) if isinstance(v, torch.Tensor) else v) for k, v in collated.items()}
    host["spect"] = host["spect"].float()
    want = losses(host)
    assert all(np.isfinite(got)) and got == want and got[0] > 0
