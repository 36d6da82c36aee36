"""beat_this_amd.dataset on the CPU, through the library's host twin (bt_train_batch_host, csrc/data.hip): items against the
reference's own dataset.py / augment.py recorded over the seeded synthetic data folder of tests/dataset_reference.py
(tests/golden/dataset_reference.npz, tools/make_dataset_golden.py), random plans against the numpy restatement, the rounding
and range edges of the framewise targets, the errors, and the data module's splits."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import dataset_reference as R
from conftest import GOLDEN

Z = np.load(os.path.join(GOLDEN, "dataset_reference.npz"))
META = json.loads(str(Z["meta"]))


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return R.build_data_folder(str(tmp_path_factory.mktemp("dataset")))


def make(folder, items, **kwargs):
    from beat_this_amd.dataset import BeatTrackingDataset

    return BeatTrackingDataset(items, folder, spect_fps=R.FPS, **kwargs)


# ---- the reference's items ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_items_equal_the_reference_bit_for_bit(folder, name):
    items, kwargs, index = R.CASES[name]
    ds = make(folder, items, **kwargs)
    for seed in R.SEEDS:
        key = f"{name}.{seed}"
        want = META["cases"][key]
        np.random.seed(seed)
        got = ds[index]
        assert list(got) == ["spect", "spect_path", "dataset", "start_frame", "truth_beat", "truth_downbeat", "downbeat_mask",
                             "padding_mask", "truth_orig_beat", "truth_orig_downbeat"]
        assert got["start_frame"] == want["start_frame"] and got["spect_path"] == want["spect_path"], key
        assert got["dataset"] == want["dataset"], key
        assert isinstance(got["downbeat_mask"], torch.Tensor) and bool(got["downbeat_mask"]) == want["downbeat_mask"]
        for k in ("truth_beat", "truth_downbeat", "padding_mask"):
            assert got[k].dtype == np.bool_ and np.array_equal(got[k], Z[f"{key}.{k}"]), (key, k)
        for k in ("truth_orig_beat", "truth_orig_downbeat"):
            assert isinstance(got[k], bytes) and got[k] == Z[f"{key}.{k}"].tobytes(), (key, k)
        spect = got["spect"]
        assert str(spect.dtype) == want["spect_dtype"] and list(spect.shape) == want["spect_shape"], key
        assert np.array_equal(spect[:, 0], Z[f"{key}.col0"]), key
        assert hashlib.sha256(np.ascontiguousarray(spect).tobytes()).hexdigest() == want["sha256"], key
        assert spect.flags.writeable


def test_the_recorded_cases_cover_what_they_are_named_for():
    """(the golden itself: augmented member names, clamped part counts, padding, stretched annotations are in it)"""
    paths = {k: v["spect_path"] for k, v in META["cases"].items()}
    assert any("_ps" in p for k, p in paths.items() if k.startswith("pitch."))
    assert any("_ts" in p for k, p in paths.items() if k.startswith("tempo."))
    assert any("_ps-" in p or "_ts-" in p for p in paths.values())
    assert not Z["shorter_padded.0.padding_mask"].all() and Z["shorter_padded.0.padding_mask"][:97].all()
    assert META["cases"]["whole_piece.0"]["spect_shape"] == [400, 128]
    assert META["cases"]["deterministic.0"]["start_frame"] == 125 and META["cases"]["deterministic_plus1.0"]["start_frame"] == 0
    assert META["cases"]["rwc_stem.0"]["dataset"] == "rwc_jazz" and not META["cases"]["one_column_no_downbeats.0"]["downbeat_mask"]
    col0 = Z["mask_permute.0.col0"].astype(np.int64)
    assert (np.diff(col0) != 1).any() and sorted(col0) == list(range(col0.min(), col0.min() + 150))
    assert (Z["mask_zero.0.col0"] == 0).sum() > 1


def test_a_dataloader_collates_the_items(folder):
    ds = make(folder, R.ALPHA, train_length=R.TRAIN_LENGTH, augmentations={"mask": R.MASK_SHORT})
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=4)))
    assert batch["spect"].shape == (4, R.TRAIN_LENGTH, 128) and batch["spect"].dtype == torch.float16
    assert batch["truth_beat"].dtype == torch.bool and batch["padding_mask"][3, 97:].sum() == 0
    assert ds.get_frame_count(3) == 97 and ds.get_beat_count(0) == len(ds.items[0]["beat_time"])
    assert ds.get_downbeat_count(0) == (ds.items[0]["beat_value"] == 1).sum() and len(ds[[0, 1]]) == 2


# ---- random plans against the numpy restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("store_dtype, spect_dtype", [(np.float16, np.float16), (np.float16, np.float32), (np.float32, np.float32),
                                                      (np.float32, np.float16)])
def test_random_plans_equal_the_numpy_restatement(store_dtype, spect_dtype):
    from beat_this_amd.dataset import plan as P

    rng = np.random.default_rng(11)
    for case in range(40):
        rows = int(rng.integers(2, 700))
        store = (rng.standard_normal((rows, 128)) * 10.0 ** rng.integers(-9, 5)).astype(store_dtype)
        store[:, 0] = np.arange(rows) % 2048
        if case % 5 == 0:   # values a conversion must get right: subnormal halves, ties, the overflow edge, infinities, NaN
            with np.errstate(over="ignore"):
                store[0, 1:9] = np.array([6e-8, 2.98e-8, 2.9803e-8, 65519.9, 65520.0, np.inf, -np.inf, np.nan], store_dtype)
        n = int(rng.integers(1, rows + 1))
        start = int(rng.integers(0, rows - n + 1))
        L = n + int(rng.integers(0, 70))
        ops = R.random_ops(rng, n) if n > 1 else []
        time = np.sort(rng.uniform(-1.0, (rows + 50) / 50, int(rng.integers(0, 60))))
        value = rng.integers(1, 5, time.size).astype(np.int32)
        plan = P.ItemPlan(start, n, start, [P.MaskOp(*op) for op in ops], 0, time.size, True)
        got = P.run_host(store, [plan], L, time, value, 50, spect_dtype=spect_dtype)
        with np.errstate(over="ignore"):
            want = R.item(store, start, n, L, ops, time, value, 50, spect_dtype)
        assert got["spect"][0].tobytes() == want[0].tobytes(), case
        for k, w in zip(("truth_beat", "truth_downbeat", "padding_mask"), want[1:]):
            assert np.array_equal(got[k][0], w), (case, k)
        assert got["downbeat_mask"].tolist() == [True]


def test_float32_to_float16_rounds_like_numpy_on_every_exponent():
    from beat_this_amd.dataset import plan as P

    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2 ** 32, 64 * 128 * 16, dtype=np.uint64).astype(np.uint32)
    bits[:4096] = (bits[:4096] & 0x807FE000) | (rng.integers(100, 145, 4096).astype(np.uint32) << 23) | 0x1000   # exact ties
    store = bits.view(np.float32).reshape(-1, 128)
    n = store.shape[0]
    got = P.run_host(store, [P.ItemPlan(0, n, 0, [], 0, 0, False)], n, np.zeros(0), np.zeros(0, np.int32), 50,
                     spect_dtype=np.float16, want_targets=False)["spect"][0]
    with np.errstate(over="ignore", invalid="ignore"):
        want = store.astype(np.float16)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint16)[~nan], want.view(np.uint16)[~nan])
    back = P.run_host(want, [P.ItemPlan(0, n, 0, [], 0, 0, False)], n, np.zeros(0), np.zeros(0, np.int32), 50,
                      spect_dtype=np.float32, want_targets=False)["spect"][0]
    assert np.array_equal(back.view(np.uint32)[~nan], want.astype(np.float32).view(np.uint32)[~nan])


def targets(time, value, start, n, L=None):
    """-> (beat frames, downbeat frames) of the excerpt [start, start + n) padded to L, from the host twin; checked against
    the restatement on the way"""
    from beat_this_amd.dataset import plan as P

    time, L = np.asarray(time, np.float64), L or n
    store = np.zeros((start + n, 128), np.float16)
    r = P.run_host(store, [P.ItemPlan(start, n, start, [], 0, time.size, True)], L, time, np.asarray(value, np.int32), 50,
                   want_spect=False)
    _, beat, down, pad = R.item(store, start, n, L, [], time, np.asarray(value, np.int32), 50)
    assert np.array_equal(r["truth_beat"][0], beat) and np.array_equal(r["truth_downbeat"][0], down)
    assert np.array_equal(r["padding_mask"][0], pad)
    return np.flatnonzero(beat).tolist(), np.flatnonzero(down).tolist()


def test_the_edges_of_the_framewise_targets():
    # exactly on a half frame: ties go to the even frame (np.round), 0.25 s * 50 = 12.5 -> 12, 0.27 -> 13.5 -> 14
    assert targets([0.25, 0.27], [1, 2], 0, 100) == ([12, 14], [12])
    assert 0.25 * 50 == 12.5 and 0.27 * 50 == 13.5
    # an annotation in front of the excerpt that rounds up into its frame 0: 1.991 s * 50 = 99.55 -> 100 = start
    assert targets([1.97, 1.991, 3.0], [2, 1, 1], 100, 40) == ([0], [0])
    # one that rounds down to just before it stays out: 1.989 * 50 = 99.45 -> 99
    assert targets([1.989], [1], 100, 40) == ([], [])
    # an annotation exactly on the end frame is excluded, the one before it is kept
    assert targets([2.78, 2.80], [1, 1], 100, 40) == ([39], [39])
    # padding never carries a target
    assert targets([0.5, 1.0], [1, 1], 0, 40, 64) == ([25], [25])
    # no annotation in range, no annotation at all
    assert targets([0.1, 9.0], [1, 1], 100, 40) == ([], [])
    assert targets([], [], 0, 40) == ([], [])
    # two annotations on one frame; a downbeat needs the value 1
    assert targets([0.50, 0.505, 0.7], [2, 1, 3], 0, 64) == ([25, 35], [25])


# ---- errors -------------------------------------------------------------------------------------------------------------------------
def test_a_mask_not_shorter_than_the_excerpt_raises(folder):
    from beat_this_amd.dataset.augment import augment_mask_

    ds = make(folder, R.ALPHA, train_length=R.TRAIN_LENGTH, augmentations={"mask": dict(R.MASK_PERMUTE, min_len=2, max_len=2)})
    np.random.seed(0)
    with pytest.raises(ValueError):
        ds[3]   # 97 frames, masks of 100
    with pytest.raises(ValueError):
        augment_mask_(np.zeros((100, 128), np.float16), {"mask": dict(R.MASK_ZERO, min_len=2, max_len=2)}, 50)
    with pytest.raises(ValueError, match="Unsupported mask operation"):
        augment_mask_(np.zeros((200, 128), np.float16), {"mask": dict(R.MASK_ZERO, kind="blur")}, 50)
    with pytest.raises(ValueError, match="128"):
        augment_mask_(np.zeros((200, 64), np.float16), {"mask": R.MASK_ZERO}, 50)


def write_piece(root, dataset, piece, spect, beats, has_downbeats=True, loose=True):
    ann = os.path.join(root, "annotations", dataset)
    os.makedirs(os.path.join(ann, "annotations", "beats"), exist_ok=True)
    json.dump({"has_downbeats": has_downbeats}, open(os.path.join(ann, "info.json"), "w"))
    with open(os.path.join(ann, "annotations", "beats", piece + ".beats"), "w") as f:
        f.write("".join(f"{t}\t{v}\n" for t, v in beats))
    os.makedirs(os.path.join(root, "audio", "spectrograms", dataset, piece), exist_ok=True)
    np.save(os.path.join(root, "audio", "spectrograms", dataset, piece, "track.npy"), spect)


def test_what_the_store_refuses(tmp_path):
    root = str(tmp_path)
    beats = [(0.5, 1), (1.0, 2), (1.5, 3)]
    write_piece(root, "d", "half", np.zeros((60, 128), np.float16), beats)
    write_piece(root, "d", "single", np.zeros((60, 128), np.float32), beats)
    write_piece(root, "d", "double", np.zeros((60, 128), np.float64), beats)
    write_piece(root, "d", "narrow", np.zeros((60, 81), np.float16), beats)
    write_piece(root, "d", "unsorted", np.zeros((60, 128), np.float16), [(0.5, 1), (1.5, 2), (1.0, 3)])
    assert len(make(root, ["d/half"])) == 1 and len(make(root, ["d/single"])) == 1
    with pytest.raises(ValueError, match="mixed dtypes"):
        make(root, ["d/half", "d/single"])
    with pytest.raises(ValueError, match="float16 or float32"):
        make(root, ["d/double"])
    with pytest.raises(ValueError, match="128"):
        make(root, ["d/narrow"])
    with pytest.raises(ValueError, match="ascending"):
        make(root, ["d/unsorted"])
    with pytest.raises(ValueError, match="Unsupported augmentations"):
        make(root, ["d/half"], augmentations={"noise": {}})
    from beat_this_amd.dataset import BeatDataModule

    with pytest.raises(ValueError, match="Unsupported augmentations"):
        BeatDataModule(root, augmentations={"pitch": R.PITCH, "reverb": {}})
    with pytest.raises(RuntimeError, match="ROCm GPUs only"):
        make(root, ["d/half"], device="cpu").batch([0])


def test_the_host_twin_refuses_tables_that_point_outside():
    from beat_this_amd.dataset import plan as P

    store = np.zeros((50, 128), np.float16)
    none = (np.zeros(0), np.zeros(0, np.int32), 50)
    for plan in (P.ItemPlan(10, 41, 0, [], 0, 0, True),                                   # rows 10 .. 51 of 50
                 P.ItemPlan(0, 40, 0, [], 0, 3, True),                                    # 3 annotations of 0
                 P.ItemPlan(0, 40, 0, [P.MaskOp(30, 11, P.ZERO, ())], 0, 0, True),        # frames 30 .. 41 of 40
                 P.ItemPlan(0, 40, 0, [P.MaskOp(0, 10, P.PERMUTE, ((0, 5, 6), (6, 0, 4)))], 0, 0, True),   # part reads 5 .. 11 of 10
                 P.ItemPlan(0, 40, 0, [P.MaskOp(0, 10, P.PERMUTE, ((2, 0, 8),))], 0, 0, True)):            # parts start at 2
        with pytest.raises(ValueError):
            P.run_host(store, [plan], 40, *none)
    with pytest.raises(ValueError):
        P.run_host(store, [P.ItemPlan(0, 40, 0, [], 0, 0, True)], 39, *none)   # longer than the batch


def test_struct_layouts_match_the_library():
    from beat_this_amd import _lib
    from beat_this_amd.dataset import plan as P

    P._check_layout()
    sizes = (C.c_int32 * 10)()
    _lib.lib().bt_train_batch_struct_sizes(sizes)
    assert list(sizes)[:3] == [C.sizeof(_lib.TrainItem), C.sizeof(_lib.TrainOp), C.sizeof(_lib.TrainPart)] == [48, 20, 8]
    assert list(sizes)[3:] == [_lib.TrainItem.ann_begin.offset, _lib.TrainItem.n.offset, _lib.TrainItem.op_begin.offset,
                               _lib.TrainItem.has_downbeats.offset, _lib.TrainOp.kind.offset, _lib.TrainOp.part_begin.offset,
                               _lib.TrainPart.old_off.offset]


# ---- augment.py ------------------------------------------------------------------------------------------------------------------------
def test_augment_helpers_follow_the_reference():
    from pathlib import Path

    from beat_this_amd.dataset import MemmappedNpzFile, augment as A
    from beat_this_amd.bundle import SpectBundle

    assert MemmappedNpzFile is SpectBundle and not hasattr(A, "number_of_precomputed_augmentations")
    names = A.precomputed_augmentation_filenames({"pitch": {"min": -1, "max": 2}, "tempo": {"min": -8, "max": 8, "stride": 8}})
    assert names == ["track.npy", "track_ps-1.npy", "track_ps1.npy", "track_ps2.npy", "track_ts-8.npy", "track_ts8.npy"]
    assert A.precomputed_augmentation_filenames({"tempo": {"min": -4, "max": 4, "stride": 4}}, ext="wav") == \
        ["track.wav", "track_ts-4.wav", "track_ts4.wav"]
    item = {"spect_path": Path("d/p/track.npy"), "beat_time": np.array([1.0, 2.0, 3.3])}
    assert A.shift_filename(item, -3)["spect_path"] == Path("d/p/track_ps-3.npy") and A.shift_filename(item, 0) == item
    assert A.stretch_filename(item, -12)["spect_path"] == Path("d/p/track_ts-12.npy")
    assert A.stretch_annotations(item, 0) is item and A.shift_annotations(item, 4) is item
    assert np.array_equal(A.stretch_annotations(item, -12)["beat_time"], item["beat_time"] / (1.0 + -12 / 100))
    np.random.seed(4)
    got = A.augment_pitchtempo(item, {"pitch": R.PITCH, "tempo": R.TEMPO})
    np.random.seed(4)
    if np.random.randint(2) == 0:
        want = f"track_ps{np.random.randint(-5, 7)}.npy".replace("_ps0", "")
    else:
        want = f"track_ts{np.random.choice(np.arange(-20, 21, 4))}.npy".replace("_ts0", "")
    assert got["spect_path"].name == want
    # apply_mask_excerpt: in place on numpy arrays and tensors, the same draw gives the same frames
    x = np.arange(1, 40 * 3 + 1, dtype=np.float32).reshape(40, 3)
    np.random.seed(9)
    a = x.copy()
    A.apply_mask_excerpt(a, "permute", 5, 9)
    np.random.seed(9)
    t = torch.from_numpy(x.copy())
    A.apply_mask_excerpt(t, "permute", 5, 9)
    assert np.array_equal(a, t.numpy()) and not np.array_equal(a, x) and np.array_equal(np.sort(a[:, 0]), x[:, 0])
    A.apply_mask_excerpt(a[5:9], "zero", 0, 0)
    assert not a[5:9].any() and a[9:].all()
    assert A.augment_mask_(x, {}, 50) is x


def test_augment_mask_equals_the_restated_sequence_of_in_place_masks():
    from beat_this_amd.dataset import plan as P
    from beat_this_amd.dataset.augment import augment_mask_

    rng = np.random.default_rng(2)
    for seed, params in enumerate((R.MASK_PERMUTE, R.MASK_ZERO, R.MASK_TINY, R.MASK_PERMUTE, R.MASK_PERMUTE)):
        x = rng.standard_normal((150 + 37 * seed, 128)).astype(np.float32 if seed % 2 else np.float16)
        np.random.seed(seed)
        got = augment_mask_(x.copy(), {"mask": params}, 50)
        np.random.seed(seed)
        ops = P.plan_mask(len(x), params, 50)
        assert np.array_equal(got, R.apply_ops(x.copy(), [tuple(op) for op in ops])) and ops
        np.random.seed(seed)
        assert np.array_equal(augment_mask_(torch.from_numpy(x.copy()), {"mask": params}, 50).numpy(), got)


# ---- the data module ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.SETUPS))
def test_data_module_setups_equal_the_reference(folder, name, capsys):
    from beat_this_amd.dataset import BeatDataModule

    want = META["setups"][name]
    dm = BeatDataModule(folder, train_length=R.TRAIN_LENGTH, spect_fps=R.FPS, **R.SETUPS[name])
    dm.setup("fit")
    dm.setup("test")
    assert dm.train_items == want["train_items"] and dm.val_items == want["val_items"] and dm.test_items == want["test_items"]
    assert (len(dm.train_dataset), len(dm.val_dataset), len(dm.test_dataset)) == (want["train_len"], want["val_len"], want["test_len"])
    assert [item["dataset"] for item in dm.train_dataset.items] == want["train_datasets"]
    assert dm.get_train_positive_weights() == want["positive_weights"]
    out = capsys.readouterr().out
    assert "Validation set:" in out and "Training set:" in out and "Test set:" in out
    if name in ("fold2", "no_val"):   # a piece without its augmented members is in the item list and skipped by the dataset
        assert want["train_len"] < len(want["train_items"])
        assert "because not all necessary spectrograms are there." in out
    dm.setup("predict")
    assert dm.predict_dataset is dm.test_dataset and dm.test_dataset.train_length is None
    loader = dm.train_dataloader()
    assert (loader.batch_size, loader.shuffle, loader.drop_last, len(loader)) == (8, True, True, want["train_len"] // 8)
    assert (dm.val_dataloader().shuffle, dm.val_dataloader().drop_last, dm.test_dataloader().batch_size) == (False, False, 1)
    assert len(dm.val_dataloader()) == -(-want["val_len"] // 8) and dm.predict_dataloader().batch_size == 1


def test_predict_on_the_validation_split_uses_whole_pieces(folder):
    from beat_this_amd.dataset import BeatDataModule

    dm = BeatDataModule(folder, train_length=R.TRAIN_LENGTH, spect_fps=R.FPS, predict_datasplit="val", num_workers=3)
    dm.setup("predict")
    assert dm.predict_dataset.train_length is None and len(dm.predict_dataset) == len(dm.val_items)
    assert [str(i["spect_path"]).rsplit("/", 1)[0] for i in dm.predict_dataset.items] == dm.val_items


def test_oversampling_counts_and_item_skipping_equal_the_reference(folder, capsys):
    for factor in R.OVERSAMPLING:
        want = META["oversampling"][str(factor)]
        ds = make(folder, R.ALPHA, train_length=R.TRAIN_LENGTH, length_based_oversampling_factor=factor)
        assert len(ds) == want["length"]
        assert [ds.get_frame_count(i) for i in range(len(ds))] == want["frames"]
        assert [ds.get_beat_count(i) for i in range(len(ds))] == want["beats"]
        assert [int(ds.get_downbeat_count(i)) for i in range(len(ds))] == want["downbeats"]
        assert f"Training set oversampled from 4 to {want['length']} excerpts." in capsys.readouterr().out
    ds = make(folder, ["alpha/a_long", "alpha/a_plain"], augmentations={"pitch": R.PITCH})
    assert len(ds) == 1 and "Skipping alpha/a_plain because not all necessary spectrograms are there." in capsys.readouterr().out
