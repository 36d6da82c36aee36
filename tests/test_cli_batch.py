"""The command line's batching helpers (--device-decode, --batch N), no GPU needed: how tasks are cut into batches, what a
file costs, and that the two options stay out of the parsed arguments unless given."""
from pathlib import Path

import wav_cases as W
from beat_this_amd import cli


def test_new_options_are_absent_unless_given():
    d = vars(cli.get_parser().parse_args(["x.wav"]))
    assert "device_decode" not in d and "batch" not in d            # run()'s defaults (False, 1) are today's behaviour
    d = vars(cli.get_parser().parse_args(["x.wav", "--device-decode", "--batch", "6"]))
    assert d["device_decode"] is True and d["batch"] == 6
    import inspect

    p = inspect.signature(cli.run).parameters
    assert p["device_decode"].default is False and p["batch"].default == 1


def test_cut_batches_caps_files_bytes_and_frames():
    items = [(k, b, f) for k, (b, f) in enumerate([(10, 1), (10, 1), (10, 1), (10, 1), (10, 1)])]
    assert list(cli.cut_batches(items, 2)) == [[0, 1], [2, 3], [4]]
    assert list(cli.cut_batches(items, 8)) == [[0, 1, 2, 3, 4]]
    assert list(cli.cut_batches(items, 8, max_bytes=25)) == [[0, 1], [2, 3], [4]]
    assert list(cli.cut_batches(items, 8, max_frames=3)) == [[0, 1, 2], [3, 4]]
    assert list(cli.cut_batches([], 4)) == []
    # a single file above a cap goes alone, and the files around it keep their order
    big = [("a", 5, 1), ("b", 1000, 1), ("c", 5, 1), ("d", 5, 500), ("e", 5, 1)]
    assert list(cli.cut_batches(big, 8, max_bytes=100, max_frames=100)) == [["a"], ["b"], ["c"], ["d"], ["e"]]
    assert cli.BATCH_MAX_FRAMES + 1500 < 2 ** 31
    # an item is taken only when its batch is being formed (the command line claims outputs as it goes)
    taken = []

    def source():
        for k in range(5):
            taken.append(k)
            yield k, 1, 1

    g = cli.cut_batches(source(), 2)
    assert next(g) == [0, 1] and taken == [0, 1, 2]


def test_batch_cost_is_exact_for_pcm_and_bounded_by_bytes_otherwise(tmp_path):
    p = W.write_wav(tmp_path / "a.wav", "s16", W.samples("s16", 2, 44100 * 3), rate=44100)
    assert cli.batch_cost(p) == (44100 * 3 * 4, 152)
    q = tmp_path / "b.mp3"
    q.write_bytes(b"x" * 20000)
    assert cli.batch_cost(q) == (20000, 1002)
    assert cli.batch_cost(Path(tmp_path / "missing.flac")) == (0, 2)
    # the byte cap bounds the frames of files that cannot be probed
    assert cli.BATCH_MAX_BYTES // 20 + 2 + 1500 < 2 ** 31
