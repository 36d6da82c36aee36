"""csrc/stretch.hip on the device against its fp64 numpy twin (tests/stretch_reference.py), through the C ABI with guard bands
and both poisons, and beat_this_amd.preprocess end to end on a small dataset.

The gate of every comparison is ten times e_ref, the twin's own fp32 mode against its fp64 mode on the same input (DESIGN.md
section 13).  The metric is the relative L2 distance over the whole output: a near-tie between neighbouring magnitudes may
pick another peak in one frame on either side, which a maximum would turn into a failure of one sample."""
import functools
import json

import numpy as np
import pytest
import torch

import stretch_reference as R
from gpu_util import POISONS, Guarded, assert_intact, dev, report
from stretch_reference import SR, assert_clicks_confined, assert_sine_shifted, assert_sine_stretched, click_train, sine

pytestmark = pytest.mark.gpu

LENGTH_FACTORS = {"1": 1.0, "1/1.2": 1 / 1.2, "1/0.8": 1 / 0.8, "2^(6/12)": 2.0 ** (6 / 12), "2^(-5/12)": 2.0 ** (-5 / 12)}
STEPS = {"1": 1.0, "2^(6/12)": 2.0 ** (6 / 12), "2^(-5/12)": 2.0 ** (-5 / 12), "2": 2.0}
FIXED_N = (2049, 4096, 5000, 3 * 2048 + 1, 132300)


def scan_boundary(L):
    """(N, N'): the longest input whose frames fill exactly one block of the prefix sum, and the shortest that starts a second"""
    from beat_this_amd import _lib

    B = _lib.STRETCH_SCAN_BLOCK
    n = int((B - 1) * R.HS / L)
    while R.n_frames(R.out_len(n, L)) <= B:
        n += 1
    lo = n - 1
    assert R.n_frames(R.out_len(lo, L)) == B and R.n_frames(R.out_len(n, L)) == B + 1
    return lo, n


def lengths(L):
    return FIXED_N + scan_boundary(L)


@functools.lru_cache(maxsize=None)
def signal(n):
    return R.test_signal(n, seed=n % 9973)


@functools.lru_cache(maxsize=None)
def stretch_ref(n, L):
    """(fp64 twin, e_ref) of the test signal of length n, computed once"""
    y64 = R.stretch(signal(n), L, np.float64)
    return y64, R.rel_l2(R.stretch(signal(n), L, np.float32), y64)


@functools.lru_cache(maxsize=None)
def device_tables():
    from beat_this_amd import tables

    return torch.from_numpy(tables.stretch_tables()).to(dev()), torch.from_numpy(tables.resample_ratio_table()).to(dev())


def ratio_table():
    from beat_this_amd import tables

    return tables.resample_ratio_table(), tables.RATIO_TAPS_PER_CROSSING, tables.RATIO_CROSSINGS


def run_stretch(x, L, poison, short_by=0):
    """bt_stretch on guarded buffers filled with ``poison`` (the output and the workspace wholly): -> (rc, output)"""
    from beat_this_amd import _lib

    lib = _lib.lib()
    n = len(x)
    m = lib.bt_stretch_out_len(n, L)
    ws_bytes = lib.bt_stretch_workspace_bytes(n, L)
    assert m == R.out_len(n, L) and ws_bytes > 0
    gi = Guarded((n,), torch.float32).fill(poison, data=torch.from_numpy(x).to(dev()))
    go = Guarded((m,), torch.float32).fill(poison)
    ws = Guarded((ws_bytes,), torch.uint8).fill(poison)
    rc = lib.bt_stretch(_lib.stream_ptr(dev()), device_tables()[0].data_ptr(), gi.ptr(), n, L, go.ptr(), m, ws.ptr(),
                        ws_bytes - short_by)
    torch.cuda.synchronize()
    assert_intact(("input", gi), ("output", go), ("workspace", ws))
    assert torch.equal(gi.t.cpu(), torch.from_numpy(x))
    return rc, go.t.cpu().numpy()


def run_resample(x, step, n_out, poison):
    from beat_this_amd import _lib

    gi = Guarded((len(x),), torch.float32).fill(poison, data=torch.from_numpy(x).to(dev()))
    go = Guarded((n_out,), torch.float32).fill(poison)
    rc = _lib.lib().bt_resample_ratio(_lib.stream_ptr(dev()), gi.ptr(), len(x), step, device_tables()[1].data_ptr(), go.ptr(), n_out)
    torch.cuda.synchronize()
    assert_intact(("input", gi), ("output", go))
    return rc, go.t.cpu().numpy()


@pytest.mark.parametrize("which", range(len(FIXED_N) + 2))
@pytest.mark.parametrize("Lname", list(LENGTH_FACTORS))
def test_stretch_matches_the_twin(Lname, which):
    L = LENGTH_FACTORS[Lname]
    n = lengths(L)[which]
    x = signal(n)
    y64, e_ref = stretch_ref(n, L)
    outs = []
    for poison in POISONS:
        rc, y = run_stretch(x, L, poison)
        assert rc == 0
        outs.append(y)
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))      # two runs, two poisons: the same bits
    assert np.isfinite(outs[0]).all()
    err = R.rel_l2(outs[0], y64)
    print(f"stretch N = {n}, L = {Lname}: e_ref = {e_ref:.3e}, device = {err:.3e}, ratio = {err / e_ref:.2f}")
    report("stretch_vs_twin", N=n, L=Lname, frames=R.n_frames(len(y64)), e_ref=e_ref, device=err, ratio=err / e_ref)
    assert err <= 10 * e_ref
    if L == 1.0:
        err_x = R.rel_l2(outs[0], x)
        print(f"   against the input: {err_x:.3e}")
        assert err_x <= 10 * e_ref


@pytest.mark.parametrize("name", list(STEPS))
def test_resample_ratio_matches_the_twin(name):
    step = STEPS[name]
    x = signal(20000)
    n_out = int(len(x) / step)
    tab, P, Z = ratio_table()
    y64 = R.resample_ratio(x, step, n_out, tab, P, Z)
    e_ref = R.rel_l2(R.resample_ratio(x, step, n_out, tab, P, Z, np.float32), y64)
    outs = []
    for poison in POISONS:
        rc, y = run_resample(x, step, n_out, poison)
        assert rc == 0
        outs.append(y)
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    err = R.rel_l2(outs[0], y64)
    print(f"resample step = {name}: e_ref = {e_ref:.3e}, device = {err:.3e}, ratio = {err / e_ref:.2f}")
    report("resample_ratio_vs_twin", step=name, e_ref=e_ref, device=err, ratio=err / e_ref)
    assert err <= 10 * e_ref


@pytest.mark.parametrize("semitones", [6, -5])
def test_pitch_shift_end_to_end(semitones):
    from beat_this_amd.preprocessing import pitch_shift

    x = signal(30000)
    tab, P, Z = ratio_table()
    y64 = R.pitch_shift(x, semitones, tab, P, Z)
    e_ref = R.rel_l2(R.pitch_shift(x, semitones, tab, P, Z, np.float32), y64)
    y = pitch_shift(torch.from_numpy(x).to(dev()), semitones)
    assert y.shape == (len(x),) and y.dtype == torch.float32
    err = R.rel_l2(y.cpu().numpy(), y64)
    print(f"pitch shift {semitones:+d}: e_ref = {e_ref:.3e}, device = {err:.3e}, ratio = {err / e_ref:.2f}")
    report("pitch_shift_vs_twin", semitones=semitones, e_ref=e_ref, device=err, ratio=err / e_ref)
    assert err <= 10 * e_ref
    assert torch.equal(y, pitch_shift(torch.from_numpy(x).to(dev()), semitones))


def test_workspace_and_argument_errors():
    from beat_this_amd import _lib
    from beat_this_amd.preprocessing import resample_ratio, stretch_length, time_stretch

    lib = _lib.lib()
    x = signal(4096)
    rc, _ = run_stretch(x, 1 / 1.2, POISONS[0], short_by=1)
    assert rc == _lib.BT_ERR_WORKSPACE
    with pytest.raises(RuntimeError):
        _lib.check(rc)
    d = torch.from_numpy(x).to(dev())
    out = torch.empty(3 * len(x), dtype=torch.float32, device=dev())
    ws = torch.empty(lib.bt_stretch_workspace_bytes(len(x), 2.0), dtype=torch.uint8, device=dev())
    for L in (0.49, 2.01, float("nan")):
        assert lib.bt_stretch_workspace_bytes(len(x), L) == 0 and lib.bt_stretch_out_len(len(x), L) == 0
        assert lib.bt_stretch(_lib.stream_ptr(dev()), device_tables()[0].data_ptr(), d.data_ptr(), len(x), L, out.data_ptr(),
                              int(len(x) * 2), ws.data_ptr(), ws.numel()) == _lib.BT_ERR_ARG
        with pytest.raises(ValueError):
            stretch_length(d, L)
        with pytest.raises(ValueError):
            time_stretch(d, 1.0 / L)
    assert lib.bt_stretch_workspace_bytes(_lib.STRETCH_MAX_SAMPLES + 1, 1.0) == 0
    assert lib.bt_stretch_workspace_bytes(0, 1.0) == 0
    assert lib.bt_stretch(_lib.stream_ptr(dev()), device_tables()[0].data_ptr(), d.data_ptr(), len(x), 1.0, out.data_ptr(),
                          len(x) + 1, ws.data_ptr(), ws.numel()) == _lib.BT_ERR_ARG      # n_out is not the stretched length
    for step in (0.2, 4.5, float("nan")):
        assert lib.bt_resample_ratio(_lib.stream_ptr(dev()), d.data_ptr(), len(x), step, device_tables()[1].data_ptr(),
                                     out.data_ptr(), 100) == _lib.BT_ERR_ARG
        with pytest.raises(ValueError):
            resample_ratio(d, step)
    with pytest.raises(RuntimeError):
        stretch_length(torch.from_numpy(x), 1.0)                 # no CPU path
    with pytest.raises(ValueError):
        stretch_length(d.double(), 1.0)
    torch.cuda.synchronize()


def test_sine_and_click_properties_on_the_device():
    from beat_this_amd.preprocessing import pitch_shift, stretch_length, time_stretch

    x = torch.from_numpy(sine(SR)).to(dev())
    for factor in (1.2, 0.8):
        assert_sine_stretched(time_stretch(x, factor).cpu().numpy(), SR, 1 / factor)
    for semitones in (6, -5):
        assert_sine_shifted(pitch_shift(x, semitones).cpu().numpy(), SR, semitones)
    c = torch.from_numpy(click_train()).to(dev())
    for L in (1 / 1.2, 1.0, 1 / 0.8):
        assert_clicks_confined(stretch_length(c, L).cpu().numpy(), L)


def _write_wav(path, sr, data):
    from scipy.io import wavfile

    wavfile.write(str(path), sr, (np.clip(data, -1, 1) * 32767).astype(np.int16))


def test_preprocess_end_to_end(tmp_path):
    from beat_this_amd import preprocess as PP
    from beat_this_amd.dataset import BeatTrackingDataset
    from beat_this_amd.dataset.augment import precomputed_augmentation_filenames
    from beat_this_amd.inference import Audio2Frames
    from beat_this_amd.preprocessing import load_audio

    audio = tmp_path / "orig" / "toy"
    audio.mkdir(parents=True)
    stereo = np.stack([R.test_signal(2 * 48000, 11, 48000), R.test_signal(2 * 48000, 12, 48000)], 1)
    _write_wav(audio / "toy_stereo.wav", 48000, stereo)
    _write_wav(audio / "toy_mono.wav", 22050, R.test_signal(3 * 22050, 13, 22050))
    _write_wav(audio / "toy_unannotated.wav", 22050, R.test_signal(22050, 14, 22050))
    _write_wav(audio / "gtzan_speech_x.wav", 22050, R.test_signal(22050, 15, 22050))
    data = tmp_path / "data"
    beats = data / "annotations" / "toy" / "annotations" / "beats"
    beats.mkdir(parents=True)
    for stem, dur in (("toy_stereo", 2.0), ("toy_mono", 3.0), ("gtzan_speech_x", 1.0)):
        t = np.arange(0.25, dur, 0.5)
        (beats / f"{stem}.beats").write_text("".join(f"{v:.3f}\t{1 + i % 4}\n" for i, v in enumerate(t)))
    (data / "annotations" / "toy" / "info.json").write_text(json.dumps({"has_downbeats": True}))
    csv_path = tmp_path / "audio_paths.csv"
    csv_path.write_text(f"toy,{audio}\n")
    argv = ["--orig_audio_paths", str(csv_path), "--pitch_shift", "-1:1", "--time_stretch", "20:20", "--data-dir", str(data)]
    assert PP.main(argv) == 0
    aug = PP.augmentations_of((-1, 1), (20, 20))
    names = precomputed_augmentation_filenames(aug)
    assert names == ["track.npy", "track_ps-1.npy", "track_ps1.npy", "track_ts-20.npy", "track_ts20.npy"]
    spect_dir = data / "audio" / "spectrograms" / "toy"
    assert sorted(p.name for p in spect_dir.iterdir()) == ["toy_mono", "toy_stereo"]
    assert (data / "audio" / "spectrograms" / "toy.npz").exists()
    a2f = Audio2Frames(checkpoint_path=None, device=dev())
    for stem in ("toy_mono", "toy_stereo"):
        files = {n: np.load(spect_dir / stem / n) for n in names}
        assert sorted(p.name for p in (spect_dir / stem).iterdir()) == sorted(names)
        assert all(a.dtype == np.float16 and a.ndim == 2 and a.shape[1] == 128 for a in files.values())
        sig, sr = load_audio(audio / f"{stem}.wav")
        want = a2f.signal2spect(sig, sr).to(torch.float16).cpu().numpy()
        assert np.array_equal(files["track.npy"].view(np.uint16), want.view(np.uint16))
        n22 = -(-len(sig) * 22050 // sr)
        assert len(want) == 1 + n22 // 441
        for p in (-20, 20):
            v = n22 / (1 + p / 100)
            allowed = {1 + n // 441 for n in range(int(np.floor(v - 1)), int(np.ceil(v + 1)) + 1)}
            assert len(files[f"track_ts{p}.npy"]) in allowed
        for k in (-1, 1):
            assert len(files[f"track_ps{k}.npy"]) == len(want)
            assert not np.array_equal(files[f"track_ps{k}.npy"], files["track.npy"])
    ds = BeatTrackingDataset(["toy/toy_mono", "toy/toy_stereo"], data, train_length=64, augmentations=aug, device=dev())
    assert len(ds) == 2
    np.random.seed(0)
    seen = set()
    for _ in range(40):
        for i in range(len(ds)):
            item = ds[i]
            assert item["spect"].shape == (64, 128)
            seen.add(str(item["spect_path"]))
    assert seen == {f"toy/{stem}/{n}" for stem in ("toy_mono", "toy_stereo") for n in names}
    # a second run writes nothing
    before = {p: p.stat().st_mtime_ns for p in (data / "audio").rglob("*") if p.is_file()}
    pre = PP.Preprocessor(data, (-1, 1), (20, 20))
    pre.run(PP.read_audio_paths(csv_path))
    pre.create_bundles()
    assert pre.written == 0
    assert before == {p: p.stat().st_mtime_ns for p in (data / "audio").rglob("*") if p.is_file()}
