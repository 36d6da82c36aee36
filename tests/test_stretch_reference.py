"""The numpy twin of csrc/stretch.hip (tests/stretch_reference.py) on its own, and the host side of
beat_this_amd.preprocess: every property that tests/test_gpu_stretch.py asserts of the device is first true of the twin here.
No GPU is needed."""
import os
import zipfile

import numpy as np
import pytest

import stretch_reference as R
from beat_this_amd import _lib, tables
from beat_this_amd import preprocess as PP
from beat_this_amd.bundle import SpectBundle
from beat_this_amd.dataset.augment import precomputed_augmentation_filenames
from beat_this_amd.dataset.mmnpz import MemmappedNpzFile

TAB = tables.resample_ratio_table()
P, Z = tables.RATIO_TAPS_PER_CROSSING, tables.RATIO_CROSSINGS
SR, sine, click_train = R.SR, R.sine, R.click_train
assert_sine_stretched, assert_sine_shifted, assert_clicks_confined = R.assert_sine_stretched, R.assert_sine_shifted, R.assert_clicks_confined
click_centroid_offsets = R.click_centroid_offsets


def test_tables_match_the_header():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "beat_this_amd.h")).read()
    assert f"#define BT_STRETCH_TABLE_DOUBLES {len(tables.stretch_tables())}\n" in header
    assert f"#define BT_RESAMPLE_RATIO_TAPS {P}\n" in header and f"#define BT_RESAMPLE_RATIO_CROSSINGS {Z}\n" in header
    assert f"#define BT_STRETCH_SCAN_BLOCK {_lib.STRETCH_SCAN_BLOCK}\n" in header
    assert (_lib.RESAMPLE_RATIO_TAPS, _lib.RESAMPLE_RATIO_CROSSINGS, _lib.STRETCH_TABLE_DOUBLES) == (P, Z, 6146)
    assert len(TAB) == P * Z + 1 and TAB.dtype == np.float32
    assert "stretch.hip" in _lib.SOURCES
    for name in ("bt_stretch", "bt_stretch_workspace_bytes", "bt_stretch_out_len", "bt_resample_ratio"):
        assert name in _lib.EXPORTS


def test_unit_length_factor_returns_the_input():
    x = R.test_signal(20000, seed=1)
    y64, y32 = R.stretch(x, 1.0), R.stretch(x, 1.0, np.float32)
    e_ref = R.rel_l2(y32, y64)
    err = R.rel_l2(y64, x)
    print(f"L = 1: |twin64 - x| = {err:.3e}, e_ref = {e_ref:.3e}, |twin32 - x| = {R.rel_l2(y32, x):.3e}")
    assert len(y64) == len(x) and y32.dtype == np.float32
    assert err <= 10 * e_ref
    assert R.rel_l2(y32, x) <= 10 * e_ref      # (phi = q(X1) whatever the peaks are: no decision can differ at L = 1)


@pytest.mark.parametrize("L", [1 / 1.2, 1 / 0.8])
def test_sine_keeps_its_frequency_when_stretched(L):
    x = sine(SR)
    for dtype in (np.float64, np.float32):
        assert_sine_stretched(R.stretch(x, L, dtype), len(x), L)


@pytest.mark.parametrize("semitones", [6, -5])
def test_sine_moves_by_the_pitch_ratio(semitones):
    x = sine(SR)
    assert_sine_shifted(R.pitch_shift(x, semitones, TAB, P, Z), len(x), semitones)


@pytest.mark.parametrize("L", [1 / 1.2, 1.0, 1 / 0.8])
def test_clicks_stay_confined(L):
    x = click_train()
    for dtype in (np.float64, np.float32):
        y = R.stretch(x, L, dtype)
        assert_clicks_confined(y, L)
    print(f"L = {L:.4f}: click energy centroid offsets (samples) = {[round(v, 1) for v in click_centroid_offsets(y, L)]}")


def test_out_of_range_length_factor():
    for L in (0.49, 2.01, float("nan")):
        with pytest.raises(ValueError):
            R.stretch(sine(4096), L)


def test_signal_has_no_flips_on_strong_partials():
    """the yardstick e_ref may contain bins whose owner differs between the fp32 and the fp64 mode (near-ties of weak
    neighbouring magnitudes), but not among the strong partials of the test signal"""
    x = R.test_signal(SR // 2, seed=7)
    for L in (1 / 1.2, 2.0 ** (6 / 12)):
        _, d64 = R.stretch(x, L, np.float64, details=True)
        _, d32 = R.stretch(x, L, np.float32, details=True)
        strong = d64["mag"] >= 0.01 * d64["mag"].max(axis=1, keepdims=True)
        assert strong.sum() > 0
        flips = d64["own"] != d32["own"]
        print(f"L = {L:.4f}: {int(flips.sum())} of {flips.size} owners differ, {int((flips & strong).sum())} on strong bins")
        assert not (flips & strong).any()


def resampler_quality(resample, step, n_in=6000, edge=450, n_pass=12, n_stop=6):
    """(pass-band ripple in dB, worst spurious level in dB re the input tone) from tones at fractions of the LOWER Nyquist
    frequency: pass band (0, 0.913], stop band [1, input Nyquist) where the input has one.  A pass-band tone is fitted
    (least squares) at its expected output frequency: the gain gives the ripple, the residual counts as spurious; a
    stop-band tone is spurious altogether.  ``edge`` output samples at either end are left out."""
    n_out = int(n_in / step)
    lower = min(0.5, 0.5 / step)
    j, m = np.arange(n_in), np.arange(n_out)
    sl = slice(edge, n_out - edge)
    fracs = list(np.linspace(0.02, 0.913, n_pass)) + (list(np.linspace(1.0, 0.999 * 0.5 / lower, n_stop)) if step > 1 else [])
    ripple, spur = 0.0, 0.0
    for frac in fracs:
        f = frac * lower * (1 + 1e-4 * np.sqrt(2))          # cycles per input sample, off every grid
        y = resample(np.sin(2 * np.pi * f * j), step, n_out)[sl]
        if frac <= 0.913:
            B = np.stack([np.sin(2 * np.pi * f * step * m), np.cos(2 * np.pi * f * step * m)], 1)[sl]
            coef = np.linalg.lstsq(B, y, rcond=None)[0]
            ripple = max(ripple, abs(20 * np.log10(np.hypot(*coef))))
            spur = max(spur, np.sqrt(2 * np.mean((y - B @ coef) ** 2)))
        else:
            spur = max(spur, np.sqrt(2 * np.mean(y ** 2)))
    return ripple, 20 * np.log10(spur)


def test_resampler_is_no_worse_than_the_rational_path():
    h, half = tables.resample_filter(1, 2)
    ref_ripple, ref_spur = resampler_quality(lambda x, s, n: R.resample_rational(x, 1, 2, h, half, n), 2.0)
    print(f"rational 2:1 path: ripple {ref_ripple:.2e} dB, spurious {ref_spur:.1f} dB")
    for step in (1.0, 2.0 ** (6 / 12), 2.0 ** (-5 / 12), 2.0):
        ripple, spur = resampler_quality(lambda x, s, n: R.resample_ratio(x, s, n, TAB, P, Z), step)
        print(f"step {step:.4f}: ripple {ripple:.2e} dB, spurious {spur:.1f} dB")
        assert ripple <= ref_ripple and spur <= ref_spur


def test_resampler_identity_and_fp32_mode():
    x = R.test_signal(3000, seed=3)
    y = R.resample_ratio(x, 1.0, len(x), TAB, P, Z)
    assert R.rel_l2(y[600:-600], x[600:-600]) < 1e-2      # (the signal's 7.4 kHz partial and the noise above 0.913 Nyquist are filtered)
    y32 = R.resample_ratio(x, 2.0 ** (6 / 12), 2000, TAB, P, Z, np.float32)
    assert y32.dtype == np.float32 and R.rel_l2(y32, R.resample_ratio(x, 2.0 ** (6 / 12), 2000, TAB, P, Z)) < 1e-5


# ---- beat_this_amd.preprocess: names, order, bundle layout, arguments ----------------------------------------------------
def test_argument_parsing():
    assert PP.ints("-5:6") == (-5, 6) and PP.ints("20:4") == (20, 4) and PP.ints("") is None
    aug = PP.augmentations_of((-5, 6), (20, 4))
    assert aug == {"pitch": {"min": -5, "max": 6}, "tempo": {"min": -20, "max": 20, "stride": 4}}
    names = precomputed_augmentation_filenames(aug)
    assert len(names) == 22 and names[0] == "track.npy"      # the track, 11 pitch shifts, 10 tempo changes
    assert [PP.variant_of(n) for n in ("track.npy", "track_ps-5.npy", "track_ps6.npy", "track_ts-20.npy", "track_ts8.npy")] == \
        [(None, 0), ("pitch", -5), ("pitch", 6), ("tempo", -20), ("tempo", 8)]
    assert {PP.variant_of(n)[0] for n in names[1:12]} == {"pitch"} and {PP.variant_of(n)[0] for n in names[12:]} == {"tempo"}
    assert PP.augmentations_of(None, (20,)) == {"tempo": {"min": -20, "max": 20, "stride": 1}}


def test_length_limit_arithmetic():
    names = precomputed_augmentation_filenames(PP.augmentations_of((-5, 6), (20, 4)))
    assert PP.max_stretched_length(1000, 22050, ["track.npy"]) == 0
    n = 10 * 60 * 22050
    longest = PP.max_stretched_length(n, 22050, names)          # six semitones up is the longest: 2^(6/12) of 2 n samples
    assert R.out_len(2 * n, 2.0 ** 0.5) <= longest <= R.out_len(2 * n, 2.0 ** 0.5) + 2
    assert PP.max_stretched_length(n, 22050, ["track_ts20.npy"]) == 2 * n + 1      # shorter out than in: the input counts
    assert PP.max_stretched_length(n, 22050, ["track_ts-20.npy"]) == int(2 * n * 1.25) + 1
    assert longest < _lib.STRETCH_MAX_SAMPLES < PP.max_stretched_length(2 * n, 22050, names)   # 10 minutes fit, 20 do not


def test_audio_paths_csv(tmp_path):
    p = tmp_path / "paths.csv"
    p.write_text('ballroom,/data/ballroom\n"with, comma", /x/y\n\n')
    assert PP.read_audio_paths(p) == {"ballroom": "/data/ballroom", "with, comma": "/x/y"}


def test_interrupted_writes_leave_no_file(tmp_path, monkeypatch):
    def interrupted(path, array):
        with open(path, "wb") as f:
            f.write(b"half")
        raise KeyboardInterrupt

    monkeypatch.setattr(PP.np, "save", interrupted)
    target = tmp_path / "track_ts8.npy"
    with pytest.raises(KeyboardInterrupt):
        PP.save_spectrogram(target, np.zeros((3, 128), np.float16))
    assert not target.exists()
    spect_dir = tmp_path / "toy"
    (spect_dir / "piece").mkdir(parents=True)                  # (track.npy is missing: the bundle cannot be completed)
    with pytest.raises(FileNotFoundError):
        PP.create_npz(spect_dir, spect_dir.with_suffix(".npz"), ["track.npy"])
    assert not spect_dir.with_suffix(".npz").exists()


def test_bundle_layout(tmp_path):
    aug = PP.augmentations_of((-1, 1), (20, 20))
    names = precomputed_augmentation_filenames(aug)
    assert names == ["track.npy", "track_ps-1.npy", "track_ps1.npy", "track_ts-20.npy", "track_ts20.npy"]
    rng = np.random.default_rng(0)
    spect_dir = tmp_path / "audio" / "spectrograms" / "toy"
    data = {}
    for stem in ("b_piece", "a_piece"):
        (spect_dir / stem).mkdir(parents=True)
        for n in names:
            data[f"{stem}/{n[:-4]}"] = rng.standard_normal((int(rng.integers(5, 9)), 128)).astype(np.float16)
            PP.save_spectrogram(spect_dir / stem / n, data[f"{stem}/{n[:-4]}"])
    npz = spect_dir.with_suffix(".npz")
    assert PP.create_npz(spect_dir, npz, names)
    with zipfile.ZipFile(npz) as z:
        assert [i.filename for i in z.infolist()] == [f"{s}/{n}" for s in ("a_piece", "b_piece") for n in names]
        assert all(i.compress_type == zipfile.ZIP_STORED for i in z.infolist())
    for reader in (SpectBundle, MemmappedNpzFile):
        with reader(npz) as b:
            assert list(b) == [f"{s}/{n[:-4]}" for s in ("a_piece", "b_piece") for n in names]
            for k, v in data.items():
                assert b[k].dtype == np.float16 and np.array_equal(b[k], v)
    with np.load(npz) as z:
        assert np.array_equal(z["a_piece/track_ts20"], data["a_piece/track_ts20"])
    stamp = npz.stat().st_mtime_ns
    assert not PP.create_npz(spect_dir, npz, names) and npz.stat().st_mtime_ns == stamp      # an existing bundle is kept
