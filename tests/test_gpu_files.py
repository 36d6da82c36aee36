"""Files -> beats with the PCM decode on the MI355X: Audio2Frames.files2waves, File2Beats.many / many_async,
File2Beats(device_decode=True) and ``cli.run(..., device_decode=True, batch=N)`` against the host route they replace --
waveforms bit for bit, beats array-equal, the command line's outputs byte for byte -- and the defaults, which run none of it."""
import numpy as np
import pytest
import torch

import wav_cases as W

pytestmark = pytest.mark.gpu


def _clicks(seconds, seed, sr):
    from beat_this_amd import weights

    return weights.synthetic_audio(seconds, seed=seed, sr=sr) / 2.5


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> path, in a directory of its own; plus the checkpoint.  16-bit mono at 22050 Hz (3 s, and 40 s: two chunks),
    24-bit stereo at 44100 Hz, three channels of f32 at 48000 Hz, and a u8 file whose valid bits differ from its container:
    ``wav.probe`` declines it, ``load_audio`` reads it."""
    from oracle.cases import CLI_CASE, lightning_checkpoint, pcm16_wav

    root = tmp_path_factory.mktemp("files")
    audio = root / "audio"
    audio.mkdir()
    ck = root / "m.ckpt"
    torch.save(lightning_checkpoint(CLI_CASE["hparams"], CLI_CASE["weight_seed"], CLI_CASE["style"], False), ck)
    pcm16_wav(audio / "a_short.wav", 3.0, CLI_CASE["audio_seed"], 22050)
    pcm16_wav(audio / "b_long.wav", 40.0, CLI_CASE["audio_seed"] + 1, 22050)
    x = _clicks(5.0, 3, 44100)
    s24 = np.clip(np.round(np.stack([x, 0.5 * np.roll(x, 7)], 1) * (2 ** 23 - 1)), -2 ** 23, 2 ** 23 - 1).astype(np.int64)
    W.write_wav(audio / "c_s24_stereo.wav", "s24", s24, rate=44100, **W.EXTRA_VARIANTS["odd"])
    x = _clicks(5.0, 4, 48000).astype(np.float32)
    f32 = np.stack([x, np.float32(1e-4) * np.roll(x, 3), -x * np.float32(0.999)], 1)
    W.write_wav(audio / "d_f32_three.wav", "f32", f32, rate=48000, extensible=True)
    x = _clicks(4.0, 5, 22050)
    u8 = np.clip(np.round(x * 127.0 + 128.0), 0, 255).astype(np.int64)
    W.write_wav(audio / "e_u8_declined.wav", "u8", u8, rate=22050, extensible=True, valid_bits=7)
    names = ["a_short.wav", "b_long.wav", "c_s24_stereo.wav", "d_f32_three.wav", "e_u8_declined.wav"]
    return dict(ck=ck, dir=audio, paths={n: audio / n for n in names})


def _host_wave(path):
    from beat_this_amd.inference import _host_mono, load_audio

    signal, sr = load_audio(path)
    return _host_mono(signal), sr


@pytest.fixture(scope="module")
def f2b(files):
    from beat_this_amd.inference import File2Beats

    return File2Beats(str(files["ck"]), "cuda:0", float16=False, dbn=False)


ORDER = ["c_s24_stereo.wav", "a_short.wav", "e_u8_declined.wav", "d_f32_three.wav", "b_long.wav"]   # rates mixed up


def test_probe_takes_four_of_the_five(files):
    from beat_this_amd import wav

    got = {n: wav.probe(p) for n, p in files["paths"].items()}
    assert got["e_u8_declined.wav"] is None and all(v is not None for n, v in got.items() if n != "e_u8_declined.wav")
    assert (got["c_s24_stereo.wav"].format, got["c_s24_stereo.wav"].channels, got["c_s24_stereo.wav"].data_offset % 4) == (2, 2, 2)
    assert (got["d_f32_three.wav"].format, got["d_f32_three.wav"].channels) == (4, 3)


def test_files2waves_has_the_host_routes_bits(files, f2b):
    paths = [files["paths"][n] for n in ORDER]
    waves = f2b.files2waves(paths)
    assert len(waves) == len(paths)
    for n, p, (w, sr) in zip(ORDER, paths, waves):
        want, want_sr = _host_wave(p)
        assert sr == want_sr and w.is_cuda and w.dtype == torch.float32 and w.data_ptr() % 16 == 0
        assert W.same_bits(w.cpu().numpy(), want) is None, (n, W.same_bits(w.cpu().numpy(), want))
    assert f2b.files2waves([]) == []
    # one file alone (no reader threads), and the single-file entry point
    for n in ("c_s24_stereo.wav", "d_f32_three.wav"):
        want, want_sr = _host_wave(files["paths"][n])
        (w, sr), = f2b.files2waves([str(files["paths"][n])])
        w1, sr1 = f2b.file2wave(files["paths"][n])
        assert sr == sr1 == want_sr
        assert W.same_bits(w.cpu().numpy(), want) is None and W.same_bits(w1.cpu().numpy(), want) is None
    assert f2b.file2wave(files["paths"]["e_u8_declined.wav"]) is None


def test_many_equals_audio2beats_many_per_rate_group(files, f2b):
    from beat_this_amd.inference import Audio2Beats

    paths = [files["paths"][n] for n in ORDER]
    got = f2b.many(paths)
    assert len(got) == len(paths)
    host = [_host_wave(p) for p in paths]
    for rate in sorted({sr for _, sr in host}):
        idx = [k for k, (_, sr) in enumerate(host) if sr == rate]
        want = Audio2Beats.many_async(f2b, [host[k][0] for k in idx], rate).result()
        for k, (b, d) in zip(idx, want):
            assert np.array_equal(got[k][0], b) and np.array_equal(got[k][1], d), ORDER[k]
            assert len(b) > 2
    # the order of the output follows the paths
    again = f2b.many(paths[::-1])
    for a, b in zip(again[::-1], got):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_many_async_logits_have_the_batchs_frames(files, f2b):
    paths = [files["paths"][n] for n in ORDER]
    handle = f2b.many_async(paths)
    beat, down, off = handle.logits
    frames = []
    for p in paths:
        w, sr = _host_wave(p)
        frames.append(1 + (-(-len(w) * 22050 // sr)) // 441)
    assert list(np.diff(off)) == frames and beat.shape == down.shape == (sum(frames),)
    res = handle.result()
    # one rate: the handle hands out the group's own tensors
    h1 = f2b.many_async([files["paths"]["b_long.wav"], files["paths"]["a_short.wav"]])
    b1, d1, off1 = h1.logits
    assert list(np.diff(off1)) == [frames[4], frames[1]]
    k = ORDER.index("b_long.wav")
    assert torch.equal(b1[: frames[4]], beat[off[k]: off[k + 1]])
    r1 = h1.result()
    assert np.array_equal(r1[0][0], res[k][0]) and np.array_equal(r1[0][1], res[k][1])


@pytest.mark.parametrize("dbn", [False, True])
def test_device_decode_equals_the_host_route(files, dbn):
    from beat_this_amd.inference import File2Beats

    off = File2Beats(str(files["ck"]), "cuda:0", float16=False, dbn=dbn)
    on = File2Beats(str(files["ck"]), "cuda:0", float16=False, dbn=dbn, device_decode=True)
    assert off.device_decode is False and on.device_decode is True
    on.model = off.model
    for n, p in files["paths"].items():
        a, b = off(str(p)), on(str(p))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), n
        assert len(a[0]) > 2


def _run(files, out, **kw):
    from beat_this_amd import cli

    args = dict(inputs=[str(files["dir"])], model=str(files["ck"]), output=str(out), suffix=".beats", append=False,
                skip_existing=False, touch_first=False, dbn=False, gpu=0, float16=False, activations=True)
    args.update(kw)
    out.mkdir(exist_ok=True)
    cli.run(**args)


def _messages(err):
    """the command line's own messages (a progress bar writes to the same stream)"""
    import re

    return re.findall(r'Could not process "[^"]*"\. Rerun with this file alone for details\.', err)


def _outputs(out):
    return {p.name: p.read_bytes() for p in sorted(out.iterdir())}


def test_cli_batches_write_what_the_loop_writes(files, tmp_path, capsys):
    bad = files["dir"] / "bb_corrupt.wav"
    bad.write_bytes(W.wav_bytes("s16", W.samples("s16", 1, 3000), magic=b"RF64"))     # load_audio rejects it, today and here
    try:
        ref, new, new2 = tmp_path / "ref", tmp_path / "new", tmp_path / "new2"
        _run(files, ref)
        msg_ref = _messages(capsys.readouterr().err)
        _run(files, new, device_decode=True, batch=3)
        msg_new = _messages(capsys.readouterr().err)
        _run(files, new2, batch=2, dbn=True, activations=False)
        capsys.readouterr()
        _run(files, tmp_path / "ref2", dbn=True, activations=False)
        capsys.readouterr()
    finally:
        bad.unlink()
    want = _outputs(ref)
    assert sorted(want) == sorted([n.replace(".wav", e) for n in ORDER for e in (".beats", ".npy")])
    assert _outputs(new) == want                      # .beats texts and --activations arrays, byte for byte
    assert all(len(v) > 20 for v in want.values())
    assert len(msg_ref) == 1 and "bb_corrupt.wav" in msg_ref[0] and msg_new == msg_ref
    assert _outputs(new2) == _outputs(tmp_path / "ref2")


def test_cli_batches_honour_skip_existing_and_touch_first(files, tmp_path, capsys):
    ref, out = tmp_path / "ref", tmp_path / "out"
    _run(files, ref, activations=False)
    want = _outputs(ref)
    out.mkdir()
    (out / "b_long.beats").write_text("mine\n")
    (out / "d_f32_three.beats").write_text("")       # another process's claim
    _run(files, out, activations=False, device_decode=True, batch=3, skip_existing=True, touch_first=True)
    got = _outputs(out)
    assert got["b_long.beats"] == b"mine\n" and got["d_f32_three.beats"] == b""
    for n in ("a_short.beats", "c_s24_stereo.beats", "e_u8_declined.beats"):
        assert got[n] == want[n]
    # skip_existing alone: what is there stays, nothing else is missing
    (out / "a_short.beats").write_text("kept\n")
    (out / "c_s24_stereo.beats").unlink()
    _run(files, out, activations=False, batch=4, skip_existing=True)
    got = _outputs(out)
    assert got["a_short.beats"] == b"kept\n" and got["b_long.beats"] == b"mine\n" and got["c_s24_stereo.beats"] == want["c_s24_stereo.beats"]
    assert _messages(capsys.readouterr().err) == []


def test_cli_defaults_run_none_of_the_new_code(files, tmp_path, monkeypatch):
    from beat_this_amd import cli, inference, wav

    calls = []
    for mod, name in ((wav, "probe"), (wav, "read_raw"), (inference.Audio2Frames, "files2waves"),
                      (inference.Audio2Frames, "file2wave"), (inference.File2Beats, "many_async"), (cli, "cut_batches")):
        real = getattr(mod, name)
        monkeypatch.setattr(mod, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])
    _run(files, tmp_path / "o1")
    _run(files, tmp_path / "o2", activations=False)
    cli.run(inputs=[str(files["paths"]["a_short.wav"])], model=str(files["ck"]), output=str(tmp_path / "one.beats"), suffix=".beats",
            append=False, skip_existing=False, touch_first=False, dbn=False, gpu=0, float16=False, activations=False)
    assert calls == []
    assert cli.get_parser().parse_args(["x.wav"]).__dict__.keys() == {"inputs", "model", "output", "suffix", "append",
                                                                        "skip_existing", "touch_first", "dbn", "gpu", "float16",
                                                                        "activations"}
    a = cli.get_parser().parse_args(["x.wav", "--device-decode", "--batch", "6"])
    assert a.device_decode is True and a.batch == 6
    _run(files, tmp_path / "o3", device_decode=True, batch=2)      # ... and the wrappers do see the opt-in
    assert {"probe", "read_raw", "files2waves", "many_async", "cut_batches"} <= set(calls)
    assert _outputs(tmp_path / "o3") == _outputs(tmp_path / "o1")
