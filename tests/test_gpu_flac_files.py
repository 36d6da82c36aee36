"""Files -> beats with the FLAC decode on the MI355X: the same audio as a WAV and as a FLAC file through
Audio2Frames.files2waves, File2Beats.many, File2Beats(device_decode=True) and ``cli.run(..., device_decode=True, batch=N)``
-- waveforms bit for bit, beats array-equal, the command line's outputs byte for byte --, a corrupt FLAC file that fails
alone with ``load_audio``'s message, and the defaults, which never look at a FLAC header."""
import numpy as np
import pytest
import torch

import flac_cases as F
import wav_cases as W

pytestmark = pytest.mark.gpu


def _ints(seconds, seed, sr, bits, channels):
    from beat_this_amd import weights

    x = weights.synthetic_audio(seconds, seed=seed, sr=sr) / 2.5
    full = (1 << (bits - 1)) - 1
    cols = [x] + [0.5 * np.roll(x, 7 * c) for c in range(1, channels)]
    return np.clip(np.round(np.stack(cols, 1) * full), -full - 1, full).astype(np.int64)


def _flac(name, pcm, bps, rate, block, stereo):
    frames = []
    for k, at in enumerate(range(0, len(pcm), block)):
        n = min(block, len(pcm) - at)
        porder = 4 if n % 16 == 0 else 0          # (the last frame is whatever is left)
        lpc = dict(type="lpc", coefs=[7800, -3100, 900, -300], precision=14, shift=12, porder=porder)
        fixed = dict(type="fixed", order=2, porder=porder)
        sub = [lpc if (k + c) % 2 == 0 else fixed for c in range(pcm.shape[1])]
        frames.append(dict(n=n, subframes=sub, **({"assign": (8, 9, 10, 1)[k % 4]} if stereo else {})))
    return F.build(name, pcm, bps, rate, frames, extra_blocks=[(4, b"\0" * 40), (1, bytes(1000))], max_block=block)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """x: 6 s of 16-bit stereo at 44100 Hz as x.wav and x.flac (frames of 4096, LPC and fixed subframes, all stereo modes);
    y: 5 s of 24-bit mono at 22050 Hz as y.wav and y.flac (frames of 1152); the checkpoint."""
    from oracle.cases import CLI_CASE, lightning_checkpoint

    root = tmp_path_factory.mktemp("flac_files")
    audio = root / "audio"
    audio.mkdir()
    ck = root / "m.ckpt"
    torch.save(lightning_checkpoint(CLI_CASE["hparams"], CLI_CASE["weight_seed"], CLI_CASE["style"], False), ck)
    x = _ints(6.0, 3, 44100, 16, 2)
    y = _ints(5.0, 4, 22050, 24, 1)
    W.write_wav(audio / "x.wav", "s16", x, rate=44100)
    W.write_wav(audio / "y.wav", "s24", y, rate=22050)
    cx, cy = _flac("x", x, 16, 44100, 4096, True), _flac("y", y, 24, 22050, 1152, False)
    (audio / "x.flac").write_bytes(cx.data)
    (audio / "y.flac").write_bytes(cy.data)
    return dict(ck=ck, dir=audio, paths={n: audio / n for n in ("x.wav", "x.flac", "y.wav", "y.flac")}, cases=dict(x=cx, y=cy))


@pytest.fixture(scope="module")
def f2b(files):
    from beat_this_amd.inference import File2Beats

    return File2Beats(str(files["ck"]), "cuda:0", float16=False, dbn=False)


def test_wav_and_flac_of_the_same_audio_give_the_same_waveforms(files, f2b):
    from beat_this_amd import flac, wav

    P = files["paths"]
    assert flac.probe(P["x.flac"]) is not None and wav.probe(P["x.flac"]) is None and flac.probe(P["x.wav"]) is None
    order = ["x.wav", "y.flac", "x.flac", "y.wav"]
    waves = dict(zip(order, f2b.files2waves([P[n] for n in order])))
    for stem, rate in (("x", 44100), ("y", 22050)):
        (a, ra), (b, rb) = waves[stem + ".wav"], waves[stem + ".flac"]
        assert ra == rb == rate and b.is_cuda and b.dtype == torch.float32 and b.data_ptr() % 16 == 0
        assert W.same_bits(b.cpu().numpy(), a.cpu().numpy()) is None
        assert W.same_bits(b.cpu().numpy(), files["cases"][stem].reference()) is None
        # one file alone (bt_flac_decode, no device table), and the single-file entry point
        (c, rc), = f2b.files2waves([str(P[stem + ".flac"])])
        d, rd = f2b.file2wave(P[stem + ".flac"])
        assert rc == rd == rate and torch.equal(c, b) and torch.equal(d, b)


def test_many_and_device_decode_give_identical_beats(files, f2b):
    from beat_this_amd.inference import File2Beats

    P = files["paths"]
    got = f2b.many([P["x.wav"], P["x.flac"], P["y.flac"], P["y.wav"]])
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]) and len(got[0][0]) > 2
    assert np.array_equal(got[2][0], got[3][0]) and np.array_equal(got[2][1], got[3][1]) and len(got[2][0]) > 2
    on = File2Beats(str(files["ck"]), "cuda:0", float16=False, dbn=False, device_decode=True)
    on.model = f2b.model
    for name, k in (("x.flac", 0), ("y.flac", 2)):
        wav_beats = on(str(P[name.replace(".flac", ".wav")]))
        beats = on(str(P[name]))
        assert np.array_equal(beats[0], wav_beats[0]) and np.array_equal(beats[1], wav_beats[1])
        assert len(beats[0]) == len(got[k][0])


def _run(files, out, **kw):
    from beat_this_amd import cli

    args = dict(inputs=[str(files["dir"])], model=str(files["ck"]), output=str(out), suffix=".beats", append=False,
                skip_existing=False, touch_first=False, dbn=False, gpu=0, float16=False, activations=False)
    args.update(kw)
    out.mkdir(exist_ok=True)
    cli.run(**args)


def _messages(err):
    import re

    return re.findall(r'Could not process "[^"]*"\. Rerun with this file alone for details\.', err)


def test_cli_batch_writes_identical_beats_and_a_corrupt_flac_fails_alone(files, f2b, tmp_path, capsys):
    from beat_this_amd.inference import File2Beats
    from beat_this_amd.preprocessing import load_audio

    c = files["cases"]["y"]
    data = bytearray(c.data)
    data[c.frame_starts[3] + 40] ^= 0x10                       # one bit inside the fourth frame: its CRC-16 no longer holds
    bad = files["dir"] / "xx_corrupt.flac"
    bad.write_bytes(bytes(data))
    try:
        with pytest.raises(RuntimeError, match="Could not load audio") as host:
            load_audio(str(bad))                               # what this file meets on the host route, today and here
        on = File2Beats(str(files["ck"]), "cuda:0", float16=False, dbn=False, device_decode=True)
        on.model = f2b.model
        assert on.file2wave(bad) is None
        with pytest.raises(RuntimeError) as device:
            on(str(bad))
        assert str(device.value) == str(host.value)
        with pytest.raises(RuntimeError, match="Could not load audio"):
            f2b.files2waves([files["paths"]["x.flac"], bad])
        out = tmp_path / "out"
        _run(files, out, device_decode=True, batch=2)
        msgs = _messages(capsys.readouterr().err)
    finally:
        bad.unlink()
    got = {p.name: p.read_bytes() for p in sorted(out.iterdir())}
    assert sorted(got) == ["x.beats", "y.beats"]
    assert len(msgs) == 1 and "xx_corrupt.flac" in msgs[0]
    assert len(got["x.beats"]) > 20 and len(got["y.beats"]) > 20
    # x.wav and x.flac (and y.*) share an output name: the WAV files and the FLAC files apart, compared byte for byte
    outs = []
    for ext in (".wav", ".flac"):
        o = tmp_path / ext[1:]
        _run(files, o, inputs=[str(files["paths"]["x" + ext]), str(files["paths"]["y" + ext])], device_decode=True, batch=2)
        outs.append({p.name: p.read_bytes() for p in sorted(o.iterdir())})
    assert outs[0] == outs[1] == got
    assert _messages(capsys.readouterr().err) == []


def test_defaults_never_probe_a_flac_file(files, tmp_path, monkeypatch):
    from beat_this_amd import cli, flac, inference

    calls = []
    for mod, name in ((flac, "probe"), (flac, "read_raw"), (inference.Audio2Frames, "_flac2waves")):
        real = getattr(mod, name)
        monkeypatch.setattr(mod, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])
    wavs = [str(files["paths"]["x.wav"]), str(files["paths"]["y.wav"])]
    _run(files, tmp_path / "o1", inputs=wavs)
    cli.run(inputs=wavs[:1], model=str(files["ck"]), output=str(tmp_path / "one.beats"), suffix=".beats", append=False,
            skip_existing=False, touch_first=False, dbn=False, gpu=0, float16=False, activations=False)
    assert calls == []
    _run(files, tmp_path / "o2", inputs=[str(files["paths"]["x.flac"]), str(files["paths"]["y.flac"])], device_decode=True, batch=2)
    assert {"probe", "read_raw", "_flac2waves"} <= set(calls)
    assert {p.name: p.read_bytes() for p in (tmp_path / "o2").iterdir()} == {p.name: p.read_bytes() for p in (tmp_path / "o1").iterdir()}
