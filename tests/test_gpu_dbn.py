"""DBN post-processing on the MI355X (csrc/dbn.hip): the device Viterbi against the host recursion and the numpy oracle
(tests/dbn_reference.py), the ragged device decode against the oracle on the same logits, and the track API / CLI with
dbn=True end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

import dbn_reference as R
from gpu_util import dev, report

pytestmark = pytest.mark.gpu


def _pp():
    from beat_this_amd.postprocessor import Postprocessor

    return Postprocessor(type="dbn")


def _device_viterbi(pp, h, dens):
    from beat_this_amd import _lib

    lib = _lib.lib()
    T = len(dens)
    tab = pp._dbn_tables.ctypes.data
    d_dens = torch.from_numpy(dens).to(dev())
    path = torch.full((max(T, 1),), -1, dtype=torch.int32, device=dev())
    lp = torch.zeros(1, dtype=torch.float64, device=dev())
    ws = torch.empty(lib.bt_dbn_workspace_bytes(tab, 1, T), dtype=torch.uint8, device=dev())
    _lib.check(lib.bt_dbn_viterbi(_lib.stream_ptr(dev()), tab, pp._dbn_device_tables(dev()).data_ptr(), h, d_dens.data_ptr(), T,
                                  path.data_ptr(), lp.data_ptr(), ws.data_ptr(), ws.numel()))
    torch.cuda.synchronize()
    return path.cpu().numpy()[:T], float(lp.item())


def _host_viterbi(pp, h, dens):
    from beat_this_amd import _lib

    T = len(dens)
    path = np.zeros(max(T, 1), np.int32)
    lp = C.c_double()
    _lib.check(_lib.lib().bt_dbn_viterbi_host(pp._dbn_tables.ctypes.data, h, dens.ctypes.data, T, path.ctypes.data, C.byref(lp)))
    return path[:T], lp.value


@pytest.mark.parametrize("T", [1, 13, 14, 15, 1500, 15000])
def test_device_viterbi_bit_identical_to_host_and_oracle(T):
    pp = _pp()
    rng = np.random.default_rng(T)
    dens = np.log(rng.random((T, 3)) * 0.999 + 1e-4)
    for h, hmm in enumerate(R.hmms()):
        gp, gl = _device_viterbi(pp, h, dens)
        hp, hl = _host_viterbi(pp, h, dens)
        assert np.array_equal(gp, hp) and np.float64(gl).view(np.int64) == np.float64(hl).view(np.int64), (T, h)
        if T <= 1500:   # (the oracle keeps a T x states backpointer table; 15000 frames is covered by the host recursion)
            op, ol = R.viterbi(hmm, dens)
            assert np.array_equal(gp, op) and gl == ol, (T, h)


def _logits(T, seed):
    rng = np.random.default_rng(seed)
    return (torch.from_numpy(rng.normal(size=T) * 3 - 1).float(), torch.from_numpy(rng.normal(size=T) * 3 - 3).float())


def test_device_decode_single_batched_masked_and_ragged_match_oracle():
    pp = _pp()
    # single track
    b, d = _logits(3000, 1)
    gb, gd = pp(b.to(dev()), d.to(dev()))
    ob, od = R.postp_dbn(b, d)
    assert np.array_equal(gb, ob) and np.array_equal(gd, od)
    # batch with a padding mask
    B, T = 3, 1200
    bb = torch.stack([_logits(T, 10 + k)[0] for k in range(B)])
    dd = torch.stack([_logits(T, 10 + k)[1] for k in range(B)])
    mask = torch.ones(B, T, dtype=torch.bool)
    mask[1, 900:] = False
    mask[2, 40:] = False
    gb, gd = pp(bb.to(dev()), dd.to(dev()), mask.to(dev()))
    for k in range(B):
        ob, od = R.postp_dbn(bb[k][mask[k]], dd[k][mask[k]])
        assert np.array_equal(gb[k], ob) and np.array_equal(gd[k], od), k
    # ragged: one launch triple for 6 tracks equals per-track calls
    lens = [1, 13, 500, 2500, 0, 1800]
    tracks = [_logits(n, 30 + i) for i, n in enumerate(lens)]
    beat = torch.cat([t[0] for t in tracks]).to(dev())
    down = torch.cat([t[1] for t in tracks]).to(dev())
    off = np.concatenate([[0], np.cumsum(lens)])
    many = pp.ragged(beat, down, off)
    for k, (tb, td) in enumerate(tracks):
        one = pp(tb.to(dev()), td.to(dev()))
        assert np.array_equal(many[k][0], one[0]) and np.array_equal(many[k][1], one[1]), k
        if lens[k] <= 2500:
            ob, od = R.postp_dbn(tb, td)
            assert np.array_equal(many[k][0], ob) and np.array_equal(many[k][1], od), k
    # two runs are bit-identical
    again = pp.ragged(beat, down, off)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(many, again))


def _a2b(dbn, float16=False):
    from beat_this_amd import weights as W
    from beat_this_amd.inference import Audio2Beats
    from beat_this_amd.model import BeatThis

    hp = W.resolve_hparams("small0")
    m = BeatThis(**{k: hp[k] for k in ("spect_dim", "transformer_dim", "ff_mult", "n_layers", "head_dim", "stem_dim")})
    m.load_state_dict(W.random_state_dict(hp, seed=4, style="lively"))
    a2b = Audio2Beats(checkpoint_path=None, device=dev(), float16=float16, dbn=dbn)
    a2b.model = m.to(dev())
    return a2b


@pytest.mark.parametrize("seconds", [30.0, 300.0])
def test_audio2beats_dbn_matches_oracle_on_its_logits(seconds):
    from beat_this_amd import weights as W

    a2b = _a2b(True)
    sig = W.synthetic_audio(seconds, seed=7)
    beats, downbeats = a2b(sig, 22050)
    bl, dl = a2b.spect2frames(a2b.signal2spect(sig, 22050))
    ob, od = R.postp_dbn(bl.cpu(), dl.cpu())
    report("dbn_audio2beats", seconds=seconds, n_beats=len(beats), n_downbeats=len(downbeats))
    assert np.array_equal(beats, ob) and np.array_equal(downbeats, od)
    # the batched track API: one ragged decode for all tracks
    sigs = [sig, W.synthetic_audio(12.0, seed=8)]
    many = a2b.many(sigs, 22050)
    assert np.array_equal(many[0][0], beats) and np.array_equal(many[0][1], downbeats)
    b2, d2 = a2b(sigs[1], 22050)
    assert np.array_equal(many[1][0], b2) and np.array_equal(many[1][1], d2)


def test_f32x3_range_guard_repeats_before_the_dbn_decodes():
    """BT_PREC_F32X3 with a forward whose range flag fires: the batch is repeated on the exact path and the DBN decodes
    the repeated logits, as the minimal path does."""
    from beat_this_amd import weights as W
    from beat_this_amd.inference import Audio2Beats
    from beat_this_amd.model import BeatThis

    hp = W.resolve_hparams("small0")
    sd = W.random_state_dict(hp, seed=6, style="lively")
    sd["frontend.linear.weight"] = sd["frontend.linear.weight"] * 3.0e5
    sd["frontend.linear.bias"] = sd["frontend.linear.bias"] * 3.0e5
    m = BeatThis(**{k: hp[k] for k in ("spect_dim", "transformer_dim", "ff_mult", "n_layers", "head_dim", "stem_dim")})
    m.load_state_dict(sd)
    m = m.to(dev())
    a2b = Audio2Beats(checkpoint_path=None, device=dev(), float16="f32x3", dbn=True)
    a2b.model = m
    sigs = [W.synthetic_audio(40.0, seed=90), W.synthetic_audio(12.0, seed=91)]
    before = m.engine().last_fallbacks
    h = a2b.many_async(sigs, 22050)
    got = h.result()
    assert m.engine().last_fallbacks > before
    beat, down, off = h.logits
    assert torch.isfinite(beat).all() and torch.isfinite(down).all()
    for k in range(len(sigs)):
        ob, od = R.postp_dbn(beat[off[k]: off[k + 1]].cpu(), down[off[k]: off[k + 1]].cpu())
        assert np.array_equal(got[k][0], ob) and np.array_equal(got[k][1], od), k
    m.fp32_split_gemms = False
    want = a2b.many(sigs, 22050)
    for (gb, gd), (wb, wd) in zip(got, want):
        assert np.array_equal(gb, wb) and np.array_equal(gd, wd)


def test_file2beats_and_cli_with_dbn(tmp_path):
    from beat_this_amd import cli
    from beat_this_amd.inference import File2Beats, load_audio
    from oracle.cases import CLI_CASE, lightning_checkpoint, pcm16_wav

    ck = tmp_path / "m.ckpt"
    torch.save(lightning_checkpoint(CLI_CASE["hparams"], CLI_CASE["weight_seed"], CLI_CASE["style"], False), ck)
    wav = tmp_path / "clicks.wav"
    pcm16_wav(wav, 30.0, CLI_CASE["audio_seed"], CLI_CASE["sr"])
    f2b = File2Beats(str(ck), "cuda:0", float16=False, dbn=True)
    beats, downbeats = f2b(str(wav))
    signal, sr = load_audio(wav)
    bl, dl = f2b.spect2frames(f2b.signal2spect(signal, sr))
    ob, od = R.postp_dbn(bl.cpu(), dl.cpu())
    assert np.array_equal(beats, ob) and np.array_equal(downbeats, od)
    out = tmp_path / "clicks.beats"
    cli.run(inputs=[str(wav)], model=str(ck), output=str(out), suffix=".beats", append=False, skip_existing=False,
            touch_first=False, dbn=True, gpu=0, float16=False, activations=False)
    lines = out.read_text().splitlines()
    assert len(lines) == len(beats)
    assert [float(l.split("\t")[0]) for l in lines] == pytest.approx(list(beats))
