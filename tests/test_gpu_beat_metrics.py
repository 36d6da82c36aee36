"""Beat-tracking metrics on the MI355X (csrc/metrics.hip): the ragged device call against the host code (which
test_beat_metrics.py holds to tests/metrics_reference.py), under guard bands and poisoned memory, and the bundle evaluator
(beat_this_amd/evaluate.py) end to end against the numpy oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import metrics_reference as R
from conftest import ROOT
from gpu_util import POISONS, Guarded, assert_intact, dev, report

pytestmark = pytest.mark.gpu

EXACT = [0, 1, 2, 5, 6, 7, 8, 9, 10, 11]
TH = (0.07, 0.04, 0.175, 0.175)


def _csr(tracks):
    ref = np.concatenate([r for r, _ in tracks] + [np.zeros(1)])
    est = np.concatenate([e for _, e in tracks] + [np.zeros(1)])
    roff = np.zeros(len(tracks) + 1, np.int64)
    eoff = np.zeros(len(tracks) + 1, np.int64)
    roff[1:] = np.cumsum([r.size for r, _ in tracks])
    eoff[1:] = np.cumsum([e.size for _, e in tracks])
    return ref, roff, est, eoff


def host_rows(tracks, mbt=-np.inf):
    from beat_this_amd import _lib

    ref, roff, est, eoff = _csr(tracks)
    out = np.zeros((len(tracks), 12))
    _lib.check(_lib.lib().bt_beat_metrics_host(ref.ctypes.data, roff.ctypes.data, est.ctypes.data, eoff.ctypes.data,
                                               len(tracks), mbt, *TH, out.ctypes.data))
    return out


def _compare(got, want, what):
    bad = np.nonzero((got[:, EXACT].view(np.int64) != want[:, EXACT].view(np.int64)).any(1))[0]
    assert bad.size == 0, f"{what}: {bad.size} tracks differ, first {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"
    np.testing.assert_allclose(got[:, 3:5], want[:, 3:5], rtol=1e-12, atol=0, err_msg=what)


def _fuzz_with_gaps():
    """the fuzz set with empty tracks between non-empty ones, a few invalid tracks, and the 20 000-beat track among short ones"""
    tracks = R.fuzz_tracks(seed=12, n_tracks=2000, long_tracks=1)
    long = tracks.pop()
    z = np.zeros(0)
    for i in (0, 5, 6, 300, 1500):
        tracks.insert(i, (z, z) if i % 2 == 0 else (z, np.arange(8) * 0.5))
    tracks.insert(777, long)
    tracks.insert(900, (np.array([6.0, 8.0, 7.0]), np.arange(5.0, 9.0)))   # decreasing after the 5 s trim too
    tracks.insert(901, (np.arange(5.0, 9.0), np.array([np.nan, 6.0])))
    tracks.append((np.arange(10.0), np.arange(10.0)))
    return tracks


@pytest.mark.parametrize("trim", [None, 5])
def test_device_matches_host_fuzz(trim):
    from beat_this_amd.metrics import beat_metrics_many

    tracks = _fuzz_with_gaps()
    res = beat_metrics_many([r for r, _ in tracks], [e for _, e in tracks], eval_trim_beats=trim, raise_on_invalid=False)
    keys = ("F-measure", "Precision", "Recall", "Cemgil", "CemgilMax", "CMLc", "CMLt", "AMLc", "AMLt", "n_ref", "n_est", "status")
    got = np.stack([res[k] for k in keys], 1)
    want = host_rows(tracks, -np.inf if trim is None else float(trim))
    st = want[:, 11]
    assert np.count_nonzero(st) == 2 and np.array_equal(st, got[:, 11])
    ok = st == 0
    _compare(got[ok], want[ok], f"device vs host, trim {trim}")
    assert np.isnan(got[~ok, :9]).all()
    np.testing.assert_array_equal(res["Cemgil_reported"], (res["Cemgil"] + res["CemgilMax"]) / 2)
    rel = np.abs(got[ok, 3:5] - want[ok, 3:5]) / np.maximum(np.abs(want[ok, 3:5]), 1e-300)
    report("beat_metrics_fuzz", trim=str(trim), tracks=len(tracks), cemgil_max_rel=float(rel.max()))
    # n_tracks = 1, and the one long track alone
    for one in (tracks[1], tracks[777]):
        r1 = beat_metrics_many([one[0]], [one[1]], eval_trim_beats=trim)
        g1 = np.array([[r1[k][0] for k in keys]])
        _compare(g1, host_rows([one], -np.inf if trim is None else float(trim)), "one track")
    with pytest.raises(ValueError, match="track 900: reference events not in increasing order"):
        beat_metrics_many([r for r, _ in tracks], [e for _, e in tracks], eval_trim_beats=trim)


def test_device_guarded():
    """bt_beat_metrics with every buffer in its own guarded allocation: inputs' and output's bands poisoned, the workspace
    wholly poisoned (0xFF: NaN / -1; 0x7B) -- bit-identical rows, intact bands, the host rows; a workspace one byte short is
    refused with BT_ERR_WORKSPACE"""
    from beat_this_amd import _lib

    tracks = R.fuzz_tracks(seed=13, n_tracks=66, long_tracks=1)
    tracks.insert(3, (np.zeros(0), np.zeros(0)))
    tracks.insert(40, (np.arange(4.0), np.zeros(0)))
    ref, roff, est, eoff = _csr(tracks)
    n = len(tracks)
    L = _lib.lib()
    wsb = L.bt_beat_metrics_workspace_bytes(n, int(roff[-1]), int(eoff[-1]))
    assert wsb > 0
    ins = {"ref": torch.from_numpy(ref), "roff": torch.from_numpy(roff), "est": torch.from_numpy(est),
           "eoff": torch.from_numpy(eoff)}
    st = _lib.stream_ptr(dev())
    runs = []
    for p in (0x00,) + POISONS:
        g = {k: Guarded(v.shape, v.dtype).fill(p, v.to(dev())) for k, v in ins.items()}
        ws = Guarded((wsb,), torch.uint8).fill(p)
        out = Guarded((n, 12), torch.float64).fill(p)
        _lib.check(L.bt_beat_metrics(st, g["ref"].ptr(), g["roff"].ptr(), g["est"].ptr(), g["eoff"].ptr(), n, 5.0, *TH,
                                     ws.ptr(), wsb, out.ptr()))
        torch.cuda.synchronize()
        assert_intact(*((f"{k} (fill 0x{p:02X})", v) for k, v in {**g, "ws": ws, "out": out}.items()))
        for k, v in ins.items():
            assert torch.equal(g[k].t.cpu(), v), f"input {k} was modified"
        runs.append(out.t.cpu().numpy().copy())
        if p == POISONS[0]:
            short = L.bt_beat_metrics(st, g["ref"].ptr(), g["roff"].ptr(), g["est"].ptr(), g["eoff"].ptr(), n, 5.0, *TH,
                                      ws.ptr(), wsb - 1, out.ptr())
            assert short == _lib.BT_ERR_WORKSPACE
            torch.cuda.synchronize()
            assert torch.equal(out.t.cpu(), torch.from_numpy(runs[-1])), "a refused call wrote its output"
    for p, r in zip(POISONS, runs[1:]):
        assert np.array_equal(r.view(np.int64), runs[0].view(np.int64)), f"rows differ under fill 0x{p:02X}"
    _compare(runs[0], host_rows(tracks, 5.0), "guarded device vs host")


# ---- the bundle evaluator end to end -----------------------------------------------------------------------------------
FPS = 50


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """a seeded small0 checkpoint file, a bundle 'synth.npz' of <stem>/track fp16 spectrograms made from synthetic audio, and
    an annotation tree with two-column .beats files (one piece one-column) near the spectrograms' own pulse"""
    from beat_this_amd import weights as W
    from beat_this_amd.inference import Audio2Frames

    tmp = tmp_path_factory.mktemp("evalb")
    hp = W.HPARAMS["small0"]
    ckpt = {"state_dict": {"model." + k: v for k, v in W.random_state_dict(hp, seed=4, style="lively").items()},
            "hyper_parameters": dict(hp)}
    ckpt_path = tmp / "model.ckpt"
    torch.save(ckpt, ckpt_path)
    a2f = Audio2Frames(checkpoint_path=None, device=dev())
    spects = {}
    for i, sec in enumerate((12.0, 31.0, 7.5, 45.0)):
        sig = W.synthetic_audio(sec, seed=20 + i)
        spects[f"piece{i}/track"] = a2f.signal2spect(sig, 22050).cpu().numpy().astype(np.float16)
    bundle = tmp / "synth.npz"
    np.savez(bundle, **spects)
    ann = tmp / "annotations" / "synth" / "annotations" / "beats"
    ann.mkdir(parents=True)
    rng = np.random.default_rng(9)
    for i, (k, s) in enumerate(spects.items()):
        dur = s.shape[0] / FPS
        beats = np.arange(rng.uniform(0, 0.5), dur + 3, rng.uniform(0.4, 0.7))   # some past the end: cut by the evaluator
        if i == 2:
            (ann / f"piece{i}.beats").write_text("".join(f"{float(b)!r}\n" for b in beats))
        else:
            (ann / f"piece{i}.beats").write_text("".join(f"{float(b)!r}\t{j % 4 + 1}\n" for j, b in enumerate(beats)))
    return dict(ckpt=ckpt, ckpt_path=ckpt_path, bundle=bundle, ann=tmp / "annotations", tmp=tmp, spects=spects)


def _oracle_metrics(truth, preds, trim=5):
    """the script's per-piece values from the numpy oracle: F, (cemgil + cemgil_max) / 2, CMLt, AMLt"""
    r = R.trim_beats(truth, trim)
    e = R.trim_beats(preds, trim)
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = R.cemgil(r, e)
        cont = R.continuity(r, e)
        return R.f_measure(r, e), np.mean(c), cont[1], cont[3]


@pytest.mark.parametrize("dbn", [False, True])
@pytest.mark.parametrize("float16", [False, True])
def test_evaluate_bundle_matches_oracle(setup, dbn, float16):
    from beat_this_amd.bundle import SpectBundle, predict_bundle
    from beat_this_amd.evaluate import evaluate_bundle, load_beat_annotations
    from beat_this_amd.inference import Spect2Frames
    from beat_this_amd.postprocessor import Postprocessor

    s2f = Spect2Frames(setup["ckpt"], dev(), float16=float16)
    res = evaluate_bundle(None, setup["bundle"], setup["ann"], float16=float16, dbn=dbn, spect2frames=s2f)
    assert list(res["piece"]) == [f"synth/piece{i}/track.npy" for i in range(4)] and set(res["dataset"]) == {"synth"}
    # the same Spect2Frames + Postprocessor outputs, computed here
    post = Postprocessor(type="dbn" if dbn else "minimal")
    with SpectBundle(setup["bundle"]) as bun:
        mine = {k: post(b, d) for k, b, d in predict_bundle(s2f, bun)}
    n_beats = 0
    for i, piece in enumerate(res["piece"]):
        key = f"piece{i}/track"
        pb, pd = res["predictions"][i]
        assert np.array_equal(pb, mine[key][0]) and np.array_equal(pd, mine[key][1])
        n_beats += pb.size
        tb, td = load_beat_annotations(setup["ann"] / "synth" / "annotations" / "beats" / f"piece{i}.beats")
        end = setup["spects"][key].shape[0] / FPS
        tb, td = tb[tb < end], td[td < end]
        for target, t, p in (("beat", tb, pb), ("downbeat", td, pd)):
            want = _oracle_metrics(t, p)
            got = [res["metrics"][f"{k}_{target}"][i] for k in ("F-measure", "Cemgil", "CMLt", "AMLt")]
            assert got[0] == want[0] and got[2] == want[2] and got[3] == want[3], (piece, target, got, want)
            assert got[1] == pytest.approx(want[1], rel=1e-12, abs=0)
    assert n_beats > 0, "the seeded model predicted no beats: the comparison would be vacuous"
    for k, v in res["metrics"].items():
        assert res["averaged"][k] == np.mean(v) and res["dataset_metrics"][k]["synth"] == np.mean(v)
    report("evaluate_bundle", dbn=dbn, float16=float16, beats=n_beats, F_beat=float(res["averaged"]["F-measure_beat"]))


def test_self_annotations_score_one(setup, tmp_path):
    """annotations written from the model's own predictions (.beats with inferred beat numbers) score F = 1"""
    from beat_this_amd.evaluate import evaluate_bundle
    from beat_this_amd.inference import Spect2Frames
    from beat_this_amd.utils import save_beat_tsv

    s2f = Spect2Frames(setup["ckpt"], dev(), float16=True)
    first = evaluate_bundle(None, setup["bundle"], setup["ann"], spect2frames=s2f)
    root = tmp_path / "ann"
    for piece, (b, d) in zip(first["piece"], first["predictions"]):
        stem = piece.split("/")[1]
        save_beat_tsv(b, d, root / "synth" / "annotations" / "beats" / f"{stem}.beats")
    again = evaluate_bundle(None, setup["bundle"], root, spect2frames=s2f)
    scored = again["raw"]["beat"]["n_ref"] > 0
    assert scored.any()
    assert (again["metrics"]["F-measure_beat"][scored] == 1).all()
    dscored = again["raw"]["downbeat"]["n_ref"] > 0
    assert (again["metrics"]["F-measure_downbeat"][dscored] == 1).all()


def test_cli_blocks_and_dump(setup, tmp_path):
    from beat_this_amd.evaluate import evaluate_bundle
    from beat_this_amd.inference import Spect2Frames
    from beat_this_amd.utils import infer_beat_numbers

    dump = tmp_path / "preds.npz"
    cmd = [sys.executable, "-m", "beat_this_amd.evaluate", "--models", str(setup["ckpt_path"]), "--bundle", str(setup["bundle"]),
           "--annotations", str(setup["ann"]), "--dump-predictions", str(dump)]
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = r.stdout
    assert "Metrics\n" in out and "Dataset metrics\n" in out
    for target in ("beat", "downbeat"):
        for k in ("F-measure", "Cemgil", "CMLt", "AMLt"):
            assert f"\n{k}_{target}: " in out and f"\n{k}_{target}\nsynth: " in out
    res = evaluate_bundle(None, setup["bundle"], setup["ann"], spect2frames=Spect2Frames(setup["ckpt"], dev(), float16=True))
    assert f"F-measure_beat: {res['averaged']['F-measure_beat']}\n" in out
    saved = np.load(dump)
    assert sorted(saved.files) == sorted(res["piece"])
    for piece, (b, d) in zip(res["piece"], res["predictions"]):
        a = saved[piece]
        assert np.array_equal(a[:, 0], b) and np.array_equal(a[:, 1], infer_beat_numbers(b, d))
    # two models: mean +- std rounded to 3 places; no dump with several models
    r2 = subprocess.run(cmd[:5] + [str(setup["ckpt_path"])] + cmd[5:-2], cwd=ROOT, env=env, capture_output=True, text=True,
                        timeout=600)
    assert r2.returncode == 0, r2.stderr[-3000:]
    f = round(float(res["averaged"]["F-measure_beat"]), 3)
    assert f"F-measure_beat: {f} +- 0.0\n" in r2.stdout
    r3 = subprocess.run(cmd[:5] + [str(setup["ckpt_path"])] + cmd[5:], cwd=ROOT, env=env, capture_output=True, text=True,
                        timeout=600)
    assert "cannot dump predictions when doing inference for multiple models" in r3.stdout
