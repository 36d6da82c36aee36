"""mir_eval.beat's goto, p_score and information_gain on the MI355X (csrc/metrics.hip, bt_beat_metrics_ext): the ragged device
call against the host code (which test_beat_metrics_ext.py holds to the numpy oracle) under that test's gates, twice for
repeatability, under guard bands and poisoned memory, and through beat_metrics_many and the bundle evaluator."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import metrics_ext_util as U
import metrics_reference as R
from conftest import ROOT
from gpu_util import POISONS, Guarded, assert_intact, dev, report

pytestmark = pytest.mark.gpu

PSCORE_TRACK = (np.array([10.001, 10.002, 10.003]), np.array([9.5, 10.0, 10.5]))   # one reference index: BT_METRICS_PSCORE


def device_rows(tracks, mbt=-np.inf, ext=U.EXT):
    from beat_this_amd import _lib

    ref, roff, est, eoff = U.csr(tracks)
    t = [torch.from_numpy(a).to(dev()) for a in (ref, roff, est, eoff)]
    n = len(tracks)
    L = _lib.lib()
    wsb = L.bt_beat_metrics_ext_workspace_bytes(n, int(roff[-1]), int(eoff[-1]))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev())
    out = torch.full((n, 12), -1.0, dtype=torch.float64, device=dev())
    _lib.check(L.bt_beat_metrics_ext(_lib.stream_ptr(dev()), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                                     n, float(mbt), *ext, ws.data_ptr(), wsb, out.data_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _fuzz_with_gaps():
    """the 2001 fuzz tracks with empty tracks between them, the 20 000-beat track among short ones, invalid tracks (decreasing,
    NaN, later than 30000 s) and a track without a P-score"""
    tracks = list(U.fuzz())
    long = tracks.pop()
    z = np.zeros(0)
    for i in (0, 5, 6, 300, 1500):
        tracks.insert(i, (z, z) if i % 2 == 0 else (z, np.arange(8) * 0.5))
    tracks.insert(777, long)
    tracks.insert(900, (np.array([6.0, 8.0, 7.0]), np.arange(5.0, 9.0)))
    tracks.insert(901, (np.arange(5.0, 9.0), np.array([np.nan, 6.0])))
    tracks.insert(902, PSCORE_TRACK)
    tracks.insert(903, (np.arange(5.0, 9.0), np.array([6.0, 30000.5])))
    tracks.append((np.arange(10.0), np.arange(10.0)))
    return tracks


@pytest.mark.parametrize("trim", [None, 5])
def test_device_matches_host_fuzz(trim):
    tracks = _fuzz_with_gaps()
    mbt = -np.inf if trim is None else float(trim)
    got = device_rows(tracks, mbt)
    want = U.host_rows(tracks, mbt)
    st = want[:, 11]
    assert st[900] == 2 and st[901] == 1 << 3 and st[903] == 4 << 3 and st[902] == 256
    assert np.count_nonzero(st.astype(int) & ~256) == 3 and np.count_nonzero(st == 256) >= 1
    worst = U.compare(got, want, tracks, f"device vs host, trim {trim}", mbt)
    bad = (st.astype(int) & ~256) != 0
    assert np.isnan(got[bad, :11]).all() and not np.isnan(got[~bad][:, [0, 3, 4, 11]]).any()
    assert np.count_nonzero(got[:, 0] == 1) >= 150
    again = device_rows(tracks, mbt)
    assert np.array_equal(again.view(np.int64), got.view(np.int64)), "two calls differ"
    for one in (tracks[1], tracks[777], tracks[902]):   # n_tracks = 1, and the long track alone
        U.compare(device_rows([one], mbt), U.host_rows([one], mbt), [one], "one track", mbt)
    report("beat_metrics_ext_fuzz", trim=str(trim), tracks=len(tracks), **worst)


def test_device_other_arguments():
    """other bins, thresholds and half-to-even windows than the defaults, on a part of the set"""
    tracks = _fuzz_with_gaps()[880:1000] + U.dense_tracks()
    at = lambda idx: (np.asarray(idx) - 0.5) / 100
    tracks += [(at(i), np.array([0.0, 0.02, 0.5, 1.04])) for i in ([1, 3, 6], [1, 4, 8], [1, 51, 106], [1, 64, 126])]
    for ext in ((0.35, 0.2, 0.2, 0.2, 1), (0.35, 0.2, 0.2, 1.0, 2), (0.2, 0.1, 0.3, 0.5, 40), (0.5, 0.3, 0.1, 0.05, 1024)):
        U.compare(device_rows(tracks, 5.0, ext), U.host_rows(tracks, 5.0, ext), tracks, f"device vs host, {ext}", 5.0, ext)
    assert tracks[120][1].size > 4096 and device_rows(tracks[120:121])[0, 8] > 2000   # (estimates in more than one block)
    rows = device_rows(tracks[-4:], -np.inf, (0.35, 0.2, 0.2, 1.0, 41))
    assert list(rows[:2, 7]) == [2.0, 4.0]


def test_device_guarded():
    """every buffer in its own guarded allocation, the workspace and the output poisoned (0xFF: NaN / -1; 0x7B): the same bits
    under every fill, intact bands, untouched inputs; a workspace one byte short and bins out of range launch nothing"""
    from beat_this_amd import _lib

    tracks = R.fuzz_tracks(seed=13, n_tracks=66, long_tracks=1)
    tracks.insert(3, (np.zeros(0), np.zeros(0)))
    tracks.insert(40, (np.arange(4.0), np.zeros(0)))
    tracks.insert(41, PSCORE_TRACK)
    ref, roff, est, eoff = U.csr(tracks)
    n = len(tracks)
    L = _lib.lib()
    wsb = L.bt_beat_metrics_ext_workspace_bytes(n, int(roff[-1]), int(eoff[-1]))
    assert wsb > 0
    ins = {"ref": torch.from_numpy(ref), "roff": torch.from_numpy(roff), "est": torch.from_numpy(est),
           "eoff": torch.from_numpy(eoff)}
    st = _lib.stream_ptr(dev())
    runs = []
    for p in (0x00,) + POISONS:
        g = {k: Guarded(v.shape, v.dtype).fill(p, v.to(dev())) for k, v in ins.items()}
        ws = Guarded((wsb,), torch.uint8).fill(p)
        out = Guarded((n, 12), torch.float64).fill(p)
        call = lambda bins=41, ws_bytes=wsb: L.bt_beat_metrics_ext(
            st, g["ref"].ptr(), g["roff"].ptr(), g["est"].ptr(), g["eoff"].ptr(), n, 5.0, *U.EXT[:4], bins, ws.ptr(), ws_bytes,
            out.ptr())
        _lib.check(call())
        torch.cuda.synchronize()
        assert_intact(*((f"{k} (fill 0x{p:02X})", v) for k, v in {**g, "ws": ws, "out": out}.items()))
        for k, v in ins.items():
            assert torch.equal(g[k].t.cpu(), v), f"input {k} was modified"
        runs.append(out.t.cpu().numpy().copy())
        if p == POISONS[0]:
            assert call(ws_bytes=wsb - 1) == _lib.BT_ERR_WORKSPACE
            assert call(bins=0) == _lib.BT_ERR_ARG and call(bins=1025) == _lib.BT_ERR_ARG
            torch.cuda.synchronize()
            assert np.array_equal(out.t.cpu().numpy().view(np.int64), runs[-1].view(np.int64)), "a refused call wrote"
    for p, r in zip(POISONS, runs[1:]):
        assert np.array_equal(r.view(np.int64), runs[0].view(np.int64)), f"rows differ under fill 0x{p:02X}"
    U.compare(runs[0], U.host_rows(tracks, 5.0), tracks, "guarded device vs host", 5.0)


def test_many_extended_matches_drop_ins():
    from beat_this_amd import metrics as M

    tracks = [t for t in U.fuzz()[:40] if t[0].size > 1 and t[1].size > 1][:20]
    assert len(tracks) == 20
    truths, preds = [r for r, _ in tracks], [e for _, e in tracks]
    plain = M.beat_metrics_many(truths, preds, eval_trim_beats=None)
    res = M.beat_metrics_many(truths, preds, eval_trim_beats=None, extended=True)
    assert list(res) == list(plain) + list(M.EXT_KEYS)
    for k, v in plain.items():
        assert np.array_equal(v, res[k], equal_nan=True), k
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i, (r, e) in enumerate(tracks):
            assert res["Goto"][i] == M.goto(r, e) and res["P-score"][i] == M.p_score(r, e)
            assert res["Information gain"][i] == pytest.approx(M.information_gain(r, e), rel=1e-12, abs=1e-15)
    assert (res["status_ext"] == 0).all()
    other = M.beat_metrics_many(truths, preds, eval_trim_beats=None, extended=True, bins=11, p_score_threshold=0.1)
    assert other["Information gain"][0] == pytest.approx(M.information_gain(*tracks[0], bins=11), rel=1e-12, abs=1e-15)
    assert other["P-score"][0] == M.p_score(*tracks[0], p_score_threshold=0.1)
    # a track without a P-score is invalid like any other, but only for the extended call
    truths.insert(7, PSCORE_TRACK[0])
    preds.insert(7, PSCORE_TRACK[1])
    assert M.beat_metrics_many(truths, preds, eval_trim_beats=None)["status"][7] == 0
    with pytest.raises(ValueError, match="track 7: p_score undefined"):
        M.beat_metrics_many(truths, preds, eval_trim_beats=None, extended=True)
    kept = M.beat_metrics_many(truths, preds, eval_trim_beats=None, extended=True, raise_on_invalid=False)
    assert kept["status_ext"][7] == M.STATUS_PSCORE and np.isnan(kept["P-score"][7]) and kept["Goto"][7] == 0


# ---- the bundle evaluator ------------------------------------------------------------------------------------------------------
FPS = 50
PLAIN_KEYS = ("F-measure", "Cemgil", "CMLt", "AMLt")
NEW_KEYS = ("Goto", "P-score", "Information gain")


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """a seeded small0 checkpoint file and a bundle 'synth.npz' of two <stem>/track fp16 spectrograms of synthetic audio (as
    test_gpu_beat_metrics.py builds them)"""
    from beat_this_amd import weights as W
    from beat_this_amd.inference import Audio2Frames

    tmp = tmp_path_factory.mktemp("evalx")
    hp = W.HPARAMS["small0"]
    ckpt = {"state_dict": {"model." + k: v for k, v in W.random_state_dict(hp, seed=4, style="lively").items()},
            "hyper_parameters": dict(hp)}
    ckpt_path = tmp / "model.ckpt"
    torch.save(ckpt, ckpt_path)
    a2f = Audio2Frames(checkpoint_path=None, device=dev())
    spects = {}
    for i, sec in enumerate((31.0, 45.0)):
        sig = W.synthetic_audio(sec, seed=21 + 2 * i)
        spects[f"piece{i}/track"] = a2f.signal2spect(sig, 22050).cpu().numpy().astype(np.float16)
    bundle = tmp / "synth.npz"
    np.savez(bundle, **spects)
    ann = tmp / "annotations" / "synth" / "annotations" / "beats"
    ann.mkdir(parents=True)
    rng = np.random.default_rng(9)
    for i, s in enumerate(spects.values()):
        beats = np.arange(rng.uniform(0, 0.5), s.shape[0] / FPS, rng.uniform(0.4, 0.7))
        (ann / f"piece{i}.beats").write_text("".join(f"{float(b)!r}\t{j % 4 + 1}\n" for j, b in enumerate(beats)))
    return dict(ckpt=ckpt, ckpt_path=ckpt_path, bundle=bundle, ann=tmp / "annotations", tmp=tmp)


def test_evaluate_bundle_extended(setup, tmp_path):
    from beat_this_amd import metrics as M
    from beat_this_amd.evaluate import evaluate_bundle
    from beat_this_amd.inference import Spect2Frames
    from beat_this_amd.utils import save_beat_tsv

    s2f = Spect2Frames(setup["ckpt"], dev(), float16=True)
    plain = evaluate_bundle(None, setup["bundle"], setup["ann"], spect2frames=s2f)
    res = evaluate_bundle(None, setup["bundle"], setup["ann"], spect2frames=s2f, extended=True)
    assert "p_score_undefined" not in plain and list(plain["metrics"]) == [f"{k}_{t}" for t in ("beat", "downbeat")
                                                                          for k in PLAIN_KEYS]
    assert list(res["metrics"]) == list(plain["metrics"]) + [f"{k}_{t}" for t in ("beat", "downbeat") for k in NEW_KEYS]
    for k, v in plain["metrics"].items():
        assert np.array_equal(v, res["metrics"][k]) and plain["averaged"][k] == res["averaged"][k]
    n_beats = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in range(len(res["piece"])):
            for t, target in enumerate(("beat", "downbeat")):
                want = M.evaluate(res["truth"][i][t], res["predictions"][i][t])
                n_beats += res["predictions"][i][t].size
                assert res["metrics"][f"Goto_{target}"][i] == want["Goto"]
                assert res["metrics"][f"P-score_{target}"][i] == want["P-score"]
                assert res["metrics"][f"Information gain_{target}"][i] == pytest.approx(want["Information gain"], rel=1e-12,
                                                                                        abs=1e-15)
    assert n_beats > 0, "the seeded model predicted no beats: the comparison would be vacuous"
    for k, v in res["metrics"].items():
        assert res["averaged"][k] == np.mean(v) and res["dataset_metrics"][k]["synth"] == np.mean(v)
    assert set(res["raw"]["beat"]) >= set(M.EXT_KEYS) and res["p_score_undefined"] == {"beat": [], "downbeat": []}
    # annotations written from the model's own predictions score 1 on all three
    root = tmp_path / "ann"
    for piece, (b, d) in zip(res["piece"], res["predictions"]):
        save_beat_tsv(b, d, root / "synth" / "annotations" / "beats" / f"{piece.split('/')[1]}.beats")
    again = evaluate_bundle(None, setup["bundle"], root, spect2frames=s2f, extended=True)
    scored = again["raw"]["beat"]["n_ref"] >= 5   # (Goto's slice needs two inner beats for its std)
    assert scored.any()
    for k in NEW_KEYS:
        assert (again["metrics"][f"{k}_beat"][scored] == 1).all(), (k, again["metrics"][f"{k}_beat"])
    report("evaluate_bundle_extended", beats=n_beats, goto_beat=float(res["averaged"]["Goto_beat"]),
           pscore_beat=float(res["averaged"]["P-score_beat"]), ig_beat=float(res["averaged"]["Information gain_beat"]))


def test_cli_all_metrics(setup):
    cmd = [sys.executable, "-m", "beat_this_amd.evaluate", "--models", str(setup["ckpt_path"]), "--bundle", str(setup["bundle"]),
           "--annotations", str(setup["ann"])]
    env = dict(os.environ, PYTHONPATH=ROOT)
    outs = []
    for extra in ([], ["--all-metrics"]):
        r = subprocess.run(cmd + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(r.stdout)
    plain, full = outs
    for target in ("beat", "downbeat"):
        for k in PLAIN_KEYS:
            assert f"\n{k}_{target}: " in plain and f"\n{k}_{target}: " in full
        for k in NEW_KEYS:
            assert f"\n{k}_{target}: " in full and f"\n{k}_{target}\nsynth: " in full
            assert f"{k}_{target}" not in plain
    # without the switch the printout is today's: the "Metrics" block with it is the plain one plus the new keys' lines
    def head(out):
        lines = out.splitlines()
        return lines[:lines.index("Dataset metrics")]

    assert head(plain) == [l for l in head(full) if not l.startswith(tuple(k + "_" for k in NEW_KEYS))]
    assert len(head(full)) == len(head(plain)) + 2 * len(NEW_KEYS)
