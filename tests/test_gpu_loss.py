"""The training losses on the MI355X (csrc/loss.hip): the device against the host twin bit for bit, reproducibility and
batch independence, the autograd modules against the reference's recorded values and gradients (fp32, fp16, bf16, autocast),
capture in a CUDA graph, guard bands and poisoned memory, and ``evaluate --loss`` end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import loss_reference as R
from conftest import ROOT
from gpu_util import POISONS, Guarded, assert_intact, dev, report
from test_loss import CASES, KINDS, ORACLE, check_against_golden

pytestmark = pytest.mark.gpu


def _ragged(seed, n_rows, tol=3, max_len=900):
    rows = R.fuzz_rows(seed=seed, n_rows=n_rows, tol=tol, max_len=max_len)
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([x.size for x, _, _ in rows])
    return (np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows]), np.concatenate([r[2] for r in rows]),
            off)


def device_call(kind, tol, pw, x, y, m, off):
    """bt_bce_loss on fresh device buffers -> numpy dict of every output"""
    from beat_this_amd import _lib

    L = _lib.lib()
    d = dev()
    n, lens = off.size - 1, np.diff(off)
    X, Y, OFF = (torch.from_numpy(a).to(d) for a in (x, y, off))
    M = None if m is None else torch.from_numpy(m).to(d)
    wsb = L.bt_bce_loss_workspace_bytes(n, int(lens.max()))
    ws = torch.empty(wsb, dtype=torch.uint8, device=d)
    rs = torch.empty(n, dtype=torch.float64, device=d)
    rc = torch.empty(n, dtype=torch.int64, device=d)
    loss = torch.empty((), dtype=torch.float32, device=d)
    g = torch.empty(x.size, dtype=torch.float32, device=d)
    t = torch.empty(x.size, dtype=torch.float32, device=d)
    _lib.check(L.bt_bce_loss(_lib.stream_ptr(d), kind, tol, pw, None, X.data_ptr(), 0, Y.data_ptr(), 0, _lib.ptr(M), 0,
                             OFF.data_ptr(), n, int(lens.min()), int(lens.max()), ws.data_ptr(), wsb, rs.data_ptr(),
                             rc.data_ptr(), loss.data_ptr(), 0, g.data_ptr(), t.data_ptr()))
    torch.cuda.synchronize()
    return dict(row_sum=rs.cpu().numpy(), row_count=rc.cpu().numpy(), loss=float(loss), grad=g.cpu().numpy(),
                terms=t.cpu().numpy())


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _same(a, b, what=""):
    """bit-identical, NaN payloads aside (a NaN made on the device is not the x86 host's default NaN) -> "" or a description
    of the first differences"""
    na, nb = np.isnan(a), np.isnan(b)
    ca, cb = np.where(na, 0, a).astype(a.dtype), np.where(nb, 0, b).astype(b.dtype)
    bad = np.flatnonzero((na != nb) | (ca.view(np.uint32 if a.dtype == np.float32 else np.uint64) !=
                                       cb.view(np.uint32 if b.dtype == np.float32 else np.uint64)))
    if bad.size == 0:
        return ""
    return f"{what}: {bad.size} of {a.size} differ, first " + ", ".join(f"[{i}] {a[i]!r} vs {b[i]!r}" for i in bad[:5])


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_device_matches_host_bitwise(kind):
    """terms and gradients bit-identical to bt_bce_loss_host (NaN payloads aside), row sums within 1e-12 (the same trees);
    a second run identical; a row alone identical to the same row inside the ragged batch"""
    from beat_this_amd.loss import loss_host

    x, y, m, off = _ragged(60 + kind, 300)
    x[5] = np.nan        # a NaN in row 0, infinities further on
    x[off[3] + 20] = np.inf
    x[off[4] + 30] = -np.inf
    h = loss_host(kind, 3, 2.7, x, y, m, off)
    a = device_call(kind, 3, 2.7, x, y, m, off)
    msg = _same(a["terms"], h["terms"], "terms") + _same(a["grad"], h["grad"], "grad")
    assert not msg, msg
    assert np.array_equal(a["row_count"], h["row_count"])
    fin = np.isfinite(h["row_sum"])
    assert np.array_equal(np.isnan(a["row_sum"]), np.isnan(h["row_sum"]))
    np.testing.assert_allclose(a["row_sum"][fin], h["row_sum"][fin], rtol=1e-12, atol=0)
    b = device_call(kind, 3, 2.7, x, y, m, off)
    for k in ("terms", "grad", "row_sum", "row_count"):
        assert _bits_equal(a[k], b[k]), k
    for r in (7, 150, 299):
        s = slice(off[r], off[r + 1])
        one = device_call(kind, 3, 2.7, x[s].copy(), y[s].copy(), m[s].copy(), np.array([0, off[r + 1] - off[r]], np.int64))
        assert _bits_equal(one["grad"], a["grad"][s]) and _bits_equal(one["terms"], a["terms"][s])
        assert _bits_equal(one["row_sum"], a["row_sum"][r:r + 1])
    report("loss_device_vs_host", kind=kind, rows=300, frames=int(off[-1]),
           row_sums_identical=not _same(a["row_sum"], h["row_sum"]))


def _module(c):
    from beat_this_amd.model.loss import MaskedBCELoss, ShiftTolerantBCELoss, SplittedShiftTolerantBCELoss

    cls = {"MaskedBCELoss": MaskedBCELoss, "ShiftTolerantBCELoss": ShiftTolerantBCELoss,
           "SplittedShiftTolerantBCELoss": SplittedShiftTolerantBCELoss}[c["cls"]]
    return cls(pos_weight=c["pw"]) if c["cls"] == "MaskedBCELoss" else cls(pos_weight=c["pw"], tolerance=c["tol"])


def _run_module(c, dtype, autocast=False, module_on_gpu=True):
    d = dev()
    fn = _module(c)
    if module_on_gpu:
        fn = fn.to(d)
    x = torch.from_numpy(c["x"]).to(d, dtype).requires_grad_(True)
    y = torch.from_numpy(c["y"]).to(d, torch.float16 if c["dtype"] == "float16" else torch.float32)
    m = None if c["m"] is None else torch.from_numpy(c["m"]).to(d)
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        v = fn(x, y, m) if (m is not None or c["cls"].startswith("Splitted")) else fn(x, y)
    v.backward()
    return v, x.grad


def test_backward_matches_reference_golden():
    n = 0
    for c in CASES:
        dtype = torch.float16 if c["dtype"] == "float16" else torch.float32
        v, g = _run_module(c, dtype, module_on_gpu=c["i"] % 2 == 0)
        assert v.dtype == dtype and v.dim() == 0 and g.dtype == dtype
        check_against_golden(c, float(v.detach()), g.double().cpu().numpy())
        n += 1
    report("loss_backward_golden", cases=n)


def test_bf16_and_autocast():
    """bf16 logits: value and gradient against the oracle on the bf16-rounded logits; under autocast the result is fp32 and
    equals the fp32 result"""
    for c in CASES:
        if c["dtype"] != "float32" or not np.isfinite(c["value"]):
            continue
        v, g = _run_module(c, torch.bfloat16)
        assert v.dtype == torch.bfloat16 and g.dtype == torch.bfloat16
        xb = torch.from_numpy(c["x"]).to(torch.bfloat16).double().numpy()
        ov, og = R.loss(ORACLE[KINDS[c["cls"]]], c["tol"], c["pw"], xb, c["y"].astype(np.float64), c["m"])
        assert float(v) == pytest.approx(ov, rel=1e-2, abs=1e-3), c["i"]
        gg = g.double().cpu().numpy()
        assert np.abs(gg - og).max() <= 1e-2 * max(np.abs(og).max(), 1e-30), c["i"]
        va, ga = _run_module(c, torch.float32, autocast=True)
        v32, g32 = _run_module(c, torch.float32)
        assert va.dtype == torch.float32 and torch.equal(va, v32) and torch.equal(ga, g32), c["i"]


def test_module_errors_on_gpu():
    from beat_this_amd.model.loss import ShiftTolerantBCELoss, SplittedShiftTolerantBCELoss

    d = dev()
    fn = ShiftTolerantBCELoss()
    with pytest.raises(RuntimeError):
        fn(torch.zeros(30, device=d), torch.zeros(30, device=d))   # 1-D with a tolerance
    with pytest.raises(RuntimeError):
        fn(torch.zeros(2, 12, device=d), torch.zeros(2, 12, device=d))   # T < 1 + 4 tol
    fn(torch.zeros(2, 13, device=d), torch.zeros(2, 13, device=d))
    with pytest.raises(ValueError):
        fn(torch.zeros(2, 20, device=d), torch.zeros(2, 21, device=d))
    one = ShiftTolerantBCELoss(tolerance=0)(torch.zeros(30, device=d), torch.zeros(30, device=d))   # no pooling: any shape
    assert float(one) == pytest.approx(np.log(2), rel=1e-6)
    with pytest.raises(TypeError):
        SplittedShiftTolerantBCELoss()(torch.zeros(2, 20, device=d), torch.zeros(2, 20, device=d))


def test_graph_capture_and_replay():
    """forward + backward captured in a CUDA graph (no host synchronisation inside): replays give the eager bits, also after
    new logits are copied into the captured input"""
    from beat_this_amd.model.loss import ShiftTolerantBCELoss

    d = dev()
    gen = torch.Generator(device="cpu").manual_seed(3)
    x = (torch.randn(8, 1500, generator=gen) * 3).to(d).requires_grad_(True)
    y = (torch.rand(8, 1500, generator=gen) < 0.04).float().to(d)
    m = (torch.rand(8, 1500, generator=gen) < 0.95).to(d)
    fn = ShiftTolerantBCELoss(pos_weight=2.7).to(d)

    def eager():
        x.grad = None
        v = fn(x, y, m)
        v.backward()
        return v.detach().clone(), x.grad.clone()

    v0, g0 = eager()
    s = torch.cuda.Stream(d)
    s.wait_stream(torch.cuda.current_stream(d))
    with torch.cuda.stream(s):
        for _ in range(3):
            eager()
    torch.cuda.current_stream(d).wait_stream(s)
    x.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sv = fn(x, y, m)
        sv.backward()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(sv, v0) and torch.equal(x.grad, g0)
    new = (torch.randn(8, 1500, generator=gen) * 3).to(d)
    with torch.no_grad():
        x.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    vg, gg = sv.clone(), x.grad.clone()
    v1, g1 = eager()
    assert torch.equal(vg, v1) and torch.equal(gg, g1) and not torch.equal(v1, v0)


def test_device_guarded():
    """bt_bce_loss and bt_bce_loss_backward with every buffer in its own guarded allocation: input bands poisoned, the
    workspace and every output wholly poisoned (0xFF, 0x7B) -- bit-identical outputs, intact bands, unmodified inputs; a
    workspace one byte short is refused with BT_ERR_WORKSPACE and writes nothing"""
    from beat_this_amd import _lib

    L = _lib.lib()
    x, y, m, off = _ragged(71, 40, max_len=1300)
    n, N, lens = off.size - 1, x.size, np.diff(off)
    wsb = L.bt_bce_loss_workspace_bytes(n, int(lens.max()))
    ins = {"x": torch.from_numpy(x), "y": torch.from_numpy(y), "m": torch.from_numpy(m), "off": torch.from_numpy(off),
           "go": torch.tensor([0.75], dtype=torch.float32)}
    st = _lib.stream_ptr(dev())
    runs = []
    for p in (0x00,) + POISONS:
        g = {k: Guarded(v.shape, v.dtype).fill(p, v.to(dev())) for k, v in ins.items()}
        ws = Guarded((wsb,), torch.uint8).fill(p)
        outs = {"rs": Guarded((n,), torch.float64).fill(p), "rc": Guarded((n,), torch.int64).fill(p),
                "loss": Guarded((1,), torch.float32).fill(p), "grad": Guarded((N,), torch.float32).fill(p),
                "terms": Guarded((N,), torch.float32).fill(p), "gin": Guarded((N,), torch.float16).fill(p)}

        def call(wsbytes):
            return L.bt_bce_loss(st, 1, 3, 2.7, None, g["x"].ptr(), 0, g["y"].ptr(), 0, g["m"].ptr(), 0, g["off"].ptr(), n,
                                 int(lens.min()), int(lens.max()), ws.ptr(), wsbytes, outs["rs"].ptr(), outs["rc"].ptr(),
                                 outs["loss"].ptr(), 0, outs["grad"].ptr(), outs["terms"].ptr())

        if p == POISONS[0]:
            assert call(wsb - 1) == _lib.BT_ERR_WORKSPACE
            torch.cuda.synchronize()
            assert (outs["grad"].t.view(torch.uint8) == p).all(), "a refused call wrote its output"
        _lib.check(call(wsb))
        _lib.check(L.bt_bce_loss_backward(st, outs["grad"].ptr(), N, g["go"].ptr(), 0, int((lens - 12).sum()),
                                          outs["gin"].ptr(), 1))
        torch.cuda.synchronize()
        assert_intact(*((f"{k} (fill 0x{p:02X})", v) for k, v in {**g, **outs, "ws": ws}.items()))
        for k, v in ins.items():
            assert torch.equal(g[k].t.cpu(), v), f"input {k} was modified"
        runs.append({k: v.t.cpu().numpy().copy() for k, v in outs.items()})
    for p, r in zip(POISONS, runs[1:]):
        for k in r:
            assert _bits_equal(r[k], runs[0][k]), f"{k} differs under fill 0x{p:02X}"
    from beat_this_amd.loss import loss_host

    h = loss_host(1, 3, 2.7, x, y, m, off)
    msg = _same(runs[0]["grad"], h["grad"], "grad") + _same(runs[0]["terms"], h["terms"], "terms")
    assert not msg, msg
    want = (h["grad"] * np.float32(0.75 / int((lens - 12).sum()))).astype(np.float16)
    assert np.abs(runs[0]["gin"].astype(np.float64) - want.astype(np.float64)).max() <= 1e-3 * np.abs(want).max()
    assert runs[0]["loss"][0] == pytest.approx(h["loss"], rel=1e-6)


def test_piece_losses_names_a_short_piece():
    from beat_this_amd.loss import ShiftTolerantBCELoss, piece_losses

    d = dev()
    lg = [torch.zeros(40, device=d), torch.zeros(12, device=d)]
    with pytest.raises(ValueError, match="piece ds/b/track.npy has 12 frames"):
        piece_losses(ShiftTolerantBCELoss(), lg, [np.zeros(40), np.zeros(12)], names=["ds/a/track.npy", "ds/b/track.npy"])


# ---- evaluate --loss end to end ------------------------------------------------------------------------------------------
FPS = 50
PW = {"beat": 2.5, "downbeat": 6.0}


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """a seeded small0 checkpoint (loss_type and pos_weights in its hyper-parameters), a bundle of fp16 spectrograms from
    synthetic audio, two-column .beats files and one one-column file (no downbeats)"""
    from beat_this_amd import weights as W
    from beat_this_amd.inference import Audio2Frames

    tmp = tmp_path_factory.mktemp("evall")
    hp = W.HPARAMS["small0"]
    ckpt = {"state_dict": {"model." + k: v for k, v in W.random_state_dict(hp, seed=4, style="lively").items()},
            "hyper_parameters": dict(hp, loss_type="shift_tolerant_weighted_bce", pos_weights=PW)}
    ckpt_path = tmp / "model.ckpt"
    torch.save(ckpt, ckpt_path)
    a2f = Audio2Frames(checkpoint_path=None, device=dev())
    spects = {}
    for i, sec in enumerate((12.0, 31.0, 7.5)):
        sig = W.synthetic_audio(sec, seed=30 + i)
        spects[f"piece{i}/track"] = a2f.signal2spect(sig, 22050).cpu().numpy().astype(np.float16)
    bundle = tmp / "synth.npz"
    np.savez(bundle, **spects)
    ann = tmp / "annotations" / "synth" / "annotations" / "beats"
    ann.mkdir(parents=True)
    rng = np.random.default_rng(10)
    for i, (k, s) in enumerate(spects.items()):
        beats = np.arange(rng.uniform(0, 0.5), s.shape[0] / FPS + 3, rng.uniform(0.4, 0.7))
        if i == 2:
            (ann / f"piece{i}.beats").write_text("".join(f"{float(b)!r}\n" for b in beats))
        else:
            (ann / f"piece{i}.beats").write_text("".join(f"{float(b)!r}\t{j % 4 + 1}\n" for j, b in enumerate(beats)))
    return dict(ckpt=ckpt, ckpt_path=ckpt_path, bundle=bundle, ann=tmp / "annotations", spects=spects)


def test_evaluate_loss_matches_oracle(setup):
    from beat_this_amd.bundle import SpectBundle, predict_bundle
    from beat_this_amd.evaluate import evaluate_bundle, framewise_targets
    from beat_this_amd.inference import Spect2Frames

    s2f = Spect2Frames(setup["ckpt"], dev(), float16=True)
    res = evaluate_bundle(setup["ckpt"], setup["bundle"], setup["ann"], spect2frames=s2f, loss=True)
    met = res["metrics"]
    assert np.array_equal(met["loss_total"], met["loss_beat"] + met["loss_downbeat"])
    assert met["loss_downbeat"][2] == 0 and (met["loss_downbeat"][:2] > 0).all() and (met["loss_beat"] > 0).all()
    with SpectBundle(setup["bundle"]) as bun:
        logits = {k: (b.double().cpu().numpy(), d.double().cpu().numpy()) for k, b, d in predict_bundle(s2f, bun)}
    for i in range(3):
        key = f"piece{i}/track"
        T = setup["spects"][key].shape[0]
        beat, down, dm = framewise_targets(setup["ann"] / "synth" / "annotations" / "beats" / f"piece{i}.beats", T)
        s, n, _ = R.row_terms("shift_tolerant", 3, PW["beat"], logits[key][0].astype(np.float32), beat, None)
        assert met["loss_beat"][i] == pytest.approx(s / n, rel=1e-5), i
        s, n, _ = R.row_terms("shift_tolerant", 3, PW["downbeat"], logits[key][1].astype(np.float32), down,
                              np.full(T, dm, np.float32))
        assert met["loss_downbeat"][i] == pytest.approx(s / n, rel=1e-5, abs=1e-12), i
    for k in ("loss_beat", "loss_downbeat", "loss_total"):
        assert res["averaged"][k] == np.mean(met[k]) and res["dataset_metrics"][k]["synth"] == np.mean(met[k])
    plain = evaluate_bundle(setup["ckpt"], setup["bundle"], setup["ann"], spect2frames=s2f)
    assert not any(k.startswith("loss") for k in plain["metrics"])
    report("evaluate_loss", loss_total=float(res["averaged"]["loss_total"]))


def test_evaluate_cli_loss_flag(setup):
    cmd = [sys.executable, "-m", "beat_this_amd.evaluate", "--models", str(setup["ckpt_path"]), "--bundle", str(setup["bundle"]),
           "--annotations", str(setup["ann"])]
    env = dict(os.environ, PYTHONPATH=ROOT)
    outs = {}
    for flag in ([], ["--no-loss"], ["--loss"]):
        r = subprocess.run(cmd + flag, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[" ".join(flag)] = r.stdout
    assert outs[""] == outs["--no-loss"] and "loss_" not in outs[""]
    with_loss = outs["--loss"]
    for k in ("loss_beat", "loss_downbeat", "loss_total"):
        assert f"\n{k}: " in with_loss and f"\n{k}\nsynth: " in with_loss
    # the loss blocks aside, the output is the plain one (the dataset block of a loss key is its name, a value and a rule)
    drop = set()
    lines = with_loss.splitlines()
    for j, l in enumerate(lines):
        if l in ("loss_beat", "loss_downbeat", "loss_total"):
            drop.update((j, j + 1, j + 2))
    kept = [l for j, l in enumerate(lines) if j not in drop and not l.startswith("loss_")]
    assert kept == outs[""].splitlines()
