"""DBN post-processing on the MI355X (csrc/dbn.hip): the device Viterbi against the host recursion and the numpy oracle
(tests/dbn_reference.py), the ragged device decode against the oracle on the same logits, the case table of
tests/dbn_cases.py (structure, a real trim, empty outcomes, ties, non-finite densities) on four table sets, and the track
API / CLI with dbn=True end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

import dbn_cases as D
import dbn_reference as R
from gpu_util import dev, report
from test_dbn import _host_rows, _with_tables

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


# ---- the case table of tests/dbn_cases.py on the device ------------------------------------------------------------------
_SETS = list(enumerate(D.table_sets()))
_SET_IDS = [D.set_id(ts) for _, ts in _SETS]
_NAMES = list(D.cases(50))
_PPS = {}


def _pp_set(si):
    if si not in _PPS:
        from beat_this_amd.postprocessor import Postprocessor

        ts = D.table_sets()[si]
        _PPS[si] = _with_tables(Postprocessor(type="dbn", fps=ts[0]), ts)
    return _PPS[si]


def _device_rows(pp, tracks):
    """bt_dbn_decode on float32 tracks [(beat, downbeat)] in one launch triple -> the (frame, beat number) int32 rows of
    each track (Postprocessor keeps only the times and which of them are downbeats)"""
    from beat_this_amd import _lib

    lib = _lib.lib()
    lens = np.asarray([len(b) for b, _ in tracks], dtype=np.int64)
    n, total = len(lens), int(lens.sum())
    off = np.concatenate([[0], np.cumsum(lens)])
    logits = torch.cat([t[0].float() for t in tracks] + [t[1].float() for t in tracks]).to(dev())
    spans = torch.from_numpy(np.stack([off[:-1], total + off[:-1], lens, off[:-1]], 1).astype(np.int32)).to(dev())
    tab = pp._dbn_tables.ctypes.data
    ws = torch.empty(lib.bt_dbn_workspace_bytes(tab, n, total), dtype=torch.uint8, device=dev())
    out = torch.full((n + 2 * total,), -7, dtype=torch.int32, device=dev())
    _lib.check(lib.bt_dbn_decode(_lib.stream_ptr(dev()), tab, pp._dbn_device_tables(dev()).data_ptr(), logits.data_ptr(), 0,
                                 spans.data_ptr(), n, total, out.data_ptr(), ws.data_ptr(), ws.numel()))
    o = out.cpu().numpy()
    return [o[n + 2 * off[k]: n + 2 * off[k] + 2 * o[k]].reshape(-1, 2) for k in range(n)]


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", _NAMES)
@pytest.mark.parametrize("si,ts", _SETS, ids=_SET_IDS)
def test_device_single_track_matches_oracle_and_host(si, ts, name):
    pp = _pp_set(si)
    fps = ts[0]
    beat, down = D.cases(fps)[name]
    with np.errstate(divide="ignore", invalid="ignore"):
        want = D.expected(si, name)
    got = pp(beat.to(dev()), down.to(dev()))
    assert got[0].dtype == np.float64 and got[1].dtype == np.float64
    assert _same(got, D.split(want)) and _same(got, pp(beat, down))
    rows, = _device_rows(pp, [(beat, down)])
    assert np.array_equal(rows, _host_rows(pp, beat, down))
    assert np.array_equal(rows[:, 0] / float(fps), want[:, 0]) and np.array_equal(rows[:, 1], want[:, 1])


@pytest.mark.parametrize("si,ts", _SETS, ids=_SET_IDS)
def test_device_one_ragged_launch_with_empty_outcomes_between_long_tracks(si, ts):
    """all cases in one pp.ragged, the tracks that decode to nothing (and a zero-length one) between the long ones: every
    track equals its single-track result and the host decoder's rows, twice bit-identically"""
    pp = _pp_set(si)
    c = D.cases(ts[0])
    empty = list(D.EMPTY) + ["zero"]
    order = []
    for i, name in enumerate(n for n in _NAMES if n not in D.EMPTY):
        order.append(name)
        if i % 5 == 1:
            order.append(empty[(i // 5) % len(empty)])
    assert all(order.count(e) == 1 for e in empty) and order[-1] not in empty
    tracks = [(torch.zeros(0), torch.zeros(0)) if n == "zero" else c[n] for n in order]
    beat = torch.cat([t[0] for t in tracks]).to(dev())
    down = torch.cat([t[1] for t in tracks]).to(dev())
    off = np.concatenate([[0], np.cumsum([len(t[0]) for t in tracks])])
    many = pp.ragged(beat, down, off)
    rows = _device_rows(pp, tracks)
    for k, (name, (tb, td)) in enumerate(zip(order, tracks)):
        if name in empty:
            assert len(many[k][0]) == 0 and len(many[k][1]) == 0 and len(rows[k]) == 0, name
        if name != "zero":
            assert _same(many[k], pp(tb.to(dev()), td.to(dev()))), name
            assert np.array_equal(rows[k], _host_rows(pp, tb, td)), name
    again = pp.ragged(beat, down, off)
    assert all(_same(a, b) for a, b in zip(many, again))


def test_device_masked_batch_padding_does_not_leak_into_the_trim():
    """four tracks of different lengths padded with 0.0 logits (sigmoid 0.5: far above the threshold, unlike silence)"""
    pp = _pp_set(0)
    names = ["lead_tail", "bpm90_3", "fill_m1000", "lone17"]
    c = D.cases(50)
    T = max(len(c[n][0]) for n in names)
    bb, dd = torch.zeros(len(names), T), torch.zeros(len(names), T)
    mask = torch.zeros(len(names), T, dtype=torch.bool)
    for k, n in enumerate(names):
        L = len(c[n][0])
        bb[k, :L], dd[k, :L], mask[k, :L] = c[n][0], c[n][1], True
    assert len({int(m.sum()) for m in mask}) == len(names)
    gb, gd = pp(bb.to(dev()), dd.to(dev()), mask.to(dev()))
    for k, n in enumerate(names):
        assert _same((gb[k], gd[k]), D.split(D.expected(0, n))), n


@pytest.mark.parametrize("how", ["float64_pair", "float64_buffer", "float64_ragged_buffer", "float16", "bfloat16"])
def test_device_decode_dtypes(how):
    """the f64 = 1 load path of the front kernel (separate tensors: one concatenation; the two halves of one buffer: no
    copy) and half-precision logits, against the oracle on the same values"""
    pp = _pp_set(0)
    names = ["lead_tail", "bpm90_3", "sat40", "fill_m1000"]
    c = D.cases(50)
    if how == "float64_ragged_buffer":
        lens = [len(c[n][0]) for n in names]
        total = sum(lens)
        buf = torch.cat([c[n][0].double() for n in names] + [c[n][1].double() for n in names]).to(dev())
        b, d = buf[:total], buf[total:]
        assert d.data_ptr() == b.data_ptr() + 8 * total
        got = pp.ragged(b, d, np.concatenate([[0], np.cumsum(lens)]))
        for k, n in enumerate(names):
            assert _same(got[k], D.split(D.expected(0, n))), n
        return
    for n in names:
        beat, down = c[n]
        if how.startswith("float64"):
            want = D.split(D.expected(0, n))   # (float32 -> float64 is exact)
            if how == "float64_pair":
                b, d = beat.double().to(dev()), down.double().to(dev())
                assert d.data_ptr() != b.data_ptr() + 8 * len(beat)
            else:
                buf = torch.cat([beat.double(), down.double()]).to(dev())
                b, d = buf[: len(beat)], buf[len(beat):]
                assert d.data_ptr() == b.data_ptr() + 8 * len(beat)   # the no-copy branch of _dbn_ragged_async
        else:
            dt = getattr(torch, how)
            b, d = beat.to(dt).to(dev()), down.to(dt).to(dev())
            want = R.postp_dbn(beat.to(dt), down.to(dt))
        assert _same(pp(b, d), want), n


def _trimmed_densities(beat, down):
    """R.log_densities of the trimmed R.combined_act: what the front kernel hands the Viterbi kernel"""
    act = R.combined_act(beat, down)
    idx = np.nonzero(act >= R.PARAMS["threshold"])[0]
    assert idx.any()
    with np.errstate(divide="ignore", invalid="ignore"):
        return R.log_densities(act[idx.min(): idx.max() + 1])


@pytest.mark.parametrize("what", list(D.DENSITY_KINDS) + ["lead_tail", "flat0", "sat40", "bpm215_4"])
@pytest.mark.parametrize("si,ts", _SETS, ids=_SET_IDS)
def test_device_viterbi_on_structured_and_non_finite_densities(si, ts, what):
    """kernel (2) alone: path and log probability equal bt_dbn_viterbi_host bit for bit, and the oracle's Viterbi (a NaN log
    probability matches a NaN).  The 60 fps set fills the last of the kernel's 8 state slots per thread."""
    pp = _pp_set(si)
    fps, kw = ts
    all_dens = [D.densities(what, T) for T in (40, 300)] if what in D.DENSITY_KINDS else [_trimmed_densities(*D.cases(fps)[what])]
    for dens in all_dens:
        dens = np.ascontiguousarray(dens)
        T = len(dens)
        for h, hmm in enumerate(R.models_for(fps, **kw)):
            gp, gl = _device_viterbi(pp, h, dens)
            hp, hl = _host_viterbi(pp, h, dens)
            op, ol = R.viterbi(hmm, dens)
            if np.isnan(hl):
                assert np.isnan(gl) and np.isnan(ol), (T, h)
            else:
                assert np.float64(gl).view(np.int64) == np.float64(hl).view(np.int64) and gl == ol, (T, h)
            if np.isinf(hl):    # no path: neither side writes one
                assert len(op) == 0, (T, h)
            else:
                assert np.array_equal(gp, hp) and np.array_equal(gp, op), (T, h)
            if what in ("inf10", "col0"):
                assert hl == -np.inf, (T, h)
            elif what == "sat40":
                assert np.isinf(dens[:, 0]).any() and np.isfinite(hl), (T, h)


@pytest.mark.parametrize("P,bpb,phase", D.clean_trains())
def test_device_clean_train_decodes_to_its_own_beats(P, bpb, phase):
    """the spec-level property of tests/test_dbn.py on the device: no oracle involved"""
    pp = _pp_set(0)
    beat, down, frames, numbers = D.clean_train(P, bpb, phase)
    rows, = _device_rows(pp, [(beat, down)])
    assert np.array_equal(rows[:, 0], frames) and np.array_equal(rows[:, 1], numbers)
    gb, gd = pp(beat.to(dev()), down.to(dev()))
    assert np.array_equal(gb, frames / 50.0) and np.array_equal(gd, frames[numbers == 1] / 50.0)


def test_device_long_trimmed_track_matches_host():
    """20000 frames, 3000 silent on each side of a train whose tempo changes twice: `first` = 3003 and a trimmed length
    far below the span (the backpointer base comes from the span, the recursion and the backtrack run over the trimmed
    length).  Against the host decoder only: the oracle's backpointer table would be 14000 x 5796."""
    pp = _pp_set(0)
    beat, down = D.long_trimmed()
    assert len(beat) == 20000
    rows, = _device_rows(pp, [(beat, down)])
    host = _host_rows(pp, beat, down)
    assert np.array_equal(rows, host)
    assert len(rows) > 400 and rows[0, 0] >= 3000 and rows[-1, 0] < 17000
    assert _same(pp(beat.to(dev()), down.to(dev())), pp(beat, down))
