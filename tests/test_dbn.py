"""DBN post-processing (Postprocessor(type="dbn"), reference postprocessor.py:28-37,138-173) on the host, no GPU needed:
the library's tables against the independent numpy re-statement of madmom's algorithm (tests/dbn_reference.py), and the
host decoder (bt_dbn_host / bt_dbn_host_act / bt_dbn_viterbi_host) against the oracle, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import dbn_cases as D
import dbn_reference as R
from dbn_cases import _pulses


def _pp(fps=50):
    from beat_this_amd import _lib
    from beat_this_amd.postprocessor import Postprocessor

    _lib.build()
    return Postprocessor(type="dbn", fps=fps)


def _parse(blob):
    """the table blob (layout: include/beat_this_amd.h, bt_dbn_tables)"""
    b = blob.tobytes()
    i32 = lambda off, n: np.frombuffer(b, np.int32, n, off)
    hdr = i32(0, 6)
    return dict(K=int(hdr[1]), n_hmm=int(hdr[2]), spb=int(hdr[3]), nnz=int(hdr[4]), beats=i32(24, 4), num_states=i32(40, 4),
                init=np.frombuffer(b, np.float64, 4, 56), obs_norm=np.frombuffer(b, np.float64, 1, 88)[0],
                threshold=np.frombuffer(b, np.float64, 1, 96)[0], intervals=i32(104, 256), first=i32(1128, 256),
                band_ptr=i32(2152, 258), band_from=i32(3184, 1536), logp=np.frombuffer(b, np.float64, 1536, 9328),
                cnt=np.frombuffer(b, np.uint8, 16 * 256, 21616).reshape(16, 256))


def test_tables_equal_the_oracle_state_space_and_transitions():
    pp = _pp()
    t = _parse(pp._dbn_tables)
    assert len(pp._dbn_tables) == 25712
    K = t["K"]
    iv = t["intervals"][:K]
    assert K == 42 and np.array_equal(iv, np.arange(14, 56)) and np.array_equal(iv, R.beat_intervals())
    assert t["spb"] == 1449 and t["n_hmm"] == 2 and list(t["beats"][:2]) == [3, 4]
    assert list(t["num_states"][:2]) == [4347, 5796]
    assert t["obs_norm"] == 15.0 and t["threshold"] == 0.05
    assert t["nnz"] == 880   # tempo transitions per beat boundary at 50 fps
    _compare_tables(t, R.hmms())


@pytest.mark.parametrize("ts", D.table_sets()[1:], ids=D.set_id)
def test_tables_equal_the_oracle_on_the_other_table_sets(ts):
    """25 fps, 60 fps (8036 of the kernel's 8192 states, 1216 of its 1536 transitions) and the log-spaced interval branch
    (num_tempi=20 at 50 fps): every constant comes from the oracle"""
    from beat_this_amd.postprocessor import dbn_tables

    fps, kw = ts
    _pp()
    models = R.models_for(fps, **kw)
    iv = R.beat_intervals(fps, num_tempi=kw.get("num_tempi", 60))
    t = _parse(dbn_tables(fps, **kw))
    K = t["K"]
    assert K == len(iv) and np.array_equal(t["intervals"][:K], iv)
    assert t["spb"] == iv.sum() and t["n_hmm"] == 2 and list(t["beats"][:2]) == [3, 4]
    assert list(t["num_states"][:2]) == [3 * iv.sum(), 4 * iv.sum()]
    assert t["obs_norm"] == 15.0 and t["threshold"] == 0.05
    if fps == 60:
        assert (K, t["num_states"][1], t["nnz"]) == (49, 8036, 1216)
    if fps == 25:
        assert (K, t["num_states"][1]) == (21, 1428)
    if kw:   # the log-spaced branch: at least num_tempi intervals, not all consecutive
        assert K >= kw["num_tempi"] and K < 42 and (np.diff(iv) > 1).any()
    _compare_tables(t, models)


def _compare_tables(t, models):
    """the parsed blob against the oracle's BarHMM list: states, transitions bit for bit, observation pointers"""
    K = t["K"]
    iv = t["intervals"][:K]
    for h, hmm in enumerate(models):
        assert hmm.num_states == t["num_states"][h]
        assert t["init"][h] == hmm.init   # bit for bit
        # first / last states of every beat
        for b in range(hmm.num_beats):
            assert np.array_equal(hmm.first_states[b], b * t["spb"] + t["first"][:K])
            assert np.array_equal(hmm.last_states[b], b * t["spb"] + t["first"][:K] + iv - 1)
        # tempo transitions: same predecessors in the same order, same log probabilities
        assert hmm.tempo_nnz == t["nnz"]
        for b in range(hmm.num_beats):
            for j in range(K):
                s = hmm.first_states[b][j]
                lo, hi = hmm.indptr[s], hmm.indptr[s + 1]
                e0, e1 = t["band_ptr"][j], t["band_ptr"][j + 1]
                frm = t["band_from"][e0:e1]
                assert np.array_equal(hmm.indices[lo:hi], hmm.last_states[b - 1][frm])
                assert np.array_equal(hmm.log_probs[lo:hi].view(np.int64), t["logp"][e0:e1].view(np.int64))
        # every other state: the single predecessor s - 1 with log probability 0
        counts = np.diff(hmm.indptr)
        others = np.setdiff1d(np.arange(hmm.num_states), np.concatenate(hmm.first_states))
        assert (counts[others] == 1).all() and np.array_equal(hmm.indices[hmm.indptr[others]], others - 1)
        assert (hmm.log_probs[hmm.indptr[others]] == 0).all()
        # observation pointers: leading runs of cnt[b][j] states (2 in beat 0, 1 elsewhere)
        ptr = np.zeros(hmm.num_states, int)
        for b in range(hmm.num_beats):
            for j in range(K):
                s0 = b * t["spb"] + t["first"][j]
                ptr[s0: s0 + t["cnt"][b, j]] = 2 if b == 0 else 1
        assert np.array_equal(ptr, hmm.pointers)


def test_viterbi_host_matches_oracle_on_given_densities():
    from beat_this_amd import _lib

    pp = _pp()
    rng = np.random.default_rng(3)
    for T in (1, 13, 14, 15, 300):
        dens = np.log(rng.random((T, 3)) * 0.999 + 1e-4)
        for h, hmm in enumerate(R.hmms()):
            path = np.zeros(T, np.int32)
            lp = C.c_double()
            _lib.check(_lib.lib().bt_dbn_viterbi_host(pp._dbn_tables.ctypes.data, h, dens.ctypes.data, T, path.ctypes.data,
                                                      C.byref(lp)))
            op, ol = R.viterbi(hmm, dens)
            assert lp.value == ol and np.array_equal(path, op), (T, h)


def _check(pp, beat, down, mask=None):
    got_b, got_d = pp(beat, down, mask)
    if beat.ndim == 1:
        got_b, got_d = [got_b], [got_d]
        beat, down = beat[None], down[None]
        mask = None if mask is None else mask[None]
    for k in range(beat.shape[0]):
        m = torch.ones(beat.shape[1], dtype=torch.bool) if mask is None else mask[k].bool()
        ob, od = R.postp_dbn(beat[k][m], down[k][m])
        assert np.array_equal(got_b[k], ob) and np.array_equal(got_d[k], od), k
        assert got_b[k].dtype == np.float64 and got_d[k].dtype == np.float64
    return got_b, got_d


def test_pulse_trains_match_oracle():
    pp = _pp()
    # 120 bpm 4/4 (25 frames per beat)
    b, d = _check(pp, *_pulses(1500, 25.0, 4))
    assert 55 <= len(b[0]) <= 61 and 13 <= len(d[0]) <= 16
    assert np.allclose(np.diff(b[0]), 0.5)
    # 100 bpm 3/4: the 3-beat HMM wins (beat numbers 1..3)
    beat, down = _pulses(1500, 30.0, 3, seed=1)
    _check(pp, beat, down)
    rows = pp.dbn(R.combined_act(beat, down))
    assert rows[:, 1].max() == 3 and np.array_equal(rows, R.dbn(R.combined_act(beat, down)))
    # a tempo change half way: 120 bpm, then 90 bpm
    b1, d1 = _pulses(750, 25.0, 4, seed=2)
    b2, d2 = _pulses(750, 33.333, 4, seed=3)
    _check(pp, torch.cat([b1, b2]), torch.cat([d1, d2]))


def test_random_logits_match_oracle():
    pp = _pp()
    rng = np.random.default_rng(11)
    for T in (50, 400, 1500):
        beat = torch.from_numpy(rng.normal(size=T) * 3 - 1).float()
        down = torch.from_numpy(rng.normal(size=T) * 3 - 3).float()
        _check(pp, beat, down)
    # float64 and float16 logits (the reference's .double() is exact on both)
    beat = torch.from_numpy(rng.normal(size=500) * 3 - 1)
    _check(pp, beat, torch.from_numpy(rng.normal(size=500) * 3 - 3))
    _check(pp, beat.half(), (beat * 0.7 - 2).half())


def test_threshold_edge_cases():
    pp = _pp()
    low = torch.full((300,), -8.0)
    b, d = pp(low, low)                 # all frames below the threshold
    assert len(b) == 0 and len(d) == 0 and b.dtype == np.float64
    only0 = low.clone()
    only0[0] = 8.0                      # madmom's `if idx.any()`: a lone frame 0 counts as none
    b, d = _check(pp, only0, low)
    assert len(b[0]) == 0 and len(d[0]) == 0
    assert pp.dbn(np.zeros((0, 2))).shape == (0, 2)
    rng = np.random.default_rng(5)
    for T in (1, 2, 13):                # shorter than the shortest beat interval
        _check(pp, torch.from_numpy(rng.normal(size=T) * 4).float(), torch.from_numpy(rng.normal(size=T) * 4 - 2).float())
    one = torch.tensor([8.0])
    assert len(pp(one, one)[0]) == 0


def test_padding_mask_and_batch():
    pp = _pp()
    rng = np.random.default_rng(9)
    B, T = 3, 700
    beat = torch.from_numpy(rng.normal(size=(B, T)) * 3 - 1).float()
    down = torch.from_numpy(rng.normal(size=(B, T)) * 3 - 3).float()
    mask = torch.ones(B, T, dtype=torch.bool)
    mask[1, 500:] = False
    mask[2, 100:] = False
    got_b, got_d = _check(pp, beat, down, mask)
    assert isinstance(got_b, tuple) and len(got_b) == B
    _check(pp, beat, down)   # no mask
    # 1-D input with a mask
    _check(pp, beat[1], down[1], mask[1])


def test_unsupported_parameters_raise():
    from beat_this_amd.postprocessor import Postprocessor, dbn_tables

    _pp()
    with pytest.raises(ValueError, match="states"):
        Postprocessor(type="dbn", fps=200)    # 60 log-spaced intervals of 56..218 frames: too many states for LDS
    with pytest.raises(ValueError, match="at most 255"):
        dbn_tables(50, min_bpm=1.0, num_tempi=1000)
    with pytest.raises(ValueError):
        dbn_tables(50, beats_per_bar=(3, 4, 5, 6, 7))


def test_postprocessor_accepts_6_to_60_fps():
    from beat_this_amd.postprocessor import Postprocessor

    _pp()
    for fps in (6, 25, 60):
        assert Postprocessor(type="dbn", fps=fps).fps == fps
    with pytest.raises(ValueError, match="8568 states"):
        Postprocessor(type="dbn", fps=61)
    for fps in (1, 5):
        with pytest.raises(ValueError):
            Postprocessor(type="dbn", fps=fps)


def _with_tables(pp, ts):
    """`pp` on the tables of one table set (num_tempi is not a Postprocessor argument: its tables are swapped)"""
    from beat_this_amd.postprocessor import DBN, dbn_tables

    fps, kw = ts
    assert pp.fps == fps
    if kw:
        pp._dbn_tables, pp._dbn_dev = dbn_tables(fps, **kw), {}
        pp.dbn = DBN(pp._dbn_tables, fps)
    return pp


def _pp_for(ts):
    return _with_tables(_pp(ts[0]), ts)


def _host_rows(pp, beat, down):
    """bt_dbn_host: the (frame, beat number) int32 rows of one track"""
    from beat_this_amd import _lib

    lb, ld = np.ascontiguousarray(beat.double().numpy()), np.ascontiguousarray(down.double().numpy())
    rows = np.zeros((max(len(lb), 1), 2), np.int32)
    n = C.c_int32(0)
    _lib.check(_lib.lib().bt_dbn_host(pp._dbn_tables.ctypes.data, lb.ctypes.data, ld.ctypes.data, len(lb), rows.ctypes.data, C.byref(n)))
    return rows[: n.value]


_SETS = list(enumerate(D.table_sets()))


@pytest.mark.parametrize("name", list(D.cases(50)))
@pytest.mark.parametrize("si,ts", _SETS, ids=[D.set_id(ts) for _, ts in _SETS])
def test_case_table_host_decoder_matches_oracle(si, ts, name):
    """every case of tests/dbn_cases.py through Postprocessor on CPU tensors, bt_dbn_host and bt_dbn_host_act: rows
    identical to the oracle's (beat times, beat numbers), outputs float64"""
    pp = _pp_for(ts)
    fps = ts[0]
    beat, down = D.cases(fps)[name]
    with np.errstate(divide="ignore", invalid="ignore"):
        want = D.expected(si, name)
        wb, wd = D.split(want)
        gb, gd = pp(beat, down)
        assert gb.dtype == np.float64 and gd.dtype == np.float64
        assert np.array_equal(gb, wb) and np.array_equal(gd, wd)
        rows = _host_rows(pp, beat, down)
        assert np.array_equal(rows[:, 0] / float(fps), want[:, 0]) and np.array_equal(rows[:, 1], want[:, 1])
        act = pp.dbn(R.combined_act(beat, down))
        assert act.dtype == np.float64 and np.array_equal(act, want)


def test_case_table_does_not_degenerate():
    """guards on the oracle's own output at 50 fps: each case still exercises what it was written for"""
    e = lambda name: D.expected(0, name)
    with np.errstate(divide="ignore", invalid="ignore"):
        for name in ("silent", "lone0", "all_sat", "nan_down"):
            assert len(e(name)) == 0, name
        assert set(D.EMPTY) == {"silent", "lone0", "all_sat", "nan_down"}
        assert np.array_equal(e("lone17")[:, 0] * 50, [17]) and np.array_equal(e("lone_last")[:, 0] * 50, [299])
        assert len(e("lead_tail")) == 16 and e("lead_tail")[0, 0] * 50 == 140
        assert e("fill_m1000")[0, 0] * 50 >= 50
        for bpm in (56, 90, 120, 200):
            assert e(f"bpm{bpm}_3")[:, 1].max() == 3 and e(f"bpm{bpm}_4")[:, 1].max() == 4, bpm
        assert len(e("nan_beat")) == 16 and len(e("inf_beat")) == 16
    # the trim is real: lead_tail keeps 16 periods of a 748-frame track
    beat, down = D.cases(50)["lead_tail"]
    assert len(beat) == 137 + 400 + 211
    # sat40 / all_sat really make the no-beat density -inf, fill_m1000 really underflows the sigmoid to eps / 2
    act = R.combined_act(*D.cases(50)["all_sat"])
    assert (1.0 - act.sum(1) == 0).all()
    act = R.combined_act(*D.cases(50)["sat40"])
    assert (1.0 - act.sum(1) == 0).any()
    act = R.combined_act(*D.cases(50)["fill_m1000"])
    assert (act[:50] == 0.5e-5).all()


@pytest.mark.parametrize("si,ts", _SETS, ids=[D.set_id(ts) for _, ts in _SETS])
def test_viterbi_host_matches_oracle_on_non_finite_densities(si, ts):
    """10 % of the entries -inf, one NaN entry, the no-beat column all -inf, and a NaN in the last frame (the final argmax's
    NaN rule): path and log probability equal the oracle's (== or both NaN)"""
    from beat_this_amd import _lib

    pp = _pp_for(ts)
    fps, kw = ts
    for kind in D.DENSITY_KINDS:
        for T in (40, 300):
            dens = D.densities(kind, T)
            for h, hmm in enumerate(R.models_for(fps, **kw)):
                path = np.zeros(T, np.int32)
                lp = C.c_double()
                _lib.check(_lib.lib().bt_dbn_viterbi_host(pp._dbn_tables.ctypes.data, h, dens.ctypes.data, T, path.ctypes.data,
                                                          C.byref(lp)))
                op, ol = R.viterbi(hmm, dens)
                assert lp.value == ol or (np.isnan(lp.value) and np.isnan(ol)), (kind, T, h)
                assert np.array_equal(path[: len(op)], op), (kind, T, h)
                if kind in ("inf10", "col0"):
                    assert ol == -np.inf and len(op) == 0, (kind, T, h)
                elif kind == "nan1":
                    assert np.isfinite(ol) and len(op) == T, (kind, T, h)
                else:
                    assert np.isnan(ol) and len(op) == T, (kind, T, h)


@pytest.mark.parametrize("P,bpb,phase", D.clean_trains())
def test_clean_train_decodes_to_its_own_beats(P, bpb, phase):
    """spec level, no oracle: a clean train of period P frames (215 .. 55 bpm at 50 fps) decodes to exactly its beat frames,
    numbered 1 .. beats_per_bar from the first one.  (Default tables only: at 25 and 60 fps the slowest 3/4 trains decode
    at double tempo, the model's own octave choice, and the oracle agrees with it.)"""
    pp = _pp()
    beat, down, frames, numbers = D.clean_train(P, bpb, phase)
    rows = _host_rows(pp, beat, down)
    assert np.array_equal(rows[:, 0], frames) and np.array_equal(rows[:, 1], numbers)
    gb, gd = pp(beat, down)
    assert np.array_equal(gb, frames / 50.0) and np.array_equal(gd, frames[numbers == 1] / 50.0)
