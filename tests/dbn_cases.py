"""The DBN decoder's case table, shared by tests/test_dbn.py (host decoder) and tests/test_gpu_dbn.py (device decoder):
logits with musical structure, a real threshold trim, the empty outcomes, exact ties and non-finite densities, for every
table set the decoder is tested on.  Plain data and numpy; the expected rows come from the oracle (tests/dbn_reference.py)
and are computed once per (table set, case) for the whole test run."""
import numpy as np
import torch

BPMS = (55, 56, 90, 120, 200, 215)


def _pulses(T, period, beats_per_bar, phase=3, hi=6.0, lo=-6.0, seed=0, lead=0, tail=0, noise=0.5):
    """a pulse train of T frames: `hi` on every beat (and on the downbeat row every `beats_per_bar` beats), `lo` plus
    normal noise of standard deviation `noise` elsewhere (0 = clean); `lead` / `tail` frames of -9.0 around it"""
    rng = np.random.default_rng(seed)
    beat = np.full(T, lo) + rng.normal(size=T) * noise
    down = np.full(T, lo) + rng.normal(size=T) * noise
    for n, f in enumerate(np.arange(phase, T, period)):
        f = int(round(f))
        if f < T:
            beat[f] = hi
            if n % beats_per_bar == 0:
                down[f] = hi
    pad = lambda x: np.concatenate([np.full(lead, -9.0), x, np.full(tail, -9.0)])
    return torch.from_numpy(pad(beat)).float(), torch.from_numpy(pad(down)).float()


def table_sets():
    """(fps, dbn_tables keyword arguments): the default tables; 21 intervals / 1428 states; 49 intervals / 8036 of the
    kernel's 8192 states; the log-spaced interval branch"""
    return [(50, {}), (25, {}), (60, {}), (50, {"num_tempi": 20})]


def set_id(ts):
    fps, kw = ts
    return f"fps{fps}" + "".join(f"-{k}{v}" for k, v in kw.items())


_CASES = {}


def cases(fps):
    """name -> (beat, downbeat) float32 logits"""
    if fps in _CASES:
        return _CASES[fps]
    P = 60.0 * fps / 120
    c = {}
    for bpm in BPMS:
        period = 60.0 * fps / bpm
        for bpb in (3, 4):
            c[f"bpm{bpm}_{bpb}"] = _pulses(int(round(24 * period)) + 5, period, bpb, seed=bpm + bpb)
    T16 = int(round(16 * P))
    c["lead_tail"] = _pulses(T16, P, 4, seed=21, lead=137, tail=211)
    c["clean"] = _pulses(T16, P, 4, noise=0)
    silent = torch.full((300,), -8.0)
    c["silent"] = (silent, silent.clone())
    for name, f in (("lone0", 0), ("lone17", 17), ("lone_last", 299)):
        b = silent.clone()
        b[f] = 8.0
        c[name] = (b, silent.clone())
    b, d = _pulses(T16, P, 4, seed=22)
    c["sat40"] = (torch.where(b > 0, torch.full_like(b, 40.0), b), torch.where(d > 0, torch.full_like(d, 40.0), d))
    b, d = _pulses(T16, P, 4, seed=23)
    for x in (b, d):
        x[:50] = -1000.0    # what aggregate_kernel writes for a frame no chunk covers
        x[-30:] = -1000.0
    c["fill_m1000"] = (b, d)
    c["all_sat"] = (torch.full((200,), 40.0), torch.full((200,), 40.0))
    c["flat0"] = (torch.zeros(200), torch.zeros(200))
    c["flat_hi_lo"] = (torch.full((200,), 3.0), torch.full((200,), -3.0))
    at = int(round(3 + 8 * P))   # the third downbeat of the 400-frame train
    for name, row, val in (("nan_beat", 0, float("nan")), ("nan_down", 1, float("nan")), ("inf_beat", 0, float("inf"))):
        bd = _pulses(400, P, 4, seed=24)
        bd[row][at] = val
        c[name] = bd
    for T in (1, 2, 13):
        rng = np.random.default_rng(100 + T)
        c[f"short{T}"] = (torch.from_numpy(rng.normal(size=T) * 3 - 1).float(), torch.from_numpy(rng.normal(size=T) * 3 - 3).float())
    _CASES[fps] = c
    return c


EMPTY = ("silent", "lone0", "all_sat", "nan_down")   # the cases that decode to no rows (checked at 50 fps in test_dbn.py)
# these depend only on index rules and exactly representable values: never reseeded
STRUCTURAL = ("flat0", "flat_hi_lo", "sat40", "all_sat", "fill_m1000", "lone0", "lone17", "lone_last", "silent", "clean")

_EXPECTED = {}


def expected(si, name):
    """the oracle's (N, 2) float64 rows (beat time, beat number) of case `name` under table_sets()[si]"""
    import dbn_reference as R

    if (si, name) not in _EXPECTED:
        fps, kw = table_sets()[si]
        beat, down = cases(fps)[name]
        _EXPECTED[si, name] = R.dbn(R.combined_act(beat, down), fps, models=R.models_for(fps, **kw))
    return _EXPECTED[si, name]


def split(rows):
    """(N, 2) rows -> (beat times, downbeat times), as Postprocessor returns them"""
    return rows[:, 0], rows[rows[:, 1] == 1][:, 0]


def densities(kind, T, seed=0):
    """(T, 3) log densities with non-finite entries: "inf10" 10 % of the entries -inf; "nan1" one NaN entry (a beat
    density half way); "col0" the no-beat column all -inf; "nan_last" a NaN beat density in the last frame, which reaches
    the final argmax (numpy's: the first NaN wins) and makes the log probability NaN"""
    rng = np.random.default_rng([seed, T])
    dens = np.log(rng.random((T, 3)) * 0.999 + 1e-4)
    if kind == "inf10":
        dens[rng.random((T, 3)) < 0.1] = -np.inf
    elif kind == "nan1":
        dens[T // 2, 1] = np.nan
    elif kind == "col0":
        dens[:, 0] = -np.inf
    elif kind == "nan_last":
        dens[T - 1, 1] = np.nan
    else:
        raise ValueError(kind)
    return dens


DENSITY_KINDS = ("inf10", "nan1", "col0", "nan_last")


def clean_trains():
    """the spec-level property (default tables): a clean train of period P decodes to exactly its own beat frames"""
    return [(P, bpb, phase) for P in (14, 15, 35, 54, 55) for bpb in (3, 4) for phase in (0, 3, P - 1)]


def clean_train(P, bpb, phase):
    T = phase + 20 * P + 1
    beat, down = _pulses(T, P, bpb, phase=phase, noise=0)
    frames = np.arange(phase, T, P)
    return beat, down, frames, np.arange(len(frames)) % bpb + 1


def long_trimmed():
    """20000 frames at 50 fps: 3000 silent, a 14000-frame train whose tempo changes twice, 3000 silent"""
    parts = [_pulses(5000, 25.0, 4, seed=31), _pulses(4000, 33.333, 4, seed=32), _pulses(5000, 20.0, 4, seed=33)]
    sil = torch.full((3000,), -9.0)
    return torch.cat([sil] + [p[0] for p in parts] + [sil]), torch.cat([sil] + [p[1] for p in parts] + [sil])
