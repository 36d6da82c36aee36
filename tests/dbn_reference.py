"""Independent numpy float64 re-statement of madmom's DBNDownBeatTrackingProcessor with the reference's arguments
(beat_this/model/postprocessor.py:28-37,138-173): the oracle of tests/test_dbn.py and tests/test_gpu_dbn.py.

Written from madmom's published algorithm (BeatStateSpace / BarStateSpace / BarTransitionModel /
RNNDownBeatTrackingObservationModel / Viterbi / the `correct` step), NOT pinned against madmom itself, which cannot be
installed here; it shares no code with beat_this_amd.  One deliberate choice: the transition probabilities and the initial
log probability go through Python's scalar libm ``math.exp`` / ``math.log`` rather than numpy's vector loops, whose last
bit depends on the CPU's SIMD dispatch (AVX-512 and baseline builds of numpy differ on 8 of the 880 log probabilities at
50 fps) -- madmom's own tables therefore differ by an ulp from machine to machine, and the oracle pins the libm value.
"""
from __future__ import annotations

import math

import numpy as np
import torch

PARAMS = dict(beats_per_bar=(3, 4), min_bpm=55.0, max_bpm=215.0, fps=50, transition_lambda=100.0, num_tempi=60,
              observation_lambda=16.0, threshold=0.05)


def beat_intervals(fps=50, min_bpm=55.0, max_bpm=215.0, num_tempi=60):
    lo, hi = 60.0 * fps / max_bpm, 60.0 * fps / min_bpm
    iv = np.arange(np.round(lo), np.round(hi) + 1)
    if num_tempi is not None and num_tempi < len(iv):
        n = num_tempi
        while True:
            iv = np.unique(np.round(np.logspace(np.log2(lo), np.log2(hi), n, base=2)))
            if len(iv) >= num_tempi:
                break
            n += 1
    return iv.astype(int)


class BarHMM:
    """state space, sparse transition model (CSR over (to, from), ascending from) and observation pointers of one bar"""

    def __init__(self, num_beats, intervals, transition_lambda=100.0, observation_lambda=16.0):
        iv = np.asarray(intervals)
        self.num_beats = nb = num_beats
        pos = np.concatenate([np.linspace(0, 1, i, endpoint=False) for i in iv])
        ints = np.concatenate([np.full(i, i) for i in iv])
        spb = len(pos)
        first = np.concatenate([[0], np.cumsum(iv)[:-1]])
        last = np.cumsum(iv) - 1
        self.positions = np.concatenate([pos + b for b in range(nb)])
        self.state_intervals = np.tile(ints, nb)
        self.num_states = S = spb * nb
        self.first_states = [first + b * spb for b in range(nb)]
        self.last_states = [last + b * spb for b in range(nb)]
        # transitions: s-1 -> s with probability 1 except into first states
        to = np.arange(S)
        frm = to - 1
        prob = np.ones(S)
        keep = np.ones(S, bool)
        keep[np.concatenate(self.first_states)] = False
        to, frm, prob = list(to[keep]), list(frm[keep]), list(prob[keep])
        ratio = iv[None, :].astype(float) / iv[:, None].astype(float)       # rows = from, columns = to
        p = np.vectorize(math.exp)(-transition_lambda * np.abs(ratio - 1.0))
        p[p <= np.spacing(1)] = 0
        p = p / np.sum(p, axis=1)[:, None]
        self.tempo_nnz = int((p != 0).sum())
        fi, ti = np.nonzero(p)
        for b in range(nb):
            to += list(self.first_states[b][ti])
            frm += list(self.last_states[b - 1][fi])
            prob += list(p[fi, ti])
        to, frm, prob = np.array(to), np.array(frm), np.array(prob)
        order = np.lexsort((frm, to))
        to, frm, prob = to[order], frm[order], prob[order]
        self.indptr = np.searchsorted(to, np.arange(S + 1))
        self.indices = frm
        self.log_probs = np.array([math.log(x) for x in prob])
        self.init = math.log(1.0 / S)
        thr = 1.0 / observation_lambda
        self.pointers = np.zeros(S, dtype=int)
        self.pointers[self.positions % 1 < thr] = 1
        self.pointers[self.positions < thr] = 2


def log_densities(act, observation_lambda=16.0):
    act = np.asarray(act, dtype=np.float64)
    d = np.empty((len(act), 3))
    d[:, 0] = np.log((1.0 - np.sum(act, axis=1)) / (observation_lambda - 1))
    d[:, 1] = np.log(act[:, 0])
    d[:, 2] = np.log(act[:, 1])
    return d


def viterbi(hmm: BarHMM, dens):
    """madmom's Viterbi: transition before the first observation, strict '>' (lowest predecessor wins ties),
    first-index argmax at the end; -inf -> empty path.  Vectorised over states, one slot of the CSR rows at a time."""
    T, S = len(dens), hmm.num_states
    v = np.full(S, hmm.init)
    counts = np.diff(hmm.indptr)
    slots = [np.nonzero(counts > r)[0] for r in range(counts.max())]
    bt = np.empty((T, S), dtype=np.uint16)
    for t in range(T):
        cur = np.full(S, -np.inf)
        ptr = hmm.indices[hmm.indptr[:-1]].copy()
        for r, st in enumerate(slots):
            e = hmm.indptr[st] + r
            tp = v[hmm.indices[e]] + hmm.log_probs[e]
            with np.errstate(invalid="ignore"):
                upd = tp > cur[st]
            cur[st[upd]] = tp[upd]
            ptr[st[upd]] = hmm.indices[e[upd]]
        v = cur + dens[t, hmm.pointers]
        bt[t] = ptr
    if T == 0:
        return np.zeros(0, dtype=int), -np.inf
    state = int(np.argmax(v))
    logp = v[state]
    if np.isinf(logp):
        return np.zeros(0, dtype=int), logp
    path = np.empty(T, dtype=int)
    for t in range(T - 1, -1, -1):
        path[t] = state
        state = bt[t, state]
    return path, logp


_HMMS = {}


def hmms(fps=50):
    if fps not in _HMMS:
        iv = beat_intervals(fps, PARAMS["min_bpm"], PARAMS["max_bpm"], PARAMS["num_tempi"])
        _HMMS[fps] = [BarHMM(nb, iv, PARAMS["transition_lambda"], PARAMS["observation_lambda"]) for nb in PARAMS["beats_per_bar"]]
    return _HMMS[fps]


_MODELS = {}


def models_for(fps=50, **kw):
    """the BarHMM list of one table set: PARAMS with `fps` and the overrides in `kw` (such as num_tempi=20)"""
    p = dict(PARAMS, fps=fps, **kw)
    key = tuple(sorted(p.items()))
    if key not in _MODELS:
        iv = beat_intervals(p["fps"], p["min_bpm"], p["max_bpm"], p["num_tempi"])
        _MODELS[key] = [BarHMM(nb, iv, p["transition_lambda"], p["observation_lambda"]) for nb in p["beats_per_bar"]]
    return _MODELS[key]


def dbn(act, fps=50, models=None):
    """DBNDownBeatTrackingProcessor.process: (T, 2) activation -> (N, 2) rows (beat time, beat number); `models`: the
    list of BarHMM to decode with (default hmms(fps))"""
    models = hmms(fps) if models is None else models
    act = np.asarray(act, dtype=np.float64)
    first = 0
    idx = np.nonzero(act >= PARAMS["threshold"])[0]
    if idx.any():
        first = max(first, np.min(idx))
        last = min(len(act), np.max(idx) + 1)
    else:
        last = first
    act = act[first:last]
    if not act.any():
        return np.empty((0, 2))
    dens = log_densities(act, PARAMS["observation_lambda"])
    results = [viterbi(h, dens) for h in models]
    best = int(np.argmax([r[1] for r in results]))
    path, logp = results[best]
    if len(path) == 0:
        return np.empty((0, 2))
    hmm = models[best]
    beat_numbers = hmm.positions[path].astype(int) + 1
    beat_range = hmm.pointers[path] >= 1
    idx = np.nonzero(np.diff(beat_range.astype(int)))[0] + 1
    if beat_range[0]:
        idx = np.r_[0, idx]
    if beat_range[-1]:
        idx = np.r_[idx, beat_range.size]
    beats = np.empty(0, dtype=int)
    if idx.any():
        for left, right in idx.reshape((-1, 2)):
            peak = np.argmax(act[left:right]) // 2 + left
            beats = np.hstack((beats, peak))
    return np.vstack(((beats + first) / float(fps), beat_numbers[beats])).T


def combined_act(beat, downbeat):
    """postp_dbn / _postp_dbn_item for one unpadded track of logits"""
    eps = 1e-5
    bp = torch.as_tensor(beat).double().sigmoid() * (1 - eps) + eps / 2
    dp = torch.as_tensor(downbeat).double().sigmoid() * (1 - eps) + eps / 2
    bp, dp = bp.cpu().numpy(), dp.cpu().numpy()
    return np.vstack((np.maximum(bp - dp, eps / 2), dp)).T


def postp_dbn(beat, downbeat, fps=50, models=None):
    """(beat times, downbeat times) of one track of logits, as Postprocessor(type="dbn") returns them"""
    out = dbn(combined_act(beat, downbeat), fps, models)
    return out[:, 0], out[out[:, 1] == 1][:, 0]
