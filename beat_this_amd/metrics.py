"""mir_eval.beat on the library's code: the paper's metrics (the reference's Metrics, pl_module.py:320-339: trim_beats,
f_measure, cemgil, continuity) and the rest of the module (goto, p_score, information_gain, evaluate;
DESIGN.md section 28), restated in csrc/metrics.hip.  mir_eval is never imported, and nothing here is pinned against it.

Drop-in forms (``trim_beats``, ``validate``, ``f_measure``, ``cemgil``, ``goto``, ``p_score``, ``continuity``,
``information_gain``, ``evaluate``, and the reference's ``Metrics``) take mir_eval's arguments, return what it returns, raise
``ValueError`` where it raises (and, in addition, on non-finite times) and warn where it warns; they run the library's host
code (bt_beat_metrics_host, bt_beat_metrics_ext_host).  ``beat_metrics_many`` scores many tracks on the device: one
bt_beat_metrics call, and with ``extended=True`` one bt_beat_metrics_ext call on the same upload."""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np
import torch

from . import _lib

COLUMNS = ("F", "P", "R", "Cemgil", "CemgilMax", "CMLc", "CMLt", "AMLc", "AMLt", "n_ref", "n_est", "status")
MAX_TIME = 30000.0
DEFAULTS = dict(f_measure_threshold=0.07, cemgil_sigma=0.04, continuity_phase_threshold=0.175,
                continuity_period_threshold=0.175)
# BT_METRICS_* status bits (include/beat_this_amd.h); those of the estimates are shifted left by 3
STATUS_NONFINITE, STATUS_UNSORTED, STATUS_LATE, STATUS_NEAREST, STATUS_OFFSETS = 1, 2, 4, 64, 128
STATUS_PSCORE = 256   # bt_beat_metrics_ext only: p_score undefined (no interval between distinct reference indices)
EXT_COLUMNS = ("Goto", "PScore", "InfoGain", "GotoCriteria", "GotoTrackLen", "GotoMean", "GotoStd", "PWindow", "PHits",
               "EntropyFwd", "EntropyBwd", "status")
EXT_DEFAULTS = dict(goto_threshold=0.35, goto_mu=0.2, goto_sigma=0.2, p_score_threshold=0.2, bins=41)
# beat_metrics_many(extended=True)'s keys for the columns of a bt_beat_metrics_ext row
EXT_KEYS = ("Goto", "P-score", "Information gain", "GotoCriteria", "GotoTrackLen", "GotoMean", "GotoStd", "PWindow", "PHits",
            "EntropyFwd", "EntropyBwd", "status_ext")


def _thresholds(kw):
    unknown = set(kw) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown threshold(s) {sorted(unknown)}; known: {sorted(DEFAULTS)}")
    t = {**DEFAULTS, **kw}
    return (t["f_measure_threshold"], t["cemgil_sigma"], t["continuity_phase_threshold"], t["continuity_period_threshold"])


def _events(x, what):
    a = np.asarray(x, dtype=np.float64)
    if a.ndim != 1:
        raise ValueError(f"{what} times should be a 1-d array, but shape={a.shape}")
    return np.ascontiguousarray(a)


def validate(reference_beats, estimated_beats):
    """mir_eval.beat.validate: warn on empty input; raise ValueError for events after 30000 s, not 1-d or decreasing (and,
    unlike mir_eval, for non-finite times, which the library's status word also flags)."""
    if np.size(reference_beats) == 0:
        warnings.warn("Reference beats are empty.")
    if np.size(estimated_beats) == 0:
        warnings.warn("Estimated beats are empty.")
    for what, beats in (("reference", reference_beats), ("estimated", estimated_beats)):
        beats = np.asarray(beats, dtype=np.float64)
        if (beats > MAX_TIME).any():
            raise ValueError(f"An event at time {beats.max()} was found which is greater than the maximum allowable time of "
                             f"max_time = {MAX_TIME} (did you supply event times in seconds?)")
        if beats.ndim != 1:
            raise ValueError(f"Event times should be 1-d numpy ndarray, but shape={beats.shape}")
        if not np.isfinite(beats).all():
            raise ValueError(f"{what} event times must be finite")
        if (np.diff(beats) < 0).any():
            raise ValueError("Events should be in increasing order.")


def _host_row(ref, est, thresholds, min_beat_time=-np.inf) -> np.ndarray:
    ref, est = _events(ref, "reference"), _events(est, "estimated")
    out = np.zeros(len(COLUMNS), np.float64)
    roff = np.array([0, ref.size], np.int64)
    eoff = np.array([0, est.size], np.int64)
    _lib.check(_lib.lib().bt_beat_metrics_host(ref.ctypes.data, roff.ctypes.data, est.ctypes.data, eoff.ctypes.data, 1,
                                               float(min_beat_time), *thresholds, out.ctypes.data))
    if out[11]:
        raise ValueError(_status_text(int(out[11])))
    return out


def _status_text(status: int) -> str:
    parts = []
    for shift, side in ((0, "reference"), (3, "estimated")):
        for bit, text in ((STATUS_NONFINITE, "not finite"), (STATUS_UNSORTED, "not in increasing order"),
                          (STATUS_LATE, f"after max_time = {MAX_TIME}")):
            if status & (bit << shift):
                parts.append(f"{side} events {text}")
    if status & STATUS_NEAREST:
        parts.append("nearest annotation not monotone in the estimates (events closer than the rounding of their distances)")
    if status & STATUS_OFFSETS:
        parts.append("bad track offsets")
    if status & STATUS_PSCORE:
        parts.append("p_score undefined: all reference beats fall into one 10 ms index (mir_eval: cannot convert float NaN "
                     "to integer)")
    return "; ".join(parts) or f"status {status}"


def trim_beats(beats, min_beat_time=5.0):
    """mir_eval.beat.trim_beats: the beats at or after ``min_beat_time``"""
    beats = np.asarray(beats)
    return beats[beats >= min_beat_time]


def f_measure(reference_beats, estimated_beats, f_measure_threshold=0.07):
    """mir_eval.beat.f_measure"""
    validate(reference_beats, estimated_beats)
    return float(_host_row(reference_beats, estimated_beats, _thresholds(dict(f_measure_threshold=f_measure_threshold)))[0])


def cemgil(reference_beats, estimated_beats, cemgil_sigma=0.04):
    """mir_eval.beat.cemgil -> (cemgil, cemgil_max over the five reference variations)"""
    validate(reference_beats, estimated_beats)
    row = _host_row(reference_beats, estimated_beats, _thresholds(dict(cemgil_sigma=cemgil_sigma)))
    return float(row[3]), float(row[4])


def continuity(reference_beats, estimated_beats, continuity_phase_threshold=0.175, continuity_period_threshold=0.175):
    """mir_eval.beat.continuity -> (CMLc, CMLt, AMLc, AMLt)"""
    validate(reference_beats, estimated_beats)
    if np.size(reference_beats) == 1:
        warnings.warn("Only one reference beat was provided, so beat intervals cannot be computed.")
    if np.size(estimated_beats) == 1:
        warnings.warn("Only one estimated beat was provided, so beat intervals cannot be computed.")
    row = _host_row(reference_beats, estimated_beats,
                    _thresholds(dict(continuity_phase_threshold=continuity_phase_threshold,
                                     continuity_period_threshold=continuity_period_threshold)))
    return tuple(float(v) for v in row[5:9])


def _ext_args(kw):
    t = {**EXT_DEFAULTS, **kw}
    bins = t["bins"]
    if int(bins) != bins:
        raise ValueError(f"bins must be an integer, not {bins!r}")
    return (float(t["goto_threshold"]), float(t["goto_mu"]), float(t["goto_sigma"]), float(t["p_score_threshold"]), int(bins))


def _host_row_ext(ref, est, min_beat_time=-np.inf, **kw) -> np.ndarray:
    """one bt_beat_metrics_ext_host row; ValueError on every status but STATUS_PSCORE, which the caller reads"""
    ref, est = _events(ref, "reference"), _events(est, "estimated")
    out = np.zeros(len(EXT_COLUMNS), np.float64)
    roff = np.array([0, ref.size], np.int64)
    eoff = np.array([0, est.size], np.int64)
    _lib.check(_lib.lib().bt_beat_metrics_ext_host(ref.ctypes.data, roff.ctypes.data, est.ctypes.data, eoff.ctypes.data, 1,
                                                   float(min_beat_time), *_ext_args(kw), out.ctypes.data))
    if int(out[11]) & ~STATUS_PSCORE:
        raise ValueError(_status_text(int(out[11])))
    return out


def _warn_single(reference_beats, estimated_beats):
    if np.size(reference_beats) == 1:
        warnings.warn("Only one reference beat was provided, so beat intervals cannot be computed.")
    if np.size(estimated_beats) == 1:
        warnings.warn("Only one estimated beat was provided, so beat intervals cannot be computed.")


def goto(reference_beats, estimated_beats, goto_threshold=0.35, goto_mu=0.2, goto_sigma=0.2):
    """mir_eval.beat.goto -> 1.0 or 0.0.  (With goto_threshold >= 1 no beat counts as incorrect and mir_eval raises
    IndexError; this returns 0.0.)"""
    validate(reference_beats, estimated_beats)
    return float(_host_row_ext(reference_beats, estimated_beats, goto_threshold=goto_threshold, goto_mu=goto_mu,
                               goto_sigma=goto_sigma)[0])


def p_score(reference_beats, estimated_beats, p_score_threshold=0.2):
    """mir_eval.beat.p_score; ValueError, as in mir_eval, when no two reference beats differ by a 10 ms index"""
    validate(reference_beats, estimated_beats)
    _warn_single(reference_beats, estimated_beats)
    row = _host_row_ext(reference_beats, estimated_beats, p_score_threshold=p_score_threshold)
    if int(row[11]) & STATUS_PSCORE:
        raise ValueError(_status_text(STATUS_PSCORE))
    return float(row[1])


def information_gain(reference_beats, estimated_beats, bins=41):
    """mir_eval.beat.information_gain (``bins``: 1 .. 1024)"""
    validate(reference_beats, estimated_beats)
    if not bins % 2:
        warnings.warn("bins parameter is even, so there will not be a bin centered at zero.")
    _warn_single(reference_beats, estimated_beats)
    return float(_host_row_ext(reference_beats, estimated_beats, bins=bins)[2])


def _filtered(fn, names, args, kwargs):
    """mir_eval.util.filter_kwargs: call fn with those of kwargs that it takes"""
    return fn(*args, **{k: v for k, v in kwargs.items() if k in names})


def evaluate(reference_beats, estimated_beats, **kwargs):
    """mir_eval.beat.evaluate: trim both arrays (``min_beat_time``, default 5.0), then every metric under mir_eval's keys in
    mir_eval's order.  Keyword names that no metric takes are ignored."""
    import collections

    reference_beats = _filtered(trim_beats, ("min_beat_time",), (reference_beats,), kwargs)
    estimated_beats = _filtered(trim_beats, ("min_beat_time",), (estimated_beats,), kwargs)
    both = (reference_beats, estimated_beats)
    scores = collections.OrderedDict()
    scores["F-measure"] = _filtered(f_measure, ("f_measure_threshold",), both, kwargs)
    scores["Cemgil"], scores["Cemgil Best Metric Level"] = _filtered(cemgil, ("cemgil_sigma",), both, kwargs)
    scores["Goto"] = _filtered(goto, ("goto_threshold", "goto_mu", "goto_sigma"), both, kwargs)
    scores["P-score"] = _filtered(p_score, ("p_score_threshold",), both, kwargs)
    (scores["Correct Metric Level Continuous"], scores["Correct Metric Level Total"], scores["Any Metric Level Continuous"],
     scores["Any Metric Level Total"]) = _filtered(continuity, ("continuity_phase_threshold", "continuity_period_threshold"),
                                                   both, kwargs)
    scores["Information gain"] = _filtered(information_gain, ("bins",), both, kwargs)
    return scores


class Metrics:
    """The reference's Metrics (pl_module.py:320-339): trim both arrays to ``eval_trim_beats`` seconds, then
    ``{"F-measure", "Cemgil"}`` for step "val" and ``{"F-measure", "Cemgil", "CMLt", "AMLt"}`` for step "test"; "Cemgil" is
    the (cemgil, cemgil_max) tuple mir_eval returns.  One host call computes every value."""

    def __init__(self, eval_trim_beats: int) -> None:
        self.min_beat_time = eval_trim_beats

    def __call__(self, truth, preds, step):
        if step not in ("val", "test"):
            raise ValueError("step must be either val or test")
        truth = trim_beats(truth, min_beat_time=self.min_beat_time)
        preds = trim_beats(preds, min_beat_time=self.min_beat_time)
        validate(truth, preds)
        row = _host_row(truth, preds, _thresholds({}))
        out = {"F-measure": float(row[0]), "Cemgil": (float(row[3]), float(row[4]))}
        if step == "test":
            out["CMLt"] = float(row[6])
            out["AMLt"] = float(row[8])
        return out


def _csr(tracks, what):
    arrs = [_events(t, f"{what} {i}") for i, t in enumerate(tracks)]
    off = np.zeros(len(arrs) + 1, np.int64)
    np.cumsum([a.size for a in arrs], out=off[1:])
    flat = np.concatenate(arrs) if arrs and off[-1] else np.zeros(1, np.float64)   # (never an empty allocation)
    return flat, off


def invalid_tracks_error(status, ignore=0):
    """the ValueError that names the first track whose status has a bit outside ``ignore``, or None"""
    bad = np.nonzero(np.asarray(status).astype(np.int64) & ~ignore)[0]
    if not bad.size:
        return None
    return ValueError(f"track {int(bad[0])}: {_status_text(int(status[bad[0]]))}"
                      + (f" (and {bad.size - 1} more tracks)" if bad.size > 1 else ""))


def beat_metrics_many(truths, preds, eval_trim_beats=5, device="cuda", raise_on_invalid=True, extended=False,
                      goto_threshold=0.35, goto_mu=0.2, goto_sigma=0.2, p_score_threshold=0.2, bins=41, **thresholds) -> dict:
    """Metrics of many tracks in ONE bt_beat_metrics call: one upload (truths, predictions and offsets in one pinned buffer),
    one launch pair, one device-to-host copy.  ``truths`` / ``preds``: sequences of 1-d beat-time arrays of equal length;
    ``eval_trim_beats``: trim_beats' min_beat_time (None keeps every beat); ``thresholds``: mir_eval's keyword names
    (f_measure_threshold, cemgil_sigma, continuity_phase_threshold, continuity_period_threshold).

    -> dict of (n_tracks,) float64 arrays: "F-measure", "Precision", "Recall", "Cemgil", "CemgilMax", "CMLc", "CMLt", "AMLc",
    "AMLt", "n_ref", "n_est", "status", and "Cemgil_reported" = (Cemgil + CemgilMax) / 2.  The last is what
    compute_paper_metrics.py prints as "Cemgil": Metrics returns mir_eval's (cemgil, cemgil_max) tuple per piece, and the
    np.mean over pieces (pl_module.py:156-160) averages both values of every tuple.
    A track whose status is non-zero (where mir_eval's validate raises) raises ValueError, or, with
    ``raise_on_invalid=False``, keeps NaN metrics and its status bits.

    ``extended=True``: one bt_beat_metrics_ext call more on the same upload, with mir_eval's ``goto_threshold``, ``goto_mu``,
    ``goto_sigma``, ``p_score_threshold`` and ``bins`` (unused otherwise).  It adds "Goto", "P-score", "Information gain", the
    quantities behind them ("GotoCriteria", "GotoTrackLen", "GotoMean", "GotoStd", "PWindow", "PHits", "EntropyFwd",
    "EntropyBwd"; include/beat_this_amd.h) and "status_ext": "status", or STATUS_PSCORE where mir_eval's p_score raises (NaN
    "P-score", "PWindow" and "PHits"; such a track is invalid too)."""
    if len(truths) != len(preds):
        raise ValueError(f"{len(truths)} truth arrays but {len(preds)} prediction arrays")
    n = len(truths)
    th = _thresholds(thresholds)
    ext = _ext_args(dict(goto_threshold=goto_threshold, goto_mu=goto_mu, goto_sigma=goto_sigma,
                         p_score_threshold=p_score_threshold, bins=bins)) if extended else None
    keys = ("F-measure", "Precision", "Recall", "Cemgil", "CemgilMax", "CMLc", "CMLt", "AMLc", "AMLt", "n_ref", "n_est",
            "status")
    if n == 0:
        out = {k: np.zeros(0) for k in keys}
        out["Cemgil_reported"] = np.zeros(0)
        if extended:
            out.update({k: np.zeros(0) for k in EXT_KEYS})
        return out
    ref, roff = _csr(truths, "truth")
    est, eoff = _csr(preds, "prediction")
    dev = torch.device(device)
    _lib.require_gpu(torch.empty(0, device=dev), "beat_metrics_many's device")
    # one host block -> one upload: [ref | est | ref offsets | est offsets] as float64 / int64 words
    host = np.concatenate([ref, est, roff.view(np.float64), eoff.view(np.float64)])
    d_in = _lib.upload(host, dev)
    d_ref = d_in.data_ptr()
    d_est = d_ref + 8 * ref.size
    d_roff = d_est + 8 * est.size
    d_eoff = d_roff + 8 * roff.size
    L = _lib.lib()
    ws_bytes = L.bt_beat_metrics_workspace_bytes(n, int(roff[-1]), int(eoff[-1]))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    d_out = torch.empty((n, len(keys)), dtype=torch.float64, device=dev)
    mbt = -np.inf if eval_trim_beats is None else float(eval_trim_beats)
    with torch.cuda.device(dev):
        _lib.check(L.bt_beat_metrics(_lib.stream_ptr(dev), d_ref, d_roff, d_est, d_eoff, n, mbt, *th, ws.data_ptr(), ws_bytes,
                                     d_out.data_ptr()))
        if extended:
            xws_bytes = L.bt_beat_metrics_ext_workspace_bytes(n, int(roff[-1]), int(eoff[-1]))
            xws = torch.empty(max(xws_bytes, 1), dtype=torch.uint8, device=dev)
            d_xout = torch.empty((n, len(EXT_KEYS)), dtype=torch.float64, device=dev)
            _lib.check(L.bt_beat_metrics_ext(_lib.stream_ptr(dev), d_ref, d_roff, d_est, d_eoff, n, mbt, *ext, xws.data_ptr(),
                                             xws_bytes, d_xout.data_ptr()))
    rows = d_out.cpu().numpy()
    out = {k: rows[:, i].copy() for i, k in enumerate(keys)}
    out["Cemgil_reported"] = (out["Cemgil"] + out["CemgilMax"]) / 2
    status = out["status"]
    if extended:
        xrows = d_xout.cpu().numpy()
        out.update({k: xrows[:, i].copy() for i, k in enumerate(EXT_KEYS)})
        status = (status.astype(np.int64) | out["status_ext"].astype(np.int64)).astype(np.float64)
    err = invalid_tracks_error(status) if raise_on_invalid else None
    if err is not None:
        raise err
    return out
