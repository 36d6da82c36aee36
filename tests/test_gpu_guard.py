"""Guard bands and poisoned memory around the device entry points (tests/gpu_util.py: Guarded).

Every buffer a call touches -- input, output, workspace -- is its own allocation with a 2 MiB band on each side, and the
forward's workspace has a gap of GAP bytes behind every region (BT_OPT_WS_GUARD).  Each case runs once on zero-filled memory
and once per poison pattern (0xFF: NaN in every float type; 0x7B: large finite values), inputs holding real data and only their
bands poisoned.  Then:
  * outputs (and, under BT_PREC_F32X3, the range-flag word) are bit-identical to the clean run: nothing reads memory the call
    did not write, nor past the end of an input;
  * every band and every workspace gap still holds its fill byte: nothing writes outside its buffer or region;
  * the clean run matches the oracle at the tolerance the entry point's own test uses.

Poisoning the whole workspace is safe for the forward: the only index-like words in it are the F32X3 attention's overflow map
(attn2.hip), written for every (sequence, head, query block) by the attention launch before its fix-up launch reads it (a word
read there selects query blocks < nblk and tokens < 32 only), and the range flag, which bt_forward_stages clears first.  The
one-call path's own regions (chunks, logits, peak frames) are written before they are read; its peak counts live in LDS."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from gpu_util import (HALF, POISONS, Guarded, _mk, assert_intact, dev, gaps_intact, report, workspace_regions)

pytestmark = pytest.mark.gpu

GAP = 1 << 20                        # BT_OPT_WS_GUARD of these tests: more than a 128-row tile of 2048 fp32 columns past a region
TOL = {0: 1e-3, 1: 5e-2, 3: 3e-4}    # logits against the oracle: exact fp32 gate, half (fp16-autocast scale), F32X3
PRECS = (0, 1, 3)


def _lib():
    from beat_this_amd import _lib as L

    return L


def _bits(t):
    return t.contiguous().view(torch.int32) if t.element_size() == 4 else t.contiguous().view(torch.int16)


def _same(a, b):
    """bit-identical (NaN patterns included)"""
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _hp(name):
    from beat_this_amd import weights as W

    hp = dict(W.resolve_hparams("small0"))
    if name in ("small0", "final0"):
        return dict(W.resolve_hparams(name))
    if name == "no_sum_head":
        hp["sum_head"] = False
    elif name == "no_partial":
        hp["partial_transformers"] = False
    elif name == "d64_ffmult2":
        hp.update(transformer_dim=64, n_layers=2, ff_mult=2)
    elif name == "d192":
        hp.update(transformer_dim=192, n_layers=2)
    else:
        hp.update(transformer_dim=256, n_layers=3)
    return hp


_MODELS = {}


def _model(name, seed=21):
    """(BeatThis on the GPU, state dict, hparams); the engine's workspace guard is on"""
    key = (name, seed)
    if key not in _MODELS:
        from beat_this_amd import weights as W
        from beat_this_amd.model import BeatThis

        _MODELS.clear()   # (one model at a time: engines hold their weights on the device)
        hp = _hp(name)
        sd = W.random_state_dict(hp, seed=seed, style="lively")
        m = BeatThis(**{k: hp[k] for k in ("spect_dim", "transformer_dim", "ff_mult", "n_layers", "head_dim", "stem_dim",
                                           "sum_head", "partial_transformers")})
        m.load_state_dict(sd)
        m = m.to(dev())
        m.engine().set_options({"ws_guard": GAP})
        _MODELS[key] = (m, sd, dict(hp, seed=seed))
    return _MODELS[key]


_SPECTS = {}


def _chunk(T, i):
    key = (T, i)
    if key not in _SPECTS:
        from beat_this_amd import weights as W

        _SPECTS[key] = torch.from_numpy(W.synthetic_spect(T, seed=1000 + 7 * T + i))
    return _SPECTS[key]


_ORACLE = {}


def _oracle(name, sd, hp, T, i):
    key = (name, hp.get("seed"), T, i)
    if key not in _ORACLE:
        from oracle import beat_this_oracle as O

        with torch.inference_mode():
            b, d = O.model_forward(sd, _chunk(T, i)[None], sum_head=hp["sum_head"])
        _ORACLE[key] = (b[0], d[0])
    return _ORACLE[key]


def _forward(eng, prec, first, last, x, pattern, check_gaps=True):
    """bt_forward_stages on guarded buffers, every byte (input bands, workspace, outputs) = pattern; -> dict of output copies"""
    L = _lib()
    lib = L.lib()
    B, T = int(x.shape[0]), int(x.shape[1])
    D = eng.packed.desc.transformer_dim
    total = lib.bt_workspace_bytes(eng._h, B, T, prec)
    regions = workspace_regions(eng._h, B, T, prec)
    ws = Guarded((total,), torch.uint8).fill(pattern)
    inp = Guarded(x.shape, torch.float32).fill(pattern, x.to(dev()))
    outs = [("beat", Guarded((B, T), torch.float32)), ("downbeat", Guarded((B, T), torch.float32))] if last == 2 else \
        [("out", Guarded((B, T, D), torch.float32))]
    for _, g in outs:
        g.fill(pattern)
    o = dict(outs)
    with torch.cuda.device(dev()):
        L.check(lib.bt_forward_stages(eng._h, L.stream_ptr(dev()), prec, first, last, inp.ptr(), B, T, ws.ptr(), total,
                                      o["out"].ptr() if last < 2 else 0, o["beat"].ptr() if last == 2 else 0,
                                      o["downbeat"].ptr() if last == 2 else 0))
    torch.cuda.synchronize()
    where = f"prec {prec} stages {first}..{last} B {B} T {T} fill 0x{pattern:02X}"
    assert_intact((f"input ({where})", inp), (f"workspace ({where})", ws), *((f"{n} ({where})", g) for n, g in outs))
    if check_gaps:
        msg = gaps_intact(ws.t, ws.pattern, regions, total, f"workspace ({where})")
        assert msg is None, msg
    assert torch.equal(inp.t, x.to(dev())), f"the input was modified ({where})"
    res = {n: g.t.clone() for n, g in outs}
    if prec == 3:
        res["range_flag"] = ws.t[:4].view(torch.int32).clone()
    del ws, inp, outs, o
    return res


def _poisoned_runs_match(eng, prec, first, last, x, check_gaps=True):
    clean = _forward(eng, prec, first, last, x, 0x00, check_gaps)
    for p in POISONS:
        got = _forward(eng, prec, first, last, x, p, check_gaps)
        for k in clean:
            assert _same(got[k], clean[k]), (f"{k} differs from the clean run under fill 0x{p:02X} (prec {prec}, stages "
                                             f"{first}..{last}, B {x.shape[0]}, T {x.shape[1]}): a read of unwritten memory")
    return clean


def _check_oracle(name, sd, hp, prec, res, T, idx, tol=None):
    err = 0.0
    for row, i in idx:
        ob, od = _oracle(name, sd, hp, T, i)
        err = max(err, float((res["beat"][row].cpu() - ob).abs().max()), float((res["downbeat"][row].cpu() - od).abs().max()))
    assert err < (tol or TOL[prec]), (name, prec, T, err)
    return err


# ---- the forward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["small0", "final0"])
def test_forward_guarded_and_poisoned(name, prec):
    """bt_forward (stages 0..2) for B in {1, 2, 11, 33} x T in {1, 37, 1012, 1500, rope_len}: clean and poisoned runs bit for
    bit, bands and region gaps intact, first and last chunk against the oracle."""
    m, sd, hp = _model(name)
    eng = m.engine()
    worst = 0.0
    t0 = time.time()
    for T in (1, 37, 1012, 1500, eng.packed.desc.rope_len):
        for B in (1, 2, 11, 33):
            x = torch.stack([_chunk(T, i) for i in range(B)])
            clean = _poisoned_runs_match(eng, prec, 0, 2, x)
            worst = max(worst, _check_oracle(name, sd, hp, prec, clean, T, [(0, 0), (B - 1, B - 1)]))
    report("guard_forward", model=name, prec=prec, err=worst, wall_s=time.time() - t0,
           peak_gb=torch.cuda.max_memory_allocated() / 1e9)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["small0", "final0"])
def test_forward_stage_ranges_guarded_and_poisoned(name, prec):
    """bt_forward_stages for every (first, last): each stage's input is the clean output of the stage before it"""
    m, sd, hp = _model(name)
    eng = m.engine()
    for B, T in ((2, 37), (3, 1500)):
        x = torch.stack([_chunk(T, i) for i in range(B)])
        front = _poisoned_runs_match(eng, prec, 0, 0, x)["out"]
        blocks = _poisoned_runs_match(eng, prec, 0, 1, x)["out"]
        _poisoned_runs_match(eng, prec, 1, 1, front)
        _poisoned_runs_match(eng, prec, 1, 2, front)
        _poisoned_runs_match(eng, prec, 2, 2, blocks)
        clean = _poisoned_runs_match(eng, prec, 0, 2, x)
        _check_oracle(name, sd, hp, prec, clean, T, [(0, 0), (B - 1, B - 1)])


@pytest.mark.parametrize("name", ["no_sum_head", "no_partial", "three_layers_d256", "d64_ffmult2", "d192"])
def test_ablation_variants_guarded_and_poisoned(name):
    """the five ablation variants of test_gpu_model.py in three precisions at two shapes (half: 2.5e-2 as there; F32X3: the 3e-4
    of the other forwards here -- these inputs put no_sum_head at 1.55e-4, just over the 1.5e-4 test_gpu_model.py holds its own
    T = 700 inputs to)"""
    m, sd, hp = _model(name)
    eng = m.engine()
    for B, T in ((2, 37), (11, 1012)):
        x = torch.stack([_chunk(T, i) for i in range(B)])
        for prec in PRECS:
            clean = _poisoned_runs_match(eng, prec, 0, 2, x)
            _check_oracle(name, sd, hp, prec, clean, T, [(0, 0), (B - 1, B - 1)], tol={0: 1e-3, 1: 2.5e-2, 3: 3e-4}[prec])


@pytest.mark.parametrize("option,value", [("x3_gemm_fp8", 2), ("x3_attn_p16", 2)])
def test_x3_options_guarded_and_poisoned(option, value):
    """BT_OPT_X3_GEMM_FP8 = 2 (hl8 operands in every main-layer GEMM) and BT_OPT_X3_ATTN_P16 = 2 (P16 in the frontend too) on
    final0: held to the 1e-3 gate like test_gpu_scale's fp8 case"""
    m, sd, hp = _model("final0")
    eng = m.engine()
    eng.set_options({option: value})
    try:
        assert eng.get_option("ws_guard") == GAP
        x = torch.stack([_chunk(1500, i) for i in range(3)])
        clean = _poisoned_runs_match(eng, 3, 0, 2, x)
        _check_oracle("final0", sd, hp, 3, clean, 1500, [(0, 0), (2, 2)], tol=1e-3)
    finally:
        eng.set_options({option: {"x3_gemm_fp8": 0, "x3_attn_p16": 1}[option]})


def _unit(eng, prec, unit, index, x, out_shape, pattern):
    L = _lib()
    lib = L.lib()
    B, T = int(x.shape[0]), int(x.shape[1])
    total = lib.bt_workspace_bytes(eng._h, B, T, prec)
    regions = workspace_regions(eng._h, B, T, prec)
    ws = Guarded((total,), torch.uint8).fill(pattern)
    inp = Guarded(x.shape, torch.float32).fill(pattern, x)
    out = Guarded(out_shape, torch.float32).fill(pattern)
    with torch.cuda.device(dev()):
        L.check(lib.bt_forward_unit(eng._h, L.stream_ptr(dev()), prec, unit, index, inp.ptr(), out.ptr(), B, T, ws.ptr(), total))
    torch.cuda.synchronize()
    where = f"unit {unit}.{index} prec {prec} fill 0x{pattern:02X}"
    assert_intact((f"input ({where})", inp), (f"workspace ({where})", ws), (f"output ({where})", out))
    msg = gaps_intact(ws.t, ws.pattern, regions, total, f"workspace ({where})")
    assert msg is None, msg
    return out.t.clone()


@pytest.mark.parametrize("prec", [0, 1])
def test_forward_units_guarded_and_poisoned(prec):
    """bt_forward_unit: the stem, a leaf of each direction, a frontend block (partial transformer, conv), frontend.linear, a
    main layer's attention and FF and the final norm, on small0 (B = 2, T = 37: partial tiles and partial 32-token blocks)"""
    L = _lib()
    m, sd, hp = _model("small0")
    eng = m.engine()
    B, T, D = 2, 37, hp["transformer_dim"]
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(s, generator=g).to(dev())   # noqa: E731
    cases = [(L.UNIT_STEM, 0, torch.stack([_chunk(T, i) for i in range(B)]).to(dev()), (B, T, 32, 32)),
             (L.UNIT_FRONT_ATTN, 0, rnd(B * T, 32, 32), (B * T, 32, 32)), (L.UNIT_FRONT_FF, 3, rnd(B * 16, T, 64), (B * 16, T, 64)),
             (L.UNIT_PARTIAL, 1, rnd(B, T, 16, 64), (B, T, 16, 64)), (L.UNIT_CONV, 1, rnd(B, T, 16, 64), (B, T, 8, 128)),
             (L.UNIT_LINEAR, 0, rnd(B, T, 4, 256), (B, T, D)), (L.UNIT_ATTN, 2, rnd(B, T, D), (B, T, D)),
             (L.UNIT_FF, 5, rnd(B, T, D), (B, T, D)), (L.UNIT_NORM, 0, rnd(B, T, D), (B, T, D))]
    for unit, index, x, shape in cases:   # (the leaves take B = sequences, T = tokens per sequence)
        clean = _unit(eng, prec, unit, index, x, shape, 0x00)
        assert torch.isfinite(clean).all(), (unit, index)
        for p in POISONS:
            assert _same(_unit(eng, prec, unit, index, x, shape, p), clean), (unit, index, hex(p))


# ---- batches on either side of the size-driven route bounds -------------------------------------------------------------
def _route_bounds(hp, T):
    """{precision: [(largest B on one side of a size-driven route change, what changes there)]} at chunk length T:
    the main layers leave the fragment-major kernels when B T ff_mult D x 4 (F32X3) / x 2 (half) reaches 2^31 bytes
    (engine.hip plan_route); the frontend convolutions and frontend.linear leave gemm3 when gemm3_supported's
    M lda x operand bytes reaches 2^31 -- both have M lda = B T 1024 (conv: M = B T F / 2 rows of lda = 2 C, F C = 512;
    linear: B T rows of 1024) -- which only matters while the main layers are still fragment-major (conv3 / lin3 need it)"""
    wide = T * hp["ff_mult"] * hp["transformer_dim"]
    out = {}
    for prec, eb in ((3, 4), (1, 2)):
        main = (0x7FFFFFFF - 1) // (wide * eb)
        front = (0x7FFFFFFF - 1) // (T * 1024 * eb)
        out[prec] = [(main, "main layers")] + ([(front, "frontend gemm3")] if front < main else [])
    return out


ROUTE_CASES = [("final0", 3, 174, "main layers"), ("final0", 1, 349, "main layers"), ("small0", 3, 349, "frontend gemm3")]


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("case", range(len(ROUTE_CASES)))
def test_forward_on_either_side_of_the_route_bound(case, side):
    """T = 1500 with B just below (side 0) and just above (side 1) a size-driven route change (final0: the main layers in
    F32X3 and half; small0 in F32X3: frontend conv / linear leave gemm3 at B = 350, the main layers only at 700).  Three
    distinct chunks at the first, middle and last positions, the others repeating them; a clean run and a 0xFF-poisoned one,
    bit for bit; every copy of a chunk bit-identical to the other copies; the distinct chunks against the oracle; below the
    bound each chunk bit-identical to itself forwarded alone (the same route)."""
    name, prec, want, what = ROUTE_CASES[case]
    m, sd, hp = _model(name)
    eng = m.engine()
    T = 1500
    assert (want, what) in _route_bounds(hp, T)[prec]
    B = want + side
    seq = [i % 3 for i in range(B)]
    seq[0], seq[B // 2], seq[-1] = 0, 1, 2
    x = torch.stack([_chunk(T, 100 + i) for i in range(3)])
    t0 = time.time()
    torch.cuda.reset_peak_memory_stats()
    res = _forward(eng, prec, 0, 2, x[seq], 0x00)
    wall = time.time() - t0
    peak = torch.cuda.max_memory_allocated() / 1e9
    poisoned = _forward(eng, prec, 0, 2, x[seq], 0xFF)
    for k in res:
        assert _same(poisoned[k], res[k]), f"{k} differs from the clean run under fill 0xFF, B = {B}"
    del poisoned
    first = {k: seq.index(k) for k in range(3)}
    for k in ("beat", "downbeat"):
        for row, c in enumerate(seq):
            assert _same(res[k][row], res[k][first[c]]), f"{k}: chunk {row} (a copy of chunk {first[c]}) differs, B = {B}"
    if prec == 3:
        assert int(res["range_flag"]) == 0
    err = 0.0
    for c in range(3):
        ob, od = _oracle(name, sd, hp, T, 100 + c)
        err = max(err, float((res["beat"][first[c]].cpu() - ob).abs().max()), float((res["downbeat"][first[c]].cpu() - od).abs().max()))
    alone_same = None
    if side == 0:
        alone_same = True
        for c in range(3):
            a = _forward(eng, prec, 0, 2, x[c:c + 1], 0xFF)
            alone_same = alone_same and _same(a["beat"][0], res["beat"][first[c]]) and _same(a["downbeat"][0], res["downbeat"][first[c]])
    report("guard_route_bound", model=name, prec=prec, B=B, err=err, alone_bit_identical=alone_same, wall_s=wall, peak_gb=peak)
    del res
    torch.cuda.empty_cache()
    assert err < TOL[prec], err
    assert alone_same in (None, True), "a chunk differs from itself forwarded alone on the same route"


# ---- the one-call path and captured forwards --------------------------------------------------------------------------
def _a2b(name="small0", prec_mode=False):
    from beat_this_amd.inference import Audio2Beats

    m, sd, hp = _model(name, seed=4)
    a2b = Audio2Beats(checkpoint_path=None, device=dev(), float16=prec_mode, dbn=False)
    a2b.model = m
    return a2b, m.engine(), sd


def _one_call(a2b, eng, sig, sr, prec, pattern, ws=None, use_graph=0):
    """bt_audio2beats_enqueue on a guarded workspace (every byte = pattern unless ws is passed in as it is) and a guarded
    waveform -> (peak frames + counts + flag, framewise logits, ws)"""
    from math import gcd

    from beat_this_amd.inference import _resample_filter

    L = _lib()
    lib = L.lib()
    g = gcd(sr, 22050)
    up, down = 22050 // g, sr // g
    plan = L.A2BPlan()
    L.check(lib.bt_audio2beats_plan(eng._h, len(sig), up, down, prec, C.byref(plan)))
    if ws is None:
        ws = Guarded((plan.ws_bytes,), torch.uint8).fill(pattern)
    wave = Guarded((len(sig),), torch.float32).fill(pattern, torch.from_numpy(sig.astype(np.float32)).to(dev()))
    h, half = _resample_filter(up, down, dev()) if up != down else (None, 0)
    host = torch.zeros(plan.result_words, dtype=torch.int32).pin_memory()
    with torch.cuda.device(dev()):
        L.check(lib.bt_audio2beats_enqueue(eng._h, L.stream_ptr(dev()), prec, C.byref(a2b.spect._get_tables()), wave.ptr(), len(sig),
                                           up, down, L.ptr(h), half, ws.ptr(), ws.nbytes, host.data_ptr(), use_graph))
    torch.cuda.synchronize()
    where = f"one call, {len(sig)} samples at {sr} Hz, prec {prec}, fill 0x{ws.pattern:02X}"
    assert_intact((f"waveform ({where})", wave), (f"workspace ({where})", ws))
    fws = ws.t[plan.off_forward:plan.off_forward + plan.forward_bytes]
    msg = gaps_intact(fws, ws.pattern, workspace_regions(eng._h, plan.B, plan.T, prec), plan.forward_bytes, f"forward workspace ({where})")
    assert msg is None, msg
    n = int(plan.n_frames)
    r = host.numpy()
    nb, nd = int(r[2 * n]), int(r[2 * n + 1])
    result = np.concatenate([r[:nb], r[n:n + nd], r[2 * n:2 * n + 3]])
    logits = ws.t[plan.off_logits:plan.off_logits + 8 * n].view(torch.float32).clone()
    return result, logits, ws, plan


@pytest.mark.parametrize("sr", [22050, 44100, 48000])
def test_one_call_guarded_and_poisoned(sr):
    """bt_audio2beats_plan / _enqueue (plain launches): 1, 2 and 11 chunks and 1501 frames (one frame over a chunk's fresh
    part); peak frames, counts, range flag and framewise logits bit-identical under poison, logits against the oracle"""
    from beat_this_amd import weights as W
    from oracle import beat_this_oracle as O

    a2b, eng, sd = _a2b()
    frames = [300, 1489 + 800, 1501] + ([15500] if sr == 22050 else [])
    for nf in frames:
        n22 = (nf - 1) * 441 + 200
        sig = W.synthetic_audio(n22 / 22050, seed=nf, sr=sr)
        res, logits, _, plan = _one_call(a2b, eng, sig, sr, 3, 0x00)
        assert plan.n_frames in (nf, nf + 1) and plan.B == max(1, -(-int(plan.n_frames) // 1488))
        for p in POISONS:
            r2, l2, _, _ = _one_call(a2b, eng, sig, sr, 3, p)
            assert np.array_equal(r2, res) and _same(l2, logits), (nf, sr, hex(p))
        with torch.inference_mode():
            ob, od = O.audio2frames(sd, sig, sr)
        n = int(plan.n_frames)
        err = max(float((logits[:n].cpu() - ob).abs().max()), float((logits[n:].cpu() - od).abs().max()))
        report("guard_one_call", sr=sr, frames=n, chunks=plan.B, err=err)
        assert err < 1e-3, (nf, err)   # (test_gpu_model.py's one-call / 44.1 kHz tests: the 1e-3 gate)


def test_one_call_graph_replay_on_a_repoisoned_workspace():
    """the engine's own captured forward (FwdGraph): call 1 runs plainly and warms, call 2 captures, then the whole workspace is
    filled with 0xFF and call 3 replays: its result and logits equal a plain run on a zeroed workspace"""
    from beat_this_amd import weights as W

    a2b, eng, _ = _a2b()
    sig = W.synthetic_audio(40.0, seed=3)
    want, want_l, _, plan = _one_call(a2b, eng, sig, 22050, 3, 0x00)
    assert plan.B == 2 and plan.T == 1500
    ws = Guarded((plan.ws_bytes,), torch.uint8).fill(0x00)
    for call in range(2):
        r, l, _, _ = _one_call(a2b, eng, sig, 22050, 3, 0x00, ws=ws, use_graph=1)
        assert np.array_equal(r, want) and _same(l, want_l), call
    ws.fill(0xFF)
    r, l, _, _ = _one_call(a2b, eng, sig, 22050, 3, 0xFF, ws=ws, use_graph=1)
    assert np.array_equal(r, want) and _same(l, want_l)


@pytest.mark.parametrize("prec", [1, 3])
def test_python_graph_entry_replay_on_a_repoisoned_workspace(prec):
    """pack._GraphEntry (B <= Engine.GRAPH_MAX_CHUNKS): warm + capture, refill its workspace with 0xFF, replay -> the logits of
    a plain forward on a zeroed workspace"""
    m, _, _ = _model("small0", seed=4)
    eng = m.engine()
    x = torch.stack([_chunk(1500, 200 + i) for i in range(3)])
    want = _forward(eng, prec, 0, 2, x, 0x00)
    e = eng.graph_forward(3, 1500, prec)
    assert e is not None, getattr(eng, "_graph_error", "")
    e.x.copy_(x.to(dev()))
    e.replay()
    torch.cuda.synchronize()
    assert _same(e.beat, want["beat"]) and _same(e.down, want["downbeat"])
    e.ws.fill_(0xFF)
    e.x.copy_(x.to(dev()))
    e.replay()
    torch.cuda.synchronize()
    assert _same(e.beat, want["beat"]) and _same(e.down, want["downbeat"])


@pytest.mark.parametrize("float16", [False, True])
def test_public_api_results_survive_repoisoned_engine_workspaces(float16):
    """Audio2Beats / many: between two rounds of calls every workspace the engine caches (_ws, _graph_ws, _a2b_ws) is filled
    with 0xFF; beats, downbeats and framewise logits do not change"""
    from beat_this_amd import weights as W

    a2b, eng, _ = _a2b(prec_mode=float16)
    sigs = [W.synthetic_audio(s, seed=int(s)) for s in (7.0, 40.0, 65.0)]

    def run():
        out = [a2b(s, 22050) for s in sigs]
        out += [r for r in a2b.many(sigs, 22050)]
        out += [tuple(t.cpu().numpy() for t in a2b.spect2frames(a2b.signal2spect(s, 22050))) for s in sigs]
        return out

    first = run()
    pools = [w for w, _ in eng._ws.values()] + list(eng.__dict__.get("_graph_ws", {}).values()) + \
        [w for w, _ in eng.__dict__.get("_a2b_ws", {}).values()]
    assert len(pools) >= 2
    with torch.inference_mode():   # (the workspaces were made inside inference mode)
        for w in pools:
            w.fill_(0xFF)
    second = run()
    for a, b in zip(first, second):
        for x, y in zip(a, b):
            assert np.array_equal(np.asarray(x), np.asarray(y))


# ---- single kernels ----------------------------------------------------------------------------------------------------
def _pad256(w):
    """weight rows padded with zeros to a multiple of 256 (the tile height the kernel reads whole)"""
    out = torch.zeros(((w.shape[0] + 255) // 256 * 256, w.shape[1]), dtype=w.dtype)
    out[:w.shape[0]] = w
    return out


def _gemm3(pattern, **kw):
    """bt_gemm3 on guarded buffers: kw maps an argument to a (host tensor or None for an output of that shape/dtype, is_input)"""
    L = _lib()
    a = L.Gemm3Args()
    bufs = {}
    for k, v in kw.items():
        if isinstance(v, tuple):
            t, shape, dtype = v
            g = Guarded(shape, dtype).fill(pattern, t.to(dev()) if t is not None else None)
            bufs[k] = g
            setattr(a, k, g.ptr())
        else:
            setattr(a, k, v)
    L.check(L.lib().bt_gemm3(L.stream_ptr(dev()), C.byref(a)))
    torch.cuda.synchronize()
    assert_intact(*((f"bt_gemm3 {k} (fill 0x{pattern:02X})", g) for k, g in bufs.items()))
    return {k: g.t.clone() for k, g in bufs.items()}


@pytest.mark.parametrize("M,K,N", [(333, 128, 512), (1500, 512, 2048)])
def test_gemm3_ff1_guarded_and_poisoned(M, K, N):
    """FF1 epilogue (RMSNorm factor from partial sums of squares, bias, GELU): M not a multiple of 128, plus the largest shape of
    test_gpu_gemm3.py that fits a guarded test quickly"""
    import math

    x = _mk((M, K), 1, 2.0).float()
    W, b = _mk((N, K), 2, 1 / math.sqrt(K)), _mk((N,), 3)
    xb, Wd = x.to(HALF()), W.float().to(HALF())
    ssq = (x.double() ** 2).view(M, K // 64, 64).sum(-1).T.contiguous().float()

    def run(p):
        return _gemm3(p, A=(xb, (M, K), HALF()), lda=K, M=M, K=K, W=(_pad256(Wd), ((N + 255) // 256 * 256, K), HALF()), N=N, epi=0,
                      bias=(b.float(), (N,), torch.float32), ssq_in=(ssq, (K // 64, M), torch.float32), ssq_parts=K // 64,
                      out=(None, (M, N), HALF()), ldo=N)["out"]

    clean = run(0x00)
    for p in POISONS:
        assert _same(run(p), clean), hex(p)
    rs = math.sqrt(K) / x.double().norm(dim=-1, keepdim=True).clamp_min(1e-12)
    ref = torch.nn.functional.gelu(xb.double() @ Wd.double().T * rs + b)
    err = float((clean.double().cpu() - ref).abs().max() / ref.abs().max())
    assert err < 6e-3, err


@pytest.mark.parametrize("M,K,N,bias", [(777, 512, 512, False), (130, 128, 128, True), (1500, 2048, 512, True)])
def test_gemm3_resid_guarded_and_poisoned(M, K, N, bias):
    """residual epilogue: x += A W^T (+ b), half shadow and partial sums of squares written; x holds real data (an in/out
    operand), every other byte is poisoned"""
    import math

    A = _mk((M, K), 4).float().to(HALF())
    W = _mk((N, K), 5, 0.5 / math.sqrt(K)).float().to(HALF())
    b = _mk((N,), 6)
    x0 = _mk((M, N), 7).float()

    def run(p):
        kw = dict(A=(A, (M, K), HALF()), lda=K, M=M, K=K, W=(_pad256(W), ((N + 255) // 256 * 256, K), HALF()), N=N, epi=1, x=(x0, (M, N), torch.float32),
                  ldx=N, xb=(None, (M, N), HALF()), ssq_out=(None, (N // 64, M), torch.float32))
        if bias:
            kw["bias"] = (b.float(), (N,), torch.float32)
        return _gemm3(p, **kw)

    clean = run(0x00)
    for p in POISONS:
        got = run(p)
        for k in ("x", "xb", "ssq_out"):
            assert _same(got[k], clean[k]), (k, hex(p))
    ref = x0.double() + A.double() @ W.double().T + (b if bias else 0)
    err = float((clean["x"].double().cpu() - ref).abs().max() / ref.abs().max())
    assert err < 1e-5, err


# ---- single-operator entry points: one guarded allocation per operand ----------------------------------------------------
def _guarded_runs(what, call, ins, outs, scratch=(), valid=None):
    """call(ptrs) once with every byte zero and once per poison pattern.  ins: name -> tensor of real data (only its bands are
    poisoned; it must come back unchanged); outs: name -> (shape, dtype), written by the call; scratch: names of outs whose
    PAYLOAD stays zero in every run (index-like words, see the callers), their bands poisoned.  valid(res) -> the parts of the
    outputs the call defines.  Asserts intact bands and bit-identical outputs; -> the clean run's outputs."""
    runs = []
    for p in (0x00,) + POISONS:
        gi = {k: Guarded(v.shape, v.dtype).fill(p, v.to(dev())) for k, v in ins.items()}
        go = {k: Guarded(*sd).fill(p, payload_byte=0 if k in scratch else None) for k, sd in outs.items()}
        call({k: g.ptr() for k, g in {**gi, **go}.items()})
        torch.cuda.synchronize()
        assert_intact(*((f"{what}: {k} (fill 0x{p:02X})", g) for k, g in {**gi, **go}.items()))
        for k, v in ins.items():
            assert torch.equal(gi[k].t, v.to(dev())), f"{what}: input {k} was modified"
        res = {k: g.t.clone() for k, g in go.items() if k not in scratch}
        runs.append(valid(res) if valid else res)
        del gi, go
    for p, r in zip(POISONS, runs[1:]):
        for k in runs[0]:
            assert _same(r[k], runs[0][k]), f"{what}: {k} differs from the clean run under fill 0x{p:02X}"
    return runs[0]


def _ragged_frames():
    """>= 65 ragged pieces: a one-frame piece, the 1488 / 1489 / 1500 / 1501-frame edges, short and multi-chunk ones"""
    rng = np.random.default_rng(7)
    return [1, 1488, 1489, 1500, 1501, 2977, 13, 4465] + [int(v) for v in rng.integers(2, 1600, 60)]


def _chunk_rows(n, T=1500, border=6):
    from oracle import beat_this_oracle as O

    return [int(s) for s in O.split_starts(n, T, border)]


def _split_ref(spect, lo, hi, starts, T):
    """rows s .. s + T - 1 of the piece [lo, hi) (absolute rows; outside the piece: zeros), float64-free: a copy"""
    out = torch.zeros((len(starts), T, 128))
    for b, s in enumerate(starts):
        a0, a1 = max(s, lo), min(s + T, hi)
        if a1 > a0:
            out[b, a0 - s:a1 - s] = spect[a0:a1]
    return out


def _aggregate_ref(cb, cd, starts, lo, hi, T, border):
    """keep_first: frame f takes the first chunk whose centre part [s + border, s + T - border) holds it"""
    n = hi - lo
    beat, down = torch.full((n,), float("nan")), torch.full((n,), float("nan"))
    for c in reversed(range(len(starts))):
        s = starts[c] - lo
        a0, a1 = max(s + border, 0), min(s + T - border, n)
        if a1 > a0:
            beat[a0:a1], down[a0:a1] = cb[c, a0 - s:a1 - s], cd[c, a0 - s:a1 - s]
    return beat, down


def test_split_and_aggregate_single_and_batch_guarded_and_poisoned():
    """bt_split_chunks / bt_aggregate per piece and bt_split_chunks_batch / bt_aggregate_batch over 68 ragged pieces, T = 1500
    chunks, against a direct restatement (both are copies: compared bit for bit).  The chunk and piece tables are inputs
    (real data, only their bands poisoned)."""
    L = _lib()
    lib, st = L.lib(), L.stream_ptr(dev())
    T, border = 1500, 6
    frames = _ragged_frames()
    off = np.concatenate([[0], np.cumsum(frames)])
    total = int(off[-1])
    g = torch.Generator().manual_seed(3)
    spect = torch.randn((total, 128), generator=g)
    rows, pieces, want = [], [], []
    for k, n in enumerate(frames):
        lo, hi = int(off[k]), int(off[k + 1])
        starts = [lo + s for s in _chunk_rows(n, T, border)]
        pieces.append((lo, hi, len(rows), len(rows) + len(starts)))
        rows += [(s, lo, hi, 0) for s in starts]
        want.append(_split_ref(spect, lo, hi, starts, T))
    B = len(rows)
    tab, ptab = torch.tensor(rows, dtype=torch.int32), torch.tensor(pieces, dtype=torch.int32)
    got = _guarded_runs("bt_split_chunks_batch", lambda p: L.check(lib.bt_split_chunks_batch(st, p["spect"], p["rows"], B, T, p["chunks"])),
                        dict(spect=spect, rows=tab), dict(chunks=((B, T, 128), torch.float32)))["chunks"].cpu()
    assert torch.equal(got, torch.cat(want)), "bt_split_chunks_batch"
    cb = torch.randn((B, T), generator=g)
    cd = torch.randn((B, T), generator=g)
    res = _guarded_runs("bt_aggregate_batch", lambda p: L.check(lib.bt_aggregate_batch(
        st, p["cb"], p["cd"], p["rows"], p["pieces"], len(pieces), max(frames), T, border, p["beat"], p["down"])),
        dict(cb=cb, cd=cd, rows=tab, pieces=ptab), dict(beat=((total,), torch.float32), down=((total,), torch.float32)))
    for k, (lo, hi, c0, c1) in enumerate(pieces):
        rb, rd = _aggregate_ref(cb[c0:c1], cd[c0:c1], [r[0] for r in rows[c0:c1]], lo, hi, T, border)
        assert torch.equal(res["beat"][lo:hi].cpu(), rb) and torch.equal(res["down"][lo:hi].cpu(), rd), (k, hi - lo)
    for k in range(8):   # the single-piece forms on the edge cases (chunk starts relative to the piece)
        lo, hi, c0, c1 = pieces[k]
        n, starts = hi - lo, _chunk_rows(hi - lo, T, border)
        s32 = torch.tensor(starts, dtype=torch.int32)
        one = _guarded_runs("bt_split_chunks", lambda p: L.check(lib.bt_split_chunks(st, p["spect"], n, p["starts"], len(starts), T, p["chunks"])),
                            dict(spect=spect[lo:hi].contiguous(), starts=s32), dict(chunks=((len(starts), T, 128), torch.float32)))
        assert torch.equal(one["chunks"].cpu(), want[k]), ("bt_split_chunks", n)
        agg = _guarded_runs("bt_aggregate", lambda p: L.check(lib.bt_aggregate(st, p["cb"], p["cd"], p["starts"], len(starts), T, border, n,
                                                                                 p["beat"], p["down"])),
                            dict(cb=cb[c0:c1].contiguous(), cd=cd[c0:c1].contiguous(), starts=s32),
                            dict(beat=((n,), torch.float32), down=((n,), torch.float32)))
        assert torch.equal(agg["beat"].cpu(), res["beat"][lo:hi].cpu()) and torch.equal(agg["down"].cpu(), res["down"][lo:hi].cpu())


def _peaks_host(x):
    L = _lib()
    x = np.ascontiguousarray(x, dtype=np.float32)
    idx = np.zeros(max(len(x), 1), np.int32)
    cnt = C.c_int32(0)
    L.check(L.lib().bt_peaks_host(x.ctypes.data, len(x), idx.ctypes.data, C.byref(cnt)))
    return idx[:cnt.value]


def test_peaks_single_and_batch_guarded_and_poisoned():
    """bt_peaks (two arrays) and bt_peaks_batch (136 ragged arrays incl. one-frame ones) against bt_peaks_host, which
    test_cabi.py holds to the oracle; index slots past a count are not defined and not compared"""
    L = _lib()
    lib, st = L.lib(), L.stream_ptr(dev())
    rng = np.random.default_rng(11)
    frames = _ragged_frames() * 2
    logits = [rng.normal(-0.5, 1.5, n).astype(np.float32) for n in frames]
    for x in logits:
        x[rng.integers(0, len(x), max(1, len(x) // 10))] = 1.25   # plateaus
    off = np.concatenate([[0], np.cumsum(frames)]).astype(np.int32)
    total = int(off[-1])
    spans = torch.tensor(np.stack([off[:-1], np.asarray(frames, np.int32)], 1), dtype=torch.int32)

    def valid(r):
        cnt = r["count"].cpu()
        return dict(count=cnt, idx=torch.cat([r["idx"][int(off[a]):int(off[a]) + int(cnt[a])].cpu() for a in range(len(frames))]))

    res = _guarded_runs("bt_peaks_batch", lambda p: L.check(lib.bt_peaks_batch(st, p["x"], p["spans"], len(frames), p["idx"], p["count"])),
                        dict(x=torch.from_numpy(np.concatenate(logits)), spans=spans),
                        dict(idx=((total,), torch.int32), count=((len(frames),), torch.int32)), valid=valid)
    want = [_peaks_host(x) for x in logits]
    assert res["count"].tolist() == [len(w) for w in want]
    assert np.array_equal(res["idx"].numpy(), np.concatenate(want))
    n = 1501
    two = np.stack([logits[4][:n], logits[4][::-1][:n]]).copy()
    res = _guarded_runs("bt_peaks", lambda p: L.check(lib.bt_peaks(st, p["x"], n, 2, p["idx"], p["count"])),
                        dict(x=torch.from_numpy(two)), dict(idx=((2, n), torch.int32), count=((2,), torch.int32)),
                        valid=lambda r: dict(count=r["count"].cpu(), idx=torch.cat([r["idx"][a, :int(r["count"][a])].cpu() for a in range(2)])))
    assert np.array_equal(res["idx"].numpy(), np.concatenate([_peaks_host(two[0]), _peaks_host(two[1])]))


@pytest.mark.parametrize("sr", [44100, 48000, 16000, 88200, 110250, 352800])
def test_resample_single_and_batch_guarded_and_poisoned(sr):
    """bt_resample and bt_resample_batch (66 ragged tracks, each in its own guarded allocation: a read past a track's end
    meets its band) against the float64 polyphase restatement test_gpu_kernels.py uses (scipy resample_poly via the oracle's
    soxr shim), relative 5e-6.  352.8 kHz (3001 taps per output, the input read from global memory) runs 24 shorter tracks.
    Some tracks start at an odd output offset: decimate_kernel then stores its outputs one by one, not as two 16-byte words."""
    import importlib.util
    import os
    from math import gcd

    from conftest import ROOT
    from beat_this_amd.inference import _resample_filter

    spec = importlib.util.spec_from_file_location("_soxr_shim", os.path.join(ROOT, "oracle", "shims", "soxr", "__init__.py"))
    shim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(shim)
    L = _lib()
    lib, st = L.lib(), L.stream_ptr(dev())
    g = gcd(sr, 22050)
    up, down = 22050 // g, sr // g
    h, half = _resample_filter(up, down, dev())
    rng = np.random.default_rng(sr)
    if sr == 352800:
        lens = [64, 65, 1000, sr // 3 + 777] + [int(v) for v in rng.integers(100, 40000, 20)]
    else:
        lens = [64, 65, 1000, sr * 3 + 777] + [int(v) for v in rng.integers(100, 20000, 62)]
    xs = [torch.from_numpy(rng.normal(0, 0.3, n).astype(np.float32)) for n in lens]
    n_out = [-(-n * up // down) for n in lens]
    refs = [torch.from_numpy(shim.resample(x.double().numpy(), sr, 22050)) for x in xs]
    assert [len(r) for r in refs] == n_out
    out_off = np.concatenate([[0], np.cumsum(n_out)])
    assert any(int(o) % 2 == 1 and n > 8 for o, n in zip(out_off[:-1], n_out))   # a track on no 16-byte boundary

    def call(p):
        tab = torch.tensor([[p[f"x{i}"], lens[i], int(out_off[i]), n_out[i]] for i in range(len(lens))], dtype=torch.int64).to(dev())
        L.check(lib.bt_resample_batch(st, tab.data_ptr(), len(lens), max(n_out), up, down, p["h"], half, p["y"]))

    res = _guarded_runs("bt_resample_batch", call, dict(h=h, **{f"x{i}": x for i, x in enumerate(xs)}),
                        dict(y=((int(out_off[-1]),), torch.float32)))["y"].cpu().double()
    for i, r in enumerate(refs):
        y = res[int(out_off[i]):int(out_off[i + 1])]
        assert float((y - r).abs().max()) <= 5e-6 * max(float(r.abs().max()), 1e-3), (i, lens[i])
    one = _guarded_runs("bt_resample", lambda p: L.check(lib.bt_resample(st, p["x"], lens[3], up, down, p["h"], half, p["y"], n_out[3])),
                        dict(x=xs[3], h=h), dict(y=((n_out[3],), torch.float32)))["y"].cpu()
    assert torch.equal(one.double(), res[int(out_off[3]):int(out_off[4])])


def test_logmel_single_and_batch_guarded_and_poisoned():
    """bt_logmel and bt_logmel_batch (66 ragged tracks, each its own guarded allocation; 2, 1488, 1489, 1500 and 1501 frames
    among them) against the oracle's float64 log-mel at test_gpu_model.py's 1e-4"""
    from beat_this_amd.preprocessing import LogMelSpect
    from oracle import beat_this_oracle as O

    L = _lib()
    lib, st = L.lib(), L.stream_ptr(dev())
    lm = LogMelSpect(device=dev())   # (owns the device tables the struct points into: kept alive for the whole test)
    tables = lm._get_tables()
    rng = np.random.default_rng(5)
    frames = [2, 1488, 1489, 1500, 1501] + [int(v) for v in rng.integers(3, 400, 61)]
    lens = [(f - 1) * 441 + int(rng.integers(0, 441)) for f in frames]
    lens[0] = 513
    xs = [torch.from_numpy((rng.normal(0, 0.1, n) + 0.3 * np.sin(np.arange(n) * 0.05)).astype(np.float32)) for n in lens]
    n_fr = [1 + n // 441 for n in lens]
    assert n_fr[:5] == frames[:5]
    f_off = np.concatenate([[0], np.cumsum(n_fr)])

    def call(p):
        tab = torch.tensor([[p[f"x{i}"], lens[i], int(f_off[i]), n_fr[i]] for i in range(len(lens))], dtype=torch.int64).to(dev())
        L.check(lib.bt_logmel_batch(st, C.byref(tables), tab.data_ptr(), len(lens), max(n_fr), p["s"]))

    res = _guarded_runs("bt_logmel_batch", call, {f"x{i}": x for i, x in enumerate(xs)},
                        dict(s=((int(f_off[-1]), 128), torch.float32)))["s"].cpu().double()
    err = 0.0
    for i, x in enumerate(xs):
        ref = O.logmel(x.double(), torch.float64)
        err = max(err, float((res[int(f_off[i]):int(f_off[i + 1])] - ref).abs().max()))
    assert err < 1e-4, err
    one = _guarded_runs("bt_logmel", lambda p: L.check(lib.bt_logmel(st, C.byref(tables), p["x"], lens[4], p["s"])),
                        dict(x=xs[4]), dict(s=((n_fr[4], 128), torch.float32)))["s"].cpu()
    assert torch.equal(one.double(), res[int(f_off[4]):int(f_off[5])])


def test_dbn_decode_and_viterbi_guarded():
    """bt_dbn_decode over 71 ragged tracks (one-frame and 1488 .. 1501-frame ones among them, and an all-silent track, a lone
    frame 0 and 100 silent leading frames: a count of 0 and a large trim offset) and bt_dbn_viterbi, against the
    host decoder bt_dbn_host / bt_dbn_viterbi_host (test_dbn.py holds those to tests/dbn_reference.py bit for bit).
    The DBN workspace is zero-filled in every run, its bands poisoned: its info, state and backpointer words are indices
    (dbn.hip ws_layout: a backpointer selects an interval of a beat and, during the backtrack, the next backpointer to read),
    and this test does not rely on every one of them being written before it is read.  The logits, span table and outputs are
    poisoned around / under their data as everywhere else; the rows past a track's count are not defined and not compared."""
    from beat_this_amd.postprocessor import Postprocessor

    L = _lib()
    lib, st = L.lib(), L.stream_ptr(dev())
    pp = Postprocessor(type="dbn")
    tables = pp._dbn_tables.ctypes.data
    d_tab = pp._dbn_device_tables(dev())
    rng = np.random.default_rng(9)
    frames = [1, 1488, 1489, 1500, 1501, 13, 14] + [int(v) for v in rng.integers(2, 900, 61)]
    quiet = {20: 300, 40: 200, 60: 400}   # position -> frames: all silent, a lone frame 0, 100 silent leading frames
    for k in sorted(quiet):
        frames.insert(k, quiet[k])
    n, total = len(frames), sum(frames)
    off = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    beat = (rng.normal(size=total) * 3 - 1).astype(np.float32)
    down = (rng.normal(size=total) * 3 - 3).astype(np.float32)
    for k, head in ((20, 300), (40, 200), (60, 100)):   # the count-0 and large-`first` writes, between ordinary tracks
        beat[off[k]:off[k] + head] = down[off[k]:off[k] + head] = -8.0
    beat[off[40]] = 8.0
    spans = np.stack([off[:-1], total + off[:-1], np.asarray(frames), off[:-1]], 1).astype(np.int32)
    wsb = lib.bt_dbn_workspace_bytes(tables, n, total)

    def valid(r):
        o = r["out"].cpu()
        return dict(counts=o[:n], rows=torch.cat([o[n + 2 * int(off[k]):n + 2 * int(off[k]) + 2 * int(o[k])] for k in range(n)]))

    res = _guarded_runs("bt_dbn_decode", lambda p: L.check(lib.bt_dbn_decode(st, tables, d_tab.data_ptr(), p["logits"], 0, p["spans"], n,
                                                                              total, p["out"], p["ws"], wsb)),
                        dict(logits=torch.from_numpy(np.concatenate([beat, down])), spans=torch.from_numpy(spans)),
                        dict(out=((n + 2 * total,), torch.int32), ws=((wsb,), torch.uint8)), scratch=("ws",), valid=valid)
    pos = 0
    for k in range(n):
        lo, hi = int(off[k]), int(off[k + 1])
        lb, ld = beat[lo:hi].astype(np.float64), down[lo:hi].astype(np.float64)
        rows = np.zeros((max(hi - lo, 1), 2), np.int32)
        cnt = C.c_int32(0)
        L.check(lib.bt_dbn_host(tables, lb.ctypes.data, ld.ctypes.data, hi - lo, rows.ctypes.data, C.byref(cnt)))
        assert (cnt.value == 0) if k in (20, 40) else (k != 60 or (cnt.value > 0 and rows[0, 0] >= 100)), (k, cnt.value)
        assert int(res["counts"][k]) == cnt.value, (k, hi - lo)
        assert np.array_equal(res["rows"][pos:pos + 2 * cnt.value].numpy(), rows[:cnt.value].reshape(-1)), (k, hi - lo)
        pos += 2 * cnt.value
    for T in (1, 1501):
        dens = np.log(rng.random((T, 3)) * 0.999 + 1e-4)
        wsv = lib.bt_dbn_workspace_bytes(tables, 1, T)
        for h in range(2):
            r = _guarded_runs("bt_dbn_viterbi", lambda p: L.check(lib.bt_dbn_viterbi(st, tables, d_tab.data_ptr(), h, p["dens"], T, p["path"],
                                                                                      p["lp"], p["ws"], wsv)),
                              dict(dens=torch.from_numpy(dens)), dict(path=((T,), torch.int32), lp=((1,), torch.float64), ws=((wsv,), torch.uint8)),
                              scratch=("ws",))
            path = np.zeros(T, np.int32)
            lp = C.c_double()
            L.check(lib.bt_dbn_viterbi_host(tables, h, dens.ctypes.data, T, path.ctypes.data, C.byref(lp)))
            assert np.array_equal(r["path"].cpu().numpy(), path) and float(r["lp"][0]) == lp.value, (T, h)


@pytest.mark.parametrize("prec", [0, 1])
def test_gemm_epilogues_guarded_and_poisoned(prec):
    """bt_gemm: STORE (RMSNorm + bias + GELU, M = 257 and 129: not tile multiples; the largest shape of test_gpu_kernels.py),
    fp32 out, RESID, QKV (RoPE + gates) and the implicit-GEMM conv, against the float64 restatements of test_gpu_kernels.py"""
    import math

    from beat_this_amd.tables import rope_table

    L = _lib()
    lib, st = L.lib(), L.stream_ptr(dev())
    dt = torch.float32 if prec == 0 else HALF()
    tol = 2e-5 if prec == 0 else 2.5e-2

    def pad(w, mult=128):
        out = torch.zeros(((w.shape[0] + mult - 1) // mult * mult, w.shape[1]), dtype=w.dtype)
        out[:w.shape[0]] = w
        return out

    def gemm(p, M, N, K, lda, epi, flags, ldo=0, ldx=0, conv=None, qkv=None):
        a = L.GemmArgs()
        a.A, a.lda, a.W, a.M, a.N, a.K, a.epi, a.flags = p["A"], lda, p["W"], M, N, K, epi, flags
        a.bias, a.out, a.ldo, a.x, a.ldx = p.get("bias", 0), p.get("out", 0), ldo, p.get("x", 0), ldx
        if conv:
            a.conv_C2, a.conv_T, a.conv_F = conv
        if qkv:
            a.gates, a.inner, a.heads, a.rope, a.pdiv, a.pmod, a.map_T, a.map_F = p["gates"], *qkv, 0, 0
            a.rope = p["rope"]
        L.check(lib.bt_gemm(st, prec, C.byref(a)))

    def rel(a, ref):
        return float((a.double().cpu() - ref).abs().max() / ref.abs().max())

    for M, K, N in ((257, 2048, 512), (129, 32, 32)):
        A, W, b = _mk((M, K), 1), _mk((N, K), 2, 1 / math.sqrt(K)), _mk((N,), 3)
        Wd = pad(W.float()).to(dt)
        ref = torch.nn.functional.gelu(A / A.norm(dim=-1, keepdim=True) * math.sqrt(K) @ W.T + b)
        out = _guarded_runs("bt_gemm STORE", lambda p: gemm(p, M, N, K, K, L.GEMM_EPI_STORE, L.GEMM_F_RMS | L.GEMM_F_A_F32 | L.GEMM_F_BIAS | L.GEMM_F_GELU, ldo=N),
                            dict(A=A.float(), W=Wd, bias=b.float()), dict(out=((M, N), dt)))["out"]
        assert rel(out, ref) < tol, (M, K, N)
        out = _guarded_runs("bt_gemm STORE f32", lambda p: gemm(p, M, N, K, K, L.GEMM_EPI_STORE, L.GEMM_F_A_F32 | L.GEMM_F_BIAS | L.GEMM_F_OUT_F32, ldo=N),
                            dict(A=A.float(), W=Wd, bias=b.float()), dict(out=((M, N), torch.float32)))["out"]
        assert rel(out, A @ W.T + b) < tol, (M, K, N)
    M, K, N = 515, 128, 64
    A, W, b, x0 = _mk((M, K), 4), _mk((N, K), 5, 0.1), _mk((N,), 6), _mk((M, N), 7)
    Wd, Ad = pad(W.float()).to(dt), A.float().to(dt)
    # (x is read and written: its own loop, the other operands poisoned around their data as in _guarded_runs)
    runs = []
    for p in (0x00,) + POISONS:
        gA, gW, gb = (Guarded(t.shape, t.dtype).fill(p, t.to(dev())) for t in (Ad, Wd, b.float()))
        gx = Guarded((M, N), torch.float32).fill(p, x0.float().to(dev()))
        gemm(dict(A=gA.ptr(), W=gW.ptr(), bias=gb.ptr(), x=gx.ptr()), M, N, K, K, L.GEMM_EPI_RESID, L.GEMM_F_BIAS, ldx=N)
        torch.cuda.synchronize()
        assert_intact(("bt_gemm RESID A", gA), ("W", gW), ("bias", gb), ("x", gx))
        runs.append(gx.t.clone())
    assert all(_same(r, runs[0]) for r in runs[1:])
    assert rel(runs[0], x0 + Ad.double() @ Wd[:N].double().T + b) < (2e-5 if prec == 0 else 4e-3)
    # QKV epilogue, main-layer form (RMSNorm + RoPE + gates), 74 rows
    heads, Cc, M = 2, 64, 74
    A = _mk((M, Cc), 10)
    Wqkv, Wg, bg = _mk((3 * Cc, Cc), 11, 1 / math.sqrt(Cc)), _mk((heads, Cc), 12, 0.2), _mk((heads,), 13)
    freqs = 10000.0 ** (-torch.arange(0, 32, 2).float() / 32)
    rope = torch.from_numpy(rope_table(freqs))
    res = _guarded_runs("bt_gemm QKV", lambda p: gemm(p, M, 3 * Cc + heads, Cc, Cc, L.GEMM_EPI_QKV, L.GEMM_F_RMS | L.GEMM_F_A_F32, ldo=3 * Cc,
                                                       qkv=(Cc, heads, 0, 1, 37)),
                        dict(A=A.float(), W=pad(torch.cat([Wqkv, Wg]).float()).to(dt), bias=bg.float(), rope=rope.float()),
                        dict(out=((M, 3 * Cc), dt), gates=((M, heads), torch.float32)))
    xn = A / A.norm(dim=-1, keepdim=True) * math.sqrt(Cc)
    qkv_ref = xn @ Wqkv.T
    ang = (torch.arange(M) % 37)[:, None].double() * freqs[None, :].double()
    cos, sin = ang.cos().repeat_interleave(2, -1)[:, None], ang.sin().repeat_interleave(2, -1)[:, None]

    def rope_cols(block):
        t = block.reshape(M, heads, 32)
        rot = torch.stack((-t[..., 1::2], t[..., 0::2]), -1).flatten(-2)
        return (t * cos + rot * sin).reshape(M, Cc)

    ref = torch.cat([rope_cols(qkv_ref[:, :Cc]), rope_cols(qkv_ref[:, Cc:2 * Cc]), qkv_ref[:, 2 * Cc:]], 1)
    assert rel(res["out"], ref) < tol
    assert rel(res["gates"], torch.sigmoid(xn @ Wg.T + bg)) < tol
    # implicit-GEMM conv, Cin = 64
    Bc, Tc, Fc, Cin = 2, 21, 8, 64
    xc, w, bias = _mk((Bc, Cin, Fc, Tc), 20), _mk((2 * Cin, Cin, 2, 3), 21, 0.1), _mk((2 * Cin,), 22)
    ref = torch.nn.functional.gelu(torch.nn.functional.conv2d(xc, w, stride=(2, 1), padding=(0, 1)) + bias[None, :, None, None])
    ref = ref.permute(0, 3, 2, 1).reshape(Bc * Tc * (Fc // 2), 2 * Cin)
    Mc = Bc * Tc * (Fc // 2)
    out = _guarded_runs("bt_gemm conv", lambda p: gemm(p, Mc, 2 * Cin, 6 * Cin, Cin, L.GEMM_EPI_STORE,
                                                        L.GEMM_F_CONV | L.GEMM_F_A_F32 | L.GEMM_F_BIAS | L.GEMM_F_GELU | L.GEMM_F_OUT_F32,
                                                        ldo=2 * Cin, conv=(2 * Cin, Tc, Fc // 2)),
                        dict(A=xc.permute(0, 3, 2, 1).contiguous().float().view(-1, Cin),
                             W=pad(w.permute(0, 3, 2, 1).reshape(2 * Cin, 6 * Cin).float()).to(dt), bias=bias.float()),
                        dict(out=((Mc, 2 * Cin), torch.float32)))["out"]
    assert rel(out, ref) < tol


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("n_seq,L_,heads", [(2, 77, 1), (3, 1500, 2)])
def test_attention_guarded_and_poisoned(prec, n_seq, L_, heads):
    """bt_attention (L = 77: not a multiple of 32; 3 x 1500: the largest shape of test_gpu_kernels.py) against the float64
    softmax restatement"""
    import math

    Lb = _lib()
    lib, st = Lb.lib(), Lb.stream_ptr(dev())
    dt = torch.float32 if prec == 0 else HALF()
    Cc = heads * 32
    qkv = _mk((n_seq * L_, 3 * Cc), 30)
    qkv[:, :Cc] *= 0.6
    gates = torch.sigmoid(_mk((n_seq * L_, heads), 31))
    qd = qkv.float().to(dt)

    def call(p):
        a = Lb.AttnArgs()
        a.qkv, a.ld, a.gates, a.out = p["qkv"], 3 * Cc, p["gates"], p["out"]
        a.n_seq, a.L, a.heads, a.inner, a.o_div, a.o_outer, a.o_inner, a.o_tok = n_seq, L_, heads, Cc, 1, L_, 0, 1
        Lb.check(lib.bt_attention(st, prec, C.byref(a)))

    out = _guarded_runs("bt_attention", call, dict(qkv=qd, gates=gates.float()), dict(out=((n_seq * L_, Cc), dt)))["out"]
    qq = qd.double()

    def split(i):
        return qq[:, i * Cc:(i + 1) * Cc].reshape(n_seq, L_, heads, 32).permute(0, 2, 1, 3)

    s = split(0) @ split(1).transpose(-1, -2) * math.log(2.0)
    ref = (torch.softmax(s, -1) @ split(2) * gates.reshape(n_seq, L_, heads).permute(0, 2, 1)[..., None])
    ref = ref.permute(0, 2, 1, 3).reshape(n_seq * L_, Cc)
    err = float((out.double().cpu() - ref).abs().max() / ref.abs().max())
    assert err < (2e-5 if prec == 0 else 2e-2), err
