"""The CPU oracle (oracle/beat_this_oracle.py) against the committed golden outputs of
the reference (tests/golden, made by oracle/make_golden*.py from the unmodified reference)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from beat_this_amd import weights as W
from oracle import beat_this_oracle as O
from oracle.cases import MODEL_CASES, POSTP_CASES


def test_split_piece_table():
    table = json.load(open(os.path.join(GOLDEN, "split_piece.json")))
    for n, row in table.items():
        n = int(n)
        starts = O.split_starts(n)
        assert [int(s) for s in starts] == row["starts"], n
        chunks, _ = O.split_chunks(torch.zeros(n, 2))
        assert [int(c.shape[0]) for c in chunks] == row["lens"], n
    # the surprises of SURVEY.md section 0 item 1
    assert table["1500"]["starts"] == [-6, 6] and table["1488"]["starts"] == [-6]
    assert len(table["15001"]["starts"]) == 11 and table["1000"]["lens"] == [1012]


def test_postprocessor_edge_cases():
    post = json.load(open(os.path.join(GOLDEN, "postp_minimal.json")))
    for name, (bs, ds) in POSTP_CASES.items():
        b = torch.full((100,), -5.0)
        d = torch.full((100,), -5.0)
        for f, v in bs:
            b[f] = v
        for f, v in ds:
            d[f] = v
        bt, dt = O.postp_minimal(b, d)
        assert bt.tolist() == post[name]["beats"], name
        assert dt.tolist() == post[name]["downbeats"], name
    rng = np.random.default_rng(post["random3000"]["seed"])
    rb = torch.from_numpy(rng.normal(-1.0, 1.5, 3000).astype(np.float32))
    rd = torch.from_numpy(rng.normal(-2.0, 1.5, 3000).astype(np.float32))
    bt, dt = O.postp_minimal(rb, rd)
    assert bt.tolist() == post["random3000"]["beats"]
    assert dt.tolist() == post["random3000"]["downbeats"]
    # the plateau quirk
    assert post["plateau3"]["beats"] == [10.5 / 50, 12 / 50]


def test_logmel_golden():
    g = np.load(os.path.join(GOLDEN, "logmel.npz"))
    s2 = O.logmel(torch.from_numpy(W.synthetic_audio(2.0, seed=11))).numpy()
    assert s2.shape == g["s2"].shape == (101, 128)
    assert np.abs(s2 - g["s2"]).max() < 2e-5
    s30 = O.logmel(torch.from_numpy(W.synthetic_audio(30.0, seed=12))).numpy()
    assert tuple(g["s30_shape"]) == s30.shape == (1501, 128)
    assert np.abs(s30[g["s30_rows"]] - g["s30_sel"]).max() < 2e-5
    tone = (0.5 * np.sin(2 * np.pi * 440.0 * np.arange(22050 * 3) / 22050.0)).astype(np.float32)
    st = O.logmel(torch.from_numpy(tone)).numpy()
    # pure tone: empty bands amplify fp32 FFT noise by 1000 -> looser bound there
    assert np.abs(st[g["tone_rows"]] - g["tone_sel"]).max() < 5e-4
    # fp64 evaluation agrees with the fp32 reference output
    s2d = O.logmel(torch.from_numpy(W.synthetic_audio(2.0, seed=11)), torch.float64).numpy()
    assert np.abs(s2d - g["s2"]).max() < 2e-5


def test_mel_filterbank_structure():
    fb = O.mel_filterbank()
    assert fb.shape == (513, 128)
    assert int((fb > 0).sum()) == 1004
    nz = (fb > 0).sum(0)
    assert int(nz.min()) == 2 and int(nz.max()) == 26


@pytest.mark.parametrize("case", [c for c in MODEL_CASES if c[1] == "small0"] + [MODEL_CASES[4]])
def test_model_forward_golden(case):
    name, hpn, wseed, style, T, iseed = case
    g = np.load(os.path.join(GOLDEN, "model_logits.npz"))
    sd = W.random_state_dict(hpn, seed=wseed, style=style)
    x = torch.from_numpy(W.synthetic_spect(T, seed=iseed))[None]
    with torch.inference_mode():
        b, d = O.model_forward(sd, x)
    assert np.abs(b[0].numpy() - g[name + "_beat"]).max() < 5e-5
    assert np.abs(d[0].numpy() - g[name + "_downbeat"]).max() < 5e-5


def test_model_batched_and_piece_golden():
    g = np.load(os.path.join(GOLDEN, "model_logits.npz"))
    sd = W.random_state_dict("small0", seed=1, style="lively")
    xb = torch.from_numpy(np.stack([W.synthetic_spect(1500, seed=20 + i) for i in range(3)]))
    with torch.inference_mode():
        b, d = O.model_forward(sd, xb)
        assert np.abs(b.numpy() - g["small0_lively_B3_beat"]).max() < 5e-5
        assert np.abs(d.numpy() - g["small0_lively_B3_downbeat"]).max() < 5e-5
        piece = torch.from_numpy(W.synthetic_spect(3100, seed=30))
        pb, pd = O.spect2frames(sd, piece)
    assert pb.shape == (3100,)
    assert np.abs(pb.numpy() - g["small0_lively_piece3100_beat"]).max() < 5e-5
    assert np.abs(pd.numpy() - g["small0_lively_piece3100_downbeat"]).max() < 5e-5


def test_end_to_end_golden():
    g = np.load(os.path.join(GOLDEN, "e2e_small0.npz"))
    sd = W.random_state_dict("small0", seed=1, style="lively")
    sig = W.synthetic_audio(40.0, seed=13)
    with torch.inference_mode():
        spect = O.logmel(torch.from_numpy(sig))
        bl, dl = O.spect2frames(sd, spect)
        assert np.abs(bl.numpy() - g["beat_logits"]).max() < 1e-4
        # identical logits -> identical beat lists, bit for bit
        bt, dt = O.postp_minimal(torch.from_numpy(g["beat_logits"]), torch.from_numpy(g["downbeat_logits"]))
    assert np.array_equal(bt, g["beats"]) and np.array_equal(dt, g["downbeats"])
    bt2, dt2 = O.postp_minimal(bl, dl)
    assert np.array_equal(bt2, g["beats"]) and np.array_equal(dt2, g["downbeats"])


def test_final0_piece_e2e_and_outlier_goldens():
    """The oracle against the reference's own final0 outputs at piece and end-to-end level, and on the trained-like "outlier"
    weight style (oracle/make_golden_final0.py)."""
    from oracle.cases import FINAL0_CASES as C

    g = np.load(os.path.join(GOLDEN, "final0_piece_e2e.npz"))
    with torch.inference_mode():
        sd = W.random_state_dict("final0", seed=C["piece"]["weight_seed"], style=C["piece"]["style"])
        pb, pd = O.spect2frames(sd, torch.from_numpy(W.synthetic_spect(C["piece"]["frames"], seed=C["piece"]["input_seed"])))
        assert pb.shape == (3100,)
        assert np.abs(pb.numpy() - g["piece_beat"]).max() < 5e-5 and np.abs(pd.numpy() - g["piece_downbeat"]).max() < 5e-5
        sd = W.random_state_dict("final0", seed=C["e2e"]["weight_seed"], style=C["e2e"]["style"])
        spect = O.logmel(torch.from_numpy(W.synthetic_audio(C["e2e"]["seconds"], seed=C["e2e"]["audio_seed"])))
        bl, dl = O.spect2frames(sd, spect)
        assert np.abs(bl.numpy() - g["e2e_beat_logits"]).max() < 1e-4 and np.abs(dl.numpy() - g["e2e_downbeat_logits"]).max() < 1e-4
        bt, dt = O.postp_minimal(bl, dl)
        assert np.array_equal(bt, g["e2e_beats"]) and np.array_equal(dt, g["e2e_downbeats"])
        sd = W.random_state_dict("final0", seed=C["outlier"]["weight_seed"], style="outlier")
        x = torch.from_numpy(W.synthetic_spect(C["outlier"]["frames"], seed=C["outlier"]["input_seed"]))[None]
        ob, od = O.model_forward(sd, x)
        assert np.abs(ob[0].numpy() - g["outlier_beat"]).max() < 1e-4 and np.abs(od[0].numpy() - g["outlier_downbeat"]).max() < 1e-4


def test_state_dict_layout():
    sd = W.random_state_dict("final0", seed=0)
    assert len(sd) == 166
    def count(d):  # nn.Module.parameters() sees the shared rotary ``freqs`` once
        return 16 + sum(v.numel() for k, v in d.items()
                        if v.dtype == torch.float32 and "running_" not in k and "freqs" not in k)
    assert count(sd) == 20_251_712
    sds = W.random_state_dict("small0", seed=0)
    assert count(sds) == 2_099_960
    fr = sd["transformer_blocks.layers.0.0.rotary_embed.freqs"]
    assert torch.allclose(fr, 10000.0 ** (-torch.arange(0, 32, 2).float() / 32))


def test_oracle_against_live_reference():
    """The oracle against the reference package's own outputs on the same seeded inputs (tests/golden/reference_live.npz,
    made by oracle/make_golden_live.py from the unmodified reference): BeatThis.forward on a short chunk, the state-dict key
    order of the reference's module, and LogMelSpect."""
    from oracle.cases import LIVE_CASES as C

    g = np.load(os.path.join(GOLDEN, "reference_live.npz"))
    c = C["forward"]
    sd = W.random_state_dict(c["hparams"], seed=c["weight_seed"], style=c["style"])
    assert list(sd.keys()) == g["state_dict_keys"].tolist()
    x = torch.from_numpy(W.synthetic_spect(c["frames"], seed=c["input_seed"]))[None]
    with torch.inference_mode():
        b, d = O.model_forward(sd, x)
    assert np.abs(b.numpy() - g["forward_beat"]).max() < 5e-5 and np.abs(d.numpy() - g["forward_downbeat"]).max() < 5e-5
    c = C["logmel"]
    a = torch.from_numpy(W.synthetic_audio(c["seconds"], seed=c["audio_seed"]))
    assert np.abs(O.logmel(a).numpy() - g["logmel"]).max() < 2e-5


def test_oracle_port_computes_what_the_live_reference_computes():
    """bench.py's cpu_baseline times the oracle ("kind": "port"): the number is only honest if the port is the code it stands
    in for.  ASSERTED here: the numerical difference on the small model, on the 1500-frame chunk that tools/port_speed.py
    times, against the reference's own output (tests/golden/reference_live.npz, oracle/make_golden_live.py).  The
    port-vs-reference time ratio is tools/port_speed.py's measurement (profiles/r06_port_vs_reference.json; round 4's port
    was 1.38 x slower per chunk because x @ W.T on non-contiguous 3-D inputs took torch's batched route where the
    reference's nn.Linear folds); it needs the reference itself and is not part of the suite."""
    from oracle.cases import LIVE_CASES as C

    g = np.load(os.path.join(GOLDEN, "reference_live.npz"))
    c = C["port_chunk"]
    sd = W.random_state_dict(W.resolve_hparams(c["hparams"]), seed=c["weight_seed"], style=c["style"])
    x = torch.from_numpy(W.synthetic_spect(c["frames"], seed=c["input_seed"]))[None]
    with torch.inference_mode():
        b, d = O.model_forward(sd, x)
    err = max(np.abs(b.numpy() - g["port_chunk_beat"]).max(), np.abs(d.numpy() - g["port_chunk_downbeat"]).max())
    assert err < 5e-5, err


def test_third_party_leaves_against_independent_implementations():
    """rotary-embedding-torch, torchaudio and soxr are absent here, so the oracle restates their published algorithms
    ("parity unpinned" at those three leaves).  Two of them can at least be held against INDEPENDENT implementations of the same
    published conventions that this image does carry (transformers 5.x) -- a shared misreading of the convention (pair
    interleaving, frequency order, sign of the rotation; slaney break point, triangle normalisation) would show as O(1), not
    as the last-digit differences of two fp32 evaluations:
      * RoPE: GPT-J's rotate_every_two / apply_rotary_pos_emb -- the interleaved-pair convention of the RoFormer paper that
        rotary-embedding-torch implements (angle(p, 2j) = angle(p, 2j + 1) = p * 10000^(-2j/d));
      * mel filterbank: transformers.audio_utils.mel_filter_bank(norm=None, mel_scale="slaney") on the same 513 bins."""
    transformers = pytest.importorskip("transformers")
    from transformers.audio_utils import mel_filter_bank
    from transformers.models.gptj import modeling_gptj as G

    b, h, n, d = 2, 3, 1500, 32
    t = torch.randn((b, h, n, d), generator=torch.Generator().manual_seed(3))
    freqs = 10000.0 ** (-torch.arange(0, d, 2).float() / d)        # (what the reference stores as rotary_embed.freqs)
    mine = O.rope(t, freqs)
    sc = G.create_sinusoidal_positions(n, d)                         # [n, d] = sin | cos of p * inv_freq
    sin, cos = sc[None, :, : d // 2].expand(b, -1, -1), sc[None, :, d // 2:].expand(b, -1, -1)
    theirs = G.apply_rotary_pos_emb(t.permute(0, 2, 1, 3), sin, cos).permute(0, 2, 1, 3)
    assert float((mine - theirs).abs().max()) < 2e-4                 # (fp32 angles at position 1500: 1e-4 rad apart)
    assert float((mine - t).abs().max()) > 1.0                       # (... and the rotation is not the identity)
    fb = mel_filter_bank(num_frequency_bins=513, num_mel_filters=128, min_frequency=30.0, max_frequency=11000.0,
                         sampling_rate=22050, norm=None, mel_scale="slaney", triangularize_in_mel_space=False)
    assert float(np.abs(fb - O.mel_filterbank().numpy()).max()) < 5e-5
    assert transformers.__version__
