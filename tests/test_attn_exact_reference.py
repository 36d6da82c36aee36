"""tests/attn_exact_reference.py without a GPU: on every case tests/test_gpu_attn_exact.py hands to the device the three emulations of
the kernels' orders of operation reproduce the fp64 expectation bit for bit, in every format the arithmetic is stored in -- so a
device mismatch is a kernel error, not a property of the inputs -- and the five mutants miss it exactly where claims() says.

What the mutant table shows, and what it does not: a counted padding slot or a dropped background key moves a row of the uniform or
graded family by one part in L (or in the graded row sum T); in a half-type row that rounds away once L passes 2^(p - 4) .. 2^p.
Such a mutant is killed at short L with the same L mod 32 and at long L through the fp32 / hl32 rows; the selection family cannot
see a counted padding slot at all (its probability is 0) but names every dropped, swapped or wrongly rescaled key."""
import numpy as np
import pytest

import attn_exact_reference as R

# the cases the mutants run on: every short one, and one of 1500-frame length per family
MUTANT_CASES = [c for c in R.all_cases() if c.L <= 272] + [R.make("selection", 1, 1499, 1), R.make("graded", 37, 91, 1493), R.make("uniform", 1500)]


def _rounded(x, fmt, half):
    return R.round_out(x, fmt, half)


@pytest.mark.parametrize("family", ["selection", "graded", "uniform"])
def test_every_emulation_reproduces_the_expectation(family):
    for case in (c for c in R.all_cases() if c.family == family):
        for name, emu in R.EMULATIONS.items():
            out, rerun = emu(case)
            for fmt, half in R.STORED[name]:
                got, want = _rounded(out, fmt, half), _rounded(case.want, fmt, half)
                assert R.same(got, want), case.describe(f"{name} as {fmt} ({half})", got, want, {"online": None, "p16": "x3"}.get(name, "half"))
            # the route the generator records is the route the emulation took
            if name == "p16":
                assert np.array_equal(~rerun, case.fast_x3), case.id
            elif name != "online":
                S, H, L = case.fast_half.shape
                own = ~case.fast_half
                group = np.stack([own[:, :, g:g + 128].any(-1) for g in range(0, L, 128)], -1).repeat(128, -1)[:, :, :L]
                assert np.array_equal(rerun, group), case.id


def test_the_cases_reach_every_key_position_and_both_routes():
    sole = np.zeros(1500, dtype=bool)
    routes = {"half": set(), "x3": set()}
    for case in (c for c in R.all_cases() if c.family == "selection"):
        size = case.sel.sum(-1, keepdims=True)
        hit = (case.sel & (size == 1)).any(axis=(0, 1, 2))           # key positions that are some query's sole selected key
        sole[:case.L] |= hit
        assert hit[case.L - 1] and hit[32 * ((case.L - 1) // 32)], case.id   # the last real key, the first key of the last block
        routes["half"] |= set(np.unique(case.fast_half).tolist())
        routes["x3"] |= set(np.unique(case.fast_x3).tolist())
        if case.L > 64:   # past the reference blocks both routes occur within one case
            assert not case.fast_half.all() and case.fast_half.any() and not case.fast_x3.all() and case.fast_x3.any(), case.id
    assert sole.all() and routes == {"half": {False, True}, "x3": {False, True}}
    big = R.make("selection", 2, 1500, 2)
    assert (big.sel[0, 0].sum(-1) == 1).all() and big.sel[0, 0].any(0).all()   # its first pair: every key alone, every key selected
    gates = np.concatenate([c.gates.reshape(-1) for c in R.all_cases()])
    assert set(np.unique(gates).tolist()) == {0.25, 0.5, 1.0}
    two = R.make("selection", 1, 128, 2)
    assert (two.gates[:, 0] != two.gates[:, 1]).all()


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_the_mutants_miss_where_the_table_says(mutant):
    killed = {}
    for name in R.APPLIES[mutant]:
        if name == "online" and mutant != "skip_the_rescale":
            continue   # (the other four change the inputs of an emulation: (b) and (c) stand for them)
        for case in MUTANT_CASES:
            out, _ = R.EMULATIONS[name](case, mutant)
            for fmt, half in R.STORED[name]:
                caught = not R.same(_rounded(out, fmt, half), _rounded(case.want, fmt, half))
                claim = R.claims(mutant, name, case, fmt, half)
                assert claim is None or claim == caught, (mutant, name, fmt, half, case.id, "claimed", claim, "caught", caught)
                if claim:
                    killed.setdefault((name, fmt, half), []).append(case.id)
    # every arithmetic x format the GPU test runs has at least one case that kills the mutant, and a 1500-frame one where the
    # format is wide enough
    for name in R.APPLIES[mutant]:
        if name == "online" and mutant != "skip_the_rescale":
            continue
        for fmt, half in R.STORED[name]:
            ids = killed.get((name, fmt, half), [])
            assert ids, (mutant, name, fmt, half)
            if fmt in ("f32", "hl32"):
                assert any(("x1499x" in i) or ("x1493x" in i) or ("x1500x" in i) for i in ids), (mutant, name, fmt, ids)


def test_unknown_mutant_is_refused():
    with pytest.raises(ValueError):
        R.emulate_p16(R.make("uniform", 33), "no_such_mutant")
