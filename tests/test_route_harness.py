"""The comparisons the training route's GPU tests share (tests/route_harness.py), on CPU tensors: what ``same_bits`` tells apart
and what ``both_poisons`` refuses."""
import struct

import pytest
import torch

from gpu_util import POISONS
from route_harness import both_poisons, same_bits

POISON_WORD = struct.unpack("<f", bytes([POISONS[1]] * 4))[0]       # 0x7B7B7B7B as an fp32 value: large and finite


def nan(payload):
    """an fp32 quiet NaN with the given mantissa bits"""
    return torch.tensor([0x7FC00000 | payload], dtype=torch.int32).view(torch.float32)


def test_same_bits_tells_the_zeros_apart():
    plus, minus = torch.tensor([0.0, 1.0]), torch.tensor([-0.0, 1.0])
    assert torch.equal(plus, minus) and not same_bits(plus, minus)
    assert same_bits(plus, plus.clone()) and same_bits(minus, minus.clone())


def test_same_bits_compares_the_dtype():
    a = torch.tensor([1.0, -2.5, 3.0e-5, 7.0])
    for other in (torch.int32, torch.uint8, torch.float16):
        b = a.view(other)
        assert bytes(a.view(torch.uint8).tolist()) == bytes(b.reshape(-1).view(torch.uint8).tolist())
        assert not same_bits(a, b) and not same_bits(b, a)
    assert not same_bits(torch.zeros(4, dtype=torch.float32), torch.zeros(4, dtype=torch.int32))


def test_same_bits_compares_the_shape():
    a = torch.arange(6.0)
    assert not same_bits(a, a.view(2, 3)) and not same_bits(a.view(2, 3), a.view(3, 2)) and not same_bits(a, a[:5])
    assert same_bits(a.view(2, 3), a.clone().view(2, 3))
    assert same_bits(a.view(2, 3).t(), a.view(2, 3).t().contiguous())           # the values, not the strides
    assert same_bits(torch.tensor(1.5), torch.tensor(1.5)) and not same_bits(torch.tensor(1.5), torch.tensor([1.5]))
    assert same_bits(torch.empty(0), torch.empty(0)) and not same_bits(torch.empty(0), torch.empty(0, dtype=torch.int64))


def test_same_bits_tells_nan_payloads_apart():
    a, b = nan(1), nan(2)
    assert a.isnan().all() and b.isnan().all()
    assert same_bits(a, a.clone()) and not same_bits(a, b)
    assert not torch.equal(a, a.clone())                                          # (what a value comparison makes of a NaN)


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32, torch.uint8, torch.bool, torch.float64, torch.float16, torch.bfloat16])
def test_same_bits_takes_any_dtype(dtype):
    a = torch.tensor([0, 1, 1, 0, 1, 1, 1]).to(dtype)                             # (7 elements: no multiple of a 32-bit word)
    b = a.clone()
    assert same_bits(a, b)
    b[3] = 1
    assert not same_bits(a, b)


def result(poison=None, **changes):
    """a result as a guarded run returns it: float tensors and an int64 counter"""
    res = {"y": torch.arange(12.0).view(3, 4), "g": torch.tensor([0.5, -0.25]), "tracked": torch.tensor([4], dtype=torch.int64)}
    res.update(changes)
    return res


def test_both_poisons_returns_the_first_of_two_equal_runs():
    seen = []

    def run(poison):
        seen.append(poison)
        return result()
    got = both_poisons("clean", run)
    assert seen == list(POISONS) and set(got) == {"y", "g", "tracked"} and same_bits(got["y"], result()["y"])


def test_both_poisons_compares_integers_exactly_and_exempts_them_from_the_poison_checks():
    word = int.from_bytes(bytes([POISONS[1]] * 4), "little")
    # an integer tensor may hold the poison word's value, and -1 (all 0xFF bytes): both are values a counter can have
    for value in (word, -1):
        both_poisons("integers", lambda p: result(tracked=torch.tensor([value, value], dtype=torch.int32)))
    both_poisons("int64", lambda p: result(tracked=torch.tensor([word | (word << 32)], dtype=torch.int64)))
    with pytest.raises(AssertionError, match="tracked differs between two runs"):
        both_poisons("integers", lambda p: result(tracked=torch.tensor([4 + (p == POISONS[1])], dtype=torch.int64)))


def test_both_poisons_refuses_one_poison_word():
    y = torch.arange(12.0).view(3, 4)
    y[1, 2] = POISON_WORD
    assert torch.isfinite(y).all()
    with pytest.raises(AssertionError, match="y keeps words of the 0x7B poison"):
        both_poisons("poisoned", lambda p: result(y=y.clone()))
    # the second run is the one filled with 0x7B: a word of it in the first run alone is a difference between the runs
    with pytest.raises(AssertionError, match="y differs between two runs"):
        both_poisons("poisoned", lambda p: result(y=y.clone()) if p == POISONS[0] else result())


def test_both_poisons_refuses_one_nan():
    g = torch.tensor([0.5, float("nan")])
    with pytest.raises(AssertionError, match="g keeps bytes of the 0xFF poison"):
        both_poisons("nan", lambda p: result(g=g.clone()))
    with pytest.raises(AssertionError, match="g keeps bytes of the 0xFF poison"):
        both_poisons("inf", lambda p: result(g=torch.tensor([0.5, float("inf")])))
    with pytest.raises(AssertionError, match="g keeps bytes of the 0xFF poison"):
        both_poisons("0xFF", lambda p: result(g=torch.full((2,), -1, dtype=torch.int32).view(torch.float32)))


def test_both_poisons_refuses_runs_that_differ():
    with pytest.raises(AssertionError, match="g differs between two runs"):
        both_poisons("differs", lambda p: result(g=torch.tensor([0.5, -0.25 if p == POISONS[0] else -0.250001])))
    with pytest.raises(AssertionError, match="g differs between two runs"):      # the sign of a zero is a difference
        both_poisons("zeros", lambda p: result(g=torch.tensor([0.5, 0.0 if p == POISONS[0] else -0.0])))
    with pytest.raises(AssertionError, match="different tensors"):
        both_poisons("keys", lambda p: result() if p == POISONS[0] else {"y": result()["y"]})


def test_both_poisons_takes_a_tuple_of_dicts():
    stats = lambda: {"running_mean": torch.tensor([1.0, 2.0]), "num_batches_tracked": torch.tensor([4], dtype=torch.int64)}
    got = both_poisons("tuple", lambda p: (result(), stats()))
    assert isinstance(got, tuple) and len(got) == 2 and set(got[1]) == {"running_mean", "num_batches_tracked"}
    bad = stats()
    bad["running_mean"][1] = POISON_WORD
    with pytest.raises(AssertionError, match="running_mean keeps words of the 0x7B poison"):
        both_poisons("tuple", lambda p: (result(), {k: v.clone() for k, v in bad.items()}))
    with pytest.raises(AssertionError, match="running_mean differs between two runs"):
        both_poisons("tuple", lambda p: (result(), stats() if p == POISONS[0] else {k: v + 1 for k, v in stats().items()}))
    with pytest.raises(AssertionError, match="y keeps bytes of the 0xFF poison"):
        both_poisons("tuple", lambda p: (result(y=torch.full((3, 4), float("nan"))), stats()))
