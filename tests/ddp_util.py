"""What the tests of the rank-ordered gradient sum share (test_ddp_reference, test_gpu_ddp): the data and the numpy sum"""
import numpy as np


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def spread_parts(world, n, stride, seed):
    """``world`` parts whose magnitudes spread over about 2^30, so that the order of the adds shows in the low bits; the gaps
    between the parts (stride > n) hold a value that would show in any sum that read them"""
    rng = np.random.default_rng(seed)
    flat = np.full((world - 1) * stride + n, 7.0e37, np.float32)
    for r in range(world):
        mant = rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n)
        flat[r * stride:r * stride + n] = (mant * np.exp2(rng.integers(-15, 16, n))).astype(np.float32)
    return flat


def sequential_sum(flat, world, n, stride, order=None):
    """((p[o0] + p[o1]) + p[o2]) + ... with one rounded np.float32 add at a time"""
    order = list(range(world)) if order is None else order
    acc = flat[order[0] * stride:order[0] * stride + n].copy()
    for r in order[1:]:
        acc = (acc + flat[r * stride:r * stride + n]).astype(np.float32)
    return acc
