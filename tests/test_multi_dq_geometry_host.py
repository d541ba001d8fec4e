"""The multi-tensor differentiable-quantization path takes every geometry the per-tensor functions take: no buckets
(bucket_size=None, `bucket == 0` at the C ABI), buckets that are no power of two, and up to 256 points per tensor.  Here
what needs no GPU: the host plan and the constructor's validation."""
import ctypes

import pytest
import torch

from quantized_distillation_amd import _lib
from quantized_distillation_amd import build as qb


@pytest.fixture(scope='module')
def lib():
    qb.build_extension()
    return _lib.load()


def plan(lib, ns, bucket):
    T = (_lib.QdDiffQuantDesc * len(ns))()
    for i, n in enumerate(ns):
        T[i].n = n
    blocks = ctypes.c_int64(0)
    tiles = lib.qd_multi_dq_plan(T, len(ns), bucket, ctypes.byref(blocks))
    return (tiles, blocks.value, [T[i].first_tile for i in range(len(ns))], [T[i].first_block for i in range(len(ns))],
            [T[i].first_row for i in range(len(ns))])


def prefix(counts):
    out, total = [], 0
    for c in counts:
        out.append(total)
        total += c
    return out, total


@pytest.mark.parametrize('ns', [[800000, 10, 0, 1025, 5000], [0, 0]])
def test_plan_without_buckets_tiles_by_1024_elements(lib, ns):
    """bucket == 0: first_tile is the prefix of ceil(n / 1024) forward tiles (an empty tensor has none); the backward fields
    are those of any other bucket, they do not depend on it."""
    tiles, rows, ft, fb, fr = plan(lib, ns, 0)
    want_ft, want_tiles = prefix([-(-n // 1024) for n in ns])
    assert ft == want_ft and tiles == want_tiles
    if ns[0] == 800000:
        assert ft == [0, 782, 783, 783, 785] and tiles == 790
    _, rows256, _, fb256, fr256 = plan(lib, ns, 256)
    assert (rows, fb, fr) == (rows256, fb256, fr256)
    assert fb == prefix([n // 1024 for n in ns])[0]


def test_plan_with_a_bucket_that_is_no_power_of_two_tiles_by_four_buckets(lib):
    ns = [800000, 10, 0, 1025, 5000]
    tiles, rows, ft, fb, fr = plan(lib, ns, 100)
    nb = [-(-n // min(n, 100)) if n else 0 for n in ns]               # 8000, 1, 0, 11, 50 buckets
    assert nb == [8000, 1, 0, 11, 50]
    want_ft, want_tiles = prefix([-(-b // 4) for b in nb])
    assert ft == want_ft == [0, 2000, 2001, 2001, 2004] and tiles == want_tiles == 2017
    _, rows256, _, fb256, fr256 = plan(lib, ns, 256)
    assert (rows, fb, fr) == (rows256, fb256, fr256)
    assert plan(lib, ns, -1)[0] == -1                                  # still refused


def test_constructor_validation_of_the_geometry():
    """bool, zero, negative and non-int bucket sizes and point counts outside 1 ... 256 raise ValueError before anything else;
    None / 100 with 256 points get past that to the device check (CPU tensors: no launch)."""
    from quantized_distillation_amd.multi_tensor import MultiTensorDiffQuant
    ts = [torch.zeros(10), torch.zeros(2000)]

    def make(num_points, bucket_size):
        return MultiTensorDiffQuant(ts, [torch.empty_like(t) for t in ts], [torch.zeros_like(t) for t in ts], num_points, bucket_size)

    for bad in (True, 0, -1, 2.5):
        with pytest.raises(ValueError, match='Bucket size must be an integer and strictly positive'):
            make(4, bad)
    for bad in (0, 257, True, 4.0, None, '4'):
        with pytest.raises(ValueError, match='points'):
            make(bad, 256)
    for bucket in (None, 100):
        with pytest.raises(RuntimeError, match='HIP device'):
            make(256, bucket)
