"""Multi-tensor K7 (qd_multi_ste_plan / qd_multi_ste_backward_f32, MultiTensorSTE): everything that can be checked without a
GPU -- the host plan's tile rule, the argument checks of both entry points before any launch, the Python class's argument
errors on CPU tensors.  The kernel itself: tests/test_hip_multi_ste.py."""
import ctypes

import pytest
import torch

from quantized_distillation_amd import _lib
from quantized_distillation_amd import build as qb

BASE = 0x7f0000001000           # a 4 KiB-aligned fake address: the plan only looks at the pointers' alignment


@pytest.fixture(scope='module')
def lib():
    qb.build_extension()
    return _lib.load()


def table(ns, offsets=None, stride=1 << 24):
    """Host descriptors with fake, distinct pointers: tensor i's x / g / out start `offsets[i]` bytes past aligned slots."""
    T = (_lib.QdSteDesc * len(ns))()
    for i, n in enumerate(ns):
        off = 0 if offsets is None else offsets[i]
        T[i].x = BASE + (3 * i) * stride + off
        T[i].g = BASE + (3 * i + 1) * stride + off
        T[i].out = T[i].g
        T[i].n = n
    return T


def plan(lib, T, bucket):
    total = ctypes.c_int64(-7)
    rc = lib.qd_multi_ste_plan(T, len(T), bucket, ctypes.byref(total))
    return rc, total.value, [T[i].first_tile for i in range(len(T))]


def rule(n, bucket, aligned=True):
    """The documented tile rule (include/qd_hip.h), restated: what qd_ste_bucket_backward_f32 does with one tensor."""
    if n == 0:
        return 0
    row = min(n, bucket)
    nb = -(-n // row)
    per_tile = {64: 4, 128: 4, 256: 4, 512: 1, 1024: 1}.get(row)
    if per_tile is None or not aligned or nb == 1:
        return nb                                    # one wave per bucket
    nfull = n // row
    return -(-nfull // per_tile) + (nb - nfull)      # register tiles over the full buckets + the ragged last bucket


def test_plan_hand_computed(lib):
    ns = [800000, 10, 0, 1025]
    # bucket 256: 3125 full buckets -> 782 register tiles; one short bucket -> 1; empty -> 0; 4 full buckets -> 1 register tile + 1 tail
    rc, total, first = plan(lib, table(ns), 256)
    assert rc == 0 and first == [0, 782, 783, 783] and total == 785
    # the same tensors 4, 8 and 12 bytes into a 16-byte granule: the register path needs 4-byte alignment only (the per-tensor
    # call's rule), so nothing moves
    for off in (4, 8, 12):
        assert plan(lib, table(ns, [off] * 4), 256) == (0, 785, [0, 782, 783, 783])
    # a pointer that is not 4-byte aligned: one wave per bucket for that tensor (3125 tiles; 5 tiles)
    rc, total, first = plan(lib, table(ns, [2, 0, 0, 2]), 256)
    assert rc == 0 and first == [0, 3125, 3126, 3126] and total == 3131
    # only `out` misaligned
    T = table(ns)
    T[3].out = T[3].x + 4096 + 1
    assert plan(lib, T, 256) == (0, 788, [0, 782, 783, 783])
    # bucket 512 / 1024: one full bucket per register tile; 100: no register path at all
    assert plan(lib, table(ns), 512) == (0, 1563 + 1 + 0 + 3, [0, 1563, 1564, 1564])       # 1562 full + tail; 10; 0; 2 full + tail
    assert plan(lib, table(ns), 1024) == (0, 782 + 1 + 0 + 2, [0, 782, 783, 783])          # 781 full + tail; 10; 0; 1 full + tail
    assert plan(lib, table(ns), 100) == (0, 8000 + 1 + 0 + 11, [0, 8000, 8001, 8001])
    # exactly one bucket: the per-tensor call sends a single bucket down the generic path
    assert plan(lib, table([256, 512, 257]), 256) == (0, 1 + 1 + 2, [0, 1, 2])


@pytest.mark.parametrize('bucket', [64, 128, 256, 512, 1024, 100, 7, 1])
def test_plan_is_a_prefix_of_the_rule(lib, bucket):
    g = torch.Generator().manual_seed(bucket)
    ns = [int(v) for v in torch.randint(0, 70000, (40,), generator=g)] + [0, 0, 1, bucket, bucket + 1, 2 * bucket, 3 << 20, 0]
    offs = [int(v) for v in torch.randint(0, 8, (len(ns),), generator=g)]
    rc, total, first = plan(lib, table(ns, offs), bucket)
    assert rc == 0
    want = [rule(n, bucket, off % 4 == 0) for n, off in zip(ns, offs)]
    assert first == [sum(want[:i]) for i in range(len(ns))] and total == sum(want)
    assert all(b >= a for a, b in zip(first, first[1:]))
    for i, n in enumerate(ns):
        if n == 0:
            assert (first[i + 1] if i + 1 < len(ns) else total) == first[i]          # an empty tensor owns no tile


def test_plan_argument_errors(lib):
    T = table([100, 200])
    total = ctypes.c_int64(0)
    assert lib.qd_multi_ste_plan(None, 2, 256, ctypes.byref(total)) == -1
    assert lib.qd_multi_ste_plan(T, 2, 0, ctypes.byref(total)) == -1
    assert lib.qd_multi_ste_plan(T, 2, -256, ctypes.byref(total)) == -1
    assert lib.qd_multi_ste_plan(T, 2, 256, None) == -1
    assert lib.qd_multi_ste_plan(T, 0, 256, ctypes.byref(total)) == -1
    T[1].n = -1
    assert lib.qd_multi_ste_plan(T, 2, 256, ctypes.byref(total)) == -1
    T[1].n = 200
    T[1].g = None                                   # a non-empty tensor without a gradient
    assert lib.qd_multi_ste_plan(T, 2, 256, ctypes.byref(total)) == -1
    T[1].n = 0                                      # ... an empty one needs no pointers
    assert lib.qd_multi_ste_plan(T, 2, 256, ctypes.byref(total)) == 0 and total.value == 1


def test_backward_checks_its_arguments_before_any_launch(lib):
    fake = ctypes.c_void_p(BASE)                    # never dereferenced on the host: every call below returns before a launch
    assert lib.qd_multi_ste_backward_f32(None, 4, 10, 256, 16, 0, None) == -1
    assert lib.qd_multi_ste_backward_f32(fake, 4, 10, 256, 1, 0, None) == -1          # levels < 2
    assert lib.qd_multi_ste_backward_f32(fake, 4, 10, 256, 16, 2, None) == -1         # unknown tie mode
    assert lib.qd_multi_ste_backward_f32(fake, 4, 10, 256, 16, -1, None) == -1
    assert lib.qd_multi_ste_backward_f32(fake, 0, 10, 256, 16, 0, None) == -1
    assert lib.qd_multi_ste_backward_f32(fake, 4, -1, 256, 16, 0, None) == -1
    assert lib.qd_multi_ste_backward_f32(fake, 4, 10, 0, 16, 0, None) == -1
    assert lib.qd_multi_ste_backward_f32(fake, 4, 0, 256, 16, 1, None) == 0           # nothing to do
    assert 'qd_multi_ste_backward_f32' not in _lib.HOST_SYMBOLS and 'qd_multi_ste_plan' not in _lib.HOST_SYMBOLS
    assert ctypes.sizeof(_lib.QdSteDesc) == 40


def test_multi_tensor_ste_argument_errors():
    from quantized_distillation_amd.multi_tensor import MultiTensorSTE
    w, g = [torch.zeros(300), torch.zeros(10)], [torch.zeros(300), torch.zeros(10)]
    with pytest.raises(RuntimeError, match='HIP device'):
        MultiTensorSTE(w, g, 16, 256)
    with pytest.raises(NotImplementedError, match='does not work with bucket_size None'):
        MultiTensorSTE(w, g, 16, None)
    with pytest.raises(ValueError):
        MultiTensorSTE([], [], 16, 256)
    for bad_s in (1, 0, 2.5):
        with pytest.raises(ValueError):
            MultiTensorSTE(w, g, bad_s, 256)
    for bad_bucket in (0, -4, 2.0, True):
        with pytest.raises(ValueError):
            MultiTensorSTE(w, g, 16, bad_bucket)
    with pytest.raises(ValueError):
        MultiTensorSTE(w, g[:1], 16, 256)
    with pytest.raises(ValueError):
        MultiTensorSTE(w, g, 16, 256, outs=[torch.zeros(300)])
    with pytest.raises(ValueError):
        MultiTensorSTE(w, g, 16, 256, tie_mode='first')
    with pytest.raises(TypeError):
        MultiTensorSTE([[0.0] * 300], g[:1], 16, 256)
    # (size mismatches between a weight and its gradient are checked after the device, which a CPU tensor never passes:
    # tests/test_hip_multi_ste.py)
