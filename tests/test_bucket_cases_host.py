"""A bucket size per tensor in the one-launch quantizer and STE backward (qd_multi_buckets_plan, qd_multi_uniform_buckets_f32,
qd_multi_ste_buckets_plan, qd_multi_ste_backward_buckets_f32; MultiTensorQuantizer / MultiTensorSTE with a sequence bucket_size;
per_channel_bucket_sizes; DistillTrainer(bucket_size='per_channel')): everything that can be checked without a GPU -- the plans
against the restated tile rules, the argument checks, the symbols, and the expected bits of every case of tests/bucket_cases.py
(libqd_host.so at (bucket_i, s_i), held to the numpy oracle).  The kernels: tests/test_hip_multi_buckets.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import bucket_cases as B
from quantized_distillation_amd import _lib
from quantized_distillation_amd import build as qb
from quantized_distillation_amd import multi_tensor
from quantized_distillation_amd.multi_tensor import MultiTensorDiffQuant, MultiTensorQuantizer, MultiTensorSTE

NEW = ('qd_multi_buckets_plan', 'qd_multi_uniform_buckets_f32', 'qd_multi_ste_buckets_plan', 'qd_multi_ste_backward_buckets_f32')
BASE = 0x7f0000001000           # a 4 KiB-aligned fake address, never dereferenced: no call below reaches a launch


@pytest.fixture(scope='module')
def lib():
    qb.build_extension()
    qb.build_host()
    return _lib.load()


class _Boom(object):
    """A tensor that may not be looked at: the checks of bucket_size come first."""

    def __getattr__(self, name):
        raise AssertionError('a tensor was touched (%s) before bucket_size was checked' % name)


def _make(cls, tensors, bucket_size, s=16, **kw):
    if cls is MultiTensorQuantizer:
        return cls(tensors, s, bucket_size, **kw)
    return cls(tensors, tensors, s, bucket_size, **kw)


# ---------------------------------------------------------------- the cases land where they say
def test_every_case_reaches_the_path_it_names():
    B.check_paths()


# ---------------------------------------------------------------- the plans against the restated tile rules
def _plan_q(lib, ns, buckets, phases=None):
    n = len(ns)
    T = (_lib.QdTensorDesc * n)()
    for i, m in enumerate(ns):
        T[i].n = m
        T[i].x = BASE + (i << 24) + 4 * (phases[i] if phases else 0)
        T[i].q = BASE + (i << 24) + (1 << 23)
        T[i].first_tile = -7
    total = ctypes.c_int64(-1)
    rc = lib.qd_multi_buckets_plan(T, (ctypes.c_int64 * n)(*buckets), n, ctypes.byref(total))
    return rc, [T[i].first_tile for i in range(n)], total.value


def _plan_ste(lib, ns, buckets, phases=None):
    n = len(ns)
    T = (_lib.QdSteDesc * n)()
    for i, m in enumerate(ns):
        T[i].n = m
        T[i].x = BASE + (i << 24) + 4 * (phases[i] if phases else 0)
        T[i].g = BASE + (i << 24) + (1 << 22) + 4 * ((i + 1) % 4)
        T[i].out = BASE + (i << 24) + (1 << 23) + 4 * ((i + 2) % 4)
        T[i].first_tile = -7
    total = ctypes.c_int64(-1)
    rc = lib.qd_multi_ste_buckets_plan(T, (ctypes.c_int64 * n)(*buckets), n, ctypes.byref(total))
    return rc, [T[i].first_tile for i in range(n)], total.value


def _prefix(tiles):
    first, total = [], 0
    for t in tiles:
        first.append(total)
        total += t
    return first, total


def test_plans_of_the_case_lists(lib):
    rc, first, total = _plan_q(lib, [c.n for c in B.Q_CASES], [c.bucket for c in B.Q_CASES], [c.phase for c in B.Q_CASES])
    want = _prefix([B.q_rule(c.n, c.bucket)['tiles'] for c in B.Q_CASES])
    assert (rc, first, total) == (0,) + want
    assert B.q_rule(2 * 70000, 70000)['tiles'] == 2 and B.q_rule(4 * 256, 256)['tiles'] == 1 and B.q_rule(1000, 100)['tiles'] == 3
    rc, first, total = _plan_ste(lib, [c.n for c in B.STE_CASES], [c.bucket for c in B.STE_CASES], [c.phase for c in B.STE_CASES])
    want = _prefix([B.ste_rule(c.n, c.bucket)['tiles'] for c in B.STE_CASES])
    assert (rc, first, total) == (0,) + want
    assert B.ste_rule(5 * 64, 64)['tiles'] == 2 and B.ste_rule(3 * 512 + 7, 512)['tiles'] == 4 and B.ste_rule(700, 100)['tiles'] == 7


@pytest.mark.parametrize('n', [0, 1, 63, 256, 1000, 4097, 70001])
def test_plans_on_a_sweep_of_rows(lib, n):
    """Every bucket size 1 .. 1100 (rows up to min(n, 1100)) in one table, tensor j under bucket j + 1."""
    buckets = list(range(1, 1101))
    ns = [n] * len(buckets)
    rc, first, total = _plan_q(lib, ns, buckets)
    assert (rc, first, total) == (0,) + _prefix([B.q_rule(n, b)['tiles'] for b in buckets])
    rc, first, total = _plan_ste(lib, ns, buckets, [j % 4 for j in range(len(buckets))])
    assert (rc, first, total) == (0,) + _prefix([B.ste_rule(n, b)['tiles'] for b in buckets])
    if n:                                                   # the rule in words: a DPP row per bucket up to 256, a wave above
        for b in (1, 100, 256, 257, 1100):
            r = B.q_rule(n, b)
            assert r['row'] == min(n, b) and r['nb'] == -(-n // r['row'])
            assert r['tiles'] == (-(-r['nb'] // 4) if r['row'] <= 256 else r['nb'])


def test_the_plans_agree_with_the_scalar_plans_at_equal_entries(lib):
    ns = [800000, 10, 0, 1025, 256, 3]
    for bucket in (256, 64, 100, 7):                        # rows up to 256: the tile of qd_multi_plan
        T = (_lib.QdTensorDesc * len(ns))()
        for i, m in enumerate(ns):
            T[i].n = m
            T[i].x = T[i].q = BASE
        total = lib.qd_multi_plan(T, len(ns), bucket)
        assert _plan_q(lib, ns, [bucket] * len(ns))[1:] == ([T[i].first_tile for i in range(len(ns))], total)
    for bucket in (256, 512, 100, 1024):                    # the STE plan: ste_cut both times
        T = (_lib.QdSteDesc * len(ns))()
        for i, m in enumerate(ns):
            T[i].n = m
            T[i].x = BASE + (i << 24)
            T[i].g = BASE + (i << 24) + (1 << 22) + 4 * ((i + 1) % 4)
            T[i].out = BASE + (i << 24) + (1 << 23) + 4 * ((i + 2) % 4)
        total = ctypes.c_int64(0)
        assert lib.qd_multi_ste_plan(T, len(ns), bucket, ctypes.byref(total)) == 0
        assert _plan_ste(lib, ns, [bucket] * len(ns))[1:] == ([T[i].first_tile for i in range(len(ns))], total.value)


def test_the_plan_calls_refuse_bad_arguments(lib):
    for plan, desc in ((lib.qd_multi_buckets_plan, _lib.QdTensorDesc), (lib.qd_multi_ste_buckets_plan, _lib.QdSteDesc)):
        def table(ns, null=None):
            T = (desc * len(ns))()
            for i, m in enumerate(ns):
                T[i].n = m
                for f, _t in desc._fields_:
                    if f not in ('n', 'first_tile') and f != null:
                        setattr(T[i], f, BASE + 64 * i)
                T[i].first_tile = -7
            return T
        total = ctypes.c_int64(-5)
        ok = (ctypes.c_int64 * 3)(256, 7, 1000)
        T = table([10, 0, 5000])
        assert plan(T, ok, 3, ctypes.byref(total)) == 0 and total.value > 0
        assert plan(None, ok, 3, ctypes.byref(total)) == -1
        assert plan(T, None, 3, ctypes.byref(total)) == -1
        assert plan(T, ok, 3, None) == -1
        assert plan(T, ok, 0, ctypes.byref(total)) == -1 and plan(T, ok, -2, ctypes.byref(total)) == -1
        for bad in (0, -1, -256):                           # a buckets entry <= 0, wherever it sits (an empty tensor's too)
            for at in range(3):
                arr = (ctypes.c_int64 * 3)(256, 7, 1000)
                arr[at] = bad
                fresh, total.value = table([10, 0, 5000]), -5
                assert plan(fresh, arr, 3, ctypes.byref(total)) == -1
                assert total.value == -5 and [fresh[i].first_tile for i in range(3)] == [-7] * 3, 'a refused plan wrote'
        assert plan(table([10, -1, 5000]), ok, 3, ctypes.byref(total)) == -1
        for f, _t in desc._fields_:                          # a tensor with elements needs every pointer; an empty one none
            if f not in ('n', 'first_tile'):
                assert plan(table([10, 0, 5000], null=f), ok, 3, ctypes.byref(total)) == -1, f
                assert plan(table([0, 0, 0], null=f), ok, 3, ctypes.byref(total)) == 0 and total.value == 0


def test_the_launch_calls_check_their_arguments_before_any_launch(lib):
    fake, lv, bk, cell = (ctypes.c_void_p(BASE), ctypes.c_void_p(BASE + 512), ctypes.c_void_p(BASE + 1024), ctypes.c_void_p(BASE + 64))
    nan, inf = float('nan'), float('inf')

    def quant(table=fake, levels=lv, buckets=bk, nt=4, tiles=10, clamp=0, me=0.0, stoch=1, seed=7, seed_cell=None):
        return lib.qd_multi_uniform_buckets_f32(table, levels, buckets, nt, tiles, clamp, me, stoch, seed, seed_cell, None)

    def ste(table=fake, levels=lv, buckets=bk, nt=4, tiles=10, tie=0):
        return lib.qd_multi_ste_backward_buckets_f32(table, levels, buckets, nt, tiles, tie, None)

    for f in (quant, ste):
        assert f(table=None) == -1 and f(levels=None) == -1 and f(buckets=None) == -1
        for off in (1, 2, 3):                                       # the level array: 4-byte aligned
            assert f(levels=ctypes.c_void_p(BASE + 512 + off)) == -1
        for off in range(1, 8):                                     # the bucket array: 8-byte aligned
            assert f(buckets=ctypes.c_void_p(BASE + 1024 + off)) == -1
        assert f(nt=0) == -1 and f(nt=-3) == -1 and f(tiles=-1) == -1
        assert f(tiles=0) == 0                                      # nothing to do
        assert f(tiles=0, levels=None) == -1 and f(tiles=0, buckets=None) == -1      # ... but not with a bad argument
    for me in (0.0, -0.05, nan, -inf):                              # clamp != 0 needs a positive limit
        assert quant(clamp=1, me=me) == -1, me
    assert quant(seed_cell=ctypes.c_void_p(BASE + 68)) == -1        # the seed word: 8-byte aligned
    assert quant(tiles=0, clamp=1, me=0.05, seed_cell=cell) == 0 and quant(tiles=0, stoch=0) == 0
    assert ste(tie=2) == -1 and ste(tie=-1) == -1


# ---------------------------------------------------------------- header, binding and exports agree
def _header_prototype(name):
    text = open(os.path.join(_lib.INCLUDE, 'qd_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, text)
    assert m, name
    return [' '.join(a.split()) for a in m.group(1).split(',')]


def _same_kind(ctype, c_arg):
    if '*' in c_arg:
        return ctype is ctypes.c_void_p or issubclass(ctype, ctypes._Pointer)
    kind = c_arg.rsplit(' ', 1)[0]
    return ctype is {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'uint64_t': ctypes.c_uint64, 'float': ctypes.c_float}[kind]


def test_the_four_symbols_are_exported_declared_and_bound(lib):
    out = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH], text=True)
    exported = set(re.findall(r' T (qd_[a-z0-9_]+)', out))
    for name in NEW:
        assert name in exported, name
        res, args = _lib.SIGNATURES[name]
        proto = _header_prototype(name)
        assert res is ctypes.c_int and len(args) == len(proto) and all(_same_kind(a, p) for a, p in zip(args, proto)), (name, proto)
        assert name not in _lib.HOST_SYMBOLS                                   # device library only
        assert hasattr(lib, name)
    for name in NEW[1::2]:
        proto = _header_prototype(name)
        assert proto[0].endswith('* table') and proto[1:4] == ['const int32_t* levels', 'const int64_t* buckets', 'int ntensors']
    for name in NEW[0::2]:
        assert _header_prototype(name)[1:] == ['const int64_t* buckets', 'int ntensors', 'int64_t* total_tiles_out']
    header = open(os.path.join(_lib.INCLUDE, 'qd_hip.h')).read()
    assert int(re.search(r'#define QD_ABI_VERSION (\d+)', header).group(1)) == _lib.ABI_VERSION == lib.qd_abi_version() == 3


# ---------------------------------------------------------------- per_channel_bucket_sizes
def test_per_channel_bucket_sizes():
    ts = [torch.zeros(8, 3, 3, 3), torch.zeros(10, 64), torch.zeros(16), torch.zeros(()), torch.zeros(0), torch.zeros(0, 5),
          torch.zeros(3, 0), torch.zeros(1, 7), torch.zeros(4, 2, 5).transpose(0, 1)]
    assert multi_tensor.per_channel_bucket_sizes(ts) == [27, 64, 16, 1, 1, 5, 1, 7, 20]
    assert multi_tensor.per_channel_bucket_sizes([]) == []
    for t, b in zip(ts[:3], [27, 64, 16]):
        assert b == (t[0].numel() if t.dim() >= 2 else max(t.numel(), 1))
    assert multi_tensor.per_channel_bucket_sizes(iter(ts[:2])) == [27, 64]      # any iterable
    meta = [torch.empty(6, 4, device='meta')]                                   # no data is looked at
    assert multi_tensor.per_channel_bucket_sizes(meta) == [4]


# ---------------------------------------------------------------- the classes: validation before any device work
@pytest.mark.parametrize('cls', [MultiTensorQuantizer, MultiTensorSTE])
@pytest.mark.parametrize('bad', [[256], [256, 64, 16], [256, 0], [256, -64], [256, 2.5], [True, 64], [256, None], [256, '64'], [],
                                 'ab', [256, 2 ** 63]])
def test_a_bad_list_raises_value_error_before_any_tensor_is_touched(cls, bad):
    with pytest.raises(ValueError, match='bucket_size'):
        _make(cls, [_Boom(), _Boom()], bad)


@pytest.mark.parametrize('cls', [MultiTensorQuantizer, MultiTensorSTE])
def test_a_wrong_length_is_worded_like_the_level_counts(cls):
    with pytest.raises(ValueError, match='bucket_size has 3 entries for 2 tensors: need one per tensor'):
        _make(cls, [_Boom(), _Boom()], [256, 64, 16])
    with pytest.raises(ValueError, match='s has 3 entries for 2 tensors: need one per tensor'):
        _make(cls, [_Boom(), _Boom()], [256, 64], s=[16, 4, 2])


@pytest.mark.parametrize('cls', [MultiTensorQuantizer, MultiTensorSTE])
def test_the_scalar_checks_are_what_they_were(cls):
    for bad in (0, -4, 2.5):
        with pytest.raises(ValueError, match='bucket_size must be a positive integer'):
            _make(cls, [_Boom()], bad)
    with pytest.raises(NotImplementedError, match='bucket_size None'):
        MultiTensorSTE([_Boom()], [_Boom()], 16, None)


@pytest.mark.parametrize('cls', [MultiTensorQuantizer, MultiTensorSTE])
@pytest.mark.parametrize('sizes,s', [([256, 64], 16), ((7, 4096), [16, 4]), ([256, 256], 16), (np.array([100, 1]), 2)])
def test_a_valid_list_gets_as_far_as_the_device_check(cls, sizes, s):
    with pytest.raises(RuntimeError, match='HIP device'):          # CPU tensors: there is no host form of the launch
        _make(cls, [torch.zeros(300), torch.zeros(5)], sizes, s=s)
    with pytest.raises(TypeError, match='torch.Tensor'):           # ... and the tensors are looked at only after the list passed
        _make(cls, [_Boom(), _Boom()], sizes, s=s)


def test_the_combinations_that_are_not_built_say_so():
    x = [torch.zeros(300), torch.zeros(5)]
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(NotImplementedError, match='bucket_size per tensor together with fp16 / bf16 outputs'):
            MultiTensorQuantizer(x, 16, [256, 5], out_dtype=dt)
        with pytest.raises(NotImplementedError, match='bucket_size per tensor together with fp16 / bf16 outputs'):
            MultiTensorQuantizer(x, 16, [256, 5], outputs=[t.to(dt) for t in x])
        with pytest.raises(NotImplementedError, match='bucket_size per tensor together with fp16 / bf16 grads'):
            MultiTensorSTE(x, [t.to(dt) for t in x], 16, [256, 5])
        with pytest.raises(RuntimeError, match='HIP device'):       # one bucket size: as far as the device check, as before
            MultiTensorQuantizer(x, 16, 256, out_dtype=dt)
    with pytest.raises(NotImplementedError, match='MultiTensorDiffQuant with a bucket_size per tensor'):
        MultiTensorDiffQuant([_Boom()], [_Boom()], [_Boom()], 4, [256])
    with pytest.raises(NotImplementedError, match='MultiTensorDiffQuant with a bucket_size per tensor'):
        MultiTensorDiffQuant([_Boom()], [_Boom()], [_Boom()], 4, (256,))
    with pytest.raises(ValueError, match='Bucket size must be an integer'):     # ... and what it refused it refuses
        MultiTensorDiffQuant([_Boom()], [_Boom()], [_Boom()], 4, 2.5)
    with pytest.raises(NotImplementedError, match='uniformQuantization'):
        MultiTensorQuantizer([_Boom(), _Boom()], 16, [256, 64], subtract_mean=True)


def test_trainer_rejects_a_bad_bucket_size_before_it_builds_anything():
    from harness.distill import DistillTrainer
    for bad in ([256, 0], [256, 2.5], [True, 64], 'per_layer', [256, None]):
        with pytest.raises(ValueError, match='bucket_size'):
            DistillTrainer(_Boom(), _Boom(), 'cpu', bucket_size=bad)


# ---------------------------------------------------------------- the expected bits: libqd_host.so, held to the numpy oracle
@pytest.mark.parametrize('opt', list(B.OPTIONS))
@pytest.mark.parametrize('variant', ['finite', 'nonfinite'])
def test_expected_bits_of_the_quantizer_cases(lib, variant, opt):
    for i, c in enumerate(B.Q_CASES):
        got, want = B.expected_q(i, variant, opt), B.oracle_q(i, variant, opt)
        assert got.size == c.n and B.same(got, want), (c.id, variant, opt, int((got.view(np.int32) != want.view(np.int32)).sum()))
        if c.n and variant == 'nonfinite':
            assert np.isnan(got).any()
        elif c.n:
            assert np.isfinite(got).all()
    if opt == 'stoch':                                       # the draws are in use (9 x 64: finite buckets in both variants)
        assert not B.same(B.expected_q(8, variant, 'stoch'), B.expected_q(8, variant, 'det'))


@pytest.mark.parametrize('tie_mode', ['reference', 'true_arg'])
def test_expected_bits_of_the_ste_cases(lib, tie_mode):
    for i, c in enumerate(B.STE_CASES):
        want = B.expected_ste(i, tie_mode)                   # asserts that every bucket's sum is order-free
        got = B.host_ste(i, tie_mode)
        assert got.size == c.n and B.same(got, want), (c.id, tie_mode)
        if c.n:
            assert not B.same(got, B.ste_data(i)[1]), 'the bucket sums show in the output'
