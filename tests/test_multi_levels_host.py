"""A level count per tensor in the one-launch classes and in the compressed checkpoints (qd_multi_uniform_levels_f32,
qd_multi_uniform_global_levels_f32, qd_multi_ste_backward_levels_f32; MultiTensorQuantizer / MultiTensorSTE with a sequence s;
save_compressed(s=[...])): everything that can be checked without a GPU.  The kernels: tests/test_hip_multi_levels.py."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import quantization
from quantized_distillation_amd import _lib, compressed
from quantized_distillation_amd import build as qb
from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer, MultiTensorSTE

NEW = ('qd_multi_uniform_levels_f32', 'qd_multi_uniform_global_levels_f32', 'qd_multi_ste_backward_levels_f32')
BASE = 0x7f0000001000           # a 4 KiB-aligned fake address, never dereferenced: every call below returns before a launch


@pytest.fixture(scope='module')
def lib():
    qb.build_extension()
    return _lib.load()


class _Boom(object):
    """A tensor that may not be looked at: the checks of s come first."""

    def __getattr__(self, name):
        raise AssertionError('a tensor was touched (%s) before s was checked' % name)


def _make(cls, tensors, s):
    if cls is MultiTensorQuantizer:
        return cls(tensors, s, 256)
    return cls(tensors, tensors, s, 256)


# ---------------------------------------------------------------- the classes: validation of a sequence s
@pytest.mark.parametrize('cls', [MultiTensorQuantizer, MultiTensorSTE])
@pytest.mark.parametrize('bad', [[16], [16, 4, 2], [16, 1], [16, 2.5], [True, 4], [16, None], [16, '4'], [], 'ab'])
def test_a_bad_list_raises_value_error_before_any_tensor_is_touched(cls, bad):
    with pytest.raises(ValueError, match='s '):
        _make(cls, [_Boom(), _Boom()], bad)


@pytest.mark.parametrize('cls', [MultiTensorQuantizer, MultiTensorSTE])
def test_the_scalar_checks_are_what_they_were(cls):
    for bad in (1, 2.5, 0, -4):
        with pytest.raises(ValueError, match='s must be an integer >= 2'):
            _make(cls, [_Boom()], bad)


@pytest.mark.parametrize('cls', [MultiTensorQuantizer, MultiTensorSTE])
@pytest.mark.parametrize('s', [[16, 4], (256, 256), [2, 1000]])
def test_a_valid_list_gets_as_far_as_the_device_check(cls, s):
    with pytest.raises(RuntimeError, match='HIP device'):          # CPU tensors: there is no host form of the launch
        _make(cls, [torch.zeros(300), torch.zeros(5)], s)
    with pytest.raises(TypeError, match='torch.Tensor'):           # ... and the tensors are looked at only after s passed
        _make(cls, [_Boom(), _Boom()], s)


def test_what_raised_before_still_raises_with_a_list():
    with pytest.raises(NotImplementedError, match='uniformQuantization'):
        MultiTensorQuantizer([_Boom(), _Boom()], [16, 4], 256, subtract_mean=True)
    with pytest.raises(NotImplementedError, match='bucket_size None'):
        MultiTensorSTE([_Boom(), _Boom()], [_Boom(), _Boom()], [16, 4], None)


# ---------------------------------------------------------------- the C ABI: symbols, prototypes, argument checks
def _header_prototype(name):
    text = open(os.path.join(_lib.INCLUDE, 'qd_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, text)
    assert m, name
    return [' '.join(a.split()) for a in m.group(1).split(',')]


def _ctype_of(c_arg):
    if '*' in c_arg:
        return ctypes.c_void_p
    kind = c_arg.rsplit(' ', 1)[0]
    return {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'uint64_t': ctypes.c_uint64, 'float': ctypes.c_float,
            'size_t': ctypes.c_size_t}[kind]


def test_the_three_symbols_are_exported_and_declared_in_the_header_order(lib):
    out = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH], text=True)
    exported = set(re.findall(r' T (qd_[a-z0-9_]+)', out))
    for name in NEW:
        assert name in exported, name
        res, args = _lib.SIGNATURES[name]
        proto = _header_prototype(name)
        assert res is ctypes.c_int and args == [_ctype_of(a) for a in proto], (name, proto)
        assert proto[0].endswith('* table') and proto[1] == 'const int32_t* levels' and proto[2] == 'int ntensors'
        assert name not in _lib.HOST_SYMBOLS                                   # device library only
    assert _lib.ABI_VERSION == lib.qd_abi_version() == 3                       # additive: the version stays


def test_entry_points_check_their_arguments_before_any_launch(lib):
    fake, lv, cell, ws = (ctypes.c_void_p(BASE), ctypes.c_void_p(BASE + 512), ctypes.c_void_p(BASE + 64),
                          ctypes.c_void_p(BASE + 4096))
    ab = ctypes.c_void_p(BASE + 8192)
    nan, inf = float('nan'), float('inf')

    def bucketed(table=fake, levels=lv, nt=4, tiles=10, bucket=256, clamp=0, me=0.0, stoch=1, seed=7, seed_cell=None):
        return lib.qd_multi_uniform_levels_f32(table, levels, nt, tiles, bucket, clamp, me, stoch, seed, seed_cell, None)

    def glob(table=fake, levels=lv, nt=4, tiles=10, clamp=0, me=0.0, stoch=1, seed=7, seed_cell=None, alpha_beta=ab,
             workspace=ws, nbytes=80):
        return lib.qd_multi_uniform_global_levels_f32(table, levels, nt, tiles, clamp, me, stoch, seed, seed_cell, alpha_beta,
                                                      workspace, nbytes, None)

    def ste(table=fake, levels=lv, nt=4, tiles=10, bucket=256, tie=0):
        return lib.qd_multi_ste_backward_levels_f32(table, levels, nt, tiles, bucket, tie, None)

    for f in (bucketed, glob, ste):
        assert f(table=None) == -1
        assert f(levels=None) == -1
        for off in (1, 2, 3):                                       # the level array: 4-byte aligned
            assert f(levels=ctypes.c_void_p(BASE + 512 + off)) == -1
        assert f(nt=0) == -1 and f(nt=-3) == -1
        assert f(tiles=-1) == -1
        assert f(tiles=0) == 0                                      # nothing to do
        assert f(tiles=0, levels=None) == -1                        # ... but not with a bad argument
    for f in (bucketed, glob):
        for me in (0.0, -0.05, nan, -inf):                          # clamp != 0 needs a positive limit
            assert f(clamp=1, me=me) == -1, me
        assert f(seed_cell=ctypes.c_void_p(BASE + 68)) == -1        # the seed word: 8-byte aligned
        assert f(tiles=0, clamp=1, me=0.05, seed_cell=cell) == 0 and f(tiles=0, stoch=0) == 0
    for f in (bucketed, ste):
        assert f(bucket=0) == -1 and f(bucket=-256) == -1
    assert ste(tie=2) == -1 and ste(tie=-1) == -1
    assert glob(alpha_beta=None) == -1
    assert glob(tiles=0, workspace=None, nbytes=0) == 0
    for kw in ({}, {'clamp': 1, 'me': 0.05}, {'stoch': 0}, {'seed_cell': cell}):      # the workspace: total_tiles * 8 bytes
        assert glob(nbytes=79, **kw) == -2
        assert glob(workspace=None, **kw) == -2
        assert glob(workspace=ctypes.c_void_p(BASE + 4096 + 8), **kw) == -2
    assert glob(nbytes=0, levels=None) == -1                        # an invalid argument wins over the workspace


# ---------------------------------------------------------------- compressed checkpoints with a level count per tensor
S_LIST = [256, 4, 16, 3, 256]
SIZES = [0, 5, 256 * 3 + 7, 2048, 1000]


def _tensors():
    g = torch.Generator().manual_seed(20)
    return {'t%d' % i: torch.randn(n, generator=g) for i, n in enumerate(SIZES)}


@pytest.mark.parametrize('bucket', [256, None])
def test_save_and_load_with_a_level_count_per_tensor(tmp_path, bucket):
    tensors = _tensors()
    path = str(tmp_path / 'mixed.qdz')
    compressed.save_compressed(path, tensors, s=S_LIST, bucket_size=bucket)
    back = compressed.load_compressed(path)
    assert list(back) == list(tensors)
    for (name, t), s in zip(tensors.items(), S_LIST):
        want = quantization.uniformQuantization(t, s, bucket_size=bucket)[0] if t.numel() else t
        assert torch.equal(back[name].view(torch.int32), want.view(torch.int32)), (name, s)
    head = {e['name']: e['levels'] for e in compressed.read_header(path)['tensors']}
    assert [head[n] for n in tensors] == S_LIST


@pytest.mark.parametrize('bucket', [256, None])
def test_a_list_of_equal_values_writes_the_bytes_of_the_scalar(tmp_path, bucket):
    tensors = _tensors()
    a, b = str(tmp_path / 'scalar.qdz'), str(tmp_path / 'list.qdz')
    compressed.save_compressed(a, tensors, s=16, bucket_size=bucket)
    compressed.save_compressed(b, tensors, s=[16] * 5, bucket_size=bucket)
    assert open(a, 'rb').read() == open(b, 'rb').read()


def test_the_entries_go_to_the_quantized_tensors(tmp_path):
    """quantize_first_last=False: the first and the last tensor are stored raw and have no entry in s."""
    tensors = _tensors()
    path = str(tmp_path / 'inner.qdz')
    compressed.save_compressed(path, tensors, s=[4, 16, 3], bucket_size=256, quantize_first_last=False)
    back = compressed.load_compressed(path)
    names = list(tensors)
    assert torch.equal(back[names[-1]], tensors[names[-1]])
    for name, s in zip(names[1:-1], [4, 16, 3]):
        assert torch.equal(back[name], quantization.uniformQuantization(tensors[name], s, bucket_size=256)[0])
    with pytest.raises(ValueError, match='one per quantized tensor'):
        compressed.save_compressed(path, tensors, s=S_LIST, bucket_size=256, quantize_first_last=False)


@pytest.mark.parametrize('bad', [[256, 4, 16, 3, 1], [256, 4, 16, 3, 257], [256, 4, 16, 3], [256, 4, 16, 3, 256, 4],
                                 [256, 4, 16, 3, 2.5], [256, 4, 16, 3, True], 'abcde'])
def test_bad_entries_raise_value_error(tmp_path, bad):
    path = str(tmp_path / 'bad.qdz')
    with pytest.raises(ValueError):
        compressed.save_compressed(path, _tensors(), s=bad, bucket_size=256)
    assert not os.path.exists(path)


# ---------------------------------------------------------------- the trainer's signature
def test_trainer_rejects_a_bad_width_list_before_it_builds_anything():
    from harness.distill import DistillTrainer
    for bad in ([8, 0], [8, 2.5], [True, 4]):
        with pytest.raises(ValueError, match='num_bits'):
            DistillTrainer(_Boom(), _Boom(), 'cpu', num_bits=bad)
