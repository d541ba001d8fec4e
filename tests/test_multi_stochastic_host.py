"""The one-launch quantizer with options (qd_multi_uniform_opt_f32 / qd_multi_uniform_global_opt_f32, MultiTensorQuantizer's
stochastic_rounding / max_element / seed_on_device): everything that can be checked without a GPU -- the seed reservation, the
argument checks of both entry points before any launch, the class's argument errors before a tensor is looked at.  The kernels
themselves: tests/test_hip_multi_stochastic.py."""
import ctypes

import pytest
import torch

from quantized_distillation_amd import _lib
from quantized_distillation_amd import build as qb
from quantized_distillation_amd.quantization import quant_functions as qf

BASE = 0x7f0000001000           # a 4 KiB-aligned fake address, never dereferenced: every call below returns before a launch
M64 = (1 << 64) - 1


@pytest.fixture(scope='module')
def lib():
    qb.build_extension()
    return _lib.load()


@pytest.fixture
def counter():
    """The process's stochastic call counter, put back afterwards."""
    saved = qf._STOCHASTIC_CALLS[0]
    yield qf._STOCHASTIC_CALLS
    qf._STOCHASTIC_CALLS[0] = saved


@pytest.mark.parametrize('host', [True])      # (the device generator's seed needs a device: tests/test_hip_multi_stochastic.py)
def test_reserve_returns_the_next_seed_and_advances_by_count(counter, host):
    for start, n in ((0, 1), (5, 60), (123456, 7)):
        counter[0] = start
        first = qf.next_stochastic_seed(peek=True, host=host)
        assert qf.reserve_stochastic_seeds(n, host=host) == first
        assert counter[0] == start + n
        assert qf.next_stochastic_seed(peek=True, host=host) == (first + n) & M64
        # tensor i of the launch == the i-th call of the loop from the same counter state
        counter[0] = start
        assert [qf.next_stochastic_seed(host=host) for _ in range(n)] == [(first + i) & M64 for i in range(n)]
        assert counter[0] == start + n


def test_reserve_across_a_wrap_of_the_low_word(counter):
    base = (torch.initial_seed() * 0x9E3779B97F4A7C15) & M64
    # the counter value that puts the next seed's low word at 0xFFFFFFFE: a reservation of 5 runs over the 32-bit boundary
    counter[0] = ((0xFFFFFFFE - (base & 0xFFFFFFFF)) - 1) & 0xFFFFFFFF
    first = qf.next_stochastic_seed(peek=True, host=True)
    assert first & 0xFFFFFFFF == 0xFFFFFFFE
    assert qf.reserve_stochastic_seeds(5, host=True) == first
    after = qf.next_stochastic_seed(peek=True, host=True)
    assert after == (first + 5) & M64 and after & 0xFFFFFFFF == 3 and (after >> 32) == ((first >> 32) + 1) & 0xFFFFFFFF
    # ... and over 2^64 itself
    counter[0] = (M64 - base) & M64                       # next seed = base + counter + 1 = 2^64 -> 0
    assert qf.next_stochastic_seed(peek=True, host=True) == 0
    counter[0] -= 2
    first = qf.reserve_stochastic_seeds(4, host=True)
    assert first == M64 - 1 and qf.next_stochastic_seed(peek=True, host=True) == 2


def test_reserve_argument_errors(counter):
    before = counter[0]
    for bad in (0, -1, 1.5, True, None, '3'):
        with pytest.raises(ValueError):
            qf.reserve_stochastic_seeds(bad, host=True)
    assert counter[0] == before


def test_entry_points_check_their_arguments_before_any_launch(lib):
    fake, cell, ws = ctypes.c_void_p(BASE), ctypes.c_void_p(BASE + 64), ctypes.c_void_p(BASE + 4096)
    ab = ctypes.c_void_p(BASE + 8192)
    nan, inf = float('nan'), float('inf')

    def bucketed(table=fake, nt=4, tiles=10, bucket=256, levels=16, clamp=0, me=0.0, stoch=1, seed=7, seed_cell=None):
        return lib.qd_multi_uniform_opt_f32(table, nt, tiles, bucket, levels, clamp, me, stoch, seed, seed_cell, None)

    def glob(table=fake, nt=4, tiles=10, levels=16, clamp=0, me=0.0, stoch=1, seed=7, seed_cell=None, alpha_beta=ab,
             workspace=ws, nbytes=80):
        return lib.qd_multi_uniform_global_opt_f32(table, nt, tiles, levels, clamp, me, stoch, seed, seed_cell, alpha_beta,
                                                   workspace, nbytes, None)

    for f in (bucketed, glob):
        assert f(table=None) == -1
        assert f(nt=0) == -1 and f(nt=-3) == -1
        assert f(tiles=-1) == -1
        assert f(levels=1) == -1 and f(levels=0) == -1
        for me in (0.0, -0.05, nan, -inf):                   # clamp != 0 needs a positive limit
            assert f(clamp=1, me=me) == -1, me
        assert f(seed_cell=ctypes.c_void_p(BASE + 68)) == -1       # the seed word: 8-byte aligned
        # total_tiles == 0: nothing to do, whatever the options (and, for the global form, whatever the workspace)
        assert f(tiles=0) == 0 and f(tiles=0, clamp=1, me=0.05, seed_cell=cell) == 0 and f(tiles=0, stoch=0) == 0
    assert bucketed(bucket=0) == -1 and bucketed(bucket=-256) == -1
    assert glob(alpha_beta=None) == -1
    assert glob(tiles=0, workspace=None, nbytes=0) == 0
    # the workspace: total_tiles * 8 bytes, 16-byte aligned -- refused before any launch, for every option
    for kw in ({}, {'clamp': 1, 'me': 0.05}, {'stoch': 0, 'clamp': 1, 'me': inf}, {'seed_cell': cell}):
        assert glob(nbytes=79, **kw) == -2
        assert glob(workspace=None, **kw) == -2
        assert glob(workspace=ctypes.c_void_p(BASE + 4096 + 8), **kw) == -2
    # an invalid argument wins over the workspace
    assert glob(nbytes=0, clamp=1, me=0.0) == -1
    for name in ('qd_multi_uniform_opt_f32', 'qd_multi_uniform_global_opt_f32'):
        assert name in _lib.SIGNATURES and name not in _lib.HOST_SYMBOLS          # device library only
    assert _lib.ABI_VERSION == lib.qd_abi_version() == 3                          # additive: the version stays


class _Boom(object):
    """A tensor list that may not be looked at: the option errors come first."""

    def __iter__(self):
        raise AssertionError('the tensors were adopted before the options were checked')


def test_class_option_errors_fire_before_any_tensor_is_adopted():
    from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer
    with pytest.raises(NotImplementedError, match='uniformQuantization'):
        MultiTensorQuantizer(_Boom(), 16, 256, subtract_mean=True)
    with pytest.raises(ValueError, match='seed_on_device'):
        MultiTensorQuantizer(_Boom(), 16, 256, seed_on_device=True)
    for bad in (True, 'x', None, [0.05]):                     # as ScalingFunction: False or a number
        with pytest.raises(ValueError, match='maxElementAllowed must be a number'):
            MultiTensorQuantizer(_Boom(), 16, 256, max_element=bad)
        with pytest.raises(ValueError, match='maxElementAllowed must be a number'):
            qf.ScalingFunction('linear', bad, False, 256)
    # valid options get as far as the tensors (CPU tensors: there is no host form of the launch)
    with pytest.raises(AssertionError, match='adopted'):
        MultiTensorQuantizer(_Boom(), 16, 256, stochastic_rounding=True, max_element=0.05, seed_on_device=True)
    with pytest.raises(RuntimeError, match='HIP device'):
        MultiTensorQuantizer([torch.zeros(300)], 16, 256, stochastic_rounding=True, max_element=0.05)


def test_trainer_signature_defaults():
    import inspect
    from harness.distill import DistillTrainer
    from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer
    p = inspect.signature(DistillTrainer.__init__).parameters
    assert p['stochastic_rounding'].default is False and p['max_element'].default is False
    p = inspect.signature(MultiTensorQuantizer.__init__).parameters
    assert [p[k].default for k in ('outputs', 'stochastic_rounding', 'max_element', 'subtract_mean', 'seed_on_device')] == \
        [None, False, False, False, False]
    p = inspect.signature(MultiTensorQuantizer.quantize).parameters
    assert p['check_pointers'].default is True and p['seed'].default is None
