"""The one-launch symbolizer without a GPU: the cases of tests/symbol_cases.py reach every body; the expected symbols, alpha and
beta (libqd_host.so's qd_uniform_f32 with its level output) equal a numpy statement of the reference's operations and, once
dequantized, uniformQuantization itself; the plan and the argument checks of the two C entry points; the argument checks of
MultiTensorSymbols, which fire before a tensor is looked at.  tests/test_hip_symbols.py holds the kernel to these bits."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import bucket_cases as B
import quantization
import symbol_cases as S
from quantized_distillation_amd import _lib
from quantized_distillation_amd import build as qb
from quantized_distillation_amd.multi_tensor import MultiTensorSymbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('qd_multi_symbols_plan', 'qd_multi_uniform_symbols_u8')


@pytest.fixture(scope='module')
def lib():
    qb.build_extension()
    qb.build_host()
    return _lib.load()


class _Boom(object):
    """A tensor that may not be looked at: the argument checks come first."""

    def __getattr__(self, name):
        raise AssertionError('a tensor was touched (%s) before the arguments were checked' % name)


def test_the_cases_reach_every_body_with_both_alignments_of_sym_and_both_sides_of_the_level_limits():
    S.check_paths()
    assert S.CASES is B.Q_CASES and len(S.CASES) == 17
    for assign in S.LEVELS:
        assert sorted({S.sym_phase(i, assign) for i in range(len(S.CASES))}) == sorted(S.SYM_PHASES)
    assert [S.sym_phase(i) for i in range(8)] == [0, 1, 2, 3, 5, 8, 15, 0]
    assert sorted(set(S.LEVELS['ladder'])) == [2, 4, 16, 17, 256] and sorted(set(S.LEVELS['rotated'])) == [2, 3, 16, 255, 256]
    assert all(a != b for a, b in zip(S.LEVELS['ladder'], S.LEVELS['rotated']))


# ---------------------------------------------------------------- the expectations against the oracle
@pytest.mark.parametrize('assign', list(S.LEVELS))
@pytest.mark.parametrize('variant', S.VARIANTS)
def test_expected_symbols_equal_the_references_operations_in_numpy(lib, variant, assign):
    nonzero = 0
    for i, c in enumerate(S.CASES):
        s = S.LEVELS[assign][i]
        sym, alpha, beta = S.expected(i, variant, assign)
        wsym, walpha, wbeta = S.numpy_symbols(S.data(i, variant), s, c.bucket)
        assert sym.dtype == np.uint8 and np.array_equal(sym, wsym), (c.id, s)
        assert S.same_f32(alpha, walpha) and S.same_f32(beta, wbeta), (c.id, s)
        assert sym.size == 0 or int(sym.max()) <= s - 1
        nonzero += int((sym != 0).sum())
    assert nonzero > 1000
    if variant == 'nonfinite':                 # a NaN bucket and the infinite ones: symbol 0 throughout
        sym, alpha, beta = S.expected(2, variant, assign)          # 4 x 256: NaN in row 0, +inf in row 1, -inf in row 3
        assert np.isnan(alpha[0]) and np.isnan(beta[0]) and np.isinf(alpha[1]) and np.isinf(beta[3])
        assert not sym[:512].any() and not sym[768:].any() and not sym[512:768].any()       # (row 2 is the constant bucket)


@pytest.mark.parametrize('assign', list(S.LEVELS))
@pytest.mark.parametrize('variant', S.VARIANTS)
def test_expected_symbols_dequantize_to_uniform_quantization(lib, variant, assign):
    for i, c in enumerate(S.CASES):
        if not c.n:
            continue
        s = S.LEVELS[assign][i]
        sym, alpha, beta = S.expected(i, variant, assign)
        got = S.numpy_dequantize(sym, alpha, beta, s, c.n, c.bucket)
        want = quantization.uniformQuantization(torch.from_numpy(np.array(S.data(i, variant))), s, bucket_size=c.bucket)[0]
        assert S.same_f32(got, want.numpy()), (c.id, s)


# ---------------------------------------------------------------- the plan and the ABI
def test_header_binding_and_library_agree_on_both_entry_points(lib):
    header = open(os.path.join(ROOT, 'include', 'qd_hip.h')).read()
    exported = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH], text=True)
    for name in ENTRIES:
        assert re.search(r'\bint %s\s*\(' % name, header), name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and name not in _lib.HOST_SYMBOLS          # device library only
        assert re.search(r' T %s\b' % name, exported) and hasattr(lib, name)
    assert 'typedef struct QdSymbolDesc' in header
    assert [f for f, _ in _lib.QdSymbolDesc._fields_] == ['x', 'sym', 'n', 'first_tile', 'first_bucket']
    assert ctypes.sizeof(_lib.QdSymbolDesc) == 40
    assert len(_lib.SIGNATURES['qd_multi_symbols_plan'][1]) == 5 and len(_lib.SIGNATURES['qd_multi_uniform_symbols_u8'][1]) == 8


def _host_table(ns, fill=True):
    t = (_lib.QdSymbolDesc * len(ns))()
    for i, n in enumerate(ns):
        t[i].n = n
        if fill:
            t[i].x, t[i].sym = 0x1000, 0x2000          # never dereferenced by the plan
        t[i].first_tile = t[i].first_bucket = -7
    return t


def _plan(lib, ns, buckets, fill=True, table=None):
    t = _host_table(ns, fill) if table is None else table
    tiles, total = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = lib.qd_multi_symbols_plan(t, (ctypes.c_int64 * len(ns))(*buckets), len(ns), ctypes.byref(tiles), ctypes.byref(total))
    return rc, [t[i].first_tile for i in range(len(ns))], [t[i].first_bucket for i in range(len(ns))], tiles.value, total.value


def test_the_plan_counts_tiles_and_buckets_by_the_restated_rule(lib):
    ns = [c.n for c in S.CASES]
    assert _plan(lib, ns, S.BUCKETS) == (0,) + S.plan_rule()
    # the ten tensors of the checkpoint test, the last bucket larger than its tensor; an all-empty list
    ns2, b2 = [300, 7, 4096, 1, 1000, 64, 9, 513, 2, 77], [75, 100, 256, 700, 37, 10, 1, 256, 1, 4096]
    assert _plan(lib, ns2, b2) == (0,) + S.plan_rule(ns2, b2)
    assert _plan(lib, [0, 0, 0], [5, 1, 256], fill=False) == (0, [0, 0, 0], [0, 0, 0], 0, 0)
    rc, ft, fb, tiles, total = _plan(lib, [1024, 0, 1025, 3], [256, 16, 256, 300])
    assert (rc, ft, fb, tiles, total) == (0, [0, 1, 1, 3], [0, 4, 4, 9], 4, 10)


def test_the_plan_refuses_what_the_sibling_plan_refuses(lib):
    assert _plan(lib, [10, 20], [256, 0])[0] == -1 and _plan(lib, [10, 20], [-1, 5])[0] == -1
    assert _plan(lib, [10, -1], [256, 256])[0] == -1
    assert _plan(lib, [10, 20], [256, 256], fill=False)[0] == -1                   # NULL pointers of tensors that have elements
    t = _host_table([10, 20])
    t[1].sym = None
    assert _plan(lib, [10, 20], [4, 4], table=t)[0] == -1
    t = _host_table([10, 0])
    t[1].x = t[1].sym = None                                                      # ... an empty tensor needs none
    assert _plan(lib, [10, 0], [4, 4], table=t)[0] == 0
    t, sizes, out = _host_table([10]), (ctypes.c_int64 * 1)(4), ctypes.c_int64(0)
    assert lib.qd_multi_symbols_plan(None, sizes, 1, ctypes.byref(out), ctypes.byref(out)) == -1
    assert lib.qd_multi_symbols_plan(t, None, 1, ctypes.byref(out), ctypes.byref(out)) == -1
    assert lib.qd_multi_symbols_plan(t, sizes, 0, ctypes.byref(out), ctypes.byref(out)) == -1
    assert lib.qd_multi_symbols_plan(t, sizes, 1, None, ctypes.byref(out)) == -1
    assert lib.qd_multi_symbols_plan(t, sizes, 1, ctypes.byref(out), None) == -1


def test_the_launch_checks_its_arrays_before_touching_the_device(lib):
    """No GPU here: every one of these returns before a launch.  (Pointers are made-up numbers, never dereferenced.)"""
    ok = dict(table=0x1000, levels=0x2000, buckets=0x3000, alpha=0x4000, beta=0x5000)

    def call(ntensors=2, tiles=5, **kw):
        a = dict(ok, **kw)
        return lib.qd_multi_uniform_symbols_u8(a['table'], a['levels'], a['buckets'], ntensors, tiles, a['alpha'], a['beta'], None)

    for name in ok:
        assert call(**{name: None}) == -1, name
    for name, off in (('levels', 2), ('buckets', 4), ('alpha', 1), ('beta', 2)):
        assert call(**{name: ok[name] + off}) == -1, name
    assert call(ntensors=0) == -1 and call(tiles=-1) == -1
    assert call(tiles=0) == 0                                                     # nothing to do: no launch


# ---------------------------------------------------------------- MultiTensorSymbols: validation before any device work
@pytest.mark.parametrize('s', [257, [16, 257], 1, [16, 1], 2.5, '16', None, [16, True]])
def test_a_bad_level_count_raises_before_any_tensor_is_touched(s):
    with pytest.raises(ValueError, match='s must be'):
        MultiTensorSymbols([_Boom(), _Boom()], s, 256)


def test_bucket_size_none_is_not_offered():
    with pytest.raises(NotImplementedError, match='bucket_size'):
        MultiTensorSymbols([_Boom(), _Boom()], 16, None)


@pytest.mark.parametrize('bad', [[256], [256, 64, 16], [256, 0], [256, -64], [256, 2.5], [True, 64], [256, None], [256, '64'], [],
                                 'ab', 0, -4, 2.5, True])
def test_a_bad_bucket_size_raises_before_any_tensor_is_touched(bad):
    with pytest.raises(ValueError, match='bucket_size'):
        MultiTensorSymbols([_Boom(), _Boom()], 16, bad)


def test_wrong_lengths_are_worded_like_the_sibling_classes():
    with pytest.raises(ValueError, match='bucket_size has 3 entries for 2 tensors: need one per tensor'):
        MultiTensorSymbols([_Boom(), _Boom()], 16, [256, 64, 16])
    with pytest.raises(ValueError, match='s has 3 entries for 2 tensors: need one per tensor'):
        MultiTensorSymbols([_Boom(), _Boom()], [16, 4, 2], [256, 64])


@pytest.mark.parametrize('sizes,s', [([256, 64], 16), ((7, 4096), [16, 256]), (100, [2, 255]), (np.array([100, 1]), 2)])
def test_valid_arguments_get_as_far_as_the_device_check(sizes, s):
    with pytest.raises(RuntimeError, match='HIP device'):          # CPU tensors: there is no host form of the launch
        MultiTensorSymbols([torch.zeros(300), torch.zeros(5)], s, sizes)
    with pytest.raises(TypeError, match='torch.Tensor'):           # ... and the tensors are looked at only after the arguments
        MultiTensorSymbols([_Boom(), _Boom()], s, sizes)
    with pytest.raises(RuntimeError, match='HIP device'):
        MultiTensorSymbols([torch.zeros(300), torch.zeros(5)], s, sizes,
                           symbols=[torch.zeros(300, dtype=torch.uint8), torch.zeros(5, dtype=torch.uint8)])
