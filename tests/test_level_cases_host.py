"""The level ladder of tests/level_cases.py without a GPU: the two oracles and the CPU path (libqd_host.so) against what the
REFERENCE computed at every level count of the ladder (tests/golden/levels.json: SHA-256 digests written by
tests/golden/gen_levels.py), the accepted range of s at every entry point that takes one, and the shared device checks of
tests/test_hip_levels.py run on CPU tensors -- which also proves those checks and their expectations right.

A digest is of bits: oracle_np, oracle_c and the product give the reference's q, alpha and beta exactly, at s = 2 .. 17 as at
2^24 + 2 (s - 1 a tie in fp32) and 2^31 - 1 (s - 1 rounds past INT_MAX); so do the stochastic branch (torch.rand replaced by
the Philox draws while the reference ran) and the 'complicated' STE backward with one term per bucket.  Dense gradients are
held to errlog's bound instead (check_k7), as everywhere else."""
import ctypes

import numpy as np
import pytest
import torch

import quantization
import quantization.help_functions as qhf
from oracle import oracle_c as oc
from oracle import oracle_np as onp
from quantized_distillation_amd import _lib, ste

import abi_contract as A
import level_cases as L

CPU = 'cpu'


@pytest.fixture(scope='module')
def fixture():
    oc.build()
    return L.load_fixture()


def _of(fixture, kind):
    cases = [c for c in fixture['cases'] if c['kind'] == kind]
    assert len(cases) % len(L.LADDER) == 0 and cases, kind
    return cases


def test_the_ladder_is_what_the_issue_lists():
    assert L.TABLE == tuple(range(2, 18)) and L.MID == (31, 32, 33, 64, 100, 128, 255, 256, 257, 1000, 4096)
    assert L.BIG == (65535, 65536, 65537, 2 ** 23, 2 ** 23 + 1, 2 ** 23 + 2, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 2, 2 ** 24 + 3, 2 ** 24 + 4,
                     2 ** 31 - 128, 2 ** 31 - 1)
    assert L.BYTE == L.TABLE + (31, 32, 33, 64, 100, 128, 255, 256)
    assert max(L.LADDER) == _lib.LEVELS_MAX and min(L.LADDER) == _lib.LEVELS_MIN and min(L.REFUSED) == _lib.LEVELS_MAX + 1
    for x in (L.inputs(1000, 3), L.grid_inputs(1000, 3), L.one_term_gradient(1283, 256, 3), L.dense_gradient(1000, 3)):
        assert x.dtype == np.float32 and np.isfinite(x).all()
    assert np.count_nonzero(L.one_term_gradient(1283, 256, 3)) == 6 and np.count_nonzero(L.one_term_gradient(50, 256, 3)) == 1


@pytest.mark.parametrize('kind', ['det', 'opt', 'stoch', 'ste'])
@pytest.mark.parametrize('which', ['np', 'c'])
def test_oracles_reproduce_the_reference_digests(fixture, which, kind):
    bad = [(c['shape'], c['s']) for c in _of(fixture, kind) if L.result_digest(kind, L.oracle_result(c, which)) != c['sha256']]
    assert not bad, ('oracle_%s differs from the reference at (shape, s):' % which, bad)


@pytest.mark.parametrize('kind', ['det', 'opt', 'stoch', 'ste'])
def test_cpu_path_reproduces_the_reference_digests(fixture, kind):
    """The Python API on CPU tensors (libqd_host.so); the stochastic cases through the C ABI with the recorded seed."""
    bad = []
    for c in _of(fixture, kind):
        r = L.api_result(c, CPU)
        if kind == 'opt':
            assert np.float32(r['mean']) == np.float32(c['mean']), (c['s'], 'the mean', r['mean'], c['mean'])
        if L.result_digest(kind, r) != c['sha256']:
            bad.append((c['shape'], c['s']))
    assert not bad, ('libqd_host.so differs from the reference at (shape, s):', bad)


def test_huffman_mean_bit_length_equals_the_reference(fixture):
    assert [h['s'] for h in fixture['huffman']] == list(L.HUFFMAN_S)
    for h in fixture['huffman']:
        s = h['s']
        model = [torch.from_numpy(t.copy()) for t in L.huffman_model(s)]
        got = qhf.get_huffman_encoding_mean_bit_length(iter(model), lambda p: quantization.uniformQuantization(p, s, bucket_size=256),
                                                       'uniform', s)
        assert abs(got - h['mean_bit_length']) <= L.HUFFMAN_TOL, (s, got, h['mean_bit_length'])


# ---------------------------------------------------------------- the accepted range of s
def test_level_count_helper():
    for s in L.LADDER:
        assert _lib.level_count(s) == s and type(_lib.level_count(float(s) if s <= 2 ** 24 else s)) is int
    assert _lib.level_count(16.0) == 16 and _lib.level_count(np.int64(17)) == 17 and _lib.level_count(np.float32(4.0)) == 4
    for bad in L.REFUSED + (1, 0, -16, 16.5, float(2 ** 31), float('inf'), float('nan'), True, '16', None, [16], 2 ** 64 + 16):
        with pytest.raises(ValueError, match=L.RANGE_TEXT):
            _lib.level_count(bad)


def test_out_of_range_s_is_refused_everywhere_before_anything_is_written(tmp_path):
    """2^32 + 16 on a CPU tensor used to return the 16-level tensor (ctypes masks the int)."""
    L.check_refusals(CPU, tmp_path)


def test_the_oracle_never_agrees_with_a_truncation():
    """oracle_c's ctypes binding refuses what does not fit its C int; oracle_np takes any s, as the reference does, and at
    2^32 + 16 gives what 2^32 + 15 levels give (sm1 = 2^32), not what 16 give."""
    oc.build()
    x = L.inputs(1283, 21)
    for s in L.REFUSED + (1, 16.5):
        with pytest.raises(ValueError):
            oc.uniform_quantize(x, s, 256)
        with pytest.raises(ValueError):
            oc.uniform_quantize_stochastic(x, s, np.zeros(x.size, np.float32), 256)
        with pytest.raises(ValueError):
            oc.ste_complicated_backward(x, x, s, 256)
    big = onp.uniform_quantize(x, 2 ** 32 + 16, 256)['q']
    assert not np.array_equal(big, onp.uniform_quantize(x, 16, 256)['q'])
    assert len(np.unique(big[:256])) > 16
    top = onp.uniform_quantize(x, 2 ** 31 - 1, 256)
    assert top['lev'].max() == 2 ** 31 - 1 and top['lev'].min() == 0                 # saturated, not wrapped
    assert oc.uniform_quantize(x, 2 ** 31 - 1, 256)['lev'].max() == 2 ** 31 - 1


def test_host_abi_refuses_257_levels_with_a_level_output():
    """level_idx holds a byte: 257 levels with it is QD_ERR_INVALID_ARGUMENT, and the sentinel-filled outputs stay."""
    lib = _lib.host()
    x = A.data(2563, 256, 50)
    A.run_case(A.k1('257 levels with level_idx', x, 256, levels=257, lev_phase=0, rc=A.ERR_INVALID), lib, CPU)
    A.run_case(A.k1('256 levels with level_idx', x, 256, levels=256, lev_phase=0), lib, CPU)


# ---------------------------------------------------------------- the device checks, on CPU tensors
@pytest.mark.parametrize('n,bucket', [(2563, 256), (2121, 100), (1000, None), (3001, 1000)])
def test_k1_on_the_ladder(n, bucket):
    L.check_k1_ladder(CPU, n, bucket, 31)


@pytest.mark.parametrize('n,bucket', [(2563, 256), (1000, None)])
def test_k1_options_on_the_ladder(n, bucket):
    L.check_k1_options(CPU, n, bucket, 32)


@pytest.mark.parametrize('n,bucket', [(643, 64), (2121, 100)])
def test_k7_on_the_ladder(n, bucket):
    L.check_k7(CPU, n, bucket, 33)


def test_host_library_errors_are_described_by_the_host_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('a CPU call reached the HIP library')
    monkeypatch.setattr(_lib, 'load', boom)
    x = torch.randn(1000)
    q = torch.full_like(x, 777.0)
    rc = _lib.host().qd_uniform_f32(x.data_ptr(), q.data_ptr(), 1000, 256, ctypes.c_int(2 ** 31), None, None, None, None, 0, 0.0, 0, 0,
                                    None, 0, None)
    assert rc == A.ERR_INVALID and bool((q == 777.0).all())
    with pytest.raises(RuntimeError, match='qd_host: .*invalid'):
        _lib.check(rc, _lib.host())
    with pytest.raises(RuntimeError, match='qd_host'):
        ste.ste_bucket_backward(x, x.clone(), -5, 16)                               # a bucket size the library refuses
