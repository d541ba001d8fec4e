"""tests/dq16_cases.py proven without a GPU, and everything of the 16-bit differentiable-quantization sweeps that needs no
device: (a) every exact case puts {0, v} on the fp32 output of nonUniformQuantization (libqd_host.so) and torch's .to(dtype)
of it shows the hand-written pattern; (b) the exact-sum gradients are 16-bit numbers; (c) the two new symbols are exported and
declared as the header declares them; the plan's refusal of odd addresses, the launches' argument checks that come before any
launch, and the dtype rules of MultiTensorDiffQuant that come before any device is needed."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

import dq16_cases as C
import exact_sum_cases as E
import out16_cases as O
import quantization
from quantized_distillation_amd import _lib
from quantized_distillation_amd import build as qb

BASE = 0x7f0000001000           # a 4 KiB-aligned fake address: never dereferenced on the host
STRIDE = 1 << 24
DTYPES = {'float16': torch.float16, 'bfloat16': torch.bfloat16}


@pytest.fixture(scope='module')
def lib():
    qb.build_extension()
    return _lib.load()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- (a) the forward table
def test_points_rows_start_at_zero_and_end_at_one():
    for k in C.FWD_K:
        p = C.points_row(k)
        assert p.size == k and p.dtype == np.float32 and bits(p)[0] == 0 and p[-1] == 1.0 and np.all(np.diff(p) > 0)
    assert np.array_equal(C.points_row(2), np.array([0, 1], np.float32))


@pytest.mark.parametrize('bucket', C.FWD_BUCKETS)
def test_every_exact_case_puts_its_value_and_its_pattern_on_the_output(bucket):
    assert len(C.EXACT) == 22
    for name, v, want in C.EXACT:
        x = C.tensor_of(v)
        for k in C.FWD_K:
            q, idx, _ = quantization.nonUniformQuantization(torch.from_numpy(x.copy()), torch.from_numpy(C.points_row(k)),
                                                            bucket_size=bucket)
            q, idx = q.reshape(-1), idx.reshape(-1).numpy()
            assert np.array_equal(bits(q.numpy()), bits(x)), (name, bucket, k, 'the case does not quantize to {0, v}')
            lo, hi = (0, k - 1) if v > 0 else (k - 1, 0)                # a negative v is the bucket's minimum: u = 0 there
            assert (idx[0::2] == lo).all() and (idx[1::2] == hi).all(), (name, bucket, k)
            for fmt, pattern in want.items():
                p16 = O.patterns(q.to(DTYPES[fmt]))
                assert (p16[0::2] == 0).all(), (name, fmt, 'the zeros are +0')
                if pattern is not None:
                    assert (p16[1::2] == pattern).all(), (name, fmt, bucket, k, '0x%04X, intended 0x%04X' % (p16[1], pattern))


@pytest.mark.parametrize('bucket', [256, None])
def test_the_non_finite_cases_give_nan_where_the_bucket_holds_one(bucket):
    for name, x in C.nonfinite():
        q = quantization.nonUniformQuantization(torch.from_numpy(x.copy()), torch.from_numpy(C.points_row(4)), bucket_size=bucket)[0]
        bad = ~torch.isfinite(q.reshape(-1)).numpy()          # (the inf itself stays an inf, everything beside it is NaN)
        if bucket is None:
            assert bad.all(), name
        else:
            assert bad[256:512].all() and not bad[:256].any() and not bad[512:].any(), name


def test_the_random_lists_hold_what_the_device_tests_need():
    for bucket in C.FWD_BUCKETS:
        ns = C.sizes(bucket)
        total = sum(C.forward_tiles(n, bucket) for n in ns)
        assert total >= C.MIN_TILES and total % 4 and ns[0] == 0 and ns[-1] == 0
        assert {1, 3, 1023, 1024, 1025} <= set(ns)
        if bucket:
            assert any(n > bucket and n % bucket for n in ns) and any(n > bucket and n % bucket == 0 for n in ns)
    for fmt in C.FORMATS:
        ts, pts = C.random_list(256, 16, fmt)
        assert pts.shape == (len(ts), 16) and np.all(np.diff(pts, axis=1) >= 0)
        wt = C.with_widening_patterns(ts, fmt)
        changed = [i for i, ((_, a), (_, b)) in enumerate(zip(ts, wt)) if not np.array_equal(a, b)]
        assert len(changed) == 3
        seen = set()
        for i in changed:
            g, n = wt[i][1], wt[i][1].size
            full = n // 1024 * 1024
            special = set(p for p, _ in C.WIDENING[fmt]) | {C.NAN16[fmt]}
            assert set(g[:full].tolist()) & special and set(g[full:].tolist()) & special      # main tiles and the remainder
            seen |= set(g.tolist()) & special
        assert seen == special


# ---------------------------------------------------------------- (b) the exact-sum gradients are 16-bit numbers
@pytest.mark.parametrize('k,bucket', [(16, 256), (16, 100), (16, None), (4, 256), (256, 256)])
def test_the_exact_sum_gradients_survive_both_16_bit_types(k, bucket):
    mc = C.m_case(k, bucket)
    assert len(mc.sizes) == 137 and max(mc.sizes) == 2049 * 1024 + 17 and mc.sizes.count(0) == 4
    values = set()
    for g in mc.g:
        values |= set(np.unique(g).tolist())
        for fmt in C.FORMATS:
            assert np.array_equal(bits(C.widen(C.to_patterns(g, fmt), fmt)), bits(g)), fmt
    assert values == {-3.0, -2.0, -1.0, 1.0, 2.0, 3.0}
    assert E.M_K == C.BWD_K and E.M_BUCKETS == C.BWD_BUCKETS


# ---------------------------------------------------------------- (c) symbols and declarations
NAMES = ('qd_multi_nearest_out16_f32', 'qd_multi_point_grad_in16_f32')


def test_both_symbols_are_exported_and_declared_with_the_headers_argument_lists(lib):
    syms = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    header = open(_lib.INCLUDE + '/qd_hip.h').read()
    ctype_of = [(r'QdDiffQuantDesc\s*\*', ('LP_QdDiffQuantDesc', 'c_void_p')), (r'float\s*\*', ('c_void_p',)), (r'void\s*\*', ('c_void_p',)),
                (r'size_t', ('c_size_t', 'c_ulong')), (r'int64_t', ('c_long', 'c_int64')), (r'int', ('c_int',))]
    for name in NAMES:
        assert re.search(r'\bT %s\b' % name, syms), name
        assert name not in _lib.HOST_SYMBOLS                                 # device library only
        m = re.search(r'\bint %s\(([^;]*)\);' % name, header)
        assert m, name
        args = [re.sub(r'/\*.*?\*/', '', a).strip() for a in m.group(1).replace('\n', ' ').split(',')]
        res, decl = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(decl) == len(args), (name, args, decl)
        for a, d in zip(args, decl):
            a = a.replace('const ', '')
            want = next(names_ for pat, names_ in ctype_of if re.match(pat, a))
            assert d.__name__ in want, (name, a, d.__name__)
        assert getattr(lib, name).argtypes == list(decl)
    assert re.search(r'#define QD_OUT_F16 1\b', header) and re.search(r'#define QD_OUT_BF16 2\b', header)
    assert re.search(r'#define QD_GRAD_F16 1\b', header) and re.search(r'#define QD_GRAD_BF16 2\b', header)
    assert C.KIND == {'float16': 1, 'bfloat16': 2}
    assert re.search(r'#define QD_ABI_VERSION 3\b', header) and lib.qd_abi_version() == 3


# ---------------------------------------------------------------- what the host checks before any launch
def table(ns, q_phase=0, g_phase=0):
    T = (_lib.QdDiffQuantDesc * len(ns))()
    for i, n in enumerate(ns):
        for j, field in enumerate(('u', 'q', 'idx', 'alpha', 'beta', 'grad')):
            setattr(T[i], field, BASE + (6 * i + j) * STRIDE + (q_phase if field == 'q' else g_phase if field == 'grad' else 0))
        T[i].n = n
    return T


def plan(lib, T, bucket):
    rows = ctypes.c_int64(-7)
    tiles = lib.qd_multi_dq_plan(T, len(T), bucket, ctypes.byref(rows))
    return tiles, rows.value, [(T[i].first_tile, T[i].first_block, T[i].first_row) for i in range(len(T))]


def test_the_plan_depends_on_no_alignment_and_refuses_odd_addresses(lib):
    ns = [0, 5, 1024, 3000, 0, 70000]
    for bucket in (0, 100, 256):
        want = plan(lib, table(ns), bucket)
        assert want[0] > 0 and want[1] == sum(min(n // 1024, 2048) + 1 for n in ns)
        for phase in C.PHASES:
            assert plan(lib, table(ns, phase, 0), bucket) == want and plan(lib, table(ns, 0, phase), bucket) == want
    for field in ('q', 'grad'):
        for odd in (1, 3, 15):
            T = table(ns)
            setattr(T[3], field, getattr(T[3], field) + odd)
            got = plan(lib, T, 256)
            assert got[0] == -1 and got[1] == -7 and all(t == (0, 0, 0) for t in got[2]), (field, odd, 'refused with nothing written')
            T[3].n = 0                                   # an empty tensor's pointers are not looked at
            assert plan(lib, T, 256)[0] > 0


def test_the_launches_check_their_arguments_before_any_launch(lib):
    fake = ctypes.c_void_p(BASE)
    fwd, bwd = lib.qd_multi_nearest_out16_f32, lib.qd_multi_point_grad_in16_f32
    for kind in (0, 3, -1):
        assert fwd(fake, 4, 10, 256, fake, 16, kind, None) == -1
        assert bwd(fake, 4, 10, 256, 16, kind, fake, fake, 1 << 20, None) == -1
    for kind in (1, 2):
        # the refusals of qd_multi_nearest_f32
        assert fwd(None, 4, 10, 256, fake, 16, kind, None) == -1 and fwd(fake, 0, 10, 256, fake, 16, kind, None) == -1
        assert fwd(fake, 4, -1, 256, fake, 16, kind, None) == -1 and fwd(fake, 4, 10, -1, fake, 16, kind, None) == -1
        assert fwd(fake, 4, 10, 256, None, 16, kind, None) == -1
        assert fwd(fake, 4, 10, 256, fake, 0, kind, None) == -1 and fwd(fake, 4, 10, 256, fake, 257, kind, None) == -1
        assert fwd(fake, 4, 0, 256, fake, 16, kind, None) == 0              # nothing to do: no launch
        # the refusals of qd_multi_point_grad_f32
        assert bwd(None, 4, 10, 256, 16, kind, fake, fake, 1 << 20, None) == -1
        assert bwd(fake, 4, 3, 256, 16, kind, fake, fake, 1 << 20, None) == -1          # fewer rows than tensors
        assert bwd(fake, 4, 4 * 2049 + 1, 256, 16, kind, fake, fake, 1 << 30, None) == -1
        assert bwd(fake, 4, 10, 256, 0, kind, fake, fake, 1 << 20, None) == -1 and bwd(fake, 4, 10, 256, 257, kind, fake, fake, 1 << 20, None) == -1
        assert bwd(fake, 4, 10, 256, 16, kind, None, fake, 1 << 20, None) == -1
        small = lib.qd_multi_point_grad_f32(fake, 4, 10, 256, 16, fake, fake, 10 * 16 * 4 - 1, None)
        assert small != 0 and small != -1                                                 # QD_ERR_WORKSPACE_TOO_SMALL
        assert bwd(fake, 4, 10, 256, 16, kind, fake, fake, 10 * 16 * 4 - 1, None) == small      # one byte short
        assert bwd(fake, 4, 10, 256, 16, kind, fake, None, 1 << 20, None) == small
        assert bwd(fake, 4, 10, 256, 16, kind, fake, ctypes.c_void_p(BASE + 8), 1 << 20, None) == small


def test_dtype_rules_come_before_any_device_is_needed():
    from quantized_distillation_amd.multi_tensor import MultiTensorDiffQuant
    w = [torch.zeros(300), torch.zeros(10)]
    h = [torch.zeros(300, dtype=torch.float16), torch.zeros(10, dtype=torch.float16)]
    b = [torch.zeros(300, dtype=torch.bfloat16), torch.zeros(10, dtype=torch.bfloat16)]
    for mixed in ([h[0], b[1]], [h[0], w[1]], [w[0], b[1]]):
        with pytest.raises(TypeError, match='outputs must all have one dtype'):
            MultiTensorDiffQuant(w, mixed, w, 4, 256)
        with pytest.raises(TypeError, match='grads must all have one dtype'):
            MultiTensorDiffQuant(w, w, mixed, 4, 256)
    for other in (torch.float64, torch.int16, torch.uint8):
        with pytest.raises(TypeError, match='float32, float16 or bfloat16'):
            MultiTensorDiffQuant(w, [t.to(other) for t in w], w, 4, 256)
        with pytest.raises(TypeError, match='float32, float16 or bfloat16'):
            MultiTensorDiffQuant(w, h, [t.to(other) for t in w], 4, 256)
    with pytest.raises(RuntimeError, match='HIP device'):                    # 16-bit lists on the CPU get as far as fp32 ones
        MultiTensorDiffQuant(w, h, b, 4, 256)
