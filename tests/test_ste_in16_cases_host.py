"""tests/ste_in16_cases.py proven without a GPU, and everything of the 16-bit-gradient STE that needs no device: the widening
table against torch and numpy, the exact-sum gradients surviving both 16-bit types, qd_multi_ste_in16_plan against
qd_multi_ste_plan (g's alignment has no say), the exported symbols and their declarations."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

import exact_sum_cases as E
import ste_in16_cases as C
from quantized_distillation_amd import _lib
from quantized_distillation_amd import build as qb

BASE = 0x7f0000001000           # a 4 KiB-aligned fake address: the plans only look at the pointers' alignment
STRIDE = 1 << 24


@pytest.fixture(scope='module')
def lib():
    qb.build_extension()
    return _lib.load()


# ---------------------------------------------------------------- 1. the widening table
@pytest.mark.parametrize('fmt', C.FORMATS)
def test_the_widening_table_is_torchs_and_numpys_widening(fmt):
    pats = np.array([p for p, _ in C.WIDENING[fmt]], np.uint16)
    want = np.array([w for _, w in C.WIDENING[fmt]], np.uint32)
    by_torch = torch.from_numpy(pats.view(np.int16).copy()).view(C.torch_dtype(fmt)).float().numpy()
    assert np.array_equal(C.bits(by_torch), want), [hex(v) for v in C.bits(by_torch)]
    assert np.array_equal(C.bits(C.widen(pats, fmt)), want), [hex(v) for v in C.bits(C.widen(pats, fmt))]
    assert len(pats) == 7
    # what the rows are meant to be
    vals = C.widen(pats, fmt).astype(np.float64)
    if fmt == 'float16':
        assert vals[0] == 2.0 ** -24 and vals[1] == 1023 * 2.0 ** -24 and vals[2] == 2.0 ** -14 and vals[3] == 65504.0
    else:
        assert vals[0] == 2.0 ** -133 and vals[1] == 127 * 2.0 ** -133 and vals[2] == 2.0 ** -126
    assert vals[4] == 0 and np.signbit(vals[4]) and vals[5] == np.inf and vals[6] == -np.inf
    for f in C.FORMATS:
        assert np.isnan(C.widen([C.NAN16[f]], f)[0]) and C.widen([C.INF16[f]], f)[0] == np.inf


@pytest.mark.parametrize('fmt', C.FORMATS)
@pytest.mark.parametrize('bucket', C.BUCKETS)
def test_the_widening_case_passes_every_pattern_through_both_bodies(fmt, bucket):
    x, g, want = C.widening_case(fmt, bucket)
    assert np.array_equal(C.bits(C.widen(g, fmt)), want)
    for lo in range(0, x.size, bucket):
        assert np.unique(x[lo:lo + bucket]).size == 1                       # constant buckets: nothing is touched
    pats = {p for p, _ in C.WIDENING[fmt]}
    assert set(g[:bucket].tolist()) == pats and set(g[6 * bucket:].tolist()) <= pats and x.size % bucket == 5
    lanes = 16 if bucket <= 256 else 64
    if bucket in C.BUCKETS_PER_TILE:                                        # every lane of a register bucket sees a subnormal
        first = np.array([p for p, _ in C.WIDENING[fmt]], np.uint16)[:2]
        assert np.isin(g[:bucket], first).reshape(-1, lanes, 4).any(axis=(0, 2)).sum() >= lanes // 2


# ---------------------------------------------------------------- 2. the exact-sum gradients are 16-bit numbers
def test_the_exact_sum_gradients_survive_both_16_bit_types():
    cases = []
    for bucket, nfull, tail, _ in E.ste_shapes():
        for s, den in E.STE_LEVELS:
            for scale in E.STE_SCALES:
                cases.append(E.ste_case(s, den, bucket, nfull, tail, scale))
    for bucket in (256, 100):
        cases += [E.ste_case(E.STE_LEVELS[r][0], E.STE_LEVELS[r][1], bucket, nfull, t) for r, nfull, t in E.MSTE_TENSORS]
    for c in cases:
        assert set(np.unique(c.g).tolist()) <= {-4.0, -3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0, 4.0}, c.id
        for fmt in C.FORMATS:
            assert np.array_equal(C.bits(C.widen(C.to_patterns(c.g, fmt), fmt)), C.bits(c.g)), (c.id, fmt)


# ---------------------------------------------------------------- 3. the plan
def table(ns, g_phase=0, f_phase=0, g_bytes=2):
    T = (_lib.QdSteDesc * len(ns))()
    for i, n in enumerate(ns):
        T[i].x = BASE + (3 * i) * STRIDE + f_phase
        T[i].g = BASE + (3 * i + 1) * STRIDE + g_phase
        T[i].out = BASE + (3 * i + 2) * STRIDE + f_phase
        T[i].n = n
    return T


def plan(fn, T, bucket):
    total = ctypes.c_int64(-7)
    rc = fn(T, len(T), bucket, ctypes.byref(total))
    return rc, total.value, [T[i].first_tile for i in range(len(T))]


@pytest.mark.parametrize('bucket', C.BUCKETS)
def test_the_in16_plan_is_the_fp32_plan_of_an_aligned_gradient(lib, bucket):
    ns = C.sizes(bucket)
    assert ns[-1] == 0 and ns[0] == 0 and C.total_tiles(bucket) >= C.MIN_TILES and C.total_tiles(bucket) % 4
    for f_phase in C.F_PHASES:
        want = plan(lib.qd_multi_ste_plan, table(ns, 0, f_phase), bucket)
        assert want[0] == 0 and want[1] == C.total_tiles(bucket)
        assert want[2] == [sum(C.tiles_of(n, bucket) for n in ns[:i]) for i in range(len(ns))]
        for g_phase in C.G_PHASES:
            assert plan(lib.qd_multi_ste_in16_plan, table(ns, g_phase, f_phase), bucket) == want, (bucket, f_phase, g_phase)
    # (the fp32 plan itself gives a 2-byte-aligned g one tile per bucket: the reason for a plan of its own; rows 512 and 1024
    # hold one bucket per register tile, so only the body differs there, not the count)
    if C.BUCKETS_PER_TILE.get(bucket) == 4:
        assert plan(lib.qd_multi_ste_plan, table(ns, 2, 0), bucket)[1] > C.total_tiles(bucket)


def test_the_in16_plan_refusals(lib):
    total = ctypes.c_int64(0)
    fn = lib.qd_multi_ste_in16_plan
    for odd in (1, 3, 15):
        T = table([100, 200])
        T[1].g = BASE + STRIDE + odd
        assert fn(T, 2, 256, ctypes.byref(total)) == -1, odd
        T[1].n = 0                                  # an empty tensor's pointers are not looked at
        assert fn(T, 2, 256, ctypes.byref(total)) == 0 and total.value == 1
    T = table([100, 200])
    assert fn(None, 2, 256, ctypes.byref(total)) == -1
    assert fn(T, 2, 0, ctypes.byref(total)) == -1
    assert fn(T, 2, -256, ctypes.byref(total)) == -1
    assert fn(T, 2, 256, None) == -1
    assert fn(T, 0, 256, ctypes.byref(total)) == -1
    T[1].n = -1
    assert fn(T, 2, 256, ctypes.byref(total)) == -1
    T[1].n = 200
    for field in ('x', 'g', 'out'):
        T = table([100, 200])
        setattr(T[1], field, None)
        assert fn(T, 2, 256, ctypes.byref(total)) == -1, field
        T[1].n = 0
        assert fn(T, 2, 256, ctypes.byref(total)) == 0 and total.value == 1


def test_the_launch_checks_its_arguments_before_any_launch(lib):
    fake = ctypes.c_void_p(BASE)                    # never dereferenced on the host: every call below returns before a launch
    fn = lib.qd_multi_ste_backward_in16_f32
    for kind in (0, 3, -1):
        assert fn(fake, fake, 4, 10, 256, kind, 0, None) == -1
    assert fn(None, fake, 4, 10, 256, 1, 0, None) == -1
    assert fn(fake, None, 4, 10, 256, 1, 0, None) == -1
    assert fn(fake, ctypes.c_void_p(BASE + 2), 4, 10, 256, 1, 0, None) == -1          # levels: 4-byte aligned
    assert fn(fake, fake, 0, 10, 256, 1, 0, None) == -1
    assert fn(fake, fake, 4, -1, 256, 1, 0, None) == -1
    assert fn(fake, fake, 4, 10, 0, 1, 0, None) == -1
    assert fn(fake, fake, 4, 10, 256, 1, 2, None) == -1                               # unknown tie mode
    assert fn(fake, fake, 4, 10, 256, 2, -1, None) == -1
    assert fn(fake, fake, 4, 0, 256, 1, 1, None) == 0 and fn(fake, fake, 4, 0, 100, 2, 0, None) == 0      # nothing to do


# ---------------------------------------------------------------- 4. symbols and declarations
def test_both_symbols_are_exported_and_declared_with_the_headers_argument_lists(lib):
    names = ('qd_multi_ste_in16_plan', 'qd_multi_ste_backward_in16_f32')
    syms = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    header = open(_lib.INCLUDE + '/qd_hip.h').read()
    ctype_of = [(r'QdSteDesc\s*\*', ('LP_QdSteDesc', 'c_void_p')), (r'int32_t\s*\*', ('c_void_p',)), (r'int64_t\s*\*', ('LP_c_long', 'LP_c_int64')),
                (r'void\s*\*', ('c_void_p',)), (r'int64_t', ('c_long', 'c_int64')), (r'int', ('c_int',))]
    for name in names:
        assert re.search(r'\bT %s\b' % name, syms), name
        assert name not in _lib.HOST_SYMBOLS                                 # device library only
        m = re.search(r'\bint %s\(([^)]*)\);' % name, header)
        assert m, name
        args = [a.strip() for a in m.group(1).replace('\n', ' ').split(',')]
        res, decl = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(decl) == len(args), (name, args, decl)
        for a, d in zip(args, decl):
            a = a.replace('const ', '')
            want = next(names_ for pat, names_ in ctype_of if re.match(pat, a))
            assert d.__name__ in want, (name, a, d.__name__)
        assert getattr(lib, name).argtypes == list(decl)
    assert re.search(r'#define QD_GRAD_F16 1\b', header) and re.search(r'#define QD_GRAD_BF16 2\b', header)
    assert C.GRAD_KIND == {'float16': 1, 'bfloat16': 2}
    assert re.search(r'#define QD_ABI_VERSION 3\b', header) and lib.qd_abi_version() == 3


def test_gradient_dtype_rules_come_before_any_device_is_needed():
    from quantized_distillation_amd.multi_tensor import MultiTensorSTE
    w = [torch.zeros(300), torch.zeros(10)]
    h = [torch.zeros(300, dtype=torch.float16), torch.zeros(10, dtype=torch.float16)]
    b = [torch.zeros(300, dtype=torch.bfloat16), torch.zeros(10, dtype=torch.bfloat16)]
    for mixed in ([h[0], b[1]], [h[0], w[1]], [w[0], b[1]]):
        with pytest.raises(TypeError, match='one dtype'):
            MultiTensorSTE(w, mixed, 16, 256)
    with pytest.raises(RuntimeError, match='HIP device'):                    # 16-bit gradients on the CPU get as far as fp32 ones
        MultiTensorSTE(w, h, 16, 256)
