"""The cases of the one-launch quantizer and STE backward with a bucket size PER TENSOR (qd_multi_buckets_plan,
qd_multi_uniform_buckets_f32, qd_multi_ste_buckets_plan, qd_multi_ste_backward_buckets_f32) -- shared by
tests/test_bucket_cases_host.py (the plans, the expected bits from libqd_host.so held to the numpy oracle; no GPU) and
tests/test_hip_multi_buckets.py (the kernels, bit for bit).  A plain helper module: no fixtures, nothing runs on import.

Every case is (n, bucket, s), a data recipe, the 4-byte phase it sits at inside a 16-byte granule and the PATH it is meant to
reach.  q_rule() / ste_rule() restate the tile rule of csrc/qd_multi.h (bucket_tiles) and of ste_cut (csrc/qd_ste.hip) in
Python; check_paths() asserts for every case that the restated rule sends it where the case says, so a case that silently lands
on another body fails on the CPU.  The shapes are the smallest that reach each path: a few thousand elements, but for the one
row longer than 64 Ki elements."""
import collections
import functools

import numpy as np

import exact_sum_cases as E
from oracle import oracle_np as onp

F32 = np.float32
M64 = 0xFFFFFFFFFFFFFFFF
LEVELS = (2, 4, 16, 17, 256)            # both sides of the 16-level table, the smallest, no power of two, the uint8 limit
SEED0 = 0xFFFFFFFFFFFFFFFA              # tensor 6 and the ones behind it wrap past 2^64
MAX_ELEMENT = 0.5
OPTIONS = {'det': dict(), 'clamp': dict(max_element=MAX_ELEMENT), 'stoch': dict(stochastic_rounding=True)}
STE_ROWS = {64: 16, 128: 16, 256: 16, 512: 64, 1024: 64}      # QD_STE_SHAPES: row -> lanes per bucket


def same(a, b):
    """Bit for bit on the int32 views, NaN positions equal (a NaN's payload is not part of any contract here)."""
    a, b = np.ascontiguousarray(a, F32).reshape(-1), np.ascontiguousarray(b, F32).reshape(-1)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb]))


# ------------------------------------------------------------------------------------------------ the tile rules, restated
def q_rule(n, bucket, aligned=True):
    """The quantizer: dict(row, nb, tiles, full, ragged) -- `full` the body of the full rows, `ragged` of a ragged last row
    (None: there is none).  aligned: x and q both 16-byte aligned."""
    if n <= 0:
        return dict(row=0, nb=0, tiles=0, full=None, ragged=None)
    row = min(n, bucket)
    nb = -(-n // row)
    has_full, has_ragged = n // row > 0, n % row != 0
    if row <= 256:
        tiles = -(-nb // 4)
        full = ('reg' if row in (64, 128, 256) else 'lanes4<16>') if aligned and row % 4 == 0 else 'row16'
        ragged = 'row16'
    else:
        tiles = nb
        full = 'wave lanes4' if aligned and row % 4 == 0 else 'wave scalar'
        ragged = 'wave scalar'
    return dict(row=row, nb=nb, tiles=tiles, full=full if has_full else None, ragged=ragged if has_ragged else None)


def ste_rule(n, bucket):
    """The STE backward (ste_cut: fp32 pointers are 4-byte aligned, which is all the register path asks for): dict(row, nb,
    nfull, vtiles, tiles, full, ragged)."""
    if n <= 0:
        return dict(row=0, nb=0, nfull=0, vtiles=0, tiles=0, full=None, ragged=None)
    row = min(n, bucket)
    nb = -(-n // row)
    if row in STE_ROWS and n > row:
        nfull = n // row
        vtiles = -(-nfull // (64 // STE_ROWS[row]))
        return dict(row=row, nb=nb, nfull=nfull, vtiles=vtiles, tiles=vtiles + nb - nfull, full='vec', ragged='wave' if nb > nfull else None)
    return dict(row=row, nb=nb, nfull=0, vtiles=0, tiles=nb, full='wave', ragged=None)


# ------------------------------------------------------------------------------------------------ the quantizer's cases
QCase = collections.namedtuple('QCase', 'id n bucket s phase full ragged')       # phase: floats past a 16-byte boundary


def _q_cases():
    table = [                                                                  # (n, bucket, phase, full rows, ragged row)
        (2 * 70000, 70000, 0, 'wave lanes4', None),                            # the long-row loop: > 64 Ki elements on one wave
        (40, 1, 0, 'row16', None),
        (4 * 256, 256, 0, 'reg', None),
        (1, 3, 0, 'row16', None),                                              # a single element (n < bucket: row 1)
        (5 * 576 + 10, 576, 0, 'wave lanes4', 'wave scalar'),
        (0, 16, 0, None, None),                                                # empty, mid-list
        (3 * 128 + 5, 128, 0, 'reg', 'row16'),
        (3 * 1001, 1001, 0, 'wave scalar', None),
        (9 * 64, 64, 0, 'reg', None),
        (300, 4096, 0, 'wave lanes4', None),                                   # n < bucket: one row of 300
        (1000, 100, 0, 'lanes4<16>', None),
        (2049, 2049, 0, 'wave scalar', None),                                  # n == bucket
        (37 * 7 + 3, 7, 0, 'row16', 'row16'),
        # the same bodies' unaligned siblings: 4, 8 and 12 bytes into a granule every full row falls back to the scalar body
        (5 * 256 + 7, 256, 1, 'row16', 'row16'),
        (3 * 576, 576, 2, 'wave scalar', None),
        (600, 100, 3, 'row16', None),
        (2 * 64, 64, 1, 'row16', None),
    ]
    return [QCase('n%d-b%d-s%d-ph%d' % (n, b, LEVELS[i % 5], ph), n, b, LEVELS[i % 5], ph, full, ragged)
            for i, (n, b, ph, full, ragged) in enumerate(table)]


Q_CASES = _q_cases()
Q_PATHS = ('reg', 'lanes4<16>', 'row16', 'wave lanes4', 'wave scalar')


@functools.lru_cache(maxsize=None)
def q_data(i, variant='finite'):
    """The input of quantizer case i.  'finite': normal values, sigma 0.4 (the 0.5 clamp bites), one constant bucket where the
    tensor has three or more (the alpha guard).  'nonfinite': the same with a NaN in the first bucket, +inf in the second (three
    or more buckets) and -inf in the last one (two or more: the ragged row where there is one)."""
    c = Q_CASES[i]
    x = (0.4 * np.random.RandomState(4000 + i).randn(c.n)).astype(F32)
    r = q_rule(c.n, c.bucket)
    if r['nb'] >= 3:
        x[2 * r['row']:min(3 * r['row'], c.n)] = F32(0.25)
    if variant == 'nonfinite' and c.n:
        x[min(r['row'], c.n) // 2] = np.nan
        if r['nb'] >= 3:
            x[r['row'] + 1] = np.inf
        if r['nb'] >= 2:
            x[c.n - 1] = -np.inf
    x.setflags(write=False)
    return x


def oracle_q(i, variant, opt):
    """The numpy oracle of quantizer case i at (bucket_i, s_i), seed SEED0 + i."""
    c, x = Q_CASES[i], q_data(i, variant)
    if c.n == 0:
        return np.zeros(0, F32)
    me = OPTIONS[opt].get('max_element', False)
    if 'stochastic_rounding' not in OPTIONS[opt]:
        return onp.uniform_quantize(x, c.s, c.bucket, max_element=me)['q'].reshape(-1)
    r = q_rule(c.n, c.bucket)
    rand = np.zeros(r['nb'] * r['row'], F32)                                   # the bucket layout: the padding draws nothing
    rand[:c.n] = onp.philox4x32_7_uniform((SEED0 + i) & M64, c.n)
    return onp.uniform_quantize_stochastic(x, c.s, rand, c.bucket, max_element=me)['q'].reshape(-1)


@functools.lru_cache(maxsize=None)
def expected_q(i, variant, opt):
    """What tensor i of the launch has to hold, bit for bit: qd_uniform_f32 of libqd_host.so at (bucket_i, s_i) with seed
    SEED0 + i.  tests/test_bucket_cases_host.py holds every one of them to oracle_q()."""
    import ctypes
    from quantized_distillation_amd import _lib
    c = Q_CASES[i]
    x = np.ascontiguousarray(q_data(i, variant))
    q = np.full(c.n, 777.0, F32)
    if c.n:
        me = OPTIONS[opt].get('max_element', False)
        rc = _lib.host().qd_uniform_f32(x.ctypes.data_as(ctypes.c_void_p), q.ctypes.data_as(ctypes.c_void_p), c.n, c.bucket, c.s,
                                        None, None, None, None, 0 if me is False else 1, float(me),
                                        int('stochastic_rounding' in OPTIONS[opt]), (SEED0 + i) & M64, None, 0, None)
        assert rc == 0, rc
    q.setflags(write=False)
    return q


# ------------------------------------------------------------------------------------------------ the STE backward's cases
SteCase = collections.namedtuple('SteCase', 'id n bucket s den phase full ragged')
STE_EXACT_LEVELS = ((2, 8), (5, 8), (17, 4), (257, 2))
# (s, den) of exact_sum_cases.ste_case: s - 1 a power of two, so that every term g (qs - u) is a multiple of one power of two
# and a bucket's sum has ONE fp32 value whatever its order -- the only inputs on which the host library, the oracle and the
# kernels must agree in every bit.  (The mixed level counts 2, 4, 16, 17, 256 run on random data against the per-tensor device
# call: tests/test_hip_multi_buckets.py.)


def _ste_cases():
    table = [                                                                  # (full buckets, tail, bucket, phase, full, ragged)
        (5, 0, 64, 0, 'vec', None),
        (5, 0, 576, 0, 'wave', None),
        (2, 1, 128, 0, 'vec', 'wave'),
        (0, 0, 16, 0, None, None),                                             # empty
        (4, 0, 256, 0, 'vec', None),
        (0, 300, 4096, 0, 'wave', None),                                       # n < bucket
        (3, 7, 512, 0, 'vec', 'wave'),
        (7, 0, 100, 0, 'wave', None),
        (2, 0, 1024, 0, 'vec', None),
        # 4 x 256 at a 4-byte phase.  fp32 data needs FOUR-byte alignment for the register path (kDataAlign, ste_cut) and an
        # fp32 tensor always has it: no misalignment of a float tensor leaves ste_vec_tile, and this case pins that the tiles
        # of an off-phase tensor are still the register tiles (its loads are then unaligned 16-byte ones).
        (4, 0, 256, 1, 'vec', None),
        (3, 5, 64, 3, 'vec', 'wave'),
    ]
    out = []
    for i, (nfull, tail, b, ph, full, ragged) in enumerate(table):
        s, den = STE_EXACT_LEVELS[i % 4]
        out.append(SteCase('n%d-b%d-s%d-ph%d' % (nfull * b + tail, b, s, ph), nfull * b + tail, b, s, den, ph, full, ragged))
    return out


STE_CASES = _ste_cases()


@functools.lru_cache(maxsize=None)
def ste_data(i):
    """(x, g) of STE case i, built as exact_sum_cases.ste_case builds them."""
    c = STE_CASES[i]
    if c.n == 0:
        return np.zeros(0, F32), np.zeros(0, F32)
    nfull, tail = (c.n // c.bucket, c.n % c.bucket) if c.n >= c.bucket else (0, c.n)
    k = E.ste_case(c.s, c.den, c.bucket, nfull, tail)
    assert k.n == c.n
    return k.x, k.g


@functools.lru_cache(maxsize=None)
def expected_ste(i, tie_mode):
    """The exact output of STE case i (exact_sum_cases.ste_expected asserts that every bucket's sum is order-free)."""
    c = STE_CASES[i]
    if c.n == 0:
        return np.zeros(0, F32)
    x, g = ste_data(i)
    out, info = E.ste_expected(E.SteCase(c.id, c.n, c.s, c.bucket, x, g), tie_mode)
    assert info['touched'] > 0
    return out


def host_ste(i, tie_mode):
    """qd_ste_bucket_backward_f32 of libqd_host.so on STE case i."""
    import ctypes
    from quantized_distillation_amd import _lib
    c = STE_CASES[i]
    x, g = (np.ascontiguousarray(a) for a in ste_data(i))
    out = np.full(c.n, 777.0, F32)
    if c.n:
        p = [a.ctypes.data_as(ctypes.c_void_p) for a in (x, g, out)]
        rc = _lib.host().qd_ste_bucket_backward_f32(p[0], p[1], p[2], c.n, c.bucket, c.s, 0 if tie_mode == 'reference' else 1, None)
        assert rc == 0, rc
    return out


# ------------------------------------------------------------------------------------------------ every case reaches its path
def check_paths():
    """Each case lands where it says under the restated rules, and the lists reach every body."""
    seen = set()
    for c in Q_CASES:
        r = q_rule(c.n, c.bucket, aligned=c.phase == 0)
        assert (r['full'], r['ragged']) == (c.full, c.ragged), (c.id, r)
        seen.update(p for p in (r['full'], r['ragged']) if p)
    assert seen == set(Q_PATHS), seen ^ set(Q_PATHS)
    assert any(c.n > 65536 and q_rule(c.n, c.bucket)['row'] > 65536 for c in Q_CASES)
    assert any(c.n == 0 for c in Q_CASES[1:-1]) and sorted(set(c.s for c in Q_CASES)) == sorted(LEVELS)
    rows = set()
    for c in STE_CASES:
        r = ste_rule(c.n, c.bucket)
        assert (r['full'], r['ragged']) == (c.full, c.ragged), (c.id, r)
        if r['full'] == 'vec':
            rows.add(r['row'])
    assert rows == set(STE_ROWS), rows
