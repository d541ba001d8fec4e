"""The cases of the one-launch symbolizer (qd_multi_symbols_plan, qd_multi_uniform_symbols_u8; MultiTensorSymbols) -- shared by
tests/test_symbol_cases_host.py (the plan, the expected bits from libqd_host.so held to a numpy statement of the reference's
operations; no GPU) and tests/test_hip_symbols.py (the kernel, bit for bit).  A plain helper module: no fixtures, nothing runs
on import.

The tensors are the 17 of bucket_cases.Q_CASES, imported and not edited: they reach every one of the five bodies (registers,
float4 on a DPP row, element by element on a DPP row, the wave per bucket in its vector and scalar form), with ragged last rows,
4-byte phases of x, n < bucket, n == bucket, an empty tensor mid-list, a single element and a 70000-element row on one wave.
Added here: a byte phase of `sym` per tensor, and a second assignment of level counts."""
import ctypes
import functools

import numpy as np

import bucket_cases as B

F32 = np.float32
CASES = B.Q_CASES
BUCKETS = [c.bucket for c in CASES]
# bytes past a 16-byte boundary at which tensor i's symbols start: the phases cycle through the list, under the second level
# assignment four positions further on -- between the two every vector body (a packed 4-symbol store) meets a sym that is 4-byte
# aligned and one that is not (the register rows are tensors 2, 6 and 8, the float4 DPP row is tensor 10: the plain cycle gives
# them 2, 15, 1 and 3; four positions on, tensor 8 sits at 8 and tensor 10 at 0)
SYM_PHASES = (0, 1, 2, 3, 5, 8, 15)
PHASE_SHIFT = {'ladder': 0, 'rotated': 4}
LADDER2 = (2, 3, 16, 255, 256)          # bucket_cases.LEVELS with 4 -> 3 and 17 -> 255
# 'ladder': the level counts of the cases (2, 4, 16, 17, 256 in turn); 'rotated': the ladder moved on by one position with 4
# replaced by 3 and 17 by 255 -- every body then meets both sides of the 16-level table and 255 / 256
LEVELS = {'ladder': [c.s for c in CASES], 'rotated': [LADDER2[(i + 1) % 5] for i in range(len(CASES))]}
VARIANTS = ('finite', 'nonfinite')


def sym_phase(i, assign='ladder'):
    return SYM_PHASES[(i + PHASE_SHIFT[assign]) % len(SYM_PHASES)]


def data(i, variant):
    return B.q_data(i, variant)


def plan_rule(ns=None, buckets=None):
    """(first_tile, first_bucket, total_tiles, total_buckets) under the restated tile rule (bucket_cases.q_rule)."""
    ns = [c.n for c in CASES] if ns is None else ns
    buckets = BUCKETS if buckets is None else buckets
    ft, fb, t, b = [], [], 0, 0
    for n, bk in zip(ns, buckets):
        r = B.q_rule(n, bk)
        ft.append(t)
        fb.append(b)
        t += r['tiles']
        b += r['nb']
    return ft, fb, t, b


def check_paths():
    """The cases reach every body, and every float4 body (a packed store) with an aligned and an unaligned sym."""
    B.check_paths()
    seen = set()
    for i, c in enumerate(CASES):
        r = B.q_rule(c.n, c.bucket, aligned=c.phase == 0)
        if r['full'] in ('reg', 'lanes4<16>', 'wave lanes4'):
            seen.update((r['full'], sym_phase(i, a) % 4 == 0) for a in LEVELS)
    assert seen == {(p, a) for p in ('reg', 'lanes4<16>', 'wave lanes4') for a in (True, False)}, seen
    for name, lv in LEVELS.items():
        assert len(lv) == len(CASES) and all(2 <= s <= 256 for s in lv)
    for body in B.Q_PATHS:          # a body that more than one tensor reaches: a level count <= 16 and one above, and 255 or 256
        mine = [i for i, c in enumerate(CASES) if body in (c.full, c.ragged)]
        both = {lv[i] for lv in LEVELS.values() for i in mine}
        if len(mine) > 1:           # (the float4 DPP row is tensor 10 alone: 2 and 3 levels; nothing in a body depends on the count)
            assert min(both) <= 16 < max(both) and both & {255, 256}, (body, both)
        assert len(both) > 1, (body, both)


# ------------------------------------------------------------------------------------------------ the reference's operations
def numpy_symbols(x, s, bucket):
    """(sym uint8 [n], alpha [nb], beta [nb]) by the reference's operations, each rounded to fp32 on its own:
    alpha = max - min (< 1e-10: 1), beta = min per bucket row of min(n, bucket) elements (a NaN makes both NaN, as torch's
    min / max do), level = rint(((x - beta) / alpha) * (s - 1)), a NaN level stored as 0."""
    x = np.asarray(x, F32).reshape(-1)
    n = x.size
    if n == 0:
        return np.zeros(0, np.uint8), np.zeros(0, F32), np.zeros(0, F32)
    row = min(n, bucket)
    nb = -(-n // row)
    alpha, beta, sym = np.empty(nb, F32), np.empty(nb, F32), np.empty(n, np.uint8)
    with np.errstate(all='ignore'):
        for k in range(nb):
            v = x[k * row:min((k + 1) * row, n)]
            mn, mx = F32(np.min(v)), F32(np.max(v))             # numpy's min / max propagate NaN
            a = F32(mx - mn)
            if a < F32(1e-10):
                a = F32(1.0)
            alpha[k], beta[k] = a, mn
            u = ((v - mn).astype(F32) / a).astype(F32)
            lev = np.rint((u * F32(s - 1)).astype(F32))
            sym[k * row:k * row + v.size] = np.where(np.isnan(lev), 0, lev).astype(np.int64).astype(np.uint8)
    return sym, alpha, beta


def numpy_dequantize(sym, alpha, beta, s, n, bucket):
    """(sym / (s - 1)) * alpha + beta, each operation rounded to fp32: what the decoders of a compressed file compute."""
    if n == 0:
        return np.zeros(0, F32)
    row = min(n, bucket)
    k = np.arange(n) // row
    with np.errstate(all='ignore'):
        w = (sym.astype(F32) / F32(s - 1)).astype(F32)
        return ((w * alpha[k]).astype(F32) + beta[k]).astype(F32)


# ------------------------------------------------------------------------------------------------ the expected bits
def host_symbols(x, s, bucket):
    """(sym, alpha, beta) of libqd_host.so's qd_uniform_f32 with its level output: the call the contract names."""
    from quantized_distillation_amd import _lib
    x = np.ascontiguousarray(x, F32).reshape(-1)
    n = x.size
    nb = B.q_rule(n, bucket)['nb']
    sym, alpha, beta, q = np.full(n, 0xA5, np.uint8), np.full(nb, 777.0, F32), np.full(nb, 777.0, F32), np.empty(n, F32)
    if n:
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)       # noqa: E731
        rc = _lib.host().qd_uniform_f32(p(x), p(q), n, bucket, s, p(alpha), p(beta), p(sym), None, 0, 0.0, 0, 0, None, 0, None)
        assert rc == 0, rc
    return sym, alpha, beta


@functools.lru_cache(maxsize=None)
def expected(i, variant, assign):
    """What tensor i of the launch has to hold: computed once, shared, read-only.  tests/test_symbol_cases_host.py holds every
    one of them to numpy_symbols() and, through numpy_dequantize(), to uniformQuantization."""
    out = host_symbols(data(i, variant), LEVELS[assign][i], CASES[i].bucket)
    for a in out:
        a.setflags(write=False)
    return out


def same_f32(a, b):
    return B.same(a, b)
