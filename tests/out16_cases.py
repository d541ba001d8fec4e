"""Rounding cases of the 16-bit outputs of the one-launch quantizer (qd_multi_uniform_out16_f32 / _global_out16_f32): small fp32
tensors whose QUANTIZED values are known exactly, so that the fp32 -> fp16 / bf16 conversion of the store meets ties, the top of
each format, the first value that overflows to inf, fp16 subnormals, negative values (and a negative zero), a NaN and an inf.

How a value is placed on the output.  A bucket that holds only 0 and one value v quantizes to exactly {0, v} at any level
count s: for v > 0 alpha = v - 0 = v, beta = 0, so 0 -> level 0 -> 0 * alpha + beta = 0 and v -> u = 1 -> level s - 1 ->
1 * alpha + beta = v; for v < 0 alpha = 0 - v, beta = v, so v -> level 0 -> beta = v and 0 -> u = 1 -> alpha + beta = +0.  Every
v here is above the 1e-10 guard on alpha.  u is exactly 0 or 1, so stochastic rounding draws but never moves a value.  Each
case is a tensor of N = 1024 elements, 0 at the even positions and v at the odd ones: every bucket of 64, 100 (its ragged last
one too), 128 or 256 elements holds both, and without buckets the tensor is one full tile.

A plain helper module (no fixtures, nothing runs on import).  tests/test_out16_cases_host.py proves the table on CPU tensors
(libqd_host.so and torch's .to(dtype)); tests/test_hip_out16.py runs it on the device."""
import numpy as np

F32 = np.float32
N = 1024
BUCKETS = (64, 100, 128, 256, None)
LEVELS = (2, 16, 17, 256)              # both sides of the 16-level table


def f32_of_bits(bits):
    return np.array([bits], np.uint32).view(F32)[0]


def _exact():
    """(name, v, {'float16': pattern, 'bfloat16': pattern}): the pattern the format named must show for v (None: not pinned
    by hand for that format -- the conversion of the fp32 result is the expectation there, as everywhere)."""
    two = lambda e: F32(2.0) ** F32(e)
    rows = [
        # bf16 keeps 8 significant bits: 1 + 2^-8 lies halfway between 1 (even) and 1 + 2^-7; 1 + 3 * 2^-8 halfway between
        # 1 + 2^-7 (odd) and 1 + 2^-6 (even)
        ('bf16 tie down', F32(1.0) + two(-8), None, 0x3F80),
        ('bf16 tie up', F32(1.0) + F32(3.0) * two(-8), None, 0x3F82),
        ('bf16 largest finite', f32_of_bits(0x7F7F0000), None, 0x7F7F),
        ('bf16 first to inf', f32_of_bits(0x7F7FFFFF), 0x7C00, 0x7F80),
        # fp16 keeps 11 significant bits
        ('fp16 tie down', F32(1.0) + two(-11), 0x3C00, None),
        ('fp16 tie up', F32(1.0) + F32(3.0) * two(-11), 0x3C02, None),
        ('fp16 largest finite', F32(65504.0), 0x7BFF, None),
        ('fp16 first to inf', F32(65520.0), 0x7C00, None),
        # fp16 subnormals: the smallest one, the tie below it (to even: zero), and three quarters of it (up)
        ('fp16 smallest subnormal', two(-24), 0x0001, None),
        ('fp16 subnormal tie to zero', two(-25), 0x0000, None),
        ('fp16 subnormal round up', F32(1.5) * two(-25), 0x0001, None),
    ]
    out = []
    for name, v, h, b in rows:
        out.append((name, F32(v), {'float16': h, 'bfloat16': b}))
        neg = {k: (None if p is None else p | 0x8000) for k, p in (('float16', h), ('bfloat16', b))}
        out.append(('negative ' + name, F32(-v), neg))          # ('negative fp16 subnormal tie to zero': a negative zero)
    return out


EXACT = _exact()
assert len(EXACT) == 22


def tensor_of(v):
    x = np.zeros(N, F32)
    x[1::2] = v
    return x


def nonfinite():
    """(name, x): a tensor whose bucket 1 (of 256; bucket 4 .. 5 of 64) holds a NaN, and one that holds +inf there -- the fp32
    launch turns that bucket (without buckets: the tensor) into NaN; the 16-bit outputs must be NaN in the same places."""
    a = tensor_of(F32(0.75))
    a[300] = np.nan
    b = tensor_of(F32(-0.75))
    b[301] = np.inf
    return [('a NaN', a), ('+inf', b)]


def all_tensors():
    """Every tensor of the table, in order: the exact cases, then the two non-finite ones."""
    return [(name, tensor_of(v)) for name, v, _ in EXACT] + nonfinite()


def patterns(t16):
    """The 16-bit patterns of a torch fp16 / bf16 tensor as a numpy uint16 array."""
    import torch
    return t16.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def assert_same16(got, want, tag):
    """got, want: torch tensors of one 16-bit dtype.  Equal bit for bit where `want` is no NaN, NaN for NaN elsewhere."""
    import torch
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, want.dtype, got.shape, want.shape)
    g, w = got.detach().cpu(), want.detach().cpu()
    nan = torch.isnan(w)
    assert bool(torch.equal(torch.isnan(g), nan)), (tag, 'NaNs in other places: %d against %d' % (int(torch.isnan(g).sum()), int(nan.sum())))
    gp, wp = patterns(g), patterns(w)
    diff = (gp != wp) & ~nan.numpy()
    assert not diff.any(), (tag, '%d of %d elements differ, first at %d: 0x%04X != 0x%04X'
                            % (diff.sum(), diff.size, np.flatnonzero(diff)[0], gp[diff][0], wp[diff][0]))
