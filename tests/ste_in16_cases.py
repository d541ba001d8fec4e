"""Cases of the one-launch STE backward on fp16 / bf16 gradients (qd_multi_ste_in16_plan / qd_multi_ste_backward_in16_f32,
MultiTensorSTE with 16-bit grads).  Nothing runs on import; tests/test_ste_in16_cases_host.py proves the tables on the CPU,
tests/test_hip_ste_in16.py runs them on the device.

16-bit data travels as numpy uint16 PATTERNS (numpy has no bfloat16); widen() is numpy's own widening of them, to_patterns()
torch's CPU rounding of fp32 values.  The yardstick of every device test is the fp32 launch on widened gradients, bit for bit
on the fp32 patterns, NaN for NaN where a NaN is expected."""
import numpy as np

F32 = np.float32
FORMATS = ('float16', 'bfloat16')
GRAD_KIND = {'float16': 1, 'bfloat16': 2}                # QD_GRAD_F16, QD_GRAD_BF16 (include/qd_hip.h)
BUCKETS = (64, 128, 256, 512, 1024, 100)                 # the five register rows of QD_STE_SHAPES and one generic row
BUCKETS_PER_TILE = {64: 4, 128: 4, 256: 4, 512: 1, 1024: 1}
G_PHASES = tuple(range(0, 16, 2))                        # bytes into a 16-byte granule: every 2-byte phase of g
F_PHASES = (0, 4, 8, 12)                                 # every 4-byte phase of x and out
PER_TENSOR_S = (2, 4, 16, 256, 5)                        # cycling: both sides of the 16-level table
MIN_TILES = 37                                           # under a cap of 3 blocks (12 waves): at least three trips per wave

# 16-bit pattern -> fp32 pattern of its exact widening.  Subnormals are kept, the sign of zero is kept, +-inf stays.
WIDENING = {
    'float16': ((0x0001, 0x33800000),        # the smallest subnormal, 2^-24
                (0x03FF, 0x387FC000),        # the largest subnormal
                (0x0400, 0x38800000),        # the smallest normal, 2^-14
                (0x7BFF, 0x477FE000),        # the largest finite, 65504
                (0x8000, 0x80000000),        # -0
                (0x7C00, 0x7F800000),        # +inf
                (0xFC00, 0xFF800000)),       # -inf
    'bfloat16': ((0x0001, 0x00010000),       # the smallest subnormal (an fp32 subnormal too)
                 (0x007F, 0x007F0000),       # the largest subnormal
                 (0x0080, 0x00800000),       # the smallest normal
                 (0x7F7F, 0x7F7F0000),       # the largest finite
                 (0x8000, 0x80000000),
                 (0x7F80, 0x7F800000),
                 (0xFF80, 0xFF800000)),
}
NAN16 = {'float16': 0x7E00, 'bfloat16': 0x7FC0}          # a quiet NaN of each format (the guard bands around g)
INF16 = {'float16': 0x7C00, 'bfloat16': 0x7F80}


def torch_dtype(fmt):
    import torch
    return {'float16': torch.float16, 'bfloat16': torch.bfloat16}[fmt]


def widen(patterns, fmt):
    """numpy's own widening of uint16 patterns to fp32."""
    p = np.ascontiguousarray(patterns, np.uint16)
    if fmt == 'float16':
        return p.view(np.float16).astype(F32)
    return (p.astype(np.uint32) << 16).view(F32)


def to_patterns(values, fmt):
    """fp32 values rounded to the format by torch on the CPU, as uint16 patterns."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(values, F32)).to(torch_dtype(fmt))
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def assert_same32(got, want, tag):
    """Bit for bit on the fp32 patterns; where the expectation is a NaN, a NaN."""
    got, want = np.ascontiguousarray(got, F32).reshape(-1), np.ascontiguousarray(want, F32).reshape(-1)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (tag, 'NaN positions', np.flatnonzero(np.isnan(got) != nan)[:8])
    bad = np.flatnonzero((bits(got) != bits(want)) & ~nan)
    assert bad.size == 0, (tag, 'first difference at', int(bad[0]), hex(int(bits(got)[bad[0]])), hex(int(bits(want)[bad[0]])))


# ---------------------------------------------------------------- the tile rule, restated (include/qd_hip.h)
def tiles_of(n, bucket):
    """Tiles of one tensor whose x and out are 4-byte aligned: what qd_multi_ste_in16_plan counts whatever g's alignment."""
    if n == 0:
        return 0
    row = min(n, bucket)
    nb = -(-n // row)
    per_tile = BUCKETS_PER_TILE.get(row)
    if per_tile is None or nb == 1:
        return nb
    nfull = n // row
    return -(-nfull // per_tile) + (nb - nfull)


def sizes(bucket):
    """The parity list's element counts: around one and two buckets, one full register tile and one bucket more, a tensor of
    several tiles with a ragged end, then padding until the tile count is at least MIN_TILES and no multiple of 4, and a
    trailing empty tensor."""
    B = bucket
    out = [0, 1, B - 1, B, B + 1, 2 * B, 2 * B + 1]
    if BUCKETS_PER_TILE.get(B) == 4:
        out += [4 * B, 5 * B - 1]
    out += [9 * B + 3]
    pad = [3 * B + 7, B + 2, 2 * B - 1]
    i = 0
    while True:
        total = sum(tiles_of(n, B) for n in out)
        if total >= MIN_TILES and total % 4:
            break
        out.append(pad[i % 3])
        i += 1
    return out + [0]


def total_tiles(bucket):
    return sum(tiles_of(n, bucket) for n in sizes(bucket))


def parity_tensors(bucket, fmt, seed=0):
    """[(x fp32, g as uint16 patterns)] of sizes(bucket): randn weights, randn gradients rounded to the format."""
    out = []
    for i, n in enumerate(sizes(bucket)):
        rng = np.random.RandomState(1000 * seed + 17 * i + bucket)
        out.append((rng.randn(n).astype(F32), to_patterns(rng.randn(n).astype(F32), fmt)))
    return out


# ---------------------------------------------------------------- the widening table as tensors
def widening_case(fmt, bucket):
    """x constant inside every bucket (the quantized bucket is constant, jmax == jmin, the kernel passes g through untouched)
    and g cycling through the table's patterns: (x, g patterns, expected fp32 patterns).  Several register tiles and a ragged
    last bucket, so both bodies pass every pattern."""
    n = 6 * bucket + 5
    x = np.repeat(np.arange(1, 8, dtype=F32) * F32(0.5), bucket)[:n].copy()
    table = WIDENING[fmt]
    idx = (np.arange(n) * 3) % len(table)
    g = np.array([table[i][0] for i in idx], np.uint16)
    want = np.array([table[i][1] for i in idx], np.uint32)
    return x, g, want


# ---------------------------------------------------------------- non-finite inputs
def nonfinite_cases(fmt, bucket):
    """[(name, x, g patterns)]: a bucket of x holding a NaN / +inf (its S is NaN at the first NaN of the quantized bucket), and g
    holding NaN, +inf and -inf at touched (the bucket's extremes) and untouched positions.  Register tiles and a ragged tail."""
    n = 5 * bucket + bucket // 2 + 1
    rng = np.random.RandomState(bucket + len(fmt))
    x0 = rng.randn(n).astype(F32)
    g0 = to_patterns(rng.randn(n).astype(F32), fmt)
    out = []
    for name, v in (('x NaN', np.nan), ('x +inf', np.inf)):
        x = x0.copy()
        x[bucket + 7] = v                    # a register-tile bucket
        x[5 * bucket + 3] = v                # the ragged last bucket
        out.append((name, x, g0.copy()))
    for name, p in (('g NaN', NAN16[fmt]), ('g +inf', INF16[fmt]), ('g -inf', INF16[fmt] | 0x8000)):
        g = g0.copy()
        for b in (0, 2, 5):                  # two register-tile buckets and the ragged one
            lo, hi = b * bucket, min((b + 1) * bucket, n)
            g[lo + int(np.argmax(x0[lo:hi]))] = p                    # touched: + S lands here
            mid = lo + (hi - lo) // 2
            mid += int(mid == lo + int(np.argmax(x0[lo:hi])) or mid == lo + int(np.argmin(x0[lo:hi])))
            g[mid] = p                                               # untouched: passed through
        g[3 * bucket + int(np.argmin(x0[3 * bucket:4 * bucket]))] = p    # touched: - S
        out.append((name, x0.copy(), g))
    return out
