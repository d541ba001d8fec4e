"""Linear and Embedding from packed weights (include/qd_infer.h, libqd_infer.so): the case list, built on the CPU and shared by
tests/test_packed_layer_cases_host.py (no GPU: the cases against the oracle and against themselves) and
tests/test_hip_packed_layers.py (the library on the device).  A plain helper module: nothing runs on import but small tables.

A weight case is one packed 2-D weight: `packed` is the numpy reference of the stream (codec_bits_cases.pack_stream) of the
ORACLE's levels, alpha and beta are the oracle's, and `w` is the weight value of the header computed in numpy fp32, one
rounding per operation:  w = ((c / (s - 1)) * alpha[k] + beta[k]) + 0.0.  test_packed_layer_cases_host.py holds w to the
oracle's q bit for bit.

Linear expectations are of two kinds.
  general   |y - y64| <= 1e-6 (sum_c |x w| + |bias|), y64 the float64 dot product of x with the bit-exact w: the project's
            reduction rule (tests/errlog.py).  Non-finite outputs must be non-finite in the same way.
  exact     bit for bit, the idiom of tests/exact_sum_cases.py: s - 1 is a power of two, every bucket holds its own minimum and
            maximum with alpha = (s - 1) 2^j and beta a multiple of 2^j, x and bias are small integers.  Every term is then
            an integer multiple of one power of two U, and sum |terms| < 2^24 U: every partial sum in every order is exact, so
            the result does not depend on the order and fmaf gives what multiply-then-add gives.  exact_condition() asserts it.

Shapes: the smallest at which each thing can go wrong (see SHAPES); one m, one count and one phase per weight case, rotated so
that every width meets every m, every count and every phase."""
import collections
import functools

import numpy as np

from codec_bits_cases import pack_stream, packed_bytes, unpack_stream
from oracle import oracle_c as oc

F32 = np.float32
BITS = (1, 2, 3, 4, 5, 6, 7, 8)
TOL = 1e-6                                   # errlog.TOL: the project's reduction rule
MS = (1, 2, 3, 8, 9, 17)                     # full and ragged m-tiles: 1, 2, 4 (3 of 4), 8, 8 + 1, 8 + 8 + 1
COUNTS = (1, 5, 300)
PHASES = (0, 4, 8, 12)                       # of x, y and out inside a 16-byte granule
EXACT_S = (2, 3, 5, 9, 17, 33, 65, 129)      # s - 1 a power of two, one per width
BIG = 10 ** 6                                # a bucket larger than every tensor here

# (rows, cols, bucket): what each is there for
SHAPES = (
    (67, 37, 256),       # rows start mid-word at every width and mid-byte at 3, 5, 6, 7 bits; buckets straddle rows; > one block of rows, ragged
    (67, 100, 256),      # buckets straddle rows at another stride
    (67, 32, 64),        # rows word aligned at every width, two rows per bucket
    (67, 5, 3),          # cols below a lane group; several buckets inside a group of four
    (67, 1, 100),        # one column: every group is ragged
    (3, 2085, 256),      # 64 * 32 + 37 columns: later trips of the column loop
    (3, 37, None),       # no buckets
    (3, 37, BIG),        # a bucket larger than the tensor: one bucket
    (1, 37, 3),          # one row
    (1, 100, 64),
    (3, 32, 100),        # a bucket size that is no power of two
    (67, 37, 100),
    (1, 2085, 100),
    (3, 100, 3),
    (3, 5, 64),          # fewer elements than one bucket
)
EXACT_SHAPES = ((67, 37, 256), (3, 2085, 256), (67, 100, 100), (3, 37, None), (67, 5, 3), (1, 100, 64), (3, 32, BIG))

Weight = collections.namedtuple('Weight', 'tag rows cols bucket s bits W lev packed alpha beta w q')


def levels_for(bits):
    """The two level counts of a width: the one that fills it and the smallest that needs it."""
    return (1 << bits, (1 << (bits - 1)) + 1)


def nbuckets(n, bucket):
    return 1 if (bucket is None or n < bucket) else -(-n // bucket)


def bucket_of(n, bucket):
    """The bucket of every flat element."""
    return np.zeros(n, np.int64) if (bucket is None or n < bucket) else np.arange(n, dtype=np.int64) // bucket


def weight_value(lev, s, alpha, beta, bucket):
    """The header's four operations in numpy fp32, each rounded on its own (numpy's float32 division is correctly rounded)."""
    k = bucket_of(lev.size, bucket)
    with np.errstate(invalid='ignore', over='ignore'):
        t = lev.astype(F32) / F32(s - 1)
        t = t * alpha.astype(F32)[k]
        t = t + beta.astype(F32)[k]
        return (t + F32(0.0)).astype(F32)


def _freeze(*arrays):
    for a in arrays:
        a.flags.writeable = False


def _weight(tag, rows, cols, bucket, s, bits, W):
    n = rows * cols
    with np.errstate(invalid='ignore'):
        r = oc.uniform_quantize(W.reshape(-1), s, bucket, want_idx=False)
    lev = r['lev'].reshape(-1)[:n].astype(np.uint8)
    packed = pack_stream(lev, bits)
    assert packed.size == packed_bytes(n, bits) and np.array_equal(unpack_stream(packed, n, bits), lev)
    alpha, beta = r['alpha'].reshape(-1).astype(F32), r['beta'].reshape(-1).astype(F32)
    assert alpha.size == beta.size == nbuckets(n, bucket)
    w = weight_value(lev, s, alpha, beta, bucket).reshape(rows, cols)
    q = r['q'].reshape(-1)[:n].reshape(rows, cols).astype(F32)
    _freeze(W, lev, packed, alpha, beta, w, q)
    return Weight(tag, rows, cols, bucket, s, bits, W, lev, packed, alpha, beta, w, q)


@functools.lru_cache(maxsize=None)
def general_weight(rows, cols, bucket, s, bits, nonfinite=False):
    """Gaussian weights of a scale per case.  nonfinite: a NaN in the first bucket (alpha NaN) and +inf in the last (alpha inf)."""
    seed = 1000 + 131 * rows + 17 * cols + 7 * bits + s + (bucket or 0) % 1000
    rng = np.random.RandomState(seed % (2 ** 31))
    W = (rng.randn(rows, cols) * (0.05 + 0.01 * bits)).astype(F32)
    if nonfinite:
        flat = W.reshape(-1)
        flat[min(5, flat.size - 1)] = np.nan
        flat[flat.size - 2] = np.inf
    tag = 'general %dx%d bucket %s s %d bits %d%s' % (rows, cols, bucket, s, bits, ' non-finite' if nonfinite else '')
    return _weight(tag, rows, cols, bucket, s, bits, W)


@functools.lru_cache(maxsize=None)
def exact_weight(rows, cols, bucket, bits):
    """s - 1 = 2^(bits - 1); bucket k: levels with a 0 and an s - 1 in it, alpha = (s - 1) 2^j, beta = b 2^j, j in {-1, 0, 1}."""
    s = EXACT_S[bits - 1]
    n = rows * cols
    rng = np.random.RandomState(5000 + 131 * rows + 17 * cols + bits)
    k = bucket_of(n, bucket)
    nb = nbuckets(n, bucket)
    lev = rng.randint(0, s, n)
    first = np.searchsorted(k, np.arange(nb))
    size = np.bincount(k, minlength=nb)
    assert size.min() >= 2, 'every bucket (the ragged last one too) needs two elements to hold its own minimum and maximum'
    lev[first] = 0
    lev[first + 1 + rng.randint(0, 10 ** 6, nb) % (size - 1)] = s - 1
    j = rng.randint(-1, 2, nb)
    b = rng.randint(-4, 5, nb)
    W = (lev * np.exp2(j)[k] + (b * np.exp2(j))[k]).astype(F32).reshape(rows, cols)          # exact in fp32: small dyadic numbers
    wt = _weight('exact %dx%d bucket %s s %d bits %d' % (rows, cols, bucket, s, bits), rows, cols, bucket, s, bits, W)
    assert np.array_equal(wt.lev, lev) and np.array_equal(wt.alpha, ((s - 1) * np.exp2(j)).astype(F32)) \
        and np.array_equal(wt.beta, (b * np.exp2(j)).astype(F32)), 'the oracle quantizes the constructed weight to its own levels'
    assert np.array_equal(wt.w, W), 'the weight value of an exact case is the constructed weight itself'
    return wt


# ---------------------------------------------------------------- inputs of the layers
@functools.lru_cache(maxsize=None)
def linear_inputs(cols, rows, m, seed, exact=False, nan_row=False):
    """(x [m, cols], bias [rows]).  exact: integers in [-2, 2] and [-8, 8]; nan_row: one NaN in the LAST row of x."""
    rng = np.random.RandomState(9000 + seed)
    if exact:
        x = rng.randint(-2, 3, (m, cols)).astype(F32)
        bias = rng.randint(-8, 9, rows).astype(F32)
    else:
        x = rng.randn(m, cols).astype(F32)
        bias = (rng.randn(rows) * 0.5).astype(F32)
    if nan_row:
        x[m - 1, cols // 2] = np.nan
    _freeze(x, bias)
    return x, bias


def linear_expected(w, x, bias):
    """(y64, sum |terms|): the float64 dot products of x with the bit-exact w (+ bias), and the magnitude the bound scales with."""
    w64, x64 = w.astype(np.float64), x.astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        # term by term: 0 x inf must be NaN exactly where IEEE makes it one (a matrix product may take other routes)
        terms = x64[:, None, :] * w64[None, :, :]
        y = terms.sum(axis=2)
        mag = np.abs(terms).sum(axis=2)
        if bias is not None:
            y = y + bias.astype(np.float64)[None, :]
            mag = mag + np.abs(bias.astype(np.float64))[None, :]
    return y, mag


def check_linear(got, y64, mag, tag, record=None):
    """got [m, rows] fp32 against the bound; non-finite expectations must be met in kind (NaN for NaN, the same infinity).
    record: errlog.check_sum, to log the achieved ratio; returns that ratio over the finite outputs."""
    got = np.asarray(got, F32).reshape(y64.shape)
    fin = np.isfinite(y64)
    assert np.array_equal(np.isnan(got), np.isnan(y64)), (tag, 'NaN where IEEE arithmetic gives none, or none where it gives one')
    inf = np.isinf(y64)
    assert np.array_equal(got[inf].astype(np.float64), y64[inf]), (tag, 'infinite outputs')
    g, w, a = got[fin].astype(np.float64), y64[fin], mag[fin]
    if record is not None:
        return record('packed_linear', g, w, a, tag, tol=TOL)
    err = np.abs(g - w)
    nz = a > 0
    ratio = float(np.max(err[nz] / a[nz])) if nz.any() else 0.0
    assert np.all(err[~nz] == 0), (tag, 'a sum with no non-zero term must be exactly 0')
    assert ratio <= TOL, (tag, 'error / sum|terms| = %.3g > %.1g' % (ratio, TOL))
    return ratio


def exact_condition(wt, x, bias):
    """The condition under which a Linear result is free of its order: every term x w and the bias are integer multiples of
    U = 2^-1 (w is lev 2^j + b 2^j with j >= -1, x and bias are integers), and sum |terms| + |bias| < 2^24 U per output."""
    U = 0.5
    w64, x64 = wt.w.astype(np.float64), x.astype(np.float64)
    assert np.all(w64 / U == np.rint(w64 / U)) and np.all(x64 == np.rint(x64)) and np.all(bias == np.rint(bias))
    mag = np.abs(x64) @ np.abs(w64).T + np.abs(bias.astype(np.float64))[None, :]
    assert mag.max() < 2.0 ** 24 * U, (wt.tag, mag.max())
    return True


@functools.lru_cache(maxsize=None)
def embedding_indices(rows, count, seed):
    """count indices with repeats; -1 and `rows` (the only two out-of-range values used) among them from 5 indices up."""
    rng = np.random.RandomState(7000 + seed)
    idx = rng.randint(0, rows, count).astype(np.int64)
    if count >= 2:
        idx[count // 2] = idx[0]                               # a repeat whatever the draw
    if count >= 5:
        idx[1], idx[count - 2] = -1, rows
    _freeze(idx)
    return idx


def embedding_expected(w, idx):
    out = np.full((idx.size, w.shape[1]), np.nan, F32)
    ok = (idx >= 0) & (idx < w.shape[0])
    out[ok] = w[idx[ok]]
    return out


def same_floats(got, want):
    """Bit for bit, a NaN for a NaN (the header leaves a NaN's sign and payload open)."""
    got, want = np.asarray(got, F32).reshape(-1), np.asarray(want, F32).reshape(-1)
    if got.shape != want.shape:
        return False
    diff = got.view(np.uint32) != want.view(np.uint32)
    return not (diff & ~(np.isnan(got) & np.isnan(want))).any()


# ---------------------------------------------------------------- the case list
Case = collections.namedtuple('Case', 'weight m count phase exact nan_row seed')


def general_cases(bits):
    """Every shape at both level counts of the width; m, count and phase rotate with the shape and the level count."""
    out = []
    for si, s in enumerate(levels_for(bits)):
        if s < 2:
            continue
        for hi, (rows, cols, bucket) in enumerate(SHAPES):
            k = hi + si * 5 + bits
            out.append(Case(general_weight(rows, cols, bucket, s, bits), MS[k % 6], COUNTS[k % 3], PHASES[k % 4], False, False, k))
    return out


def nonfinite_cases(bits):
    """A NaN bucket, an inf bucket and a NaN in the last row of x: buckets across rows, and one bucket for the tensor."""
    s = 1 << bits
    return [Case(general_weight(67, 37, 256, s, bits, True), 9, 300, 4, False, True, 40 + bits),
            Case(general_weight(3, 37, None, s, bits, True), 3, 5, 8, False, True, 50 + bits)]


def exact_cases(bits):
    out = []
    for hi, (rows, cols, bucket) in enumerate(EXACT_SHAPES):
        k = hi + bits
        out.append(Case(exact_weight(rows, cols, bucket, bits), MS[k % 6], COUNTS[k % 3], PHASES[(k + 1) % 4], True, False, 100 + k))
    return out


def all_cases(bits):
    return general_cases(bits) + nonfinite_cases(bits) + exact_cases(bits)


def inputs_of(c):
    """(x, bias or None, idx) of a case; every third case runs without a bias."""
    wt = c.weight
    x, bias = linear_inputs(wt.cols, wt.rows, c.m, c.seed, c.exact, c.nan_row)
    return x, (None if (c.seed % 3 == 0 and not c.exact) else bias), embedding_indices(wt.rows, c.count, c.seed)
