"""Inputs on which every floating-point reduction of the path has ONE possible fp32 result, whatever the order of the sum --
shared by tests/test_exact_sum_cases_host.py (the proof, the two oracles and libqd_host.so, no GPU) and
tests/test_hip_exact_sums.py (libqd_hip.so, bit for bit).  A plain helper module: no fixtures, nothing runs on import.

tests/errlog.py holds the reductions -- K6 / K6m (the point gradient), the bucket sums of K7 (the STE backward) and
qd_mean_f32 -- to 1e-6 x sum|terms|: right for rounding error, blind to one element that was dropped, doubled or given to the
wrong bin or the wrong bucket's alpha.  Here every term of a sum is an integer multiple of one power of two `unit`, and the
magnitudes of a sum's terms add up to at most 2^24 units (fp32 accumulation; 2^53 for the float64 accumulation of
qd_mean_f32): every partial sum in any order and any tree is then exactly representable, the kernels' sums have to equal the
oracle's bit for bit, and a misplaced term shows as a whole unit.  order_free() states that condition and both test modules
assert it for every case they run; a case that misses it is a bug in the case.

The kernels' launch arithmetic (which kernel a call reaches, its block size, where its loops start and end) is restated here
from csrc/qd_reductions.hip and csrc/qd_multi_dq.hip -- pg_path(), pg_blocks(), pg_geometry() -- only to AIM the cases: the
expected bits never depend on it."""
import collections
import fractions
import functools
import itertools

import numpy as np

from oracle import oracle_np as onp

F32 = np.float32
LIMIT32 = 1 << 24                      # units a sum of fp32 partial sums may reach
LIMIT64 = 1 << 53                      # the same for float64 partial sums
CAPS = (1, 2, 3)                       # qd_set_grid_cap values (tests/grid_trip_cases.py)


# ------------------------------------------------------------------------------------------------ the condition
def lowest_bit_exponent(t):
    """Per element of a float array: the exponent e of the lowest set bit of its significand (t is an odd multiple of
    2^e); +inf for a zero."""
    m, e = np.frexp(np.abs(np.asarray(t, np.float64)))
    M = (m * float(1 << 53)).astype(np.int64)                                 # exact: a 53-bit integer
    low = M & -M
    out = np.full(M.shape, np.inf)
    nz = M != 0
    out[nz] = e[nz] - 53 + np.log2(low[nz].astype(np.float64))               # (log2 of a power of two is exact)
    return out


def unit_of(terms):
    """The largest power of two that divides every term (1.0 when all are zero)."""
    e = lowest_bit_exponent(terms)
    e = e[np.isfinite(e)]
    return float(np.ldexp(1.0, int(e.min()))) if e.size else 1.0


def order_free(terms, group, ngroups, limit=LIMIT32, unit=None):
    """Assert the condition for the sums `group` cuts `terms` into, in float64 and integer arithmetic; returns (unit, the
    largest sum of magnitudes in units).  unit: the case's designed unit, else the largest one the terms allow."""
    t = np.asarray(terms).astype(np.float64).reshape(-1)
    assert np.all(np.isfinite(t))
    unit = unit_of(t) if unit is None else float(unit)
    assert unit > 0 and np.frexp(unit)[0] == 0.5, ('the unit is no power of two', unit)
    q = t / unit                                                              # exact: a division by a power of two ...
    assert np.all(np.abs(q) < 2.0 ** 52) and np.array_equal(q, np.rint(q)), 'a term is no multiple of the unit'   # ... far from underflow
    mags = np.zeros(ngroups, np.int64)
    np.add.at(mags, np.asarray(group).reshape(-1), np.abs(q).astype(np.int64))
    top = int(mags.max()) if mags.size else 0
    assert top <= limit, ('sum|term| / unit = %d > %d: the sum depends on its order' % (top, limit))
    return unit, top


def exact_sums(terms, group, ngroups, dtype=F32):
    """The sums, accumulated in float64 (exact under the condition) and stored as `dtype`; a sum with no term is +0.0."""
    s = np.bincount(np.asarray(group).reshape(-1), weights=np.asarray(terms).astype(np.float64).reshape(-1), minlength=ngroups)
    out = s.astype(dtype)
    assert np.array_equal(out.astype(np.float64), s), 'a sum is not representable: the case misses the condition'
    return out + dtype(0.0)                                                   # (-0.0 + 0.0 = +0.0)


def shuffled_fp32_sums(terms, group, ngroups, seed):
    """The same sums as a running fp32 sum over a random order of each group's terms -- what any kernel's order amounts to."""
    rng = np.random.RandomState(seed)
    group = np.asarray(group).reshape(-1)
    order = np.lexsort((rng.rand(group.size), group))
    t = np.asarray(terms, F32).reshape(-1)[order]
    ends = np.cumsum(np.bincount(group, minlength=ngroups))
    out = np.zeros(ngroups, F32)
    lo = 0
    for j, hi in enumerate(ends):
        if hi > lo:
            out[j] = np.cumsum(t[lo:hi], dtype=F32)[-1]
        lo = hi
    return out + F32(0.0)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def first_difference(got, want):
    d = np.flatnonzero(bits(got).reshape(-1) != bits(want).reshape(-1))
    return [(int(i), float(got.reshape(-1)[i]), float(want.reshape(-1)[i])) for i in d[:6]], int(d.size)


# ------------------------------------------------------------------------------------------------ K6: the point gradient
PG_N = 4 * 3 * 8 * 768 + 4 * 1000 + 3         # 77731: under caps 1 .. 3 every lane makes >= 3 rounds of 8 float4 (tests/test_hip_grid_trips.py)
PG_LENGTHS = (PG_N, PG_N - 1, PG_N - 2)       # n % 4 = 3, 2, 1
PG_BIG_N = (1 << 21) + 3                      # the real 512-block grid, the unrolled loop and the 512-row fold
PG_BUCKETS = (None, 256, 100, 7, 4)           # one alpha; the shift; BucketWalk with 1, 2, 3 elements of a float4 in the first bucket; the smallest walk
PG_K = (2, 4, 5, 16, 17, 64, 65, 128, 129, 256, 512, 513, 1024)
PG_KERNEL_OF_K = {2: 'reg', 4: 'reg', 5: 'lds', 16: 'lds', 17: 'merged', 64: 'merged', 65: 'half', 128: 'half',
                  129: 'turns', 256: 'turns', 512: 'turns', 513: 'any', 1024: 'any'}
PATTERN_ROWS = 32                              # rows of 256 float4 whose indices walk the set partitions
SCALE_EXP = -20                                # the scaled variant: g and alpha both times 2^-20

# the 15 set partitions of {0, 1, 2, 3} as restricted-growth strings: element c of a float4 belongs to block PARTITIONS[p][c]
PARTITIONS = [a for a in itertools.product(range(4), repeat=4)
              if a[0] == 0 and all(a[i] <= max(a[:i]) + 1 for i in range(1, 4))]
assert len(PARTITIONS) == 15


def geometry(n, bucket):
    """(number of buckets, elements per bucket), as the libraries' geometry()."""
    nb, row, _ = onp.bucket_geometry(n, bucket)
    return nb, row


def partition_code(idx4):
    """The set partition the four indices of every float4 realise, as a position in PARTITIONS; idx4: [m, 4]."""
    code = np.zeros(idx4.shape[0], np.int64)
    label = np.zeros(idx4.shape, np.int64)
    for c in range(1, 4):
        lab = np.full(idx4.shape[0], -1, np.int64)
        for d in range(c - 1, -1, -1):                                       # the earliest equal element gives the label
            lab = np.where(idx4[:, d] == idx4[:, c], label[:, d], lab)
        new = label[:, :c].max(axis=1) + 1
        label[:, c] = np.where(lab < 0, new, lab)
    table = {p: i for i, p in enumerate(PARTITIONS)}
    for i, row in enumerate(map(tuple, label)):
        code[i] = table[row]
    return code


def pg_indices(n, k, seed, kind='mixed'):
    """-> (idx as int64, the bin nobody uses or None).  'mixed': the first PATTERN_ROWS x 256 float4s take the 15 set
    partitions in turn -- float4 i the partition (i + i / 256) mod 15, so the float4s of ONE lane position (i mod 256, whatever
    the grid) run through all of them -- on bins that include 0 and k - 1; uniform random indices after that.  'one': every
    element in bin k - 1."""
    if kind == 'one':
        return np.full(n, k - 1, np.int64), None
    rng = np.random.RandomState(seed)
    empty = k // 2 if k >= 3 else None
    allowed = np.array([j for j in range(k) if j != empty], np.int64)
    idx = allowed[rng.randint(0, allowed.size, n)]
    npat = min(n // 4, PATTERN_ROWS * 256)
    i = np.arange(npat)
    mids = allowed[1:-1]
    M = mids.size
    if M >= 2:
        m1 = mids[i % M]
        m2 = mids[(i % M + 1 + (i // M) % (M - 1)) % M]                        # never m1: the offset is 1 .. M - 1
        pal = np.stack([np.zeros(npat, np.int64), np.full(npat, k - 1, np.int64), m1, m2], axis=1)
    else:                                                                    # k <= 4: fewer than four usable bins, blocks share them
        pal = np.stack([allowed[(i + j) % allowed.size] for j in range(4)], axis=1)
    part = np.array(PARTITIONS, np.int64)[(i + i // 256) % 15]               # [npat, 4]: block of every element
    rot = (i // 15) % 4
    idx[:4 * npat] = np.take_along_axis(pal, (part + rot[:, None]) % 4, axis=1).reshape(-1)
    return idx, empty


PgCase = collections.namedtuple('PgCase', 'id n k bucket g idx alpha empty unit')


@functools.lru_cache(maxsize=8)
def _pg_data(n, k, bucket, scaled, kind, small):
    seed = (n * 31 + k * 7 + (bucket or 0)) % (1 << 31)
    rng = np.random.RandomState(seed)
    vals = np.array([-1, 1] if small else [-3, -2, -1, 1, 2, 3], np.float64)
    sc = SCALE_EXP if scaled else 0
    g = np.ldexp(vals[rng.randint(0, vals.size, n)], sc).astype(F32)
    nb, _ = geometry(n, bucket)
    alpha = np.ldexp(1.0, np.arange(nb) % (2 if small else 3) + sc).astype(F32)      # alpha_b != alpha_{b+1} (and != alpha_{b+2} with three values)
    idx, empty = pg_indices(n, k, seed + 1, kind)
    return g, idx, alpha, empty, float(np.ldexp(1.0, 2 * sc))


def pg_case(n, k, bucket, scaled=False, kind='mixed', small=False):
    """g in {+-1, +-2, +-3} (small: {+-1}), alpha_b = 2^(b mod 3) (small: 2^(b mod 2)), both times 2^-20 when scaled."""
    g, idx, alpha, empty, unit = _pg_data(n, k, bucket, scaled, kind, small)
    name = 'k%d-n%d-b%s%s%s%s' % (k, n, bucket, '-scaled' if scaled else '', '-one-bin' if kind == 'one' else '', '-small' if small else '')
    return PgCase(name, n, k, bucket, g, idx, alpha, empty, unit)


def pg_terms(g, alpha, bucket):
    """The terms as the reference forms them: ONE fp32 product g_i alpha_bucket(i) (quant_functions.py:495)."""
    n = g.size
    nb, row = geometry(n, bucket)
    return (g * alpha[np.arange(n) // row]).astype(F32)


def pg_expected(case):
    """-> (expected fp32 sums, terms); asserts the condition (the issue's bound: sum|term| <= 12 n units <= 2^24)."""
    t = pg_terms(case.g, case.alpha, case.bucket)
    assert case.idx.min() >= 0 and case.idx.max() < case.k
    order_free(t, case.idx, case.k, LIMIT32, case.unit)
    want = exact_sums(t, case.idx, case.k)
    if case.empty is not None:
        assert bits(want)[case.empty] == 0 and not np.any(case.idx == case.empty)      # the unused bin: +0.0
    return want, t


def pg_path(k, idx_bytes, n, bucket, g_phase=0, idx_phase=0):
    """Which kernel qd_point_grad_f32 reaches and the threads of its blocks -- the dispatcher's conditions restated.  The fp32
    data needs FOUR-byte alignment only (kDataAlign = 3, csrc/qd_common.h: 16-byte loads take any dword-aligned address), so
    g at +4 bytes stays on the fast kernels; the indices need their own 16 (int64) or 4 (uint8) bytes."""
    nb, row = geometry(max(n, 1), bucket)
    pow2 = nb == 1 or (row & (row - 1)) == 0
    idx_ok = idx_phase % (16 if idx_bytes == 8 else 4) == 0
    fast = k <= 512 and idx_ok and g_phase % 4 == 0 and (nb == 1 or row >= 4)
    if not fast:
        return dict(kernel='any', threads=256 if k <= 64 else 64, columns=256 if k <= 64 else (64 if k <= 512 else 32), U=4, elementwise=True)
    threads = 256 if k <= 128 else (128 if k <= 256 else 64)
    halves = 64 < k <= 128
    lds = 16 if k <= 4 else k * (threads // 2 if halves else threads) * 4
    big = lds > 16 * 1024
    if k <= 4:
        kern = 'reg'
    elif not big:
        kern = 'lds'
    elif halves:
        kern = 'half'
    elif lds <= 64 * 1024:
        kern = 'merged'
    else:
        return dict(kernel='turns', threads=256, U=4 if idx_bytes == 8 else 8, elementwise=False, bk=0 if nb == 1 else (1 if pow2 else 2))
    return dict(kernel=kern, threads=256 if k <= 4 else threads, U=4, elementwise=False, bk=0 if nb == 1 else (1 if pow2 else 2))


def pg_blocks(path, n, k, cap):
    """The grid under a cap of 1 .. 3 blocks (the caps of the compute units' LDS never bind there)."""
    per = path['threads'] * 16 if path['kernel'] == 'any' else 256 * 4 * 2
    return max(1, min(-(-n // per), 512 if path['kernel'] != 'any' else 1 << 30, (1024 * 1024) // k, cap))


def pg_geometry(path, n, k, cap):
    """Where the loops of the kernel start and end under a cap: dict(nth, unrolled = trips of the unrolled loop for the LAST
    block (k_point_grad_fast), tail_first = the first float4 of block 0's per-lane tail loop, rounds = the uniform trip count
    of k_point_grad_turns / _any)."""
    blocks = pg_blocks(path, n, k, cap)
    BS = path['threads']
    nth = blocks * BS
    n4 = n // 4
    if path['kernel'] == 'any':
        return dict(blocks=blocks, nth=nth, rounds=-(-n // (nth * 4)))
    if path['kernel'] == 'turns':
        return dict(blocks=blocks, nth=nth, rounds=-(-n4 // (path['U'] * nth)))

    def trips(bbase):                                                        # for (ub = bbase; ub + 3 nth + BS <= n4; ub += 4 nth)
        room = n4 - 3 * nth - BS - bbase
        return room // (4 * nth) + 1 if room >= 0 else 0
    return dict(blocks=blocks, nth=nth, unrolled=trips((blocks - 1) * BS), tail_first=trips(0) * 4 * nth)


def pg_marker_positions(path, n, k, bucket, cap):
    """At most 24 elements for the one-hot launches: 0, 3, 4; both sides of the bucket edges inside a split float4 (1, 2 and 3
    elements in the first bucket) and of the first aligned one; both sides of a block boundary (4 BS); the first float4 of the
    per-lane tail; 4 (n / 4) - 1; each leftover element; n - 1."""
    geo = pg_geometry(path, n, k, cap)
    BS = path['threads']
    pos = {0, 3, 4, 4 * BS - 1, 4 * BS, 4 * (n // 4) - 1, n - 1}
    pos.update(range(4 * (n // 4), n))
    if 'tail_first' in geo:
        pos.update({4 * geo['tail_first'], 4 * geo['tail_first'] + 3})
    nb, row = geometry(n, bucket)
    if nb > 1:
        seen = set()
        for b in range(1, min(nb, 4 * row + 2)):                             # the first edge of every kind e % 4
            e = b * row
            if e % 4 not in seen and e < n:
                seen.add(e % 4)
                pos.update({e - 1, e})
        last = (nb - 1) * row                                                # the ragged last bucket
        pos.update({last - 1, last})
    pos = sorted(p for p in pos if 0 <= p < n)
    assert len(pos) <= 24, len(pos)
    return pos


def pg_marker_expected(case, e):
    """Bits of alpha[bucket(e)] in bin idx[e], +0.0 in every other bin, for g = 0 but g[e] = 1."""
    _, row = geometry(case.n, case.bucket)
    want = np.zeros(case.k, F32)
    want[case.idx[e]] = case.alpha[e // row]
    return want


# the routes to k_point_grad_any at each of its column widths (256 for k <= 64, 64 for k <= 512, 32 above):
# (k, idx_bytes, g phase, idx phase, bucket) -- the index pointer off its alignment by 8 bytes (int64) or 1 byte (uint8), with g
# at +4 bytes next to it, and buckets of 3 and 2 elements.  (g at +4 bytes ALONE is no route: see pg_path; the fast kernels run
# it, and PG_G_PHASES puts every one of them there.)
def pg_any_routes():
    out = []
    for k in (64, 512, 1024):
        out += [(k, 8, 0, 8, 256), (k, 8, 4, 8, 100), (k, 8, 0, 0, 3), (k, 8, 4, 0, 2)]
    out += [(64, 1, 0, 1, 256), (256, 1, 4, 1, 100), (64, 1, 0, 0, 2), (256, 1, 0, 0, 3)]
    return out


PG_G_PHASES = (4, 12)                          # g this many bytes into a 16-byte granule, on every kernel of the dispatcher


# ------------------------------------------------------------------------------------------------ K6m: the whole model's point gradient
M_K = (4, 16, 64, 65, 256)
M_BUCKETS = (256, 100, None)
M_BASE = (1, 3, 1023, 1024, 1025, 2053, 4096, 7 * 1024 + 1000)
M_BIG = 2049 * 1024 + 17                       # its tiles wrap the 2048 waves: min(c, W) + 1 rows, the wrapped row index
M_BIG_AT = 40
M_EMPTY = (0, 66, 67, 136)                     # first, two in a row in the middle, last
M_TENSORS = 137                                # >= 129: owner_of_tile needs a third ballot group, and tensors 131 .. 135 own full tiles
M_WAVES, M_TILE = 2048, 1024


def m_sizes():
    s = [M_BASE[i % len(M_BASE)] for i in range(M_TENSORS)]
    for i in M_EMPTY:
        s[i] = 0
    s[M_BIG_AT] = M_BIG
    return s


MCase = collections.namedtuple('MCase', 'k bucket sizes g idx alpha want')


@functools.lru_cache(maxsize=4)
def m_case(k, bucket):
    """The tensor list with K6's term construction; want[i]: the exact bits of tensor i's gradient (asserted order-free)."""
    sizes = m_sizes()
    gs, idxs, alphas, wants = [], [], [], []
    for i, n in enumerate(sizes):
        if n == 0:
            gs.append(np.zeros(0, F32)); idxs.append(np.zeros(0, np.int64)); alphas.append(np.zeros(0, F32)); wants.append(np.zeros(k, F32))
            continue
        rng = np.random.RandomState(1000 + i)
        small = n == M_BIG
        vals = np.array([-1, 1] if small else [-3, -2, -1, 1, 2, 3], np.float64)
        g = vals[rng.randint(0, vals.size, n)].astype(F32)
        nb, _ = geometry(n, bucket)
        alpha = np.ldexp(1.0, (np.arange(nb) + i) % (2 if small else 3)).astype(F32)
        idx, _ = pg_indices(n, k, 2000 + i)
        t = pg_terms(g, alpha, bucket)
        order_free(t, idx, k, LIMIT32, 1.0)
        gs.append(g); idxs.append(idx); alphas.append(alpha); wants.append(exact_sums(t, idx, k))
    return MCase(k, bucket, sizes, gs, idxs, alphas, wants)


def m_marker_positions(sizes):
    """(tensor, element): the last element of a tensor and the first of the next; a tensor's last full tile and its remainder;
    in the large tensor the first tile its wave comes back to and the ends of its last full tile."""
    out = []
    for i in (5, 6, 7, 8, 133, 134, 135):                                     # 2053, 4096, 8168, then 1 | ... 2053, 4096, 8168 in the third ballot group
        n = sizes[i]
        full = n // M_TILE * M_TILE
        out += [(i, n - 1), (i, 0)]
        if 0 < full < n:
            out += [(i, full - 1), (i, full)]
    big = M_BIG_AT
    out += [(big, 0), (big, M_WAVES * M_TILE - 1), (big, M_WAVES * M_TILE), (big, 2049 * M_TILE - 1), (big, 2049 * M_TILE), (big, M_BIG - 1),
            (big + 1, 0), (big - 1, sizes[big - 1] - 1)]
    return sorted(set(p for p in out if sizes[p[0]] > 0))


# ------------------------------------------------------------------------------------------------ K7: the bucket sums of the STE backward
STE_LEVELS = ((5, 8), (17, 4), (257, 2))       # (s, den): the level table; the computed division twice
STE_VEC_ROWS = ((64, 199), (128, 199), (256, 199), (512, 50), (1024, 50))     # (row, full buckets): the register tiles, >= 3 trips under cap 3
STE_WAVE_ROWS = ((100, 38), (513, 38), (4097, 38))                            # ste_wave_bucket
STE_SCALES = (0, -70, -104)
# x times 2^-70: alpha = (s - 1) 2^-70 is below the reference's 1e-10 (quant_functions.py:40), so scale_down sets alpha = 1 and
# every element quantizes to level 0 -- no alpha in [2^-60, 1e-10) exists, and the IEEE division is reached through the OTHER
# clause of scale_fast_ok: a numerator x - beta_q in (0, 2^-100), which x times 2^-104 gives.
STE_TIES = ('reference', 'true_arg')

SteCase = collections.namedtuple('SteCase', 'id n s bucket x g')


@functools.lru_cache(maxsize=8)
def ste_case(s, den, bucket, nfull, tail, scale_exp=0):
    """x a multiple of 1 / den in [0, s - 1] (times 2^scale_exp), every bucket of two or more elements -- the ragged last one
    too -- holding a 0 and an s - 1; g in {+-1 .. +-4}."""
    n = nfull * bucket + tail
    rng = np.random.RandomState((s * 131 + bucket * 7 + n) % (1 << 31))
    x = rng.randint(0, (s - 1) * den + 1, n).astype(np.float64) / den
    for b in range(-(-n // bucket) if n >= bucket else 1):
        lo, hi = b * bucket, min((b + 1) * bucket, n)
        if hi - lo >= 2:
            a, c = rng.choice(hi - lo, 2, replace=False)
            x[lo + a], x[lo + c] = 0.0, s - 1
    vals = np.array([-4, -3, -2, -1, 1, 2, 3, 4], np.float64)
    g = vals[rng.randint(0, 8, n)].astype(F32)
    if scale_exp:
        # every term is then g x 2^scale_exp: next to a g of 1 .. 4 the sum S would vanish in the two final additions g +- S and the
        # output would show nothing of it.  g = 0 at the first maximum and the first minimum of every bucket -- where tie mode
        # 'true_arg' adds and subtracts S -- makes the output there +S and -S themselves.
        for b in range(-(-n // bucket) if n >= bucket else 1):
            lo, hi = b * bucket, min((b + 1) * bucket, n)
            g[lo + int(np.argmax(x[lo:hi]))] = 0.0
            g[lo + int(np.argmin(x[lo:hi]))] = 0.0
    x = np.ldexp(x, scale_exp).astype(F32)
    return SteCase('s%d-b%d-n%d-2^%d' % (s, bucket, n, scale_exp), n, s, bucket, x, g)


def ste_expected(case, tie_mode):
    """-> the whole output and dict(unit, top, touched, sums); asserts that every bucket's terms are order-free, so that S has
    one possible value."""
    tm = onp.ste_bucket_terms(case.x, case.g, case.s, case.bucket, tie_mode)
    nb, row = tm['nb'], tm['row']
    n = case.n
    # the terms once more, as ste_bucket_terms forms them (it returns only their sums)
    q = onp.uniform_quantize(case.x, case.s, case.bucket)['q'].reshape(-1)
    sdq = onp.scale_down(q, case.bucket)
    qs = sdq['u'].reshape(-1)[:n]
    aq = np.repeat(sdq['alpha'].reshape(-1), row)[:n]
    bq = np.repeat(sdq['beta'].reshape(-1), row)[:n]
    u = ((case.x - bq).astype(F32) / aq).astype(F32)
    term = (case.g * (qs - u).astype(F32)).astype(F32)
    group = np.arange(n) // row
    unit, top = order_free(term, group, nb)
    sb = exact_sums(term, group, nb)
    assert np.array_equal(sb.astype(np.float64), tm['sb'])
    # out = g, + S at jmax, - S at jmin: ONE fp32 addition each, at two different places of a bucket -- no order to depend on
    touched = tm['jmax'] != tm['jmin']
    lo = np.arange(nb) * row
    out = case.g.copy()
    jx, jn = (lo + tm['jmax'])[touched], (lo + tm['jmin'])[touched]
    out[jx] = (out[jx] + sb[touched]).astype(F32)
    out[jn] = (out[jn] - sb[touched]).astype(F32)
    return out, dict(unit=unit, top=top, touched=int(touched.sum()), sums=sb)


def ste_shapes():
    """(bucket, full buckets, tail, what): the register tiles with their ragged last bucket behind them, the wave-per-bucket
    rows, and a tensor shorter than a bucket."""
    out = [(row, nfull, row - 1, 'vec') for row, nfull in STE_VEC_ROWS]
    out += [(row, nfull, 1 + row % 3, 'wave') for row, nfull in STE_WAVE_ROWS]
    out += [(256, 0, 77, 'short'), (100, 0, 1, 'one')]
    return out


# the list MultiTensorSTE runs: (level row of STE_LEVELS, full buckets, tail); bucket sizes 256 and 100
MSTE_TENSORS = ((0, 4, 3), (1, 9, 0), (2, 0, 0), (0, 12, 255), (1, 2, 1), (2, 8, 0), (0, 1, 0), (1, 0, 50), (2, 5, 99), (0, 0, 0), (1, 13, 2),
                (2, 3, 98), (0, 7, 0))


# ------------------------------------------------------------------------------------------------ qd_mean_f32
MEAN_N = (1, 3, 4, 8191, 8192, 8193, (1 << 20) + 3)


@functools.lru_cache(maxsize=8)
def mean_data(n):
    """x a multiple of 2^-10 with |x| < 2^10."""
    rng = np.random.RandomState(n % 9973)
    return (rng.randint(-(1 << 20) + 1, 1 << 20, n).astype(np.float64) / 1024.0).astype(F32)


def round_once_to_f32(q):
    """The fp32 nearest to the rational q, ties to even -- one rounding, in integer arithmetic."""
    q = fractions.Fraction(q)
    c = F32(float(q))
    cands = sorted({float(np.nextafter(c, F32(-np.inf))), float(c), float(np.nextafter(c, F32(np.inf)))})
    best = min(cands, key=lambda v: (abs(fractions.Fraction(v) - q), int(np.array([v], F32).view(np.uint32)[0]) & 1))
    return F32(best)


def mean_expected(x):
    """include/qd_hip.h: 'float64 accumulation, one rounding'.  The sum is exact (asserted); its quotient by n is rounded once
    to fp32 in integer arithmetic, and the case is required to give the same bits when the quotient passes through float64 on
    its way (what both libraries do), so the two readings of the header cannot differ on it."""
    n = x.size
    order_free(x, np.zeros(n, np.int64), 1, LIMIT64, 2.0 ** -10)
    total = int(np.rint(x.astype(np.float64) * 1024.0).astype(np.int64).sum())
    want = round_once_to_f32(fractions.Fraction(total, 1024 * n))
    via64 = F32(np.float64(total / 1024.0) / np.float64(n))
    assert bits(np.array([want]))[0] == bits(np.array([via64]))[0], 'a double-rounding case: choose other data'
    return want
