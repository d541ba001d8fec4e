"""Nearest-point assignment on ties and crowded points: the cases and their reference (numpy only, no torch).

qd_nearest_point_f32 has two assignment rules, and each is DEFINED by how it breaks a tie (include/qd_hip.h):

  distance  i = searchsorted(points, u, 'left').clip(max=k - 1), then one step down iff u is STRICTLY closer to the lower point
            (quant_functions.py:267-273);
  midpoint  #{ fp32 midpoints <= u }, a midpoint being p[j] + (p[j + 1] - p[j]) / 2 rounded at every step (:531-573).

Random points and random data never meet on a point, a midpoint or a cell boundary, so a kernel with `<` for `<=` passes every
random test.  Here at least half of the elements of every case sit EXACTLY on a point, a midpoint, a boundary of the 256-cell
or the 2048-cell table, or on the fp32 neighbour of one of those, and the point sets are the ones the device's cell tables can
go wrong on: all points in one fine cell, duplicates, points on cell boundaries, points outside [0, 1], a bell-shaped crowd.

  * reference:   ref_scale / ref_index / ref_q below, written from the reference lines; anchored to the reference program by
                 tests/golden/nonuniform.npz (tests/test_nearest_cases_host.py)
  * cases:       raw_case (prescaled == 0: x is built so that u = (x - beta) / alpha is exact), prescaled_case, multi_case
  * geometries:  ROWS -- one row per kernel the launcher can reach, the kernel named in the row and held to qd_transform_plan
                 on the CPU (check_rows_against_the_plan): a row that drifts to another kernel fails there, not silently

tests/test_nearest_cases_host.py runs every case through libqd_host.so, tests/test_hip_nearest_ties.py through libqd_hip.so.
"""
import collections
import functools
import re

import numpy as np

F = np.float32
DISTANCE, MIDPOINT = 0, 1                     # QD_ASSIGN_DISTANCE, QD_ASSIGN_MIDPOINT
RULES = (DISTANCE, MIDPOINT)
# both sides of 32 (small table / cell tables), 64 (the vector kernel's fine table), 256 (an index byte), and kMaxPoints
K = (1, 2, 3, 5, 16, 31, 32, 33, 64, 65, 200, 256, 257, 1000, 1024)
L = 1 << 16                                   # the points' lattice j / L: every midpoint is exact, on the lattice j / (2 L)
SETS = ('one cell', 'dups', 'cell bounds', 'outside', 'bell', 'uniform', 'full precision')
SETS_PER_ROW = 4                              # of the seven, rotating with k and the row: every row meets every set
TINY = F(2.0 ** -126)                         # smallest normal fp32


# ---------------------------------------------------------------------------------------------------------- the reference
def midpoints(pts):
    """k[:-1] + np.diff(k) / 2 in fp32, every step rounded (quant_functions.py:533)."""
    return (pts[:-1] + np.diff(pts) / F(2)).astype(F)


def other_midpoints(pts):
    """(p + q) / 2: NOT the reference's midpoint.  Equal to it on the lattice sets; where it differs, the smaller of the two is a
    u that tells a kernel with this form from one with the reference's."""
    return ((pts[:-1] + pts[1:]) * F(0.5)).astype(F)


def ref_index(u, pts, rule):
    """The index of every u under `rule`; a NaN u takes the last point."""
    k = pts.size
    with np.errstate(invalid='ignore'):
        if rule == DISTANCE:
            i = np.searchsorted(pts, u, side='left').clip(max=k - 1)
            lower = (i > 0) & (np.fabs(u - pts[i - 1]) < np.fabs(u - pts[i]))         # fp32 differences
            idx = i - lower
        else:
            idx = np.searchsorted(midpoints(pts), u, side='right')
    return np.where(np.isnan(u), k - 1, idx).astype(np.int64)


def geometry(n, bucket):
    """(row, number of buckets) of the bucket view (help_functions.py:67-94)."""
    if not bucket or n < bucket:
        return n, 1
    return bucket, -(-n // bucket)


def per_element(v, n, bucket):
    row, _ = geometry(n, bucket)
    return np.repeat(np.asarray(v).reshape(-1), row)[:n]


def ref_scale(x, bucket):
    """alpha = max - min per bucket (below 1e-10: 1), beta = min, u = (x - beta) / alpha; fp32, a NaN poisons its bucket."""
    n = x.size
    row, nb = geometry(n, bucket)
    rows = np.concatenate([x, np.full(nb * row - n, x[-1], F)]).reshape(nb, row)      # the padding repeats the last element
    with np.errstate(invalid='ignore'):
        mn, mx = rows.min(axis=1), rows.max(axis=1)                                  # numpy's min / max propagate a NaN
        alpha = (mx - mn).astype(F)
        alpha[alpha < F(1e-10)] = F(1)
        beta = mn.astype(F)
        u = ((x - per_element(beta, n, bucket)) / per_element(alpha, n, bucket)).astype(F)
    return alpha, beta, u


def ref_q(idx, pts, alpha, beta, n, bucket):
    """(points[idx] alpha + beta) + 0.0f, each operation rounded to fp32."""
    with np.errstate(invalid='ignore'):
        y = (pts[idx] * per_element(alpha, n, bucket)).astype(F)
        y = (y + per_element(beta, n, bucket)).astype(F)
        return (y + F(0)).astype(F)


def expect(case, pts, rule):
    """(idx, q) of a case under a rule."""
    idx = ref_index(case['u'], pts, rule)
    return idx, ref_q(idx, pts, case['alpha'], case['beta'], case['u'].size, case['bucket'])


# ------------------------------------------------------------------------------------------------------------- point sets
def points(name, k, seed):
    """k sorted fp32 points.  Every set but 'full precision' lies on the lattice j / L."""
    rng = np.random.RandomState(seed)
    if name == 'one cell':                     # inside ONE of the 2048 cells (32 lattice steps wide): duplicates above 32 points
        j = L // 2 + rng.randint(0, 32, size=k)
    elif name == 'dups':                       # runs of four equal points
        j = np.repeat(rng.randint(0, L + 1, size=(k + 3) // 4), 4)[:k]
    elif name == 'cell bounds':                # on j / 256 and j / 2048
        coarse = rng.choice(257, size=min(k - k // 2, 257), replace=False) * 8
        rest = np.setdiff1d(np.arange(2049), coarse)
        j = np.concatenate([coarse, rng.choice(rest, size=k - coarse.size, replace=False)]) * (L // 2048)
    elif name == 'outside':                    # [-1, 2): below 0 and above 1 as well
        j = rng.randint(-L, 2 * L, size=k)
        j[0] = -rng.randint(1, L)
        if k > 1:
            j[1] = L + rng.randint(1, L)
    elif name == 'bell':                       # the crowded centre a percentile initialisation produces
        j = np.rint(np.clip(0.5 + 0.11 * rng.randn(k), 0.0, 1.0) * L).astype(np.int64)
    elif name == 'uniform':
        j = rng.randint(0, L + 1, size=k)
    elif name == 'full precision':             # off the lattice: p + (q - p) / 2 and (p + q) / 2 round differently here
        for _ in range(1000):                  # ... for at least one pair, at every k
            pts = np.sort(rng.rand(k)).astype(F)
            if k == 1 or (other_midpoints(pts) != midpoints(pts)).any():
                return pts
        raise AssertionError('no point set on which the two forms of the midpoint differ')
    else:
        raise KeyError(name)
    p64 = np.sort(j) / float(L)
    pts = p64.astype(F)
    assert np.array_equal(pts.astype(np.float64), p64)
    if k > 1:                                  # every midpoint is exact
        assert np.array_equal(midpoints(pts).astype(np.float64), (p64[:-1] + p64[1:]) / 2), name
    if name == 'one cell':
        assert np.all(np.floor(p64 * 2048) == 1024)
    if name == 'outside':
        assert p64[0] < 0 and (k == 1 or p64[-1] > 1)
    return pts


Specials = collections.namedtuple('Specials', 'base near must')


def specials(pts):
    """base: the points, the midpoints and every boundary of the coarse and the fine cell table; near: the fp32 neighbours of
    those on either side; must: the points and midpoints inside [0, 1], each of which has to occur as a u.  (Off the lattice
    the midpoints in their other form, (p + q) / 2, count as midpoints too: see other_midpoints.)"""
    mid = np.concatenate([midpoints(pts), other_midpoints(pts)])
    base = np.unique(np.concatenate([pts, mid, np.arange(257, dtype=F) / F(256), np.arange(2049, dtype=F) / F(2048)]))
    near = np.unique(np.concatenate([np.nextafter(base, F(-np.inf)), np.nextafter(base, F(np.inf))]))
    must = np.unique(np.concatenate([pts, mid]))
    return Specials(base, near, must[(must >= 0) & (must <= 1)])


def is_special(u, sp):
    return np.isin(u, np.concatenate([sp.base, sp.near]))


def _fill(rng, n, sp, base, near, near_ok, reserved, last_lo):
    """n values: ~70 % from `base`, of the rest ~40 % from `near` where near_ok, else on the lattice j / (2 L); a last bucket
    [last_lo, n) of up to 64 elements and the last three elements from `base`; then every value of sp.must at a position that is not reserved (a
    random subset where the tensor is too short to hold them all).  Returns (u, whether all of sp.must was placed)."""
    u = (rng.randint(0, 2 * L + 1, size=n) / float(2 * L)).astype(F)
    sel = rng.rand(n) < 0.7
    if n - last_lo <= 64:
        sel[last_lo:] = True
    sel[max(n - 3, 0):] = True
    u[sel] = base[rng.randint(0, base.size, size=int(sel.sum()))]
    nsel = near_ok & (rng.rand(n) < 0.12)
    u[nsel] = near[rng.randint(0, near.size, size=int(nsel.sum()))]
    free = rng.permutation(np.flatnonzero(~reserved))
    must = sp.must
    if must.size:
        tail = free[free >= max(n - 3, 0)]                 # the scalar n % 4 tail: points / midpoints themselves
        u[tail] = must[rng.randint(0, must.size, size=tail.size)]
        free = free[free < max(n - 3, 0)]
    whole = free.size >= must.size
    put = must if whole else must[rng.permutation(must.size)[:free.size]]
    u[free[:put.size]] = put
    return u, whole


PAIRS = [(e, c) for e in range(-2, 3) for c in range(-2, 3)]         # x = u 2^e + c


def raw_case(pts, n, bucket, seed, unscaled=False):
    """A raw tensor for prescaled == 0.  Bucket b holds u = 0 and u = 1 at random positions and x = u 2^e + c with its own
    (e, c), so that alpha = 2^e, beta = c and u = (x - beta) / alpha exactly; `unscaled` (the 'full precision' points): e = c = 0
    everywhere, x is u.  With four or more buckets one is constant (the alpha guard: alpha = 1, u = 0) and one holds a NaN (every
    index k - 1, q NaN).  Fp32 neighbours of the special values need the 24 bits of x for themselves: only where c = 0.
    Returns x, the u the kernel must see, and the alpha / beta it must report."""
    rng = np.random.RandomState(seed)
    row, nb = geometry(n, bucket)
    lo = np.arange(nb) * row
    size = np.minimum(row, n - lo)
    b_of = np.arange(n) // row
    order = rng.permutation(len(PAIRS))
    pair = np.array(PAIRS)[order[np.arange(nb) % len(PAIRS)]] * (0 if unscaled else 1)
    e, c = pair[:, 0], pair[:, 1]
    sp = specials(pts)
    base = sp.base[(sp.base >= 0) & (sp.base <= 1)]
    near = sp.near[(sp.near >= TINY) & (sp.near <= 1)]           # (the neighbour of 0 is a denormal: 2^e u would not be exact)
    # where the 0 and the 1 of every bucket go: not onto the last three elements where the bucket has room
    room = np.maximum(size - np.where((lo + size == n) & (size >= 5), 3, 0), 1)
    p0 = np.floor(rng.rand(nb) * room).astype(np.int64)
    p1 = (p0 + 1 + np.floor(rng.rand(nb) * (room - 1)).astype(np.int64)) % room
    reserved = np.zeros(n, bool)
    reserved[lo + p0] = True
    reserved[lo + p1] = True
    const_b = nan_b = -1
    if nb >= 4:
        const_b, nan_b = rng.choice(np.arange(1, nb - 1), size=2, replace=False)
        reserved |= (b_of == const_b) | (b_of == nan_b)
    u, whole = _fill(rng, n, sp, base, near, (c == 0)[b_of], reserved, lo[-1])
    u[lo + p1] = 1                                          # (a bucket of one element: p1 == p0, the 0 below wins)
    u[lo + p0] = 0
    if const_b >= 0:
        u[b_of == const_b] = 0
    assert is_special(u, sp).mean() >= 0.5
    assert is_special(u[lo[-1]:], sp).mean() >= 0.5 and is_special(u[-3:], sp).all()
    live = b_of != nan_b
    assert not whole or np.isin(sp.must, u[live]).all()
    assert whole or n < 1000, 'only a short tensor may leave points or midpoints out'
    x64 = u.astype(np.float64) * 2.0 ** e[b_of] + c[b_of]
    if const_b >= 0:
        x64[b_of == const_b] = c[const_b]
    x = x64.astype(F)
    assert np.array_equal(x.astype(np.float64), x64), 'x = u 2^e + c is not exact in fp32'
    alpha, beta = (2.0 ** e).astype(F), c.astype(F)
    single = size == 1
    alpha[single] = 1
    if const_b >= 0:
        alpha[const_b] = 1
    if nan_b >= 0:
        x[lo[nan_b] + rng.randint(0, size[nan_b])] = np.nan
        u[b_of == nan_b] = np.nan
        alpha[nan_b] = beta[nan_b] = np.nan
    ra, rb, ru = ref_scale(x, bucket)                        # the construction delivers what it promises
    assert np.array_equal(ra, alpha, equal_nan=True) and np.array_equal(rb, beta, equal_nan=True)
    assert np.array_equal(ru, u, equal_nan=True)
    return dict(x=x, u=u, alpha=alpha, beta=beta, bucket=bucket, whole=whole)


def prescaled_case(pts, n, bucket, seed):
    """u for prescaled == 1: the same values, fp32 neighbours everywhere, and -1, -0.0, 2, +-inf, NaN, values below the first and
    above the last point; alpha a power of two and beta a small integer per bucket."""
    rng = np.random.RandomState(seed)
    row, nb = geometry(n, bucket)
    sp = specials(pts)
    extras = np.array([-1.0, -0.0, 2.0, np.inf, -np.inf, np.nan, np.nextafter(pts[0], F(-np.inf)), pts[0] - F(1),
                       np.nextafter(pts[-1], F(np.inf)), pts[-1] + F(1), 0.0, 1.0], F)
    reserved = np.zeros(n, bool)
    at = rng.choice(max(n - 3, 1), size=min(extras.size, max(n - 3, 0) // 3), replace=False)     # (before the n % 4 tail)
    reserved[at] = True
    u, whole = _fill(rng, n, sp, sp.base, sp.near, np.ones(n, bool), reserved, (nb - 1) * row)
    u[at] = extras[:at.size]
    assert is_special(u, sp).mean() >= 0.5 and is_special(u[-3:], sp).all()
    assert is_special(u[(nb - 1) * row:], sp).mean() >= 0.5
    assert not whole or np.isin(sp.must, u).all()
    assert whole or n < 1000
    assert n < 100 or (np.isnan(u).any() and np.isinf(u).any() and (u < pts[0]).any() and (u > pts[-1]).any())
    alpha = (2.0 ** rng.randint(-2, 3, size=nb)).astype(F)
    beta = rng.randint(-2, 3, size=nb).astype(F)
    return dict(x=u, u=u, alpha=alpha, beta=beta, bucket=bucket, whole=whole)


# ------------------------------------------------------------------------------------------------------------- geometries
# An index form: (idx_bytes 8 / 1 / 0 = no index output, offset of idx in bytes past 16-byte alignment, the kernels the call
# must reach).  The forms of a row run on the same tensor; the uint8 forms only up to 256 points.
Row = collections.namedtuple('Row', 'prescaled bucket n x_off fused_mode forms sets')


def _row(prescaled, bucket, n, kernels, x_off=0, fused_mode=None, forms=None, sets=SETS_PER_ROW):
    kernels = [kernels] if isinstance(kernels, str) else kernels
    forms = forms or ((8, 0), (1, 0), (0, 0))
    return Row(prescaled, bucket, n, x_off, fused_mode, tuple((w, o, kernels) for w, o in forms), sets)


I8_MISALIGNED = ((8, 8),)     # an int64 idx 8 bytes past a 16-byte boundary: the two-pass kernels, whatever the bucket size
U8_ODD = ((1, 2),)            # a uint8 idx 2 bytes past a 4-byte boundary: the pre-scaled stream refuses it, the bucket kernels do not
WAVE = 'k_bucket_wave_any<2,%d,%d>'
THREE = ['k_minmax_partial', 'k_single_apply<2>']
# Every n ends in a ragged last bucket and an n % 4 tail, and spans several tiles / chunks / blocks of its kernel.
# (fp32 data needs 4-byte alignment and nothing more -- x at +4 bytes runs the same kernel, so several rows put it there; what
# sends a call to the two-pass kernels is an int64 idx that is not 16-byte aligned.)
ROWS = [
    # ---- prescaled == 0
    _row(0, 64, 64 * 150 + 37, 'k_bucket_vec<2,16,1,4>'),
    _row(0, 128, 128 * 80 + 50, 'k_bucket_vec<2,16,2,2>', x_off=4),
    _row(0, 256, 256 * 40 + 131, 'k_bucket_vec<2,16,4,1>'),
    _row(0, 512, 512 * 20 + 301, 'k_bucket_vec<2,64,2,2>'),
    _row(0, 1024, 1024 * 10 + 515, 'k_bucket_vec<2,64,4,1>', x_off=12),
    _row(0, 2048, 2048 * 6 + 1030, 'k_bucket_vec<2,64,8,1>'),
    _row(0, 449, 449 * 23 + 130, WAVE % (3, 1)),
    _row(0, 1000, 1000 * 10 + 333, WAVE % (5, 1), x_off=8),
    _row(0, 1500, 1500 * 7 + 702, WAVE % (8, 1)),
    _row(0, 3000, 3000 * 4 + 1003, WAVE % (6, 2)),
    _row(0, 3500, 3500 * 3 + 1501, WAVE % (8, 2)),
    _row(0, 5000, 5000 * 3 + 2002, WAVE % (6, 4)),
    _row(0, 9000, 9000 * 3 + 4503, WAVE % (9, 4)),
    _row(0, 100, 100 * 70 + 43, 'k_bucket_chunk<2,8>'),
    _row(0, 12, 12 * 600 + 7, 'k_bucket_chunk<2,8>', x_off=4),
    _row(0, 33, 33 * 300 + 17, 'k_bucket_chunk_any<2,8>'),          # (its uint8 form up to 32 points stages the indices in LDS)
    _row(0, 7, 7 * 1200 + 3, 'k_bucket_chunk_any<2,8>'),
    _row(0, 250, 250 * 30 + 121, 'k_bucket_chunk_any<2,8>', x_off=4),
    _row(0, 100, 100 * 50 + 43, 'k_bucket_groups<2,16>', x_off=4, forms=I8_MISALIGNED),
    _row(0, 33, 33 * 4 + 20, 'k_bucket_groups<2,16>'),              # five buckets: too few for one chunk
    _row(0, 1000, 1000 * 10 + 333, 'k_bucket_groups<2,64>', x_off=4, forms=I8_MISALIGNED),
    _row(0, 10000, 10000 * 2 + 5003, 'k_bucket_groups<2,64>'),      # above the 9216 elements of the largest wave instance
    _row(0, 16500, 16500 * 2 + 3001, 'k_bucket_generic<2>'),
    _row(0, 0, 5003, 'k_bucket_generic<2>'),                        # one bucket, one block
    _row(0, 0, 20003, 'k_single_fused<2,1,4>', fused_mode=1),
    _row(0, 0, 20003, THREE, fused_mode=0),
    _row(0, 0, 20003, 'k_single_fused<2,1,4>', fused_mode=2),       # every block gives up at the barrier and folds alone
    _row(0, 0, 256 * 1024 + 7, 'k_single_fused<2,4,4>', fused_mode=1, forms=((8, 0),), sets=1),
    # ---- prescaled == 1
    _row(1, 256, 256 * 40 + 131, 'k_nearest_prescaled_stream<false>'),
    _row(1, 100, 100 * 70 + 43, 'k_nearest_prescaled_stream<false>', x_off=4),
    _row(1, 33, 33 * 300 + 17, 'k_nearest_prescaled_stream<true>'),
    _row(1, 0, 20003, 'k_single_apply<2>'),                         # alpha / beta copied into the slot the apply kernel reads
    _row(1, 0, 5003, 'k_bucket_generic<2>'),
    _row(1, 256, 256 * 40 + 131, 'k_bucket_vec<2,16,4,1>', forms=U8_ODD),
    _row(1, 1000, 1000 * 10 + 333, WAVE % (5, 1), forms=U8_ODD),
    _row(1, 100, 100 * 70 + 43, 'k_bucket_chunk<2,8>', x_off=4, forms=U8_ODD),
    _row(1, 33, 33 * 300 + 17, 'k_bucket_chunk_any<2,8>', forms=U8_ODD),
    _row(1, 100, 100 * 50 + 43, 'k_bucket_groups<2,16>', x_off=4, forms=I8_MISALIGNED),
    _row(1, 1000, 1000 * 10 + 333, 'k_bucket_groups<2,64>', forms=I8_MISALIGNED),
]


def k_class(rule, k):
    """The classes every kernel has to be reached in: the distance rule below and above 32 points (small table / coarse point
    table), the midpoint rule up to 32, up to 64 (no fine table on the vector kernel) and above."""
    if rule == DISTANCE:
        return 'distance k <= 32' if k <= 32 else 'distance k > 32'
    return 'midpoint k <= 32' if k <= 32 else 'midpoint k in 33..64' if k <= 64 else 'midpoint k > 64'


CLASSES = ('distance k <= 32', 'distance k > 32', 'midpoint k <= 32', 'midpoint k in 33..64', 'midpoint k > 64')
# shipped kernels of the transform launcher that the table leaves out, each with its reason
NOT_IN_THE_TABLE = {
    'k_minmax_final': 'folds the min / max partials above 8 Mi elements in one bucket: no point search, and no case that long',
}


def expected_fine(kernel, rule, k):
    """The fine cell table: midpoint rule above 32 points, except in the chunk kernels (they stage data in LDS) and, up to 64
    points, in the vector kernel."""
    if rule != MIDPOINT or k <= 32 or kernel.startswith(('k_bucket_chunk', 'k_minmax')):
        return 0
    return 0 if (kernel.startswith('k_bucket_vec') and k <= 64) else 1


def check_rows_against_the_plan(lib, queries, plan, names, shipped):
    """Every form of every row reaches the kernels it names, for every k and both rules, with `fine` as expected; and every
    shipped nearest-point instantiation of the transform kernels is reached in every class.  lib: libqd_hip.so (host-only
    call); queries / plan / names: tests/test_transform_plan.py; shipped: the kernel names in the library.
    Returns {kernel: {class: fine values seen}}."""
    reached = collections.defaultdict(lambda: collections.defaultdict(set))
    for ri, row in enumerate(ROWS):
        for k in K:
            for rule in RULES:
                for width, off, kernels in row.forms:
                    if width == 1 and k > 256:
                        continue
                    q = queries(2, row.n, row.bucket, data_misalign=row.x_off, side_bytes=width, side_misalign=off, k=k, assign_mode=rule,
                                prescaled=row.prescaled, fused_capacity=0 if row.fused_mode == 0 else 256)
                    p = plan(lib, q)
                    assert names(p) == kernels, (ri, row, k, rule, width, names(p))
                    for name in kernels:
                        fine = int(p['fine'][0]) if not name.startswith('k_minmax') else 0
                        assert fine == expected_fine(name, rule, k), (ri, name, rule, k, fine)
                        reached[name][k_class(rule, k)].add(fine)
                    if row.prescaled and width:                 # indices only: the stream, or refused
                        q['q_null'] = 1
                        got = names(plan(lib, q))
                        assert got == ([] if not indices_only_served(row, width, off) else
                                       ['k_nearest_prescaled_stream<%s>' % ('true' if geometry(row.n, row.bucket)[0] % 4 else 'false')]), (ri, got)
                        for name in got:
                            reached[name][k_class(rule, k)].add(int(plan(lib, q)['fine'][0]))
    required = [s for s in shipped if (s.startswith(('k_bucket_', 'k_single_')) and re.search(r'<2[,>]', s)) or
                s.startswith(('k_minmax_', 'k_nearest_prescaled_stream'))]
    assert len(required) >= 24
    missing = [(s, c) for s in required if s not in NOT_IN_THE_TABLE for c in CLASSES if c not in reached[s]]
    assert missing == [], 'shipped nearest-point kernels that no row reaches in some class: %s' % missing
    assert set(NOT_IN_THE_TABLE) <= set(required) and not set(NOT_IN_THE_TABLE) & set(reached)
    return {name: {c: sorted(v) for c, v in cls.items()} for name, cls in reached.items()}


def indices_only_served(row, width, off):
    """q == NULL (include/qd_hip.h): pre-scaled, n >= 4, buckets of at least 4 elements, idx 16-byte (int64) / 4-byte (uint8)
    aligned -- the stream kernel or nothing."""
    return bool(row.prescaled and width and off % (16 if width == 8 else 4) == 0 and geometry(row.n, row.bucket)[0] >= 4)


def row_sets(ki, ri, row):
    return [SETS[(ki + ri + 2 * j) % len(SETS)] for j in range(row.sets)]


@functools.lru_cache(maxsize=2)
def cases_of(k):
    """[(row index, row, set name, points, case)] of one k: built once, shared by the tests that run them, never modified."""
    ki = K.index(k)
    out = []
    for ri, row in enumerate(ROWS):
        for si, name in enumerate(row_sets(ki, ri, row)):
            seed = 100003 * k + 101 * ri + si
            pts = points(name, k, seed)
            if row.prescaled:
                case = prescaled_case(pts, row.n, row.bucket, seed + 1)
            else:
                case = raw_case(pts, row.n, row.bucket, seed + 1, unscaled=name == 'full precision')
            for a in [pts] + [v for v in case.values() if isinstance(v, np.ndarray)]:
                a.setflags(write=False)
            out.append((ri, row, name, pts, case))
    return out


# ----------------------------------------------------------------------------------------------------- multi-tensor launch
MULTI_K = (1, 2, 5, 32, 33, 64, 65, 256)
MULTI_BUCKETS = (0, 64, 256, 100, 33)
# seven tensors, one point set each; the odd ones are placed off 16-byte (u, q) and 4-byte (idx) alignment by the GPU test, so
# both the register path (full rows / tiles of aligned tensors) and the element path run.  4100 and 3333 are aligned AND ragged.
MULTI_SIZES = (4100, 2500, 1024 * 3, 777, 3333, 1025, 256 * 9)


@functools.lru_cache(maxsize=4)
def multi_case(k, bucket):
    """[(points, pre-scaled case)] of the seven tensors."""
    out = []
    for i, (name, n) in enumerate(zip(SETS, MULTI_SIZES)):
        seed = 7000003 * k + 1009 * bucket + i
        pts = points(name, k, seed)
        case = prescaled_case(pts, n, bucket, seed + 1)
        for a in [pts] + [v for v in case.values() if isinstance(v, np.ndarray)]:
            a.setflags(write=False)
        out.append((pts, case))
    return out
