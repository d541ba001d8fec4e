"""Cases of the order-statistics select (qd_order_stats_f32, csrc/qd_select.hip), of its wrapper
quantization.help_functions.order_statistics and of initialize_quantization_points on non-finite tensors, shared by
tests/test_select_host.py (CPU tensors, no GPU) and tests/test_hip_select.py (the device select, the device sort fallback, and
both against the host).  A plain helper module: no fixtures, nothing runs on import, every case is built when it is asked for.

The inputs are BIT PATTERNS: a uint32 array viewed as float32, never touched by arithmetic, so the sign and the payload of
every NaN are what was written (0xFFC00000, the NaN that 0/0 and inf - inf produce on x86, has its sign bit set).

The expected answer is an integer sort: key(v) = the bits of v made order-preserving (negative: all bits flipped, positive:
sign bit flipped), EVERY NaN canonicalised to the one largest key, np.sort of the keys, mapped back to floats.  Compared bit
for bit with two allowances (same): +0 and -0 are one value (their order among equals is arbitrary in every sort), and a
rank that lands among the NaNs must return a NaN, not the bits of a particular one.

What the groups are built to decide, and random ranks on random data decide only by luck:
  nonfinite  +-inf, +-FLT_MAX, the smallest denormal of each sign, +-0 and NaNs of both signs and four payloads; one, several,
             only NaNs; ranks 0, 1, the last non-NaN rank, the first NaN rank, n - 1; n = 1003 and n = 5.
  span       for_each_key's [head scalars][float4][tail scalars]: nvec on both sides of the 1024-lane stride and of the 4-deep
             unrolled loop's `i + 3 * stride < nvec`, every head and tail length, n shorter than the head.  The values ascend
             with the position and the allocation holds -inf decoys in front of and behind the view, so an element dropped,
             read twice or read from outside moves an answer at the ranks next to the span boundaries and at n - 1.
  blocks     n = (B - 1) * 16384 + 1 asks the launcher for B blocks: the group split and the 16-deep unrolling of
             k_sel_sum_top / sum_strided and the `b + 60 < nblocks` bound of k_sel_pick_sub.  Distinct shuffled values.
  prefix     targets CHOSEN to share 22 key bits, 12 but not 22, or none (the row sharing of k_sel_hist_sub: s_first, s_mask,
             the walk over s_prefix), runs of multiplicity 1, 2 and 1000 asked for at their first and last copy, all 32
             targets in one 22-bit prefix, all in one run of equal values, m = 1, 2, 31, 32.
  wrapper    ranks in any order with repeats, 33 / 64 / 65 distinct ranks, no ranks, a non-contiguous 2-D view."""
import contextlib
import zlib

import numpy as np
import torch

U32 = np.uint32
F32 = np.float32
NAN_KEY = 0xFFFFFFFF
NAN_PAYLOADS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF)
NEG_INF, POS_INF = 0xFF800000, 0x7F800000
# -inf, +inf, +-FLT_MAX, the smallest denormal of each sign, +-0
SPECIALS = (NEG_INF, POS_INF, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x80000001, 0x00000000, 0x80000000)
BLOCK_ELEMS = 16384                      # elements one block of the select asks for (1024 lanes x 4 floats x 4 loads in flight)
BLOCK_COUNTS = (1, 2, 3, 5, 17, 61, 64, 65, 67, 129, 256)
MIN_CUS = 256                            # the launcher caps the blocks at the CU count: the list above needs this many


# ------------------------------------------------------------------------------------------------ the expected answer
def is_nan_bits(bits):
    return (np.asarray(bits, U32) & U32(0x7FFFFFFF)) > U32(0x7F800000)


def keys_of(bits):
    b = np.asarray(bits, U32)
    k = b ^ np.where((b >> U32(31)) == 1, U32(0xFFFFFFFF), U32(0x80000000))
    return np.where(is_nan_bits(b), U32(NAN_KEY), k)


def bits_of_keys(keys):
    k = np.asarray(keys, U32)
    return np.where((k >> U32(31)) == 1, k ^ U32(0x80000000), ~k)


class Case(object):
    """bits: the uint32 ALLOCATION; the tensor is its elements [offset, offset + n), or with strided = (rows, cols, step)
    the non-contiguous view allocation.view(rows, cols)[:, ::step].  ranks: int64, as handed to order_statistics."""

    def __init__(self, cid, bits, ranks, offset=0, n=None, strided=None):
        self.id = cid
        self.bits = np.ascontiguousarray(bits, dtype=U32)
        self.offset = offset
        self.n = self.bits.size - offset if n is None else n
        self.strided = strided
        self.ranks = np.asarray(ranks, dtype=np.int64)

    def logical_bits(self):
        if self.strided:
            rows, cols, step = self.strided
            return self.bits.reshape(rows, cols)[:, ::step].reshape(-1)
        return self.bits[self.offset:self.offset + self.n]

    def tensor(self, device):
        base = torch.from_numpy(self.bits.view(np.int32)).to(device).view(torch.float32)
        if self.strided:
            rows, cols, step = self.strided
            return base.view(rows, cols)[:, ::step]
        return base[self.offset:self.offset + self.n]

    def sorted_keys(self):
        return np.sort(keys_of(self.logical_bits()))

    def expected(self):
        return bits_of_keys(self.sorted_keys()[self.ranks]).view(F32)


def same(got, want, tag=None):
    """Asserts the comparison of the module docstring; `want` is Case.expected()."""
    got = np.ascontiguousarray(got, dtype=F32)
    want = np.ascontiguousarray(want, dtype=F32)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    nan = is_nan_bits(want.view(U32))
    assert np.isnan(got[nan]).all(), (tag, 'a rank among the NaNs returned a number', got[nan][:8])
    g, w = got[~nan], want[~nan]
    zero = (g == 0) & (w == 0)
    gb, wb = np.where(zero, U32(0), g.view(U32)), np.where(zero, U32(0), w.view(U32))
    bad = np.flatnonzero(gb != wb)
    assert bad.size == 0, (tag, '%d of %d differ; first (position among the non-NaN ranks, got, want):' % (bad.size, want.size),
                           [(int(i), hex(int(gb[i])), hex(int(wb[i]))) for i in bad[:6]])


# ------------------------------------------------------------------------------------------------ the three paths of the wrapper
@contextlib.contextmanager
def _passes(value):
    import quantization.help_functions as qhf
    old = qhf.ORDER_STATS_MAX_PASSES
    qhf.ORDER_STATS_MAX_PASSES = value
    try:
        yield
    finally:
        qhf.ORDER_STATS_MAX_PASSES = old


def run(case, path):
    """order_statistics of the case on one path: 'host' (CPU tensor: np.partition), 'select' (device tensor, the radix select
    however many passes of 32 ranks it takes), 'sort' (device tensor, the torch.sort fallback), 'device' (device tensor, the
    wrapper's own choice between the two)."""
    import quantization.help_functions as qhf
    if path == 'host':
        return qhf.order_statistics(case.tensor('cpu'), case.ranks)
    t = case.tensor('cuda')
    if path == 'device':
        return qhf.order_statistics(t, case.ranks)
    with _passes(1 << 30 if path == 'select' else 0):
        return qhf.order_statistics(t, case.ranks)


def check(case, path):
    same(run(case, path), case.expected(), (case.id, path))


# ------------------------------------------------------------------------------------------------ building blocks
def distinct_finite(rng, count):
    """`count` distinct finite non-zero float32 bit patterns of both signs and every magnitude, in random order."""
    out = np.empty(0, U32)
    while out.size < count:
        b = rng.randint(0, 1 << 32, size=count + count // 4 + 64, dtype=np.uint64).astype(U32)
        b = b[((b >> U32(23)) & U32(0xFF)) != 0xFF]                    # no inf, no NaN
        b = b[(b & U32(0x7FFFFFFF)) != 0]                              # no +-0
        b = b[~np.isin(b, np.array(SPECIALS, U32))]
        out = np.unique(np.concatenate([out, b]))
    return rng.permutation(out)[:count]


def _clip_unique(ranks, n):
    return np.unique(np.clip(np.asarray(ranks, np.int64), 0, n - 1))


# ------------------------------------------------------------------------------------------------ non-finite
def _nonfinite_bits(n, nans, seed):
    rng = np.random.RandomState(seed)
    fixed = np.array(list(SPECIALS) + list(nans), U32)
    bits = np.concatenate([fixed, distinct_finite(rng, n - fixed.size)]) if n > fixed.size else fixed[:n]
    return rng.permutation(bits)


def _nonfinite_ranks(n, nnan):
    return _clip_unique([0, 1, n - nnan - 1, n - nnan, n - 1], n)


SEVERAL_NANS = (0x7FC00000, 0xFFC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
_SHORT = {p: (p, NEG_INF, POS_INF, 0x80000000, 0x00000001) for p in NAN_PAYLOADS}        # n = 5 with one NaN, in this order


def _nonfinite(cid):
    kind, what = cid.split('-')[0], cid.split('-', 1)[1]
    n = 1003 if kind == 'nf' else 5
    if what.startswith('one_'):
        p = int(what[4:], 16)
        if n == 5:
            return Case(cid, np.array(_SHORT[p], U32), _nonfinite_ranks(5, 1))
        return Case(cid, _nonfinite_bits(n, (p,), p & 0xFFFF), _nonfinite_ranks(n, 1))
    if what == 'several':
        if n == 5:
            return Case(cid, np.array((0xFFC00000, NEG_INF, 0x7F800001, POS_INF, 0xFFFFFFFF), U32), _nonfinite_ranks(5, 3))
        return Case(cid, _nonfinite_bits(n, SEVERAL_NANS, 7), _nonfinite_ranks(n, len(SEVERAL_NANS)))
    assert what == 'all'
    return Case(cid, np.resize(np.array(NAN_PAYLOADS, U32), n), _nonfinite_ranks(n, n))


NONFINITE_IDS = ['%s-%s' % (kind, what) for kind in ('nf', 'nf5')
                 for what in ['one_%08X' % p for p in NAN_PAYLOADS] + ['several', 'all']]


# ------------------------------------------------------------------------------------------------ span edges
SPAN_NVEC = (0, 1, 1023, 1024, 1025, 4095, 4096, 4097)
DECOY = NEG_INF                          # around the view: read by mistake, it becomes rank 0 and shifts every other rank


def head_of(offset, n):
    """Scalars in front of the first 16-byte boundary of a view `offset` floats into a 16-byte-aligned allocation."""
    return min((4 - offset) % 4, n)


def _span_case(cid, offset, n):
    rng = np.random.RandomState(zlib.crc32(cid.encode()) & 0x7FFFFFFF)
    values = distinct_finite(rng, n)
    values = values[np.argsort(keys_of(values))]                                  # ascending with the position
    bits = np.concatenate([np.full(offset, DECOY, U32), values, np.full(3, DECOY, U32)])
    head = head_of(offset, n)
    ntail = (n - head) % 4
    return Case(cid, bits, _clip_unique([0, n - 1, head - 1, head, n - ntail - 1, n - ntail], n), offset=offset, n=n)


def span_ids(nvec):
    """head = 0, 3, 2, 1 at offset 0, 1, 2, 3; n = 0 (nvec = 0 without head and tail) is not an array."""
    return ['span-v%d-o%d-t%d' % (nvec, off, tail) for off in range(4) for tail in range(4) if nvec or (4 - off) % 4 + tail]


SPAN_TINY_IDS = ['span-tiny-o%d-n%d' % (off, n) for off in (1, 2, 3) for n in (1, 2, 3)]    # n <= head among them


def _span(cid):
    f = cid.split('-')
    if f[1] == 'tiny':
        return _span_case(cid, int(f[2][1:]), int(f[3][1:]))
    nvec, off, tail = int(f[1][1:]), int(f[2][1:]), int(f[3][1:])
    return _span_case(cid, off, (4 - off) % 4 + 4 * nvec + tail)


# ------------------------------------------------------------------------------------------------ block counts
def blocks_n(b):
    return (b - 1) * BLOCK_ELEMS + 1


def _blocks(cid):
    b = int(cid.split('-')[1])
    n = blocks_n(b)
    rng = np.random.RandomState(b)
    perm = rng.permutation(n).astype(U32)
    bits = (U32(0x3F000000) + (perm >> U32(1))) | ((perm & U32(1)) << U32(31))    # distinct, both signs, |v| in [0.5, 1)
    ranks = np.unique(np.concatenate([[0, n - 1], rng.randint(0, n, size=64)]))
    ranks = ranks if ranks.size <= 32 else np.concatenate([ranks[:1], rng.permutation(ranks[1:-1])[:30], ranks[-1:]])
    return Case(cid, bits, np.sort(ranks))


BLOCKS_IDS = ['blocks-%d' % b for b in BLOCK_COUNTS]


# ------------------------------------------------------------------------------------------------ shared prefixes
A_TOP, A_MID = 0xC00, 0x155              # (a) one 22-bit prefix (floats just above 2.0)
B_TOP = 0x3F0                            # (b) one top bin (negative floats)
A_LOW_PINNED = (0, 1, 31, 32, 1022, 1023)
MULTIPLICITIES = (1, 2, 1000)


def _key(top, mid, low):
    return (int(top) << 20) | (int(mid) << 10) | int(low)


_prefix_cache = {}


def prefix_multiset():
    """-> dict(bits, sorted keys, and per group 'a' / 'b' / 'c' the (first rank, last rank, multiplicity) of every run)."""
    if _prefix_cache:
        return _prefix_cache
    rng = np.random.RandomState(77)
    others = np.setdiff1d(np.arange(2, 1022), A_LOW_PINNED)
    a_low = np.sort(np.concatenate([A_LOW_PINNED, rng.permutation(others)[:26]]))
    groups = {'a': [_key(A_TOP, A_MID, low) for low in a_low]}
    b_mid = np.sort(np.concatenate([[0, 1023], rng.permutation(np.arange(1, 1023))[:10]]))
    groups['b'] = [_key(B_TOP, mid, rng.randint(0, 1024)) for mid in b_mid]
    # the bins of -inf (key 0x007FFFFF, the smallest key of a number) and of +inf (0xFF800000, the largest), and 8 between
    tops = np.setdiff1d(rng.permutation(np.arange(0x008, 0xFF8))[:10], [A_TOP, B_TOP])[:8]
    groups['c'] = [int(keys_of(NEG_INF))] + [_key(t, rng.randint(0, 1024), rng.randint(0, 1024)) for t in np.sort(tops)] \
        + [int(keys_of(POS_INF))]
    assert groups['c'][0] == 0x007FFFFF and groups['c'][-1] == 0xFF800000
    chosen, mult = [], {}
    for g in 'abc':
        for i, k in enumerate(groups[g]):
            mult[k] = MULTIPLICITIES[i % 3]
            chosen.append(np.full(mult[k], k, U32))
    # background that the passes must REJECT: under (a)'s top bin with other middle digits, under (b)'s top bin with middle
    # digits no target has, and everywhere else
    back = [np.array([_key(A_TOP, m, rng.randint(0, 1024)) for m in rng.permutation(1024)[:200] if m != A_MID], U32),
            np.array([_key(B_TOP, m, rng.randint(0, 1024)) for m in np.setdiff1d(np.arange(1024), b_mid)[::4]], U32),
            keys_of(distinct_finite(rng, 4000))]
    back = np.setdiff1d(np.unique(np.concatenate(back)), np.array(sorted(mult), U32))
    keys = rng.permutation(np.concatenate(chosen + [back]))
    assert not is_nan_bits(bits_of_keys(keys)).any()
    skeys = np.sort(keys)
    _prefix_cache.update(bits=bits_of_keys(keys), sorted=skeys)
    for g in 'abc':
        runs = []
        for k in groups[g]:
            first, last = int(np.searchsorted(skeys, k, 'left')), int(np.searchsorted(skeys, k, 'right')) - 1
            assert last - first + 1 == mult[k]                           # the stated multiplicities
            runs.append((first, last, mult[k]))
        _prefix_cache[g] = runs
    return _prefix_cache


PREFIX_MIXED = 3                         # 89 first / last ranks of the 54 runs, dealt round-robin into calls of m = 32
PREFIX_IDS = ['prefix-mixed%d' % j for j in range(PREFIX_MIXED)] + ['prefix-all_in_a', 'prefix-one_run'] \
    + ['prefix-m%d' % m for m in (1, 2, 31, 32)]


def _prefix(cid):
    P = prefix_multiset()
    n, what = P['bits'].size, cid.split('-')[1]
    if what.startswith('mixed'):
        every = np.unique([r for g in 'abc' for first, last, _ in P[g] for r in (first, last)])
        assert every.size <= 32 * PREFIX_MIXED
        ranks = every[int(what[5:])::PREFIX_MIXED]
        rng = np.random.RandomState(int(what[5:]))
        while ranks.size < 32:                                           # filled up to 32 targets with background ranks
            ranks = np.unique(np.concatenate([ranks, rng.randint(0, n, size=32 - ranks.size)]))
    elif what == 'all_in_a':
        ranks = np.array([first for first, _, _ in P['a']])
    elif what == 'one_run':
        first, last, _ = [r for r in P['a'] if r[2] == 1000][0]
        ranks = np.unique(np.concatenate([[first, last], np.linspace(first, last, 32).astype(np.int64)]))
    else:
        ranks = np.array([last for _, last, _ in P['a']])[:int(what[1:])]
    assert ranks.size == (int(what[1:]) if what[0] == 'm' and what[1:].isdigit() else 32), (cid, ranks.size)
    return Case(cid, P['bits'], ranks)


# ------------------------------------------------------------------------------------------------ the wrapper
WRAPPER_IDS = ['wrap-unordered', 'wrap-33', 'wrap-64', 'wrap-65', 'wrap-empty', 'wrap-2d_view']
WRAPPER_N = 20011


def _wrapper(cid):
    what = cid.split('-')[1]
    rng = np.random.RandomState(len(what) * 131 + ord(what[0]))
    bits = _nonfinite_bits(WRAPPER_N, SEVERAL_NANS, 21)                  # the non-finite multiset, 7 NaNs at the end of the order
    n, first_nan = WRAPPER_N, WRAPPER_N - len(SEVERAL_NANS)
    if what == 'unordered':
        return Case(cid, bits, [5, 5, 0, n - 1, 777, 5, first_nan, 10000, first_nan - 1, 0, n - 1, 1])
    if what == 'empty':
        return Case(cid, bits, np.empty(0, np.int64))
    if what == '2d_view':
        case = Case(cid, bits[:20000], [], strided=(100, 200, 2))            # 100 x 100 of every other column
        m = case.logical_bits().size
        nnan = int(is_nan_bits(case.logical_bits()).sum())
        assert 0 < nnan < m                                              # some of the NaNs are in the view
        case.ranks = np.array([m - 1, 0, 17, m - nnan, m - nnan - 1, 17, m // 2], np.int64)
        return case
    distinct = int(what)                                                 # 33, 64: two passes of the select; 65: the sort
    ranks = np.concatenate([[0, first_nan - 1, first_nan, n - 1], rng.permutation(np.arange(1, first_nan - 1))[:distinct - 4]])
    ranks = rng.permutation(np.concatenate([ranks, ranks[:9]]))                           # any order, with repeats
    assert np.unique(ranks).size == distinct
    return Case(cid, bits, ranks)


# ------------------------------------------------------------------------------------------------ every case
GROUPS = dict(nonfinite=NONFINITE_IDS, span_tiny=SPAN_TINY_IDS, blocks=BLOCKS_IDS, prefix=PREFIX_IDS, wrapper=WRAPPER_IDS)
GROUPS.update(('span_v%d' % v, span_ids(v)) for v in SPAN_NVEC)
_BUILDERS = dict(nf=_nonfinite, nf5=_nonfinite, span=_span, blocks=_blocks, prefix=_prefix, wrap=_wrapper)


def case(cid):
    c = _BUILDERS[cid.split('-')[0]](cid)
    assert c.ranks.size == 0 or (c.ranks.min() >= 0 and c.ranks.max() < c.logical_bits().size), cid
    return c


def check_conditions(c):
    """What the structural cases promise: the non-NaN values are distinct or have the stated multiplicities (prefix_multiset
    asserts those), so a count that is off by one changes the returned bits."""
    group = c.id.split('-')[0]
    logical = c.logical_bits()
    if group in ('span', 'blocks'):
        assert np.unique(keys_of(logical)).size == logical.size and not is_nan_bits(logical).any(), c.id
    if group == 'span':
        assert np.all(np.diff(keys_of(logical).astype(np.int64)) > 0), c.id
        assert np.all(c.bits[:c.offset] == DECOY) and np.all(c.bits[c.offset + c.n:] == DECOY) and c.bits.size == c.offset + c.n + 3
    if group == 'blocks':
        want = -(-c.n // BLOCK_ELEMS)
        assert want == int(c.id.split('-')[1]) and c.ranks.size == min(32, c.n), (c.id, want)
    if group in ('nf', 'nf5', 'wrap'):
        nonnan = keys_of(logical[~is_nan_bits(logical)])
        zeros = np.isin(nonnan, keys_of(np.array([0, 0x80000000], U32)))
        assert np.unique(nonnan[~zeros]).size == (~zeros).sum(), c.id      # distinct apart from the pair +0, -0


# ------------------------------------------------------------------------------------------------ percentile initialisation
PCT_SHAPES = [(n, bucket, k) for n in (2000, 70001) for bucket in (256, None) for k in (4, 16, 33)]
PCT_SHAPE_IDS = ['n%d-b%s-k%d' % s for s in PCT_SHAPES]
PCT_POISONS = [('clean', None, None)] + [(name, bits, pos) for name, bits in
                                         (('nan+', 0x7FC00000), ('nan-', 0xFFC00000), ('inf+', POS_INF), ('inf-', NEG_INF))
                                         for pos in ('first', 'middle', 'last')]


def percentile_input(n, poison_bits, pos):
    """Seeded N(0, 0.05) values (the legacy RandomState stream, which numpy keeps frozen) with one element overwritten by a
    bit pattern: with bucket 256 that is one poisoned bucket among clean ones ('last': the padded one), without buckets the
    whole tensor.  -> float32 numpy array"""
    x = (np.random.RandomState(1000 + n).randn(n) * 0.05).astype(F32)
    if poison_bits is not None:
        x.view(U32)[dict(first=0, middle=n // 2, last=n - 1)[pos]] = poison_bits
    return x


def percentile_cases(shape):
    """[(id, x, bucket, k)] of one (n, bucket, k): clean, and each poison at each position."""
    n, bucket, k = shape
    return [('n%d-b%s-k%d-%s%s' % (n, bucket, k, name, '-' + pos if pos else ''), percentile_input(n, bits, pos), bucket, k)
            for name, bits, pos in PCT_POISONS]


def same_points(got, want, tag=None):
    """Quantization points: bit for bit, any NaN equal to any NaN."""
    got, want = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(U32), want[~nan].view(U32)), (tag, got, want)
