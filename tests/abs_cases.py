"""The cases of the 'absmax' / 'absnorm' scaling types (csrc/qd_abs.hip), shared by tests/test_hip_abs.py (device) and
tests/test_abs_cases_host.py (the oracle against torch's CPU ops, and the structural claims made below).  Imports without a
GPU.  The rules the cases pin are in include/qd_hip.h (NaN / inf section, abs paragraph).

A case is (id, x, bucket, kind, s, options): x 1-D fp32, bucket an int or None, kind 'absmax' / 'absnorm', s the level count,
options a dict -- subtract_mean, max_element, and for a non-finite case `planted`, the positions that hold a NaN or an
infinity.  The generators are lazy: a case's data exists while the case runs.

Expected values come from oracle/oracle_np.py: sign, u, q and the way back are exact GIVEN the norm (and the mean) the
implementation under test reports (`expect`); the norm itself is held by `check_norm` -- absmax bit for bit, absnorm to
`BOUND` where the bucket's norm is an ordinary number and to its class (NaN / +inf / replaced by 1) elsewhere.

The paths of run_abs and what reaches them:
  loop_cases       one wave per bucket: a tail under one wave, exactly one wave, several trips of a wave, ragged last buckets
  many_cases       more buckets than the capped grid has waves (65536 blocks x 4): the second trip of the bucket loop
  single_cases     one bucket: one wave up to 65536 elements, the two-stage norm (k_abs_partial / k_abs_final) above, its
                   grid-stride trip above 1024 blocks x 8192 elements, a bucket argument larger than the tensor
  option_cases     subtract_mean x max_element (the Python API adds modify_in_place and the tensor forms)
  nonfinite_cases  NaN / inf by pattern and position
  scale_cases      overflow and underflow of the squares, the 1e-10 guard and its edge
  absorbed_cases   absnorm: layouts in which an fp32 running sum per lane or thread loses every small square
NOT covered: the second trip of the apply loop of the two-stage path (more than 65536 x 4 chunks of 4096 elements) and of
k_abs_inverse (more than 65536 x 256 x 8 elements): each needs more than 1e8 elements."""
import collections

import numpy as np

import errlog
from oracle import oracle_np as onp

F32 = np.float32
Case = collections.namedtuple('Case', 'id x bucket kind s options')
KINDS = ('absmax', 'absnorm')

# |norm_dev - norm64| <= BOUND * norm64 with norm64 = sqrt(sum x^2) in float64 from exact squares: half the project's 1e-6 on
# the sum of squares (errlog.TOL; a relative error e of the sum is e / 2 of its root), fp32 squares fused or not (2^-24 of
# each, so 2^-25 of the norm), the fp32 rounding of the sum (2^-25), sqrtf (2^-24) -- 2^-23 together, and a factor two in hand.
BOUND = 5e-7 + 2.0 ** -22
TOL_ONE = F32(1e-10)                 # QD_TOL_DIFF_ZERO: a norm below it is replaced by 1
FLT_MAX = float(np.finfo(np.float32).max)

# k_abs_partial's launch (run_abs): 256 threads, 8192 elements per block, at most 1024 blocks, grid-stride
TWO_STAGE_ABOVE = 65536
PART_THREADS, PART_PER_BLOCK, PART_MAX_BLOCKS = 256, 256 * 32, 1024
GRID_MAX_BLOCKS, WAVES_PER_BLOCK = 65536, 4


def partial_blocks(n):
    """Blocks of the k_abs_partial launch on n elements: nblocks(n, 256 * 32) capped at kParts."""
    return max(1, min(-(-n // PART_PER_BLOCK), PART_MAX_BLOCKS))


def partial_block_of(i, n):
    """The block of k_abs_partial that reads element i (a grid-stride loop over 256-element slabs)."""
    return (i // PART_THREADS) % partial_blocks(n)


def is_two_stage(n, bucket):
    return onp.bucket_geometry(n, bucket)[0] == 1 and n > TWO_STAGE_ABOVE


def _case(id_, x, bucket, kind, s=8, **options):
    x = np.ascontiguousarray(x, dtype=F32)
    assert x.ndim == 1 and x.size >= 1
    return Case(id_, x, bucket, kind, int(s), options)


def random_data(n, seed, zeros_from=0):
    """randn with exact zeros every 97 elements and a few -0.0."""
    x = np.random.RandomState(seed).randn(n).astype(F32)
    x[zeros_from::97] = 0.0
    x[zeros_from + 31::193] = -0.0
    return x


# ---------------------------------------------------------------- groups
LOOP_BUCKETS = (1, 2, 7, 63, 64, 65, 100, 256, 1000, 4097)
LOOP_LEVELS = (2, 3, 8, 256, 1000)
LOOP_SEEDS = (0, 1, 2)


def loop_lengths(bucket):
    ns = (1, bucket - 1, bucket, bucket + 1, 3 * bucket + -(-bucket // 2))
    return sorted(set(n for n in ns if n >= 1))


def loop_cases(kind, bucket):
    for n in loop_lengths(bucket):
        for seed in LOOP_SEEDS:
            x = random_data(n, 1000 * seed + 7 * bucket + n % 1000)
            for s in LOOP_LEVELS:
                yield _case('loop-%s-b%d-n%d-s%d-seed%d' % (kind, bucket, n, s, seed), x, bucket, kind, s)


MANY_N, MANY_BUCKET = 600001, 2


def many_cases(kind):
    yield _case('many-%s-b%d-n%d' % (kind, MANY_BUCKET, MANY_N), random_data(MANY_N, 77), MANY_BUCKET, kind)


SINGLE_LENGTHS = (1, 63, 64, 65, 5000, 65536, 65537)
SINGLE_BIG_N = 2 ** 23 + 2 ** 20 + 5         # more than 1024 blocks x 8192: k_abs_partial's grid-stride trip (38 MB)


def single_cases(kind, which):
    """which: 'small' (bucket None at SINGLE_LENGTHS, bucket 100000 on 70000 elements) or 'big'."""
    if which == 'small':
        for n in SINGLE_LENGTHS:
            yield _case('single-%s-n%d' % (kind, n), random_data(n, 300 + n % 97, zeros_from=5), None, kind)
        yield _case('single-%s-n70000-b100000' % kind, random_data(70000, 399, zeros_from=5), 100000, kind)
    else:
        yield _case('single-%s-n%d' % (kind, SINGLE_BIG_N), random_data(SINGLE_BIG_N, 398, zeros_from=5), None, kind)


OPTION_SHAPES = ((1000, 256), (257, 256), (70001, None))
CLIP_TENTH = float(F32(1.645))               # |randn| exceeds it for about a tenth of the elements


def option_cases(kind):
    for n, bucket in OPTION_SHAPES:
        x = random_data(n, 500 + n % 89)
        x += F32(0.25)                        # a mean worth subtracting
        for sub in (False, True):
            for me in (False, CLIP_TENTH):
                yield _case('opt-%s-n%d-b%s-mean%d-clip%d' % (kind, n, bucket, sub, me is not False), x, bucket, kind,
                            subtract_mean=sub, max_element=me)


def _nan(bits):
    return np.array([bits], np.uint32).view(F32)[0]


# name -> the values planted at the position and, for the two-element patterns, at its neighbour
NONFINITE_VALUES = collections.OrderedDict([
    ('nan', (_nan(0x7FC00000),)), ('nan_neg', (_nan(0xFFC00000),)), ('nan_payload', (_nan(0x7FC12345),)),
    ('pinf', (F32(np.inf),)), ('ninf', (F32(-np.inf),)), ('both', (F32(np.inf), F32(-np.inf))), ('nan_inf', (_nan(0x7FC00000), F32(np.inf))),
])
NONFINITE_SHAPES = ((1000, 256), (257, 256), (300, 100), (5000, None), (70001, None))
PAST_FIRST_PARTIAL = 8192 * 3 + 77


def nonfinite_positions(n, bucket):
    """name -> position: the first element, the last element of a middle bucket, the last element (the source of the padding
    where the tensor is ragged); on the two-stage path an element past index 8192 * 3."""
    pos = collections.OrderedDict([('first', 0)])
    if bucket is not None:
        nb = onp.bucket_geometry(n, bucket)[0]
        pos['mid_last'] = ((nb - 1) // 2 + 1) * bucket - 1
    if is_two_stage(n, bucket):
        pos['past'] = PAST_FIRST_PARTIAL
    pos['last'] = n - 1
    return pos


def plant_at(base, values, p):
    x = np.array(base, dtype=F32, copy=True)
    where = [p] if len(values) == 1 else [p, p + 1 if p + 1 < x.size else p - 1]
    for i, v in zip(where, values):
        x[i] = v
    return x, np.array(sorted(where), np.int64)


def nonfinite_cases(kind, shape):
    """The seven patterns at every position of the shape; a whole middle bucket of NaN; the seven PATTERNS of
    tests/nonfinite_cases.py where the tensor is long enough for their fixed positions; subtract_mean once."""
    from nonfinite_cases import PATTERNS, plant
    n, bucket = shape
    base = random_data(n, 600 + n % 83)
    tag = 'nonfinite-%s-n%d-b%s' % (kind, n, bucket)
    for pname, p in nonfinite_positions(n, bucket).items():
        for vname, values in NONFINITE_VALUES.items():
            x, planted = plant_at(base, values, p)
            yield _case('%s-%s-%s' % (tag, vname, pname), x, bucket, kind, planted=planted)
    if bucket is not None:
        b = (onp.bucket_geometry(n, bucket)[0] - 1) // 2
        x = base.copy()
        x[b * bucket:(b + 1) * bucket] = np.nan
        yield _case(tag + '-nan-bucket', x, bucket, kind, planted=np.arange(b * bucket, (b + 1) * bucket, dtype=np.int64))
    if n >= 2000:
        for pattern in PATTERNS:
            x = plant(base, pattern, bucket)
            yield _case('%s-shared-%s' % (tag, pattern), x, bucket, kind, planted=np.nonzero(~np.isfinite(x))[0])
    if shape == NONFINITE_SHAPES[0]:
        x, planted = plant_at(base, NONFINITE_VALUES['nan'], 300)
        yield _case(tag + '-nan-subtract-mean', x, bucket, kind, planted=np.arange(n, dtype=np.int64), subtract_mean=True)


def scale_cases():
    """(the kind is part of the case: the overflow rules are absnorm's, the edge of the guard is absmax's)"""
    mid = random_data(768, 700)
    for kind in KINDS:
        yield _case('scale-%s-1e-30' % kind, np.full(256, 1e-30), 256, kind)                     # squares underflow to 0; max < 1e-10
        den = np.full(300, 1e-40, F32)
        den[::3] = -3e-42
        yield _case('scale-%s-denormal' % kind, den, 100, kind)
        z = mid.copy()
        z[256:512] = 0.0
        z[300] = -0.0
        yield _case('scale-%s-zero-bucket' % kind, z, 256, kind)
    yield _case('scale-absnorm-1e20', np.full(256, 1e20), 256, 'absnorm')                         # every square overflows: +inf
    x = mid.copy()
    x[256:512] = 1e20
    x[300] = -1e20
    yield _case('scale-absnorm-1e20-middle', x, 256, 'absnorm', planted=np.arange(256, 512, dtype=np.int64))
    yield _case('scale-absnorm-1e20-two-stage', np.full(70001, 1e20), None, 'absnorm')
    yield _case('scale-absnorm-1e17', np.full(256, 1e17), 256, 'absnorm')                         # finite: sum 2.56e36
    yield _case('scale-absnorm-1e17-ragged', np.full(300, -1e17), 256, 'absnorm')
    edge = F32(1e-10)
    for name, top in (('at-guard', edge), ('below-guard', np.nextafter(edge, F32(0.0)))):
        x = (np.abs(random_data(256, 701)) * top / F32(8.0)).astype(F32)
        x[17], x[200] = -top, top
        assert np.abs(x).max() == top
        yield _case('scale-absmax-%s' % name, x, 256, 'absmax')


ABSORB_N = 65536


def _absorbed(n, head, big, small, reverse=False):
    x = np.full(n, small, F32)
    if reverse:
        x[n - head:] = big
    else:
        x[:head] = big
    return x


def absorbed_cases(kind='absnorm'):
    """Every lane's (one wave per bucket: element l, l + 64, ...) or thread's (k_abs_partial: element t, t + blocks x 256, ...)
    FIRST element is large, the rest have squares just under half an ulp of the large square: 0.49 against 2^24 (half an ulp
    is 1), 15.21 against 2^28 (16).  The last two are the controls: the same values, small first."""
    one = _absorbed(ABSORB_N, 64, 4096.0, 0.7)
    yield _case('absorbed-%s-one-wave' % kind, one, None, kind)
    yield _case('absorbed-%s-three-buckets' % kind, np.tile(one, 3), ABSORB_N, kind)
    n = 2 ** 20
    head = partial_blocks(n) * PART_THREADS
    yield _case('absorbed-%s-two-stage' % kind, _absorbed(n, head, 16384.0, 3.9), None, kind)
    yield _case('absorbed-%s-one-wave-reversed' % kind, _absorbed(ABSORB_N, 64, 4096.0, 0.7, reverse=True), None, kind)
    yield _case('absorbed-%s-two-stage-reversed' % kind, _absorbed(n, head, 16384.0, 3.9, reverse=True), None, kind)


ABSORBED_BITING = 3                           # the first three of absorbed_cases


def naive_lane_norm(case):
    """What an fp32 running sum per lane / per thread gives (everything after the lanes in float64, in its favour)."""
    rows = prepared_rows(case)
    stride = partial_blocks(case.x.size) * PART_THREADS if is_two_stage(case.x.size, case.bucket) else 64
    out = []
    for r in rows:
        sq = (r * r).astype(F32)
        pad = (-sq.size) % stride
        lanes = np.concatenate([sq, np.zeros(pad, F32)]).reshape(-1, stride)
        run = np.add.accumulate(lanes, axis=0, dtype=F32)[-1]
        out.append(np.sqrt(run.astype(np.float64).sum()))
    return np.array(out)


def all_groups():
    """(group name, generator) of every case, for the host checks."""
    for kind in KINDS:
        for bucket in LOOP_BUCKETS:
            yield 'loop', loop_cases(kind, bucket)
        yield 'many', many_cases(kind)
        yield 'single', single_cases(kind, 'small')
        yield 'option', option_cases(kind)
        for shape in NONFINITE_SHAPES:
            yield 'nonfinite', nonfinite_cases(kind, shape)
        yield 'absorbed', absorbed_cases(kind)
    yield 'scale', scale_cases()


# ---------------------------------------------------------------- expectations
def _opts(case, mean):
    o = case.options
    return dict(max_element=o.get('max_element', False), subtract_mean=bool(o.get('subtract_mean', False)), mean=mean)


def expect(case, norm=None, mean=None):
    """The oracle's sign, u (padded bucket layout, flattened), norm, q and the way back of u, given the norms and the mean the
    implementation under test reports."""
    e = onp.uniform_quantize_abs(case.x, case.s, case.bucket, case.kind, norm, **_opts(case, mean))
    e['back'] = onp.inv_scale_down_abs(e['u'], e['sign'], e['norm'], e['mean'], e['n'], e['shape'])
    e['u'], e['sign'] = e['u'].reshape(-1), e['sign'].reshape(-1)
    return e


def prepared_rows(case, mean=None):
    """x after mean subtraction and clamping, as padded bucket rows (2-D fp32)."""
    o = _opts(case, mean)
    v = case.x.copy()
    with np.errstate(invalid='ignore'):
        if o['subtract_mean']:
            v = (v - (F32(np.mean(v, dtype=np.float64)) if mean is None else F32(mean))).astype(F32)
        if o['max_element'] is not False:
            v = np.clip(v, -F32(o['max_element']), F32(o['max_element'])).astype(F32)       # (np.clip keeps a NaN, as the kernels do)
    return onp.bucketize(v, case.bucket).reshape(onp.bucket_geometry(v.size, case.bucket)[0], -1)


NormRef = collections.namedtuple('NormRef', 'norm raw norm64 cls')


def norm_reference(case, mean=None):
    """Per bucket: the oracle's norm, the same before the 1e-10 guard, sqrt(sum x^2) in float64 from exact squares, and the
    class: 'nan', 'inf', 'one' (replaced by 1) or 'num'."""
    m = np.abs(prepared_rows(case, mean))
    raw = onp.abs_norm(m, case.kind).reshape(-1)
    with np.errstate(invalid='ignore', over='ignore'):
        norm64 = np.sqrt((m.astype(np.float64) ** 2).sum(axis=1)) if case.kind == 'absnorm' else m.max(axis=1).astype(np.float64)
        cls = np.where(np.isnan(raw), 'nan', np.where(np.isinf(raw), 'inf', np.where(raw < TOL_ONE, 'one', 'num')))
        norm = np.where(raw < TOL_ONE, F32(1.0), raw).astype(F32)
    return NormRef(norm, raw, norm64, cls)


def overflow_margin(case, mean=None):
    """absnorm: a bucket's sum of squares is at most 2^126 -- a factor four under FLT_MAX, so no summation order overflows
    where another does not -- or it holds a NaN / an infinity, or every one of its squares overflows.  Checked in float64."""
    m = np.abs(prepared_rows(case, mean)).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        sq = m * m
        total = sq.sum(axis=1)
    ok = (total <= 2.0 ** 126) | ~np.isfinite(m).all(axis=1) | (sq > FLT_MAX).all(axis=1)
    return bool(ok.all())


def bits_same(got, want):
    """Bit for bit: the same shape, a NaN (any payload) exactly where a NaN is expected, and the same 32 bits elsewhere -- so
    the sign of a zero and of an infinity count, which np.array_equal on floats does not see."""
    got = np.ascontiguousarray(_np(got), dtype=F32).reshape(-1)
    want = np.ascontiguousarray(_np(want), dtype=F32).reshape(-1)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]))


def sign_same(got, want):
    """The sign output: +-1 bit for bit, and == 0 (either zero) where 0 is expected; never a NaN."""
    got, want = _np(got).reshape(-1), _np(want).reshape(-1)
    return bool(got.shape == want.shape and not np.isnan(got).any() and np.array_equal(got, want))


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, 'detach') else np.asarray(a)


def check_norm(case, got, mean=None, log_kind=None):
    """Hold the per-bucket norms `got` to the reference: absmax bit for bit; absnorm within BOUND of norm64 where the norm is
    an ordinary number, and NaN / +inf / exactly 1 where the oracle's is.  Returns the worst |got - norm64| / norm64 (0 where
    none applies).  log_kind: record it in the reduction-error log under this kind (tests/errlog.py)."""
    ref = norm_reference(case, mean)
    got = np.asarray(_np(got), dtype=F32).reshape(-1)
    assert got.shape == ref.norm.shape, (case.id, got.shape, ref.norm.shape)
    if case.kind == 'absmax':
        assert bits_same(got, ref.norm), (case.id, 'absmax norm', got[:8], ref.norm[:8])
        return 0.0
    assert np.array_equal(np.isnan(got), ref.cls == 'nan'), (case.id, 'NaN norms', got[:8], ref.cls[:8])
    assert np.array_equal(got == np.inf, ref.cls == 'inf'), (case.id, '+inf norms', got[:8], ref.cls[:8])
    one = ref.cls == 'one'
    assert np.all(got[one] == F32(1.0)), (case.id, 'norms below 1e-10 are replaced by 1', got[one][:8])
    num = ref.cls == 'num'
    ratio = 0.0
    if num.any():
        ratio = float(np.max(np.abs(got[num].astype(np.float64) - ref.norm64[num]) / ref.norm64[num]))
    if log_kind is not None and num.any():
        errlog.check_norm(log_kind, got[num], ref.norm64[num], case.id, tol=BOUND, n_terms=prepared_rows(case, mean).shape[1])
    assert ratio <= BOUND, (case.id, '|norm - norm64| / norm64 = %.3g > %.3g' % (ratio, BOUND))
    return ratio


def clean_elements(case):
    """Non-finite cases: mask (unpadded) of the elements whose bucket holds no planted position, and the input with every
    planted element replaced by 1.0 -- on those elements both inputs must give the same bits."""
    n = case.x.size
    nb, row, _ = onp.bucket_geometry(n, case.bucket)
    planted = np.asarray(case.options['planted'], np.int64)
    dirty = np.zeros(nb, bool)
    dirty[planted // row] = True
    x1 = case.x.copy()
    x1[planted] = 1.0
    return ~np.repeat(dirty, row)[:n], ~dirty, x1
