"""The second and later trips of every grid-stride loop, at shapes of a few thousand elements, against the oracle.

The launchers give every wave one tile, so in the rest of the suite the loops `for (t = wave; t < ntiles; t += nwaves)` of the
kernels run once.  qd_set_grid_cap (include/qd_hip.h, a test hook) caps the grids at 1, 2 and 3 blocks; every case here is
chosen (tests/grid_trip_cases.py, held on the CPU by tests/test_grid_trip_cases.py) so that every worker then makes at least three
trips, the last one partial, next to a ragged tail -- and asserts that from the plan before it runs.  Every output is compared
bit for bit with the oracle AND with the same call under the default cap, starts as a sentinel NaN (an element no trip wrote
shows), and sits between guard elements.  A kernel without a loop, a wrong stride, a tail owner that needs more blocks than
tiles, a per-trip value hoisted out of the loop or an LDS table overwritten by a faster wave fails here."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle_c as oc
from quantized_distillation_amd import _lib

import abi_contract as A
import grid_trip_cases as C
import stochastic_cases as S
from test_hip_property import make
from test_transform_plan import NEAREST, QDQ, SCALE, queries

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
SENT_BITS = 0x7FC0BEEF                      # a quiet NaN no kernel produces
PHASES = (0, 4)                             # bytes: the 16-byte phase of the fp32 data pointers
GUARD = 8                                   # elements around every output


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


@pytest.fixture(scope='module')
def cases(lib):
    return C.find_cases(lib)


# ------------------------------------------------------------------------------------------------ buffers
class Out(object):
    """A device output of `count` elements at byte phase `phase` of a 16-byte granule, sentinel-filled, guarded both sides."""

    def __init__(self, dtype, count, phase=0):
        self.np_dtype = np.dtype(dtype)
        size = self.np_dtype.itemsize
        assert phase % size == 0 or size == 1
        lead = 16 * GUARD + phase                                             # bytes
        self.lead, self.count = lead, count
        total = lead + count * size + 16 * GUARD
        self.raw = torch.empty((total + 15) // 16 * 16, dtype=torch.uint8, device=DEV)
        assert self.raw.data_ptr() % 16 == 0
        self.fill = np.frombuffer(np.array([SENT_BITS], np.uint32).tobytes() * (self.raw.numel() // 4), np.uint8)
        self.raw.copy_(torch.from_numpy(self.fill.copy()))
        self.ptr = self.raw.data_ptr() + lead

    def get(self):
        """The output as numpy, after checking that nothing outside it was written and nothing inside it was left alone."""
        h = self.raw.cpu().numpy()
        size = self.np_dtype.itemsize
        end = self.lead + self.count * size
        assert np.array_equal(h[:self.lead], self.fill[:self.lead]) and np.array_equal(h[end:], self.fill[end:]), 'written outside the output'
        v = h[self.lead:end].copy().view(self.np_dtype)
        if size == 4:
            assert not np.any(v.view(np.uint32) == SENT_BITS), ('elements no trip wrote', np.flatnonzero(v.view(np.uint32) == SENT_BITS)[:8])
        return v


def inp(a, phase=0):
    """A device copy of `a` whose first byte sits at `phase` of a 16-byte granule; -> (keep-alive tensor, pointer)."""
    a = np.ascontiguousarray(a)
    raw = torch.zeros((a.nbytes + phase + 31) // 16 * 16, dtype=torch.uint8, device=DEV)
    raw[phase:phase + a.nbytes].copy_(torch.from_numpy(a.view(np.uint8).reshape(-1).copy()))
    return raw, raw.data_ptr() + phase


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ one transform call
def points(k):
    return A.points(k)


def call_transform(lib, mode, x, bucket, phase, opt):
    """One call of qd_uniform_f32 / qd_scale_down_f32 / qd_nearest_point_f32 through the C ABI; -> {name: numpy}."""
    n = x.size
    nb = int(lib.qd_num_buckets(n, bucket))
    padded = int(lib.qd_padded_length(n, bucket))
    ws = _lib.workspace(torch.device(DEV))
    tail = (ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    keep, xp = inp(x, phase)
    outs = {}
    if not opt.get('prescaled'):
        outs['alpha'], outs['beta'] = Out(F32, nb, 4), Out(F32, nb, 12)
    mean = opt.get('mean')
    mkeep, mp = inp(np.array([mean], F32), 8) if mean is not None else (None, None)
    me = opt.get('me')
    if mode == QDQ:
        outs['q'] = Out(F32, n, phase)
        if opt.get('lev'):
            outs['lev'] = Out(np.uint8, n, opt.get('lev_phase', 0))
        rc = lib.qd_uniform_f32(xp, outs['q'].ptr, n, bucket, opt.get('levels', 16), outs['alpha'].ptr, outs['beta'].ptr,
                                outs['lev'].ptr if 'lev' in outs else None, mp, int(me is not None), float(me or 0.0),
                                int(bool(opt.get('stochastic'))), ctypes.c_uint64(opt.get('seed', 0)), *tail)
    elif mode == SCALE:
        outs['u'] = Out(F32, padded, phase)
        rc = lib.qd_scale_down_f32(xp, outs['u'].ptr, n, bucket, outs['alpha'].ptr, outs['beta'].ptr, mp, int(me is not None),
                                   float(me or 0.0), *tail)
    else:
        k, idx_bytes = opt.get('k', 16), opt.get('idx_bytes', 8)
        pkeep, pp = inp(points(k), 0)
        if not opt.get('q_null'):
            outs['q'] = Out(F32, n, phase)
        outs['idx'] = Out(np.int64 if idx_bytes == 8 else np.uint8, n, opt.get('idx_phase', 0))
        if opt.get('prescaled'):
            akeep, ap = inp(opt['alpha'], 4)
            bkeep, bp = inp(opt['beta'], 12)
        else:
            ap, bp = outs['alpha'].ptr, outs['beta'].ptr
        rc = lib.qd_nearest_point_f32(xp, int(bool(opt.get('prescaled'))), pp, k, opt.get('assign_mode', 0),
                                      outs['q'].ptr if 'q' in outs else None, outs['idx'].ptr, idx_bytes, n, bucket, ap, bp, None, 0, 0.0,
                                      *tail)
    assert rc == 0, (rc, mode, n, bucket, opt)
    torch.cuda.synchronize()
    return {name: o.get() for name, o in outs.items()}


def expected(mode, x, bucket, opt):
    """The oracle's outputs of the same call (x: the ORIGINAL tensor, also for the pre-processed forward)."""
    n = x.size
    b = bucket or None
    if mode == QDQ:
        if opt.get('stochastic'):
            r = S.oracle(x, opt.get('levels', 16), opt['seed'], b)
        else:
            r = oc.uniform_quantize(x, opt.get('levels', 16), b, max_element=opt.get('me') or False, subtract_mean=opt.get('mean') is not None,
                                    mean=opt.get('mean'), want_idx=False)
        want = dict(q=r['q'].reshape(-1), alpha=r['alpha'].reshape(-1), beta=r['beta'].reshape(-1))
        if opt.get('lev'):
            lev = np.asarray(r['lev']).reshape(-1)[:n]
            nan = np.isnan(want['q'])                                        # a NaN level is stored as 0 (include/qd_hip.h)
            want['lev'] = np.where(nan, 0, lev).astype(np.uint8)
        return want
    if mode == SCALE:
        r = oc.scale_down(x, b, max_element=opt.get('me') or False, subtract_mean=opt.get('mean') is not None, mean=opt.get('mean'))
        pad = int(r['alpha'].size * (bucket if bucket and n >= bucket else n)) - n
        u = np.concatenate([r['u'], np.full(pad, r['u'][n - 1], F32)])       # help_functions.py:76-86: copies of the last element
        return dict(u=u, alpha=r['alpha'], beta=r['beta'])
    r = oc.nonuniform_quantize(x, points(opt.get('k', 16)), b, 'midpoint' if opt.get('assign_mode', 0) == 1 else 'distance')
    want = dict(idx=r['idx'].reshape(-1).astype(np.int64 if opt.get('idx_bytes', 8) == 8 else np.uint8))
    if not opt.get('q_null'):
        want['q'] = r['q'].reshape(-1)
    if not opt.get('prescaled'):
        want['alpha'], want['beta'] = r['alpha'], r['beta']
    return want


def query_of(mode, n, bucket, phase, opt, base):
    """The plan query of a call (what plan_call derives from the pointers)."""
    q = dict(base)
    q.pop('fused_capacity', None)
    if mode == QDQ and opt.get('lev'):
        q.update(side_bytes=1, side_misalign=opt.get('lev_phase', 0))
    if mode == NEAREST:
        q.update(k=opt.get('k', 16), assign_mode=opt.get('assign_mode', 0), side_bytes=opt.get('idx_bytes', 8),
                 side_misalign=opt.get('idx_phase', 0), prescaled=int(bool(opt.get('prescaled'))), q_null=int(bool(opt.get('q_null'))))
    return queries(mode, n, bucket, data_misalign=phase, fused_capacity=0 if 'fused_mode' in opt else 256, cus=256, **q)


def data_for(mode, n, bucket, seed, nan_bucket):
    """kind 7 of test_hip_property.make for the uniform modes: a new power-of-two scale every 97 elements, so the buckets and
    chunks one wave visits fall on both sides of the bucket-invariant-division range (div_ok differs from trip to trip).  One
    bucket two thirds into the tensor -- a second-or-later trip of every worker's, see run_case -- holds a NaN."""
    x = make(n, seed, 7 if mode != NEAREST else 0)
    where = None
    if nan_bucket and bucket:
        where = (2 * (n // bucket) // 3) * bucket + 1
        x[where] = np.nan
    return x, where


def run_case(lib, case, opt, seed, nan_bucket=True):
    """The case at its lengths and both phases: the plan's trips asserted, the default-cap call against the oracle, the capped
    calls against the oracle and, bit for bit, against the default-cap call."""
    opt = dict(case.call, **opt)
    mode, bucket = case.mode, case.bucket
    compared = 0
    prev_mode = lib.qd_set_single_fused_mode(opt['fused_mode']) if 'fused_mode' in opt else None
    try:
        for n in C.lengths_of(case):
            x, nan_at = data_for(mode, n, bucket, seed + n % 89, nan_bucket and not opt.get('stochastic'))
            call_x, o = x, dict(opt)
            if opt.get('prescaled'):                                         # the pre-processed forward: u, alpha, beta are inputs
                r = oc.scale_down(x, bucket or None)
                call_x, o['alpha'], o['beta'] = r['u'], r['alpha'], r['beta']
            want = expected(mode, x, bucket, opt)
            for phase in PHASES:
                q = query_of(mode, n, bucket, phase, opt, case.query)
                ps = C.plans_under_caps(lib, q)
                kernels = [ps[None]['launch'][0, j]['kernel'].decode() for j in range(ps[None]['nlaunch'][0])]
                assert C.family_of(case.kernel) in [C.family_of(k) for k in kernels], (case.kernel, kernels, n, phase, opt)
                for cap in C.CAPS:
                    for j, kernel in enumerate(kernels):
                        if C.family_of(kernel) in C.NOT_LOOPED:
                            continue
                        p = ps[cap]
                        assert p['launch'][0, j]['kernel'].decode() == kernel
                        units, workers, per_block, trips = C.trip_stats(kernel, p, p['launch'][:, j], np.array([n]))
                        assert trips[0] >= C.MIN_TRIPS, (kernel, n, cap, int(units[0]), int(workers[0]))
                        assert workers[0] == 1 or units[0] % workers[0] != 0, (kernel, n, cap, 'no partial last trip')
                        if nan_at is not None:                               # the NaN bucket is nobody's first trip
                            assert nan_at * units[0] // n >= workers[0], (kernel, n, cap, nan_at)
                got0 = None
                for cap in (None,) + C.CAPS:
                    with C.Capped(lib, cap):
                        got = call_transform(lib, mode, call_x, bucket, phase, o)
                    tag = (case.kernel, n, phase, cap, sorted(opt.items()))
                    assert sorted(got) == sorted(want), tag
                    for name in sorted(want):
                        assert np.array_equal(got[name], want[name], equal_nan=got[name].dtype.kind == 'f'), \
                            tag + (name, 'differs from the oracle', np.flatnonzero(~((got[name] == want[name]) | ((got[name] != got[name]) & (want[name] != want[name]))))[:8])
                    compared += 1
                    if got0 is None:
                        got0 = got
                    for name in sorted(got):
                        assert same_bits(got[name], got0[name]), tag + (name, 'differs from the call under the default cap')
            if nan_at is not None and 'alpha' in want:
                assert np.isnan(want['alpha'][nan_at // bucket]) and np.isfinite(want['alpha']).sum() == want['alpha'].size - 1
    finally:
        if prev_mode is not None:
            lib.qd_set_single_fused_mode(prev_mode)
    assert compared == len(C.lengths_of(case)) * len(PHASES) * (1 + len(C.CAPS))
    return compared


# ------------------------------------------------------------------------------------------------ the transform kernels
FAMILIES = ['k_bucket_vec', 'k_bucket_chunk', 'k_bucket_chunk_any', 'k_bucket_wave_any', 'k_bucket_groups', 'k_bucket_generic',
            'k_minmax_partial', 'k_single_apply', 'k_nearest_prescaled_stream']

# options, varied once per family and mode (on its first instantiation) and not crossed with each other
QDQ_OPTIONS = [dict(stochastic=1, seed=0x5EED0123456789), dict(mean=0.25, me=1.5), dict(lev=1), dict(levels=256, lev=1), dict(levels=256)]
SCALE_OPTIONS = [dict(mean=-0.125)]
NEAREST_OPTIONS = [dict(assign_mode=1, k=4, idx_bytes=1), dict(assign_mode=1, k=33), dict(assign_mode=0, k=33, idx_bytes=1),
                   dict(assign_mode=1, k=65, idx_bytes=1), dict(assign_mode=1, k=256), dict(assign_mode=0, k=256, idx_bytes=1)]
STREAM_OPTIONS = [dict(k=4), dict(k=33, idx_bytes=8), dict(k=65), dict(k=256, idx_bytes=8), dict(k=16, assign_mode=0),
                  dict(k=65, q_null=1), dict(k=4, idx_bytes=8, q_null=1)]


def test_every_shipped_transform_instantiation_is_run_through_three_trips(cases):
    import launch_coverage
    want = C.wanted(launch_coverage.shipped())
    missing = sorted(k for k in want if k not in cases)
    # the exceptions, by name and with their reasons: grid_trip_cases.UNREACHED (proved from the plan in test_grid_trip_cases.py)
    assert missing == sorted(C.UNREACHED) == ['k_bucket_groups<1,64>'], missing
    assert sorted({C.family_of(k) for k in cases}) == sorted(FAMILIES)
    assert lib_cap_is_default()


def lib_cap_is_default():
    lib = _lib.load()
    prev = lib.qd_set_grid_cap(-1)
    return prev == C.GRID_CAP_DEFAULT


@pytest.mark.parametrize('family', FAMILIES)
def test_every_instantiation_loops_and_matches_the_oracle_under_caps_1_2_3(lib, cases, family):
    mine = [c for k, c in sorted(cases.items()) if C.family_of(k) == family]
    assert mine
    for i, case in enumerate(mine):
        run_case(lib, case, {}, seed=1000 + 7 * i)
    assert lib_cap_is_default()


@pytest.mark.parametrize('family', FAMILIES)
def test_the_options_of_every_mode_once_per_family_under_caps_1_2_3(lib, cases, family):
    mine = [c for k, c in sorted(cases.items()) if C.family_of(k) == family]
    for mode in (QDQ, SCALE, NEAREST):
        first = [c for c in mine if c.mode == mode][:1]
        for case in first:
            if family == 'k_nearest_prescaled_stream':
                options = STREAM_OPTIONS
            else:
                options = {QDQ: QDQ_OPTIONS, SCALE: SCALE_OPTIONS, NEAREST: NEAREST_OPTIONS}[mode]
                if family == 'k_single_apply' and mode == NEAREST:            # + the pre-processed forward of one bucket: the apply kernel alone
                    options = options + [dict(prescaled=1, assign_mode=1, k=16, idx_bytes=1)]
            for j, o in enumerate(options):
                run_case(lib, case, o, seed=5000 + 11 * j)
    assert lib_cap_is_default()


# ------------------------------------------------------------------------------------------------ the other launch sites
# Every launcher outside the transform plan sizes its grid as grid_blocks(items, per_block, own cap) (csrc/qd_common.h):
# min(ceil(items / per_block), own cap, the hook's cap) blocks.  assert_trips() restates that line for the site under test and
# holds the shape to it: at least three trips for every worker under each cap, the last one partial.
def assert_trips(tag, units, items, per_block, workers_per_block, own_cap=1 << 30):
    for cap in C.CAPS:
        blocks = max(1, min(-(-items // per_block), own_cap, cap))
        workers = blocks * workers_per_block
        assert units // workers >= C.MIN_TRIPS, (tag, cap, units, workers)
        assert workers == 1 or units % workers != 0, (tag, cap, units, workers, 'no partial last trip')


def under_every_cap(lib, run, check=None, exact=True):
    """run() -> {name: numpy} under the default cap and caps 1, 2, 3; check(outputs, cap) holds each to the oracle; with
    `exact` the capped outputs equal the default-cap ones bit for bit.  Returns the outputs per cap."""
    outs = {}
    for cap in (None,) + C.CAPS:
        with C.Capped(lib, cap):
            outs[cap] = run()
        torch.cuda.synchronize()
        if check is not None:
            check(outs[cap], cap)
        if exact:
            for name in outs[None]:
                assert same_bits(np.asarray(outs[cap][name]), np.asarray(outs[None][name])), (name, cap, 'differs from the call under the default cap')
    return outs


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stream_tail():
    ws = _lib.workspace(torch.device(DEV))
    return ws.data_ptr(), ws.numel(), _lib.stream_ptr()


@pytest.mark.parametrize('bucket', [0, 33, 100])
def test_inverse_scaling_loops(lib, bucket):
    """k_inv_scale<TWO>: 4 KiB tiles over the waves of min(ceil(n / 4096), cap) blocks; bucket 33: a float4 straddles buckets."""
    n = 4 * (38 * 256 + 100) + 3
    assert_trips('k_inv_scale', -(-(n // 4) // 256), n, 256 * 4 * 4, 4)
    rng = np.random.RandomState(bucket)
    nb = int(lib.qd_num_buckets(n, bucket))
    u = rng.rand(n).astype(F32)
    alpha, beta = (rng.rand(nb) + 0.5).astype(F32), rng.randn(nb).astype(F32)
    row = bucket if bucket else n
    b = np.arange(n) // row
    for mean in (None, F32(0.375)):
        want = ((u * alpha[b]).astype(F32) + beta[b]).astype(F32) + (F32(0.0) if mean is None else mean)
        for phase in PHASES:
            ku, up = inp(u, phase)
            ka, ap = inp(alpha, 4)
            kb, bp = inp(beta, 8)
            km, mp = inp(np.array([mean], F32), 12) if mean is not None else (None, None)

            def run():
                y = Out(F32, n, phase)
                assert lib.qd_inv_scale_f32(up, y.ptr, n, bucket, ap, bp, mp, _lib.stream_ptr()) == 0
                torch.cuda.synchronize()
                return dict(y=y.get())
            under_every_cap(lib, run, lambda o, cap: np.testing.assert_array_equal(o['y'], want.astype(F32)))
    assert lib_cap_is_default()


def test_mean_argminmax_clamp_and_truncated_ste_loop(lib):
    import errlog
    n = 20003
    x = (np.random.RandomState(5).randn(n) * 3 + 1).astype(F32)
    x64 = x.astype(np.float64)
    # qd_mean_f32: float4s over the threads of min(ceil(n / 8192), 1024, cap) blocks
    assert_trips('k_sum_partial', n // 4, n, 256 * 4 * 8, 256, own_cap=1024)
    kx, xp = inp(x, 4)

    def run_mean():
        m = Out(F32, 1, 0)
        assert lib.qd_mean_f32(xp, n, m.ptr, *stream_tail()) == 0
        torch.cuda.synchronize()
        return dict(mean=m.get())
    under_every_cap(lib, run_mean, lambda o, cap: errlog.check_mean('qd_mean_f32 under a grid cap', o['mean'][0], x64.mean(), np.abs(x64).mean(),
                                                                  ('cap', cap), n_terms=n), exact=False)
    # qd_clamp_f32 / qd_truncated_ste_f32: float4s over the threads of min(ceil(n / 4096), cap) blocks
    assert_trips('k_clamp', n // 4, n, 256 * 4 * 4, 256)
    g = np.random.RandomState(6).randn(n).astype(F32)
    for phase in PHASES:
        def run_k8():
            kw = Out(F32, n, phase)
            kw.raw[kw.lead:kw.lead + 4 * n].copy_(torch.from_numpy(x.view(np.uint8).copy()))
            assert lib.qd_clamp_f32(kw.ptr, n, 1.25, _lib.stream_ptr()) == 0
            kg = Out(F32, n, phase)
            kg.raw[kg.lead:kg.lead + 4 * n].copy_(torch.from_numpy(g.view(np.uint8).copy()))
            kx2, xp2 = inp(x, phase)
            assert lib.qd_truncated_ste_f32(xp2, kg.ptr, n, 1.25, _lib.stream_ptr()) == 0
            torch.cuda.synchronize()
            return dict(w=kw.get(), g=kg.get())

        def check_k8(o, cap):
            assert np.array_equal(o['w'], np.clip(x, F32(-1.25), F32(1.25))) and np.array_equal(o['g'], np.where(np.abs(x) > F32(1.25), F32(0), g))
        under_every_cap(lib, run_k8, check_k8)
    # qd_bucket_argminmax_f32: one block per (bucket, chunk), min(nb * chunks, cap) blocks
    for nn, bucket in ((10 * 1000 + 3, 1000), (10 * 65536 + 5, 0)):
        xx = np.random.RandomState(nn % 97).randint(-50, 50, nn).astype(F32)        # ties: the FIRST occurrence wins
        nb = int(lib.qd_num_buckets(nn, bucket))
        chunks = 1 if nb > 1 else -(-nn // 65536)
        assert_trips('k_argminmax', nb * chunks, nb * chunks, 1, 1)
        ref = oc.scale_down(xx, bucket or None)
        kxx, xxp = inp(xx, 4)

        def run_arg():
            lo, hi = Out(np.int64, nb, 0), Out(np.int64, nb, 0)
            assert lib.qd_bucket_argminmax_f32(xxp, nn, bucket, None, 0, 0.0, lo.ptr, hi.ptr, *stream_tail()) == 0
            torch.cuda.synchronize()
            return dict(imin=lo.get(), imax=hi.get())
        under_every_cap(lib, run_arg, lambda o, cap: (np.testing.assert_array_equal(o['imin'], ref['imin']), np.testing.assert_array_equal(o['imax'], ref['imax'])))
    assert lib_cap_is_default()


@pytest.mark.parametrize('k,idx_bytes,kernel', [(4, 1, 'fast, register bins'), (16, 8, 'fast, LDS columns'), (100, 1, 'fast, half-wave columns'),
                                                (256, 1, 'turns'), (256, 8, 'turns'), (600, 8, 'any: k > 512'), (16, 81, 'any: idx off its alignment')])
@pytest.mark.parametrize('bucket', [0, 256, 100])
def test_point_gradient_loops(lib, k, idx_bytes, kernel, bucket):
    """K6 on its three kernels (qd_point_grad_f32: k_point_grad_fast / _turns / _any): the 1e-6 bound of the project against
    the float64 oracle under every cap, and bit-identical from run to run under the same cap."""
    import errlog
    misaligned = idx_bytes == 81
    idx_bytes = 8 if misaligned else idx_bytes
    n = 4 * 3 * 8 * 768 + 4 * 1000 + 3                                       # >= 3 rounds of 8 float4 per lane of 3 x 256 lanes, + a partial one
    # every kernel strides float4s (k_point_grad_any: elements) over the lanes of at most min(ceil(n / 2048), 512, cap) blocks
    assert_trips('k_point_grad_*', n // 4 // 8, n, 256 * 4 * 2, 256, own_cap=512)
    rng = np.random.RandomState(k + bucket)
    g = rng.randn(n).astype(F32)
    idx = rng.randint(0, k, n)
    nb = int(lib.qd_num_buckets(n, bucket))
    alpha = (rng.rand(nb) + 0.5).astype(F32)
    want, absum = oc.point_grad(g, idx.astype(np.int64), alpha, bucket or None, k)
    kg, gp = inp(g, 4)
    ki, ip = inp(idx.astype(np.int64 if idx_bytes == 8 else np.uint8), 8 if misaligned else 0)
    ka, ap = inp(alpha, 8)

    def run():
        out = Out(F32, k, 0)
        assert lib.qd_point_grad_f32(gp, ip, idx_bytes, ap, n, bucket, k, out.ptr, *stream_tail()) == 0
        torch.cuda.synchronize()
        return dict(grad=out.get())
    for cap in (None,) + C.CAPS:
        with C.Capped(lib, cap):
            a, b = run(), run()
        errlog.check_sum('K6 point gradient under a grid cap', a['grad'], want, absum, (kernel, k, bucket, cap), n_terms=n)
        assert same_bits(a['grad'], b['grad']), (kernel, k, bucket, cap, 'differs from run to run')
    assert lib_cap_is_default()


@pytest.mark.parametrize('tie_mode', ['reference', 'true_arg'])
@pytest.mark.parametrize('bucket,nbuckets', [(64, 199), (256, 199), (1024, 50), (33, 38), (1000, 38)])
def test_ste_bucket_backward_loops(lib, bucket, nbuckets, tie_mode):
    """K7 (qd_ste_bucket_backward_f32): the register tiles of k_ste_backward_vec (64 / lanes-per-bucket buckets per tile, four
    tiles per block) and the wave-per-bucket kernel k_ste_backward (four buckets per block) that also takes the ragged tail."""
    import errlog
    from quantized_distillation_amd import ste
    n = nbuckets * bucket + bucket - 1
    if bucket in (64, 256, 1024):
        bpw = 4 if bucket <= 256 else 1
        assert_trips('k_ste_backward_vec', -(-nbuckets // bpw), -(-nbuckets // bpw), 4, 4)
    else:
        assert_trips('k_ste_backward', nbuckets + 1, nbuckets + 1, 4, 4)
    x = make(n, 31 + bucket, 0 if bucket != 33 else 2)                        # (33: ties everywhere)
    g = np.random.RandomState(bucket).randn(n).astype(F32)
    xd, gd = dev(x), dev(g)

    def run():
        return dict(out=ste.ste_bucket_backward(xd, gd, bucket, 16, out=torch.empty_like(gd), tie_mode=tie_mode).cpu().numpy())
    under_every_cap(lib, run, lambda o, cap: errlog.check_ste('K7 bucket sum under a grid cap', o['out'], x, g, 16, bucket, (bucket, tie_mode, cap),
                                                            tie_mode=tie_mode))
    assert lib_cap_is_default()


def pack_bits(lev, bits):
    """Element e in bits [e * bits, (e + 1) * bits) of the stream, little endian inside a byte (include/qd_hip.h)."""
    per = 8 // bits
    lev = np.concatenate([lev.astype(np.uint8), np.zeros(-lev.size % per, np.uint8)]).reshape(-1, per)
    return (lev.astype(np.uint32) << (bits * np.arange(per, dtype=np.uint32))).sum(1).astype(np.uint8)


@pytest.mark.parametrize('bits', [1, 2, 4, 8])
def test_pack_and_unpack_loop(lib, bits):
    """qd_pack_uniform_f32 (k_pack_vec: tiles over waves), qd_pack_levels_u8 (32-bit words over threads), qd_unpack_uniform_f32
    (groups of four elements over threads: k_unpack at a power-of-two bucket, k_unpack_any elsewhere)."""
    s = 1 << bits
    sm1 = F32(s - 1)
    # pack: bucket 256, 16 lanes per bucket: 4 buckets per tile, 4 tiles per block
    nfull = 199
    n = nfull * 256 + 255
    assert_trips('k_pack_vec', -(-nfull // 4), -(-nfull // 4), 4, 4)
    x = make(n, 40 + bits, 7)
    r = oc.uniform_quantize(x, s, 256, want_idx=False)
    kx, xp = inp(x, 0)
    nbytes = int(lib.qd_packed_bytes(n, bits))

    def run_pack():
        pk, a, b = Out(np.uint8, nbytes, 0), Out(F32, nfull + 1, 4), Out(F32, nfull + 1, 8)
        assert lib.qd_pack_uniform_f32(xp, n, 256, s, bits, pk.ptr, a.ptr, b.ptr, _lib.stream_ptr()) == 0
        torch.cuda.synchronize()
        return dict(packed=pk.get(), alpha=a.get(), beta=b.get())

    def check_pack(o, cap):
        assert np.array_equal(o['packed'], pack_bits(r['lev'], bits)) and np.array_equal(o['alpha'], r['alpha']) and np.array_equal(o['beta'], r['beta'])
    under_every_cap(lib, run_pack, check_pack)
    # pack_levels: min(ceil((n / L + 1) / 1024), cap) blocks of 256 threads over n / L words of L = 32 / bits levels
    L = 32 // bits
    n2 = L * 2500 + L // 2 + 1
    assert_trips('k_pack_levels', n2 // L, n2 // L + 1, 256 * 4, 256)
    lev = np.random.RandomState(bits).randint(0, s, n2).astype(np.uint8)
    for phase in (0, 1):                                                     # the 16-byte loads of the levels, and the byte path
        kl, lp = inp(lev, phase)

        def run_levels():
            pk = Out(np.uint8, int(lib.qd_packed_bytes(n2, bits)), 0)
            assert lib.qd_pack_levels_u8(lp, n2, bits, pk.ptr, _lib.stream_ptr()) == 0
            torch.cuda.synchronize()
            return dict(packed=pk.get())
        under_every_cap(lib, run_levels, lambda o, cap: np.testing.assert_array_equal(o['packed'], pack_bits(lev, bits)))
    # unpack: min(ceil(ceil(n / 4) / 1024), cap) blocks of 256 threads over ceil(n / 4) groups
    n3 = 20003
    assert_trips('k_unpack', -(-n3 // 4), -(-n3 // 4), 256 * 4, 256)
    lev3 = np.random.RandomState(bits + 9).randint(0, s, n3).astype(np.uint8)
    kp, pp = inp(pack_bits(lev3, bits), 0)
    for bucket in (256, 33, 0):
        nb = int(lib.qd_num_buckets(n3, bucket))
        rng = np.random.RandomState(bucket + bits)
        alpha, beta = (rng.rand(nb) + 0.5).astype(F32), rng.randn(nb).astype(F32)
        bk = np.arange(n3) // (bucket or n3)
        want = ((((lev3.astype(F32) / sm1).astype(F32) * alpha[bk]).astype(F32) + beta[bk]).astype(F32) + F32(0.0)).astype(F32)
        ka, ap = inp(alpha, 4)
        kb, bp = inp(beta, 8)
        for phase in PHASES:
            def run_unpack():
                y = Out(F32, n3, phase)
                assert lib.qd_unpack_uniform_f32(pp, n3, bucket, s, bits, ap, bp, y.ptr, _lib.stream_ptr()) == 0
                torch.cuda.synchronize()
                return dict(y=y.get())
            under_every_cap(lib, run_unpack, lambda o, cap: np.testing.assert_array_equal(o['y'], want))
    assert lib_cap_is_default()


def test_histograms_loop(lib):
    """The counting entry points against np.bincount / np.digitize: every block's counters reach the fold whatever the grid."""
    import quantization.help_functions as qhf
    from quantized_distillation_amd import codec
    # uint8 symbols: 16-byte loads, U per lane and round, over the threads of min(ceil(n / 8192), 2 CUs, cap) blocks (with a
    # workspace; U = 2) or min(ceil(n / 16384), CUs, cap) (without; U = 4)
    n = 16 * 4 * 3 * 768 + 16 * 1000 + 7
    assert_trips('k_hist_atomic<2>', n // 16 // 2, n, 256 * 16 * 2, 256)
    assert_trips('k_hist_atomic<4>', n // 16 // 4, n, 256 * 16 * 4, 256)
    for k in (16, 256):
        sym = np.random.RandomState(k).randint(0, k, n).astype(np.uint8)
        want = np.bincount(sym, minlength=k).astype(np.uint64)
        ks, sp = inp(sym, 3)                                                  # a head of 13 bytes before the first 16-byte boundary

        def run_u8():
            h1, h2 = Out(np.uint64, k, 0), Out(np.uint64, k, 0)
            assert lib.qd_histogram_u8_ws(sp, n, k, h1.ptr, *stream_tail()) == 0
            assert lib.qd_histogram_u8(sp, n, k, h2.ptr, _lib.stream_ptr()) == 0
            torch.cuda.synchronize()
            return dict(ws=h1.get(), atomic=h2.get())
        under_every_cap(lib, run_u8, lambda o, cap: (np.testing.assert_array_equal(o['ws'], want), np.testing.assert_array_equal(o['atomic'], want)))
    # int64 symbols and digitized floats: min(ceil(n / 4096), 4 CUs, cap) blocks of 256 threads
    n = 40003
    assert_trips('k_hist_sym', n // 4 // 4, n, 256 * 16, 256)
    idx = dev(np.random.RandomState(1).randint(0, 17, n).astype(np.int64))
    edges = qhf._digitize_edges(16, 1e-5)
    v = dev(np.random.RandomState(2).rand(n).astype(F32))
    ed = dev(edges)
    want_i = np.bincount(idx.cpu().numpy(), minlength=17)
    want_d = np.bincount(np.digitize(v.cpu().numpy(), edges), minlength=17)

    def run_sym():
        return dict(index=qhf._device_counts('index', idx, 16).cpu().numpy(), digitize=qhf._device_counts('digitize', v, 16, ed).cpu().numpy())
    under_every_cap(lib, run_sym, lambda o, cap: (np.testing.assert_array_equal(o['index'], want_i), np.testing.assert_array_equal(o['digitize'], want_d)))
    # the one-pass level histogram at a vector bucket size: tiles over the waves of min(ceil(tiles / 4), 8 CUs, cap) blocks
    nfull = 199
    n = nfull * 256 + 3
    assert_trips('k_level_hist_vec', -(-nfull // 4), -(-nfull // 4), 4, 4)
    x = make(n, 3, 7)
    xd = dev(x)
    want_l = np.bincount(oc.uniform_quantize(x, 16, 256)['lev'], minlength=16)
    under_every_cap(lib, lambda: dict(levels=codec.level_histogram(xd, 16, 256).cpu().numpy()),
                    lambda o, cap: np.testing.assert_array_equal(o['levels'], want_l))
    assert lib_cap_is_default()


# ---- the multi-tensor launches: tiles of ALL tensors strided over the waves of min(ceil(tiles / 4), cap) blocks
def tensor_list(bucket):
    """22 tensors of one to three tiles each (a tile: four buckets, or 1024 elements without buckets) and an EMPTY one, so that
    the successive trips of one wave -- 4, 8 or 12 tiles apart -- land in different tensors."""
    unit = 4 * bucket if bucket else 1024
    sizes = [unit + 3, 2 * unit + bucket + 1 if bucket else 2 * unit + 77, 0, 3 * unit - 1, unit // 2 + 1, 2 * unit] * 4
    sizes = sizes[:22]
    kinds = (7, 0, 6, 2, 4)
    return [make(n, 900 + 7 * i, kinds[i % 5]) if n else np.zeros(0, F32) for i, n in enumerate(sizes)]


@pytest.mark.parametrize('bucket', [256, 100, None])
def test_multi_tensor_quantizer_loops(lib, bucket):
    """qd_multi_uniform_f32, its _global / _opt / _levels forms (k_multi_uniform*, k_mg_*): each tensor against the oracle."""
    from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer
    xs = tensor_list(bucket)
    live = [i for i, x in enumerate(xs) if x.size]
    xd = [dev(x) for x in xs]
    s_list = [(2, 4, 16, 256, 5)[i % 5] for i in range(len(xs))]
    forms = [('plain', dict(s=16)), ('clamp', dict(s=16, max_element=0.5)), ('stochastic', dict(s=16, stochastic_rounding=True)),
             ('levels', dict(s=s_list)), ('levels + clamp + stochastic', dict(s=s_list, max_element=0.5, stochastic_rounding=True))]
    seed0 = 0x1234ABCD5678
    for name, kw in forms:
        mt = MultiTensorQuantizer(xd, bucket_size=bucket, **kw)
        assert_trips('k_multi_uniform* (%s)' % name, mt._tiles, mt._tiles, 4, 4)
        levels = kw['s'] if isinstance(kw['s'], list) else [kw['s']] * len(xs)
        want = []
        for i in live:
            if kw.get('stochastic_rounding'):
                xi = np.clip(xs[i], F32(-0.5), F32(0.5)) if 'max_element' in kw else xs[i]
                want.append(S.oracle(xi, levels[i], seed0 + i, bucket)['q'])
            else:
                want.append(oc.uniform_quantize(xs[i], levels[i], bucket, max_element=kw.get('max_element', False), want_idx=False, want_lev=False)['q'])

        def run():
            outs = mt.quantize(seed=seed0) if kw.get('stochastic_rounding') else mt.quantize()
            return {'q%d' % i: outs[i].cpu().numpy().copy() for i in live}

        def check(o, cap):
            for i, w in zip(live, want):
                assert np.array_equal(o['q%d' % i], w, equal_nan=True), (name, bucket, cap, 'tensor', i, xs[i].size)
        under_every_cap(lib, run, check)
    assert lib_cap_is_default()


@pytest.mark.parametrize('bucket', [256, 100])
def test_multi_tensor_ste_loops(lib, bucket):
    """qd_multi_ste_backward_f32 / _levels_f32 (k_multi_ste, k_multi_ste_lv): bit-identical to the per-tensor call, which
    test_ste_bucket_backward_loops holds to the oracle; a wave that moves on to another tensor takes that tensor's level count."""
    from quantized_distillation_amd import ste
    from quantized_distillation_amd.multi_tensor import MultiTensorSTE
    xs = tensor_list(bucket) + [make(bucket - 1, 7, 0)]                      # (+ one tile: the count is then no multiple of 4)
    gs = [np.random.RandomState(i).randn(x.size).astype(F32) for i, x in enumerate(xs)]
    xd, gd = [dev(x) for x in xs], [dev(g) for g in gs]
    s_list = [(2, 4, 16, 256, 5)[i % 5] for i in range(len(xs))]
    for s in (16, s_list):
        levels = s if isinstance(s, list) else [s] * len(xs)
        want = [ste.ste_bucket_backward(xd[i], gd[i], bucket, levels[i], out=torch.empty_like(gd[i])).cpu().numpy() if xs[i].size else None
                for i in range(len(xs))]
        outs = [torch.empty_like(g) for g in gd]
        mt = MultiTensorSTE(xd, gd, s, bucket, outs=outs)
        assert_trips('k_multi_ste', mt._tiles, mt._tiles, 4, 4)

        def run():
            for o in outs:
                o.fill_(float('nan'))
            res = mt.backward()
            return {'o%d' % i: res[i].cpu().numpy().copy() for i in range(len(xs)) if xs[i].size}

        def check(o, cap):
            for i in range(len(xs)):
                if xs[i].size:
                    assert same_bits(o['o%d' % i], want[i]), (bucket, cap, 'tensor', i)
        under_every_cap(lib, run, check)
    assert lib_cap_is_default()


@pytest.mark.parametrize('bucket', [256, 100, None])
def test_multi_tensor_diff_quant_loops(lib, bucket):
    """qd_multi_nearest_f32 (k_multi_nearest / _flat, capped) and qd_multi_point_grad_f32 (a fixed grid: the cap must not
    change it): forward bit-identical to the oracle's midpoint assignment, backward within the project's 1e-6."""
    import errlog
    from quantized_distillation_amd.multi_tensor import MultiTensorDiffQuant
    k = 16
    xs = [x for x in tensor_list(bucket) if x.size]
    xs = [make(x.size, 50 + i, (0, 2)[i % 2]) for i, x in enumerate(xs)]
    gs = [np.random.RandomState(i).randn(x.size).astype(F32) for i, x in enumerate(xs)]
    xd, gd = [dev(x) for x in xs], [dev(g) for g in gs]
    outs = [torch.empty_like(x) for x in xd]
    mt = MultiTensorDiffQuant(xd, outs, gd, k, bucket)
    assert_trips('k_multi_nearest', mt._tiles, mt._tiles, 4, 4)
    pts = np.stack([np.sort(np.random.RandomState(70 + i).rand(k)).astype(F32) for i in range(len(xs))])
    pd = dev(pts)
    refs = [oc.nonuniform_quantize(x, pts[i], bucket, 'midpoint') for i, x in enumerate(xs)]

    def run():
        for o in outs:
            o.fill_(float('nan'))
        mt.forward(pd)
        gp = mt.backward()
        o = {'q%d' % i: outs[i].cpu().numpy().copy() for i in range(len(xs))}
        o.update({'idx%d' % i: mt.indices[i].cpu().numpy().copy() for i in range(len(xs))})
        o['grad'] = gp.cpu().numpy().copy()
        return o

    def check(o, cap):
        for i, r in enumerate(refs):
            assert np.array_equal(o['q%d' % i], r['q']) and np.array_equal(o['idx%d' % i], r['idx'].astype(np.uint8)), (bucket, cap, i)
            want, absum = oc.point_grad(gs[i], r['idx'], r['alpha'], bucket, k)
            errlog.check_sum('K6m point gradient under a grid cap', o['grad'][i], want, absum, (bucket, cap, i), n_terms=xs[i].size)
    under_every_cap(lib, run, check)
    assert lib_cap_is_default()


@pytest.mark.parametrize('kind', ['absmax', 'absnorm'])
def test_abs_scalings_loop(lib, kind):
    """'absmax' / 'absnorm' (k_abs_buckets: a bucket per wave; k_abs_partial + k_abs_inverse: elements over threads) with the
    checks and the norm bound of tests/test_hip_abs.py, under every cap."""
    import abs_cases as ac
    from test_hip_abs import run_api
    for case in list(ac.many_cases(kind)):
        nb = -(-case.x.size // case.bucket)
        assert_trips('k_abs_buckets', nb, nb, 4, 4, own_cap=65536)
        outs = {}
        for cap in (None,) + C.CAPS:
            with C.Capped(lib, cap):
                outs[cap] = run_api(case, twice=False)
            for name in outs[None]:
                assert same_bits(outs[cap][name], outs[None][name]), (case.id, name, cap)
    n = 70003                                                                 # one bucket above 65536 elements: the two-stage norm
    assert_trips('k_abs_partial', n, n, 256 * 32, 256, own_cap=1024)
    case = ac._case('grid-trips-single-%s' % kind, ac.random_data(n, 11), None, kind)
    for cap in (None,) + C.CAPS:
        with C.Capped(lib, cap):
            run_api(case, twice=False)
    assert lib_cap_is_default()


# ------------------------------------------------------------------------------------------------ the production path, no hook
@pytest.mark.parametrize('bucket', [256, 1000])
def test_the_capped_fine_table_grid_makes_a_second_trip_without_the_hook(lib, bucket):
    """The nearest-point mode with the midpoint rule builds the fine cell table on a grid capped at 24 blocks per compute unit
    (csrc/qd_plan.h: fine_grid_cap) -- the one place where a shipped default makes the kernels loop.  k = 256 at bucket 256
    (k_bucket_vec) and 1000 (k_bucket_wave_any), not pre-scaled, at 1.5 x the capped grid's reach + 5 elements: the second
    trip is partial.  Indices and values against numpy's count of fp32 midpoints <= u, as
    test_fine_cell_table_with_crowded_and_degenerate_points does.  (k = 65 is left to the capped cases above: on this
    tensor's 38 M elements the numpy side of ONE k takes about four seconds of CPU time, all a test here may take.)"""
    k = 256
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_block = 16 * 256 if bucket == 256 else 4 * 1000                      # k_bucket_vec<2,16,4,1>: 16 buckets per block; wave_any<2,5,1>: 4
    n = int(1.5 * 24 * cus * per_block) + 5
    p = C.plan(lib, queries(NEAREST, n, bucket, k=k, assign_mode=1, side_bytes=1, cus=cus))
    L = p['launch'][0, 0]
    kernel = L['kernel'].decode()
    assert p['fine'][0] == 1 and L['blocks'] == 24 * cus, (kernel, int(L['blocks']))
    units, workers, _, _ = C.trip_stats(kernel, p, p['launch'][:, 0], np.array([n]))
    assert workers[0] < units[0] < 2 * workers[0], (kernel, int(units[0]), int(workers[0]))      # a second, partial trip
    pts = points(k)
    x = torch.rand(n, generator=torch.Generator().manual_seed(bucket)).numpy()
    r = oc.scale_down(x, bucket)
    nb = r['alpha'].size
    mids = ((pts[:-1] + pts[1:]).astype(F32) * F32(0.5)).astype(F32)
    want_idx = np.searchsorted(mids, r['u'], side='right').astype(np.uint8)   # the count of midpoints <= u
    bk = np.arange(n) // bucket
    want_q = ((pts[want_idx] * r['alpha'][bk]).astype(F32) + r['beta'][bk]).astype(F32) + F32(0.0)
    kx, xp = inp(x, 0)
    kp, pp = inp(pts, 0)
    q, idx, a, b = Out(F32, n, 0), Out(np.uint8, n, 0), Out(F32, nb, 0), Out(F32, nb, 0)
    assert lib.qd_nearest_point_f32(xp, 0, pp, k, 1, q.ptr, idx.ptr, 1, n, bucket, a.ptr, b.ptr, None, 0, 0.0, *stream_tail()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(idx.get(), want_idx) and np.array_equal(q.get(), want_q)
    assert np.array_equal(a.get(), r['alpha']) and np.array_equal(b.get(), r['beta'])
    # the pre-processed forward of the same tensor: k_nearest_prescaled_stream on the same capped grid
    ku, up = inp(r['u'], 0)
    ka, ap = inp(r['alpha'], 0)
    kb, bp = inp(r['beta'], 0)
    p2 = C.plan(lib, queries(NEAREST, n, bucket, k=k, assign_mode=1, side_bytes=1, prescaled=1, cus=cus))
    assert p2['launch'][0, 0]['kernel'].decode().startswith('k_nearest_prescaled_stream') and p2['fine'][0] == 1
    q2, idx2 = Out(F32, n, 0), Out(np.uint8, n, 0)
    assert lib.qd_nearest_point_f32(up, 1, pp, k, 1, q2.ptr, idx2.ptr, 1, n, bucket, ap, bp, None, 0, 0.0, *stream_tail()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(idx2.get(), want_idx) and np.array_equal(q2.get(), want_q)


def test_the_grid_cap_reads_back_as_the_default_after_this_module(lib):
    assert lib.qd_set_grid_cap(C.GRID_CAP_DEFAULT) == C.GRID_CAP_DEFAULT
