"""The launcher of qd_uniform_f32 / qd_scale_down_f32 / qd_nearest_point_f32, checked by its plan -- on the CPU.

run_transform<MODE> (csrc/qd_transform.h) launches what plan_transform (csrc/qd_plan.h) returns, and qd_transform_plan returns
the same plan with the kernel names spelled out.  So everything the launcher decides can be held here without a GPU, for EVERY
bucket size 1 .. 40000 in the three modes, at four tensor lengths each (many buckets, many buckets + 1 element, three buckets +
2, one bucket + 1), with the pointers aligned and not, the side outputs asked for and not, and 4 / 33 / 65 / 256 points:

  * the capacity contracts the kernels index their LDS, registers and the tensor by (stated next to the kernel lines they
    protect in qd_bucket_vec_kernels.h and qd_bucket_row_kernels.h): a launcher slip there is an out-of-bounds access on the device;
  * the boundaries between the kernel families, and the thresholds of the single-bucket path;
  * agreement with the shipped library: every name the plan returns is a kernel of libqd_hip.so, and every shipped
    instantiation of the transform kernels is planned for some input -- a stranded instantiation fails here;
  * the launcher paths of tests/abi_contract.py as data, and the trace of profiles/dispatch_map.txt (tools/dispatch_map.py on an
    MI355X): the plan names what the GPU ran.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from quantized_distillation_amd import _lib
from quantized_distillation_amd import build as qb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

QDQ, SCALE, NEAREST = 0, 1, 2
CUS = 256                     # compute units of an MI355X; the plan takes the count as an argument
FUSED_CAP = 256               # blocks of k_single_fused resident at once there (the capacity profiles/dispatch_map.txt implies, see below)
MANY = 4099                   # "many buckets": more than any chunk holds (256), odd, so that tiles and chunks end ragged
MAX_BUCKET = 40000

QUERY = np.dtype([(f, np.int32) for f in ('mode', 'data_misalign', 'side_bytes', 'side_misalign', 'k', 'assign_mode', 'prescaled', 'q_null',
                                          'fused_capacity', 'cus')] + [('n', np.int64), ('bucket', np.int64)], align=True)
LAUNCH = np.dtype([('kernel', 'S40'), ('blocks', np.int32), ('threads', np.int32), ('lds_bytes', np.int64)], align=True)
PLAN = np.dtype([(f, np.int64) for f in ('nb', 'row', 'nvec', 'm', 'nchunks', 'nbk', 'amask')] +
                [('fine', np.int32), ('nlaunch', np.int32), ('launch', LAUNCH, (3,))], align=True)
TRANSFORM_KERNEL = re.compile(r'^(k_bucket_|k_single_|k_minmax_|k_nearest_prescaled_stream)')


@pytest.fixture(scope='module')
def lib():
    qb.build_extension()
    assert QUERY.itemsize == ctypes.sizeof(_lib.QdTransformQuery) and PLAN.itemsize == ctypes.sizeof(_lib.QdTransformPlan)
    assert LAUNCH.itemsize == ctypes.sizeof(_lib.QdPlannedLaunch)
    return _lib.load()


def queries(mode, n, bucket, data_misalign=0, side_bytes=0, side_misalign=0, k=0, assign_mode=0, prescaled=0, q_null=0,
            fused_capacity=FUSED_CAP, cus=CUS):
    n, bucket = np.broadcast_arrays(np.asarray(n, np.int64), np.asarray(bucket, np.int64))
    q = np.zeros(n.shape, QUERY)
    for name, v in (('mode', mode), ('n', n), ('bucket', bucket), ('data_misalign', data_misalign), ('side_bytes', side_bytes),
                    ('side_misalign', side_misalign), ('k', k), ('assign_mode', assign_mode), ('prescaled', prescaled),
                    ('q_null', q_null), ('fused_capacity', fused_capacity), ('cus', cus)):
        q[name] = v
    return q.reshape(-1)


def plan(lib, q):
    out = np.zeros(q.shape, PLAN)
    assert lib.qd_transform_plan(q.ctypes.data, q.size, out.ctypes.data) == 0
    return out


def names(p, i=0):
    """The kernel names of plan i, in launch order."""
    return [p['launch'][i, j]['kernel'].decode() for j in range(p['nlaunch'][i])]


def one(lib, mode, n, bucket, **kw):
    return names(plan(lib, queries(mode, n, bucket, **kw)))


def sweep_lengths(buckets):
    """(n, bucket) of the four lengths of every bucket size: many buckets, many + 1 element, three buckets + 2, one + 1."""
    b = np.asarray(buckets, np.int64)
    n = np.stack([MANY * b, MANY * b + 1, 3 * b + 2, b + 1])
    return n.reshape(-1), np.tile(b, 4)


def table_bytes(k, fine):
    """The point table at the start of a nearest-point kernel's dynamic LDS (PointStore, qd_points.h)."""
    coarse = 2 * 1024 * 4 + 2 * (256 + 4) * 4
    return np.where(k <= 32, 2 * 32 * 4, coarse + np.where(fine != 0, 2048 * 8, 0))


def lane_rule(m):
    """m buckets of a chunk are reduced side by side: from 64 on a lane takes whole buckets alone; below that 64 / m lanes share
    one -- a power of two -- except 48 .. 63, one lane per bucket."""
    return (m >= 64) | ((m & (m - 1)) == 0) | ((m >= 48) & (m <= 63))


def check_contracts(q, p, seen):
    """The capacity contracts of every planned launch of the batch (vectorised per kernel name); `seen` collects the names."""
    n, row, nb, mode, k = q['n'], p['row'], p['nb'], q['mode'], q['k']
    bucket = q['bucket']
    one_bucket = (bucket <= 0) | (n < bucket)
    assert np.array_equal(nb, np.where(one_bucket, 1, -(-n // np.maximum(bucket, 1))))             # help_functions.py:67-94
    assert np.array_equal(row, np.where(one_bucket, n, bucket))
    assert np.all((p['nlaunch'] >= 1) & (p['nlaunch'] <= 3))
    fine = p['fine']
    want_fine = (mode == NEAREST) & (k > 32) & (q['assign_mode'] == 1)
    assert np.all((fine == 0) | want_fine)
    stage8 = ((mode == QDQ) & (q['side_bytes'] != 0)) | ((mode == NEAREST) & (q['side_bytes'] != 0) & (k <= 32))
    for j in range(3):
        live = p['nlaunch'] > j
        L = p['launch'][:, j]
        # every plan: 1 <= blocks <= 2^20; on a grid capped at 24 blocks per CU whenever the fine table is built; the dynamic
        # LDS within the 64 KiB a launch may ask for without raising the limit (this path never raises it)
        assert np.all(L['blocks'][live] >= 1) and np.all(L['blocks'][live] <= 1 << 20)
        assert np.all(L['blocks'][live & (fine != 0)] <= 24 * q['cus'][live & (fine != 0)])
        assert np.all((L['lds_bytes'][live] >= 0) & (L['lds_bytes'][live] <= 64 * 1024))
        uniq, inv = np.unique(L['kernel'][live], return_inverse=True)
        idx = np.nonzero(live)[0]
        for u, name in enumerate(uniq):
            name = name.decode()
            seen.add(name)
            s = idx[inv == u]
            base, _, targs = name.partition('<')
            t = [int(a) if a.lstrip('-').isdigit() else a for a in targs.rstrip('>').split(',')] if targs else []
            blocks, threads, lds = L['blocks'][s], L['threads'][s], L['lds_bytes'][s]
            r, nn, m, nch, md, kk = row[s], n[s], p['m'][s], p['nchunks'][s], mode[s], k[s]
            if base not in ('k_minmax_partial', 'k_minmax_final', 'k_nearest_prescaled_stream'):
                assert np.all(md == t[0]), name                                        # the instantiation of the call's mode
            tab = np.where(md == NEAREST, table_bytes(kk, fine[s]), 0)
            coarse = np.where(md == NEAREST, table_bytes(kk, 0), 0)
            if base == 'k_bucket_vec':
                _, lpb, v, _u = t
                assert np.all(r == lpb * v * 4), name                                  # constexpr ROW of the kernel
                assert np.all(p['nvec'][s] == nn // r) and np.all(threads == 256) and np.all(lds == tab)
                assert np.all(fine[s] == ((kk > 64) & want_fine[s]))                   # up to 64 points the vector kernel keeps the coarse table
            elif base == 'k_bucket_chunk':
                assert t[1] == 8 and np.all(threads == 128)
                assert np.all(r % 4 == 0) and np.all((m >= 1) & (m <= 256)), name     # ab[256], yt[256]
                assert np.all(m * (r // 4) <= 8 * 64), name                            # pr[VMAX * 64], v[VMAX]
                assert np.all(lane_rule(m)), name
                assert np.all(nch == (nn // r) // m) and np.all(nch >= 1), name
                assert np.all(fine[s] == 0) and np.all(lds == 2 * (8 * 64 + 256 + 128) * 8 + coarse), name
            elif base == 'k_bucket_chunk_any':
                assert t[1] == 8 and np.all(threads == 128)
                assert np.all(m % 4 == 0) and np.all(m >= 4), name
                assert np.all(m * r // 4 + 7 <= 8 * 64), name                          # room for the lead-in: the kernel always takes it
                assert np.all(lane_rule(m)), name
                assert np.all(nch == (nn // r) // m) and np.all(nch >= 1), name
                assert np.all(fine[s] == 0), name
                assert np.all(lds == 2 * (8 * 256 + np.where(stage8[s], 8 * 64, 0)) * 4 + coarse), name
            elif base == 'k_bucket_wave_any':
                _, v, g = t
                assert np.all(r // 4 + np.where(r % 4 != 0, 2, 0) + np.where(r % 32 != 0, 7, 0) <= 64 * g * v), name      # f4 v[V]
                assert v <= 9 or t[0] != NEAREST, name                                 # no scratch in the nearest-point mode
                assert np.all(p['amask'][s] == -32) and np.all(threads == 256) and np.all(lds == tab), name
                if v <= 16:
                    assert np.all(p['nbk'][s] == nb[s]), name
                else:
                    # the leading buckets whose last float4 ends inside the tensor: a full bucket c (1-based) does so iff
                    # c * row <= the largest multiple of 4 within n; the last bucket of the tensor iff n % 4 == 0
                    whole = np.minimum(nb[s] - 1, (nn // 4 * 4) // r) + (nn % 4 == 0)
                    assert np.array_equal(p['nbk'][s], whole), name
            elif base == 'k_bucket_groups':
                assert np.all(threads == 256) and np.all(lds == tab)
                assert np.all(r <= 256) if t[1] == 16 else (t[1] == 64 and np.all((r > 256) & (r <= 16384))), name
            elif base == 'k_bucket_generic':
                assert np.all(threads == 1024) and np.all(lds == tab)
                assert np.all((r > 16384) | ((nb[s] == 1) & (nn <= 16384) & (blocks == 1))), name
            elif base == 'k_single_fused':
                _, v, w = t
                assert w == 4 and np.all(nb[s] == 1) and np.all((nn > 16384) & (nn <= 1 << 20)), name
                assert np.all(blocks == -(-(-(-(nn // 4) // 256)) // v)) and np.all(blocks <= q['fused_capacity'][s]), name
            elif base in ('k_minmax_partial', 'k_minmax_final', 'k_single_apply'):
                assert np.all(nb[s] == 1) and np.all(nn > 16384) and np.all(threads == 256), name
                if base == 'k_minmax_partial':
                    assert np.all(blocks <= 1024), name                                # kPartialBlocks: the workspace's partials
                if base == 'k_minmax_final':
                    assert np.all(nn > 8 << 20) and np.all(blocks == 1), name
            elif base == 'k_nearest_prescaled_stream':
                assert np.all(md == NEAREST) and np.all(q['prescaled'][s] == 1) and np.all(nn >= 4) and np.all(r >= 4), name
                assert np.all((r % 4 != 0) == (t[0] == 'true')) and np.all(lds == tab), name
            else:
                raise AssertionError('a kernel this test has no contract for: ' + name)


def the_sweep(lib, check_contracts=check_contracts):
    """Every bucket size 1 .. 40000 x four lengths, in every mode, with the variations of the module docstring; returns the set
    of kernel names planned.  (Unaligned pointers send every size to the two-pass kernels, and the side outputs change LDS
    sizes only: those variations run once per mode, not crossed with each other.)  `check_contracts`: what holds every batch
    (the capped sweep below adds its own assertions to the contracts)."""
    seen = set()
    n, b = sweep_lengths(np.arange(1, MAX_BUCKET + 1))
    configs = [dict(mode=QDQ), dict(mode=QDQ, side_bytes=1), dict(mode=QDQ, data_misalign=2), dict(mode=QDQ, side_bytes=1, side_misalign=1),
               dict(mode=SCALE), dict(mode=SCALE, data_misalign=1)]
    for k in (4, 33, 65, 256):
        configs.append(dict(mode=NEAREST, k=k, assign_mode=1, side_bytes=8))                       # the per-step rule, int64 indices
        configs.append(dict(mode=NEAREST, k=k, assign_mode=1, side_bytes=1, prescaled=1))          # the pre-processed forward
    configs += [dict(mode=NEAREST, k=33, assign_mode=0), dict(mode=NEAREST, k=4, assign_mode=1, side_bytes=1, side_misalign=3),
                dict(mode=NEAREST, k=65, assign_mode=1, side_bytes=8, side_misalign=8), dict(mode=NEAREST, k=256, assign_mode=1, data_misalign=3),
                dict(mode=NEAREST, k=65, assign_mode=1, side_bytes=8, prescaled=1, q_null=1)]
    for cfg in configs:
        q = queries(n=n, bucket=b, **cfg)
        p = plan(lib, q)
        if cfg.get('q_null'):                    # indices only: the stream or nothing (buckets below 4 elements)
            refused = p['nlaunch'] == 0
            assert np.array_equal(refused, p['row'] < 4)
            q, p = q[~refused], p[~refused]
        check_contracts(q, p, seen)
    # one bucket spanning the tensor: around every threshold, with the one-launch kernel allowed, too small a grid for it, and off
    ns = np.array(sorted({t + d for t in (4, 16384, 65536, 1 << 18, 1 << 20, 8 << 20, 64 << 20) for d in (-1, 0, 1, 3, 4, 5)} |
                         set(range(1, 40)) | {100000, 300001, 70001}), np.int64)
    for mode in (QDQ, SCALE, NEAREST):
        for cap in (FUSED_CAP, 16, 0):
            for extra in (dict(), dict(side_bytes=1 if mode != NEAREST else 8, side_misalign=0 if mode == SCALE else 2)):
                if mode == SCALE and extra:
                    continue
                kw = dict(k=65, assign_mode=1) if mode == NEAREST else {}
                q = queries(mode, ns, 0, fused_capacity=cap, **kw, **extra)
                check_contracts(q, plan(lib, q), seen)
    for pre in (dict(prescaled=1), dict(prescaled=1, q_null=1, side_bytes=8)):
        q = queries(NEAREST, ns[ns >= 4], 0, k=4, assign_mode=1, **pre)
        check_contracts(q, plan(lib, q), seen)
    return seen


def test_capacity_contracts_hold_for_every_bucket_size_and_every_shipped_instantiation_is_planned(lib):
    import launch_coverage
    seen = the_sweep(lib)
    shipped = set(launch_coverage.shipped())
    assert seen <= shipped, 'the plan names kernels the library does not contain: %s' % sorted(seen - shipped)
    stranded = sorted(k for k in shipped if TRANSFORM_KERNEL.match(k) and k not in seen)
    # (exceptions would be listed here by name, each with its reason; there are none)
    assert stranded == [], 'shipped instantiations that no swept input reaches: %s' % stranded
    assert len(seen) == 82                       # the transform kernels of profiles/r06_launch_coverage.json


TAIL_OWNER = re.compile(r'^k_bucket_(vec|chunk|chunk_any)<')      # these plan one block more: the block that owns the tail
GRID_CAP_DEFAULT = 1 << 20


@pytest.mark.parametrize('cap', [1, 2, 3, 7])
def test_the_plan_under_a_small_grid_cap_changes_the_geometry_and_never_the_kernel(lib, cap):
    """qd_set_grid_cap (the test hook that makes the kernels' grid-stride loops take their later trips at small shapes,
    tests/test_hip_grid_trips.py): the sweep again under a cap of 1, 2, 3 and 7 blocks.  The capacity contracts still hold,
    every launch has at most `cap` blocks (+ 1 in the families with a tail-owner block; k_single_fused is exempt: its grid must
    hold the tensor in registers) and at most `cap` min / max partials, and the kernels and everything they index with -- m,
    nchunks, nbk, nvec, fine -- are those of the uncapped plan."""
    def check(q, p, seen):
        check_contracts(q, p, seen)
        assert lib.qd_set_grid_cap(-1) == cap                  # the uncapped plan of the same batch
        try:
            p0 = plan(lib, q)
        finally:
            assert lib.qd_set_grid_cap(cap) == GRID_CAP_DEFAULT
        for f in ('nb', 'row', 'nvec', 'm', 'nchunks', 'nbk', 'amask', 'fine', 'nlaunch'):
            assert np.array_equal(p[f], p0[f]), f
        for j in range(3):
            live = p['nlaunch'] > j
            L, L0 = p['launch'][live, j], p0['launch'][live, j]
            assert np.array_equal(L['kernel'], L0['kernel']) and np.array_equal(L['threads'], L0['threads'])
            assert np.array_equal(L['lds_bytes'], L0['lds_bytes'])
            for name in np.unique(L['kernel']):
                s = L['kernel'] == name
                name = name.decode()
                if name.startswith('k_single_fused<'):
                    assert np.array_equal(L['blocks'][s], L0['blocks'][s]), name
                    continue
                room = cap + 1 if TAIL_OWNER.match(name) else cap
                assert np.all(L['blocks'][s] == np.minimum(L0['blocks'][s], room)), name      # hence <= room, and nparts <= cap
                if name == 'k_minmax_partial':
                    assert np.all(L['blocks'][s] <= cap), name                              # its blocks ARE the partials (nparts)

    assert lib.qd_set_grid_cap(cap) == GRID_CAP_DEFAULT
    try:
        seen = the_sweep(lib, check)
    finally:
        assert lib.qd_set_grid_cap(-1) == cap
    assert lib.qd_set_grid_cap(GRID_CAP_DEFAULT) == GRID_CAP_DEFAULT       # reads back as the default
    assert len(seen) == 82


def test_the_grid_cap_hook_takes_1_to_2_pow_20_and_restores_the_default_otherwise(lib):
    try:
        assert lib.qd_set_grid_cap(5) == GRID_CAP_DEFAULT and lib.qd_set_grid_cap(GRID_CAP_DEFAULT) == 5
        for bad in (0, -1, GRID_CAP_DEFAULT + 1, 1 << 30):
            assert lib.qd_set_grid_cap(3) == GRID_CAP_DEFAULT and lib.qd_set_grid_cap(bad) == 3
        assert lib.qd_set_grid_cap(1) == GRID_CAP_DEFAULT
        p = plan(lib, queries(QDQ, 1 << 26, 256))[0]                      # the headline call under a cap of one block (+ the tail owner)
        assert (p['nvec'], p['launch'][0]['blocks']) == (1 << 18, 2)
    finally:
        lib.qd_set_grid_cap(-1)
    p = plan(lib, queries(QDQ, 1 << 26, 256))[0]
    assert p['launch'][0]['blocks'] == (1 << 14) + 1


W = 'k_bucket_wave_any<%d,'
BOUNDARIES = [
    # bucket, K1 / K2 / K4 kernel (one pattern: the same in the three modes), aligned pointers, many buckets
    (255, 'k_bucket_chunk_any<%d,8>'), (256, 'k_bucket_vec<%d,16,4,1>'), (257, 'k_bucket_chunk_any<%d,8>'),
    # from 448 the sizes that are no multiple of 4 belong to the wave kernel: nf_max = 112 + 2 + 7 = 121 at 449
    (447, 'k_bucket_chunk_any<%d,8>'), (448, 'k_bucket_chunk<%d,8>'), (449, (W + '2,1>', W + '3,1>', W + '3,1>')),
    # 505 / 506: where four buckets stop fitting next to k_bucket_chunk_any's lead-in -- invisible: both are the wave kernel's
    (504, 'k_bucket_chunk<%d,8>'), (505, W + '3,1>'), (506, W + '3,1>'), (507, W + '3,1>'),
    (511, W + '3,1>'), (512, 'k_bucket_vec<%d,64,2,2>'), (513, W + '3,1>'),
    # 2048 elements = 8 rounds of one wave; 2047 / 2049 need 511 / 512 + 2 + 7 float4s: two waves per bucket
    (2047, (W + '5,2>', W + '6,2>', W + '6,2>')), (2048, 'k_bucket_vec<%d,64,8,1>'), (2049, (W + '5,2>', W + '6,2>', W + '6,2>')),
    (8191, W + '9,4>'), (8192, (W + '8,4>', W + '9,4>', W + '9,4>')), (8193, W + '9,4>'),
    # 9216 = 9 float4 x 256 lanes: the last size of the wave kernel in the nearest-point mode (no instance above 9 float4s per lane)
    (9215, (W + '12,4>', W + '16,4>', 'k_bucket_groups<%d,64>')), (9216, W + '9,4>'), (9217, (W + '12,4>', W + '16,4>', 'k_bucket_groups<%d,64>')),
    (12287, (W + '16,4>', W + '16,4>', 'k_bucket_groups<%d,64>')), (12288, (W + '12,4>', W + '16,4>', 'k_bucket_groups<%d,64>')),
    (12289, (W + '16,4>', W + '16,4>', 'k_bucket_groups<%d,64>')),
    (16383, (W + '24,4>', W + '32,4>', 'k_bucket_groups<%d,64>')), (16384, (W + '16,4>', W + '16,4>', 'k_bucket_groups<%d,64>')),
    (16385, (W + '24,4>', W + '32,4>', 'k_bucket_generic<%d>')),
    # 32767 needs 8191 + 2 + 7 float4s, more than the largest instance's 8192
    (32767, 'k_bucket_generic<%d>'), (32768, (W + '32,4>', W + '32,4>', 'k_bucket_generic<%d>')), (32769, 'k_bucket_generic<%d>'),
]


def test_the_boundaries_between_the_kernel_families(lib):
    for bucket, want in BOUNDARIES:
        for mode in (QDQ, SCALE, NEAREST):
            pat = want if isinstance(want, str) else want[mode]
            kw = dict(k=16, side_bytes=8) if mode == NEAREST else {}
            for n in (MANY * bucket, MANY * bucket + 1):
                assert one(lib, mode, n, bucket, **kw) == [pat % mode], (bucket, mode, n)
            # a misaligned data pointer (or index output): the two-pass kernels, whatever the size
            two_pass = ['k_bucket_groups<%d,16>' if bucket <= 256 else 'k_bucket_groups<%d,64>' if bucket <= 16384 else 'k_bucket_generic<%d>']
            assert one(lib, mode, MANY * bucket, bucket, data_misalign=1, **kw) == [two_pass[0] % mode]
    assert one(lib, NEAREST, MANY * 1000, 1000, k=16, side_bytes=8, side_misalign=8) == ['k_bucket_groups<2,64>']
    assert one(lib, NEAREST, MANY * 1000, 1000, k=16, side_bytes=1, side_misalign=3) == ['k_bucket_wave_any<2,5,1>']   # a uint8 idx: any address
    assert one(lib, QDQ, MANY * 1000, 1000, side_bytes=1, side_misalign=2) == ['k_bucket_groups<0,64>']               # level_idx: 4 bytes
    # too few full buckets for one chunk: the fall-through to the lane-group kernels
    for mode in (QDQ, SCALE, NEAREST):
        kw = dict(k=16) if mode == NEAREST else {}
        assert one(lib, mode, 15 * 100 + 99, 100, **kw) == ['k_bucket_groups<%d,16>' % mode]      # m = 16 buckets per chunk
        assert one(lib, mode, 16 * 100, 100, **kw) == ['k_bucket_chunk<%d,8>' % mode]
        assert one(lib, mode, 3 * 300 + 2, 300, **kw) == ['k_bucket_groups<%d,64>' % mode]        # m = 4
        assert one(lib, mode, 4 * 300, 300, **kw) == ['k_bucket_chunk<%d,8>' % mode]
        assert one(lib, mode, 59 * 33 + 32, 33, **kw) == ['k_bucket_groups<%d,16>' % mode]        # m = 60
        assert one(lib, mode, 60 * 33, 33, **kw) == ['k_bucket_chunk_any<%d,8>' % mode]
        assert one(lib, mode, 256 + 1, 256, **kw) == ['k_bucket_vec<%d,16,4,1>' % mode]           # the vector kernel from one full bucket on


def test_the_thresholds_of_the_single_bucket_path(lib):
    for mode in (QDQ, SCALE, NEAREST):
        kw = dict(k=16) if mode == NEAREST else {}
        three = ['k_minmax_partial', 'k_single_apply<%d>' % mode]
        assert one(lib, mode, 16384, 0, **kw) == ['k_bucket_generic<%d>' % mode]
        assert one(lib, mode, 16385, 0, **kw) == ['k_single_fused<%d,1,4>' % mode]
        assert one(lib, mode, 16385, 0, fused_capacity=0, **kw) == three                           # switched off, in place, capturing
        assert one(lib, mode, 16385, 0, data_misalign=2, **kw) == three
        assert one(lib, mode, 256 * 256 * 4, 0, **kw) == ['k_single_fused<%d,1,4>' % mode]        # 256 blocks at one float4 per lane
        assert one(lib, mode, 256 * 256 * 4 + 4, 0, **kw) == ['k_single_fused<%d,4,4>' % mode]
        assert one(lib, mode, 1 << 20, 0, **kw) == ['k_single_fused<%d,4,4>' % mode]
        assert one(lib, mode, 1 << 20, 0, fused_capacity=255, **kw) == three                       # not resident at once: three launches
        assert one(lib, mode, (1 << 20) + 4, 0, **kw) == three
        assert one(lib, mode, 8 << 20, 0, **kw) == three
        assert one(lib, mode, (8 << 20) + 1, 0, **kw) == ['k_minmax_partial', 'k_minmax_final', 'k_single_apply<%d>' % mode]
        assert one(lib, mode, 100, 256, **kw) == ['k_bucket_generic<%d>' % mode]                  # shorter than a bucket: one bucket
    # the pre-processed forward: the stream from two buckets on (or for indices only), else the apply kernel alone
    pre = dict(k=16, assign_mode=1, prescaled=1, side_bytes=1)
    assert one(lib, NEAREST, 1 << 22, 0, **pre) == ['k_single_apply<2>']
    assert one(lib, NEAREST, 1 << 22, 0, q_null=1, **pre) == ['k_nearest_prescaled_stream<false>']
    assert one(lib, NEAREST, 1 << 22, 33, **pre) == ['k_nearest_prescaled_stream<true>']
    assert one(lib, NEAREST, 1 << 22, 3, **pre) == ['k_bucket_chunk_any<2,8>']                    # buckets below 4 elements
    assert one(lib, NEAREST, 1 << 22, 3, q_null=1, **pre) == []                                    # ... indices only: refused
    assert one(lib, NEAREST, 1 << 22, 256, side_misalign=2, **dict(pre, side_bytes=1)) == ['k_bucket_vec<2,16,4,1>']   # the stream's uint8 idx: 4 bytes


def test_plan_fields_of_known_cases(lib):
    """m, nchunks, nbk, grid and LDS of the cases the comments of qd_plan.h quote."""
    p = plan(lib, queries(QDQ, 65 * 36 + 5, 36))[0]
    assert (p['m'], p['nchunks'], p['launch'][0]['blocks'], p['launch'][0]['threads']) == (56, 1, 2, 128)      # 504 of the 512 float4
    p = plan(lib, queries(QDQ, 65 * 33 + 2, 33, side_bytes=1))[0]
    assert (p['m'], p['nchunks'], p['launch'][0]['lds_bytes']) == (60, 1, 2 * (2048 + 512) * 4)
    p = plan(lib, queries(QDQ, 261 * 7, 7))[0]
    assert (p['m'], p['nchunks']) == (256, 1)
    p = plan(lib, queries(QDQ, 3 * 20000 + 1, 20000))[0]                                             # V = 24: the 1-element bucket is block 0's
    assert (p['nb'], p['nbk'], p['launch'][0]['blocks']) == (4, 3, 3)
    p = plan(lib, queries(NEAREST, 1 << 26, 256, k=256, assign_mode=1, side_bytes=1))[0]             # the fine table on a capped grid
    assert (p['fine'], p['launch'][0]['blocks'], p['launch'][0]['lds_bytes']) == (1, 24 * CUS, 10272 + 16384)
    p = plan(lib, queries(NEAREST, 1 << 26, 256, k=64, assign_mode=1, side_bytes=1))[0]
    assert (p['fine'], p['launch'][0]['blocks'], p['launch'][0]['lds_bytes']) == (0, (1 << 26) // 256 // 16 + 1, 10272)
    p = plan(lib, queries(QDQ, 1 << 26, 256))[0]                                                     # the headline call: one wave-tile per wave
    assert (p['nvec'], p['launch'][0]['blocks'], p['launch'][0]['lds_bytes']) == (1 << 18, (1 << 14) + 1, 0)
    assert lib.qd_transform_plan(None, 1, None) == -1
    for bad in (dict(mode=3, n=10, bucket=0), dict(mode=0, n=0, bucket=0), dict(mode=0, n=10, bucket=-1), dict(mode=0, n=10, bucket=0, cus=0)):
        q = queries(**bad)
        out = np.zeros(1, PLAN)
        assert lib.qd_transform_plan(q.ctypes.data, 1, out.ctypes.data) == -1 and out.tobytes() == bytes(PLAN.itemsize)


def test_the_launcher_paths_of_the_abi_contract_are_what_the_plan_names(lib):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import abi_contract as A
    for mode in (QDQ, SCALE, NEAREST):
        kw = dict(k=16, side_bytes=8) if mode == NEAREST else {}           # _k4_default: 16 points, int64 indices
        for bucket, nfull, path in A.BUCKET_PATHS:
            for tail in (1, 2, 3):
                for n in A.lengths(bucket, nfull, tail):
                    for px in (0, 4, 8):                                   # PHASES: 4-byte aligned data at every 16-byte phase
                        assert one(lib, mode, n, bucket, data_misalign=px, **kw) == path.kernels_of(mode), (mode, bucket, n)
        for n, path in A.SINGLE_SMALL + A.SINGLE_LARGE:
            assert one(lib, mode, n, 0, data_misalign=4, **kw) == path.kernels_of(mode), (mode, n)
    assert A.BUCKET_PATHS[16][:2] == (20000, 3) and [A.BUCKET_PATHS[16][2].kernels_of(m) for m in (0, 1, 2)] == \
        [['k_bucket_wave_any<0,24,4>'], ['k_bucket_wave_any<1,32,4>'], ['k_bucket_generic<2>']]


def trace_rows():
    """(label, [transform kernels dispatched]) of profiles/dispatch_map.txt."""
    rows = []
    for line in open(os.path.join(ROOT, 'profiles', 'dispatch_map.txt')):
        if line.startswith('#') or not line.strip():
            continue
        label, ks = line[:78].rstrip(), re.sub(r' x\d+', '', line[78:]).split(' ; ')
        rows.append((label, [k.strip() for k in ks if TRANSFORM_KERNEL.match(k.strip())]))
    return rows


def test_the_plan_names_what_the_traced_calls_dispatched(lib):
    """profiles/dispatch_map.txt is tools/dispatch_map.py --trace on an MI355X: the kernels each labelled call dispatched.  Its
    uniformQuantization, scale_down, nonUniformQuantization and diff-quant forward rows are calls of the three entry points with
    known arguments (N = 4 Mi elements of a fresh allocation unless the label says otherwise); the plan must name the same
    kernels.  The one-launch kernel's capacity is what the trace implies: N = 16388 .. 1 Mi ran k_single_fused<.,1,4> up to 256
    blocks and <.,4,4> above, so 256 blocks are resident (kFusedMaxBlocks: at most one per compute unit)."""
    N = 1 << 22

    def bkt(s):
        return 0 if s == 'None' else int(s)
    checked = 0
    for label, got in trace_rows():
        m = re.match(r'uniformQuantization s=16 bucket=(\d+) (N=4Mi|ragged N=4Mi-5)( view at \+4 B)?$', label)
        if m:
            want = one(lib, QDQ, N - 5 if 'ragged' in m.group(2) else N, bkt(m.group(1)), data_misalign=4 if m.group(3) else 0)
        elif re.match(r'uniformQuantization s=16 bucket=None N=(\d+)$', label):
            want = one(lib, QDQ, int(label.rsplit('=', 1)[1]), 0)
        elif label == 'uniformQuantization s=16 bucket=None N=1Mi in place':
            want = one(lib, QDQ, 1 << 20, 0, fused_capacity=0)
        elif re.match(r'scale_down bucket=(\d+|None) N=4Mi$', label):
            want = one(lib, SCALE, N, bkt(label.split('=')[1].split()[0]))
        else:
            m = re.match(r'(nonUniformQuantization|diff-quant forward) k=(\d+) bucket=(\d+|None) ', label)
            if not m:
                continue
            k, pre = int(m.group(2)), m.group(1) == 'diff-quant forward'
            want = one(lib, NEAREST, N, bkt(m.group(3)), k=k, assign_mode=1 if pre else 0, prescaled=int(pre),
                       side_bytes=1 if (pre and k <= 256) else 8)
        assert got == want, label
        checked += 1
    assert checked == 36 + 8 + 7 + 1 + 36 + 1 + 7 * 10
