"""tests/nearest_cases.py on the CPU: its reference against the reference program's own answers, its geometry table against
the launcher's plan, and every case through libqd_host.so (qd_nearest_point_f32, both rules, raw and pre-scaled) bit for bit.

The host library is an implementation of its own (csrc/host/qd_host.cpp); tests/test_hip_nearest_ties.py holds libqd_hip.so to
the same numpy reference on the same cases, so host and device cannot disagree on a tie without one of the two files failing."""
import ctypes
import os
import sys

import numpy as np
import pytest

import nearest_cases as C
import test_transform_plan as T
from quantized_distillation_amd import _lib
from quantized_distillation_amd import build as qb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_numpy_reference_reproduces_the_reference_programs_tie_cases(golden_nonuniform):
    """tests/golden/nonuniform.npz: the reference's indices, values, alpha and beta on its `grid` cases (x on exact midpoints
    between the points) and `dups` cases (duplicate points), under both rules."""
    G = golden_nonuniform
    seen = 0
    for i, m in enumerate(G.meta):
        if m['points'] not in ('grid', 'dups'):
            continue
        seen += 1
        x, pts, bucket = G.arr('n', i, 'x').reshape(-1), G.arr('n', i, 'pts'), m['bucket'] or 0
        alpha, beta, u = C.ref_scale(x, bucket)
        assert np.array_equal(alpha, G.arr('n', i, 'alpha').reshape(-1)) and np.array_equal(beta, G.arr('n', i, 'beta').reshape(-1)), m
        for rule, ikey, qkey in ((C.DISTANCE, 'idx', 'q'), (C.MIDPOINT, 'idx_pre', 'q_pre')):
            idx = C.ref_index(u, pts, rule)
            assert np.array_equal(idx, G.arr('n', i, ikey).reshape(-1)), (m, rule)
            assert np.array_equal(C.ref_q(idx, pts, alpha, beta, x.size, bucket), G.arr('n', i, qkey).reshape(-1)), (m, rule)
        if m['points'] == 'grid':                  # the two rules DO differ there: the cases are about ties
            assert not np.array_equal(C.ref_index(u, pts, C.DISTANCE), C.ref_index(u, pts, C.MIDPOINT))
    assert seen == 8


def test_where_an_exact_tie_goes_and_that_the_two_midpoint_forms_differ_only_off_the_lattice():
    """What the cases are built on.  With distinct lattice points a u exactly on a midpoint goes UP under both rules (the
    distance rule steps down only when strictly closer), its lower fp32 neighbour stays below under the midpoint rule, and a u
    on a point takes that point under both; and p + (q - p) / 2 equals (p + q) / 2 on every lattice set but not on
    'full precision'."""
    differ = 0
    for name in C.SETS:
        pts = C.points(name, 200, 5)
        a = (pts[:-1] + pts[1:]) * C.F(0.5)
        if name == 'full precision':
            differ = int((a != C.midpoints(pts)).sum())
        else:
            assert np.array_equal(a, C.midpoints(pts)), name
    assert differ > 0
    pts = np.unique(C.points('uniform', 64, 9))
    mid = C.midpoints(pts)
    up = np.arange(1, pts.size)
    assert np.array_equal(C.ref_index(mid, pts, C.MIDPOINT), up) and np.array_equal(C.ref_index(mid, pts, C.DISTANCE), up)
    below = np.nextafter(mid, C.F(-1))
    assert np.array_equal(C.ref_index(below, pts, C.MIDPOINT), up - 1)
    assert np.array_equal(C.ref_index(pts, pts, C.MIDPOINT), C.ref_index(pts, pts, C.DISTANCE))


@pytest.fixture(scope='module')
def hip_plan_lib():
    qb.build_extension()
    return _lib.load()


def test_every_row_reaches_the_kernel_it_names_and_every_shipped_kernel_has_a_row(hip_plan_lib, capsys):
    """qd_transform_plan (host only) on every row x k x rule x index form; the table of what was reached is printed."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import launch_coverage
    reached = C.check_rows_against_the_plan(hip_plan_lib, T.queries, T.plan, T.names, launch_coverage.shipped())
    with capsys.disabled():
        print('\nkernel: class -> fine')
        for name in sorted(reached):
            print('  %-36s %s' % (name, '; '.join('%s -> %s' % (c, reached[name][c]) for c in C.CLASSES if c in reached[name])))
    assert len(reached) == 24


def test_the_generators_hold_their_conditions_on_the_degenerate_ends():
    """The assertions inside raw_case / prescaled_case ARE the conditions (they run for every case below); here the sizes no
    row has: one element, one bucket of two, buckets of one element, four buckets exactly."""
    for k in (1, 2, 33):
        for name in C.SETS:
            pts = C.points(name, k, 3)
            for n, bucket in ((1, 0), (2, 0), (5, 1), (7, 2), (16, 4), (400, 100), (401, 100)):
                c = C.raw_case(pts, n, bucket, 17, unscaled=name == 'full precision')
                assert c['x'].size == n and np.isnan(c['x']).sum() == (1 if C.geometry(n, bucket)[1] >= 4 else 0)
                c = C.prescaled_case(pts, n, bucket, 18)
                assert c['u'].size == n


def call(lib, x, prescaled, pts, rule, n, bucket, alpha, beta, width, want_q=True):
    q = np.full(n, 777.0, C.F)
    idx = None if width == 0 else np.full(n, -1 if width == 8 else 255, np.int64 if width == 8 else np.uint8)
    rc = lib.qd_nearest_point_f32(x.ctypes.data, prescaled, pts.ctypes.data, pts.size, rule, q.ctypes.data if want_q else None,
                                  None if idx is None else idx.ctypes.data, width or 8, n, bucket, alpha.ctypes.data, beta.ctypes.data,
                                  None, 0, ctypes.c_float(0.0), None, 0, None)
    return rc, q, idx


@pytest.mark.parametrize('k', C.K)
def test_the_host_library_on_every_case(k):
    """libqd_host.so: indices, q, alpha and beta bit for bit, int64 / uint8 / no index output, and the indices-only form."""
    lib = _lib.host()
    ran = 0
    for ri, row, name, pts, case in C.cases_of(k):
        n, bucket = row.n, row.bucket
        x = np.array(case['x'])
        for rule in C.RULES:
            want_idx, want_q = C.expect(case, pts, rule)
            assert want_idx.min() >= 0 and want_idx.max() <= k - 1
            for width in sorted({w for w, _, _ in row.forms}):
                if width == 1 and k > 256:
                    continue
                tag = (k, ri, name, rule, width)
                if row.prescaled:
                    alpha, beta = np.array(case['alpha']), np.array(case['beta'])
                else:
                    alpha, beta = np.full(case['alpha'].size, 777.0, C.F), np.full(case['beta'].size, 777.0, C.F)
                rc, q, idx = call(lib, x, row.prescaled, pts, rule, n, bucket, alpha, beta, width)
                assert rc == 0, tag
                if idx is not None:
                    bad = np.flatnonzero(idx.astype(np.int64) != want_idx)
                    assert bad.size == 0, (tag, bad[:5], case['u'][bad[:5]], idx[bad[:5]], want_idx[bad[:5]])
                assert np.array_equal(q, want_q, equal_nan=True), tag
                assert np.array_equal(alpha, case['alpha'], equal_nan=True) and np.array_equal(beta, case['beta'], equal_nan=True), tag
                assert np.array_equal(x, case['x'], equal_nan=True), (tag, 'the input was modified')
                if row.prescaled and width and C.indices_only_served(row, width, 0):
                    rc, q2, idx2 = call(lib, x, 1, pts, rule, n, bucket, alpha, beta, width, want_q=False)
                    assert rc == 0 and np.array_equal(idx2, idx) and np.all(q2 == 777.0), (tag, 'indices only')
                ran += 1
    assert ran >= 2 * len(C.ROWS)
