"""The shape table of tests/grid_trip_cases.py against qd_transform_plan -- on the CPU, before any GPU time is spent on it.

Every shipped instantiation of the transform kernels (except k_single_fused and k_minmax_final, which have no grid-stride loop
to take) has a case whose plan, under a grid cap of 1, 2 and 3 blocks, makes at least three trips per worker with a partial last
trip and a ragged end; the one instantiation no valid call can take that far is named, and that claim is held here too."""
import os
import sys

import numpy as np
import pytest

from quantized_distillation_amd import _lib
from quantized_distillation_amd import build as qb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import grid_trip_cases as C  # noqa: E402
from test_transform_plan import SCALE, plan, queries  # noqa: E402


@pytest.fixture(scope='module')
def lib():
    qb.build_extension()
    return _lib.load()


@pytest.fixture(scope='module')
def cases(lib):
    return C.find_cases(lib)


def test_header_shape_lists_are_read_whole():
    assert C.VEC_SHAPES == [(64, 16, 1, 4), (128, 16, 2, 2), (256, 16, 4, 1), (512, 64, 2, 2), (1024, 64, 4, 1), (2048, 64, 8, 1)]
    assert len(C.WAVE_SHAPES[0]) == 20 and len(C.WAVE_SHAPES[1]) == 9 and len(C.WAVE_SHAPES[2]) == 7
    assert C.WAVE_SHAPES[0][0] == (2, 1) and C.WAVE_SHAPES[0][-1] == (32, 4) and C.WAVE_SHAPES[2][-1] == (9, 4)


def test_every_shipped_transform_instantiation_has_a_looping_case(lib, cases):
    import launch_coverage
    want = C.wanted(launch_coverage.shipped())
    assert len(want) == 82 - 6 - 1                                          # the transform kernels less k_single_fused<3 modes x 2> and k_minmax_final
    unreached = sorted(k for k in want if k not in cases)
    # the exceptions are listed by name in grid_trip_cases.UNREACHED, each with its reason
    assert unreached == sorted(C.UNREACHED), 'no shape takes these through %d trips under caps %s: %s' % (C.MIN_TRIPS, C.CAPS, unreached)
    assert set(cases) <= set(want)


def test_every_case_loops_as_wanted_under_every_cap(lib, cases):
    """Not the table's word for it: the trips of every case, recomputed from the plan of that one call under each cap."""
    for kernel, c in sorted(cases.items()):
        for n in C.lengths_of(c):
            assert c.bucket == 0 or n % c.bucket in (1, 2, 3, c.bucket - 1), (kernel, n)
            ps = C.plans_under_caps(lib, queries(c.mode, n, c.bucket, **c.query))
            js = [j for j in range(ps[None]['nlaunch'][0]) if ps[None]['launch'][0, j]['kernel'].decode() == kernel]
            assert len(js) == 1, (kernel, n)
            j = js[0]
            for cap in C.CAPS:
                p = ps[cap]
                assert p['launch'][0, j]['kernel'].decode() == kernel
                units, workers, per_block, trips = C.trip_stats(kernel, p, p['launch'][:, j], np.array([n]))
                assert trips[0] >= C.MIN_TRIPS, (kernel, n, cap, int(units[0]), int(workers[0]))
                assert workers[0] == 1 or units[0] % workers[0] != 0, (kernel, n, cap, 'no partial last trip')
                assert p['launch'][0, j]['blocks'] <= cap + 1
            # at the default cap the same call makes ONE trip at most: what the suite exercised before the hook
            p = ps[None]
            units, workers, _, _ = C.trip_stats(kernel, p, p['launch'][:, j], np.array([n]))
            assert units[0] <= workers[0] or C.family_of(kernel) in ('k_minmax_partial', 'k_single_apply', 'k_bucket_generic'), (kernel, n)
    assert max(n for c in cases.values() for n in C.lengths_of(c)) < 512 * 1024


def test_the_unreached_instantiation_is_unreachable(lib):
    """k_bucket_groups<1,64>: with 4-byte aligned pointers scale_down reaches it only with fewer than 5 buckets."""
    assert sorted(C.UNREACHED) == ['k_bucket_groups<1,64>']
    rows = np.arange(257, 16385, dtype=np.int64)
    for nb in (2, 3, 4, 5, 6, 9, 100):
        for tail in (0, 1):
            p = plan(lib, queries(SCALE, (nb - 1) * rows + np.where(tail, 1, rows), rows))
            hit = p['launch'][:, 0]['kernel'] == b'k_bucket_groups<1,64>'
            assert not np.any(hit & (p['nb'] > 4)), (nb, tail, rows[hit & (p['nb'] > 4)][:5])
    assert np.any(plan(lib, queries(SCALE, 3 * 300 + 2, 300))['launch'][:, 0]['kernel'] == b'k_bucket_groups<1,64>')
