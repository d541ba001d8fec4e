"""Shapes at which every grid-stride loop of the transform kernels takes its second and later trips, shared by
tests/test_grid_trip_cases.py (the table against qd_transform_plan, no GPU) and tests/test_hip_grid_trips.py (the kernels against
the oracle on the GPU).  A plain helper module: no fixtures, nothing runs on import.

The launchers size a grid with one wave-tile per wave, so below billions of elements a kernel's loop over tiles, chunks or buckets
runs once per wave.  qd_set_grid_cap (include/qd_hip.h) caps the grid at 1, 2 or 3 blocks; this module picks, for every shipped
instantiation of the transform kernels, the smallest tensor whose plan UNDER EACH OF THOSE CAPS has

  * at least three trips for every wave / lane group / block of the grid (k_bucket_wave_any: iters >= 3 -- every wave runs
    every iteration -- so that a parity of its LDS exchange buffer is used twice),
  * trip counts that differ between the waves of one block (the last trip is partial), and
  * a ragged end (n % row in 1 .. 3, and row - 1): block 0's tail path runs next to the looping bulk.

Nothing here is trusted: trip_stats() computes the trips from the plan's own blocks / nchunks / nbk / nvec / nb, and both test
modules assert the three properties from it for every case they run.  Bucket sizes come from the lists the plan itself selects
from (QD_VEC_SHAPES / QD_WAVE_SHAPES_* of csrc/qd_plan.h, read as text), tests/abi_contract.py BUCKET_PATHS and
tests/test_transform_plan.py BOUNDARIES."""
import collections
import os
import re

import numpy as np

import abi_contract as A
from test_transform_plan import BOUNDARIES, NEAREST, QDQ, SCALE, plan, queries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPS = (1, 2, 3)
GRID_CAP_DEFAULT = 1 << 20
MIN_TRIPS = 3
MAX_FULL = 2100                # full buckets tried per bucket size (bucket 1 needs 1983 buckets for a lane-group kernel; see below)

# what the coverage assertion leaves out, each with its reason
NOT_LOOPED = {
    'k_single_fused': 'its grid holds the tensor in registers and must be co-resident: sized by fused_blocks, never capped, no loop',
    'k_minmax_final': 'one block by construction: it folds the partials of k_minmax_partial',
}
# shipped instantiations that no valid call can take through three trips; tests/test_grid_trip_cases.py proves each entry from
# the plan (the entry is wrong, and the test fails, as soon as some shape reaches the kernel with that many buckets)
UNREACHED = {
    'k_bucket_groups<1,64>': 'scale_down has no side output to misalign and its fp32 pointers are 4-byte aligned by contract, so a '
                             'bucket of 257 .. 16384 elements reaches the lane-group kernel only with fewer full buckets than a chunk '
                             'holds (m <= 4): at most 4 buckets, one trip of one block at any cap',
}


def header_shapes(macro):
    """The X(...) tuples of a shape list of csrc/qd_plan.h."""
    text = open(os.path.join(ROOT, 'quantized_distillation_amd', 'csrc', 'qd_plan.h')).read()
    body = re.search(r'#define %s\(X\)((?:[^\n]*\\\n)*[^\n]*\n)' % macro, text).group(1)       # the continuation lines of the macro
    return [tuple(int(v) for v in t.split(',')) for t in re.findall(r'X\(([^)]*)\)', body)]


VEC_SHAPES = header_shapes('QD_VEC_SHAPES')                                  # (row, lanes per bucket, float4 per lane, buckets per group)
WAVE_SHAPES = {QDQ: header_shapes('QD_WAVE_SHAPES_QDQ'), SCALE: header_shapes('QD_WAVE_SHAPES_SCALE'),
               NEAREST: header_shapes('QD_WAVE_SHAPES_NEAREST')}


def wave_bucket(v, g):
    """The largest bucket size that is no multiple of 4 in the range of k_bucket_wave_any<., v, g>: row / 4 + 2 + 7 == 64 g v
    float4s (the first-fit rule of plan_transform), so the rotated last float4 and both shared edge float4s are in play."""
    return 4 * (64 * g * v - 9) + 3


def trip_stats(name, p, launch, n):
    """(units, workers, workers per block, trips) of one planned launch, from the plan alone -- vectorised over plans.
    units: what the kernel's loop strides over; workers: how many stride side by side (waves, lane groups, blocks, threads);
    trips: the FEWEST trips any worker makes (k_bucket_wave_any: the iterations all of them make)."""
    base, _, targs = name.partition('<')
    t = [int(a) if a.isdigit() else a for a in targs.rstrip('>').split(',')] if targs else []
    blocks = launch['blocks'].astype(np.int64)
    if base == 'k_bucket_vec':
        bpw = (64 // t[1]) * t[3]
        units, per_block = -(-p['nvec'] // bpw), 4
    elif base in ('k_bucket_chunk', 'k_bucket_chunk_any'):
        units, per_block = p['nchunks'], 2
    elif base == 'k_bucket_wave_any':
        units, per_block = p['nbk'], 4 // t[2]
    elif base == 'k_bucket_groups':
        units, per_block = p['nb'], 256 // t[1]
    elif base == 'k_bucket_generic':
        units, per_block = p['nb'], 1
    elif base in ('k_minmax_partial', 'k_single_apply'):
        units, per_block = n // 4, 256                                       # float4s over threads
    elif base == 'k_nearest_prescaled_stream':
        units, per_block = -(-(n // 4) // 256), 4                            # 4 KiB tiles over waves
    else:
        raise AssertionError('no loop arithmetic for ' + name)
    workers = blocks * per_block
    trips = -(-units // workers) if base == 'k_bucket_wave_any' else units // workers
    return units, workers, per_block, trips


def loops_as_wanted(name, p, launch, n):
    """>= MIN_TRIPS trips for every worker, and a partial last trip that splits the workers of ONE block (a single worker has
    nobody to differ from)."""
    units, workers, per_block, trips = trip_stats(name, p, launch, n)
    left = units % workers
    partial = np.where(workers == 1, True, (left % per_block != 0) if per_block > 1 else (left != 0))
    return (trips >= MIN_TRIPS) & partial


class Capped(object):
    """`with Capped(lib, cap):` -- the hook set, and restored whatever happens; cap None leaves the default."""

    def __init__(self, lib, cap):
        self.lib, self.cap = lib, cap

    def __enter__(self):
        if self.cap is not None:
            prev = self.lib.qd_set_grid_cap(self.cap)
            assert prev == GRID_CAP_DEFAULT, 'the grid cap was left at %d by somebody' % prev

    def __exit__(self, *exc):
        if self.cap is not None:
            self.lib.qd_set_grid_cap(-1)
        return False


def plans_under_caps(lib, q):
    """{cap: plan} for cap in (None, 1, 2, 3)."""
    out = {}
    for cap in (None,) + CAPS:
        with Capped(lib, cap):
            out[cap] = plan(lib, q)
    return out


def tails_of(bucket):
    """The two ragged ends of a bucketed case: n % row in 1 .. 3, and row - 1."""
    return (1 + bucket % 3, bucket - 1)


# one entry per way of reaching a kernel: (mode, bucket, query options, call options)
Config = collections.namedtuple('Config', 'mode bucket query call')
Case = collections.namedtuple('Case', 'kernel mode bucket nfull query call')        # n = nfull * bucket + tail, tail in tails_of(bucket)
K4 = dict(k=16, assign_mode=0, side_bytes=8)                                           # the nearest-point default: 16 points, int64 indices


def configs():
    out = []
    buckets = sorted({b for b, _, _ in A.BUCKET_PATHS} | {b for b, _ in BOUNDARIES} | {r for r, _, _, _ in VEC_SHAPES} | {4, 448, 2000})
    for mode in (QDQ, SCALE, NEAREST):
        base = dict(K4) if mode == NEAREST else {}
        for b in sorted(set(buckets) | {wave_bucket(v, g) for v, g in WAVE_SHAPES[mode]}):
            out.append(Config(mode, b, dict(base), {}))
        # the lane-group kernels behind a side output the vector accesses cannot take: level_idx off its 4 bytes, an int64 idx
        # off its 16
        if mode == QDQ:
            out += [Config(mode, b, dict(side_bytes=1, side_misalign=1), dict(lev=1, lev_phase=1)) for b in (100, 300)]
        if mode == NEAREST:
            out += [Config(mode, b, dict(base, side_misalign=8), dict(idx_phase=8)) for b in (100, 300)]
            out += [Config(mode, b, dict(k=16, assign_mode=1, side_bytes=1, prescaled=1), dict(prescaled=1, idx_bytes=1, assign_mode=1))
                    for b in (33, 100)]                                                # the pre-processed forward: the stream
    return out


def single_configs():
    """One bucket spanning the tensor, the one-launch kernel switched off: k_minmax_partial + k_single_apply."""
    out = [Config(mode, 0, dict(K4, fused_capacity=0) if mode == NEAREST else dict(fused_capacity=0), dict(fused_mode=0))
           for mode in (QDQ, SCALE, NEAREST)]
    return out


def find_cases(lib):
    """{kernel name: Case} -- for every kernel some configuration reaches, the smallest n whose plan loops as wanted under every
    cap, at both ragged ends."""
    best = {}

    def offer(kernel, n, case):
        if kernel not in best or n < best[kernel][0]:
            best[kernel] = (n, case)

    for cfg in configs():
        if cfg.bucket < 4:
            continue
        nfull = np.arange(1, MAX_FULL + 1, dtype=np.int64)
        good = np.ones(nfull.size, bool)
        kernel = None
        for tail in tails_of(cfg.bucket):
            n = nfull * cfg.bucket + tail
            ps = plans_under_caps(lib, queries(cfg.mode, n, cfg.bucket, **cfg.query))
            kern = ps[None]['launch'][:, 0]['kernel']
            kernel = kern if kernel is None else kernel
            good &= (ps[None]['nlaunch'] == 1) & (kern == kernel)
            for cap in CAPS:
                ok = np.zeros(nfull.size, bool)
                for name in np.unique(kern):
                    s = kern == name
                    ok[s] = loops_as_wanted(name.decode(), ps[cap][s], ps[cap]['launch'][s, 0], n[s])
                good &= ok
        for i in np.flatnonzero(good):
            name = kernel[i].decode()
            offer(name, int(nfull[i]) * cfg.bucket, Case(name, cfg.mode, cfg.bucket, int(nfull[i]), cfg.query, cfg.call))
    for cfg in single_configs():
        n = np.arange(16385, 16385 + 4096, dtype=np.int64)
        n = n[n % 4 != 0]                                                     # ragged: the scalar tail loop of both kernels
        ps = plans_under_caps(lib, queries(cfg.mode, n, 0, **cfg.query))
        good = ps[None]['nlaunch'] == 2
        for cap in CAPS:
            for j in range(2):
                name = ps[None]['launch'][0, j]['kernel'].decode()
                good &= loops_as_wanted(name, ps[cap], ps[cap]['launch'][:, j], n)
        i = int(np.flatnonzero(good)[0])
        for j in range(2):
            name = ps[None]['launch'][i, j]['kernel'].decode()
            offer(name, int(n[i]), Case(name, cfg.mode, 0, int(n[i]), cfg.query, cfg.call))
    return {k: c for k, (_, c) in best.items()}


def lengths_of(case):
    """The tensor lengths a case runs at."""
    if case.bucket == 0:
        return [case.nfull]                                                  # one bucket: nfull IS n
    return [case.nfull * case.bucket + t for t in tails_of(case.bucket)]


def family_of(kernel):
    return kernel.partition('<')[0]


def wanted(shipped):
    """The shipped transform instantiations the cases must reach."""
    pat = re.compile(r'^(k_bucket_|k_single_|k_minmax_|k_nearest_prescaled_stream)')
    return sorted(k for k in shipped if pat.match(k) and family_of(k) not in NOT_LOOPED)
