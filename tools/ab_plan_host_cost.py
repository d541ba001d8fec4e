#!/usr/bin/env python3
"""Host cost of one qd_uniform_f32 call through this tree's libqd_hip.so and through ANOTHER build of it (the parent commit's),
both loaded in one process under different file names and timed interleaved.

    python tools/ab_plan_host_cost.py OTHER_libqd_hip.so [repetitions, default 9] > profiles/transform_plan_host_cost.txt

The launcher plans on every call (csrc/qd_plan.h), the training loops' 500-element eager one included (DESIGN.md section 1:
about 4.5 us of host time per call, 3.1 of it hipLaunchKernel).  Two sizes: n = 500 (two buckets of 256: the loops' call) and
64 Ki elements at bucket 256.  Host time only, as tools/ab_api_overhead.py takes it: the queue kept shallow, a sync every 64
calls, the sync not timed; straight through ctypes with the arguments built once, so both libraries pay the same binding cost.
Accepted when the new median lies inside the other library's min-max range at both sizes."""
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from quantized_distillation_amd import _lib  # noqa: E402


def host_only(fn, args, reps):
    """Host time per call with the device queue kept shallow (sync every 64 calls, sync time excluded)."""
    fn(*args)
    torch.cuda.synchronize()
    tot, done = 0.0, 0
    while done < reps:
        t0 = time.perf_counter()
        for _ in range(64):
            fn(*args)
        tot += time.perf_counter() - t0
        done += 64
        torch.cuda.synchronize()
    return tot / done * 1e6


def main():
    other_path = os.path.abspath(sys.argv[1])
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    this = _lib.load()
    other = ctypes.CDLL(other_path)
    assert os.path.realpath(other_path) != os.path.realpath(_lib.LIB_PATH), 'the other library must be another file'
    res, args = _lib.SIGNATURES['qd_uniform_f32']
    other.qd_uniform_f32.restype, other.qd_uniform_f32.argtypes = res, args
    dev = torch.device('cuda:0')
    ws = _lib.workspace(dev)
    stream = _lib.stream_ptr(dev)
    sizes = (500, 64 * 1024)
    calls = {}
    for n in sizes:
        x = torch.randn(n, device=dev)
        outs = {}
        for name, lib in (('other', other), ('this', this)):
            q, a, b = torch.empty_like(x), torch.empty((n + 255) // 256, device=dev), torch.empty((n + 255) // 256, device=dev)
            argv = (x.data_ptr(), q.data_ptr(), n, 256, 16, a.data_ptr(), b.data_ptr(), None, None, 0, 0.0, 0, 0, ws.data_ptr(), ws.numel(), stream)
            assert lib.qd_uniform_f32(*argv) == 0
            outs[name] = (q, a, b)
            calls[(name, n)] = (lib.qd_uniform_f32, argv, (x, q, a, b))
        torch.cuda.synchronize()
        assert all(torch.equal(s, t) for s, t in zip(outs['other'], outs['this'])), 'the two libraries disagree'
    out = {key: [] for key in calls}
    order = (('other', other), ('this', this))
    for rep in range(reps):
        for name, _ in (order if rep % 2 == 0 else order[::-1]):
            for n in sizes:
                fn, argv, _keep = calls[(name, n)]
                out[(name, n)].append(host_only(fn, argv, 6400))
    print('Host cost of qd_uniform_f32(n, bucket 256, 16 levels) through ctypes -- this tree\'s libqd_hip.so ("this": the launcher plans,')
    print('csrc/qd_plan.h, then launches) and %s ("other": the parent commit\'s launcher), both loaded in ONE process,' % os.path.basename(other_path))
    print('%d repetitions each, interleaved (order swapped every repetition); host time only: 6400 calls, a sync every 64, not timed.' % reps)
    print('torch %s, %s' % (torch.__version__, torch.cuda.get_device_name(0)))
    print()
    print('%-8s %8s %10s %10s %10s   %s' % ('library', 'n', 'median us', 'min us', 'max us', 'all'))
    ok = True
    for n in sizes:
        for name, _ in order:
            v = out[(name, n)]
            print('%-8s %8d %10.3f %10.3f %10.3f   %s' % (name, n, statistics.median(v), min(v), max(v), ' '.join('%.3f' % t for t in v)))
        o, t = out[('other', n)], out[('this', n)]
        inside = min(o) <= statistics.median(t) <= max(o)
        ok = ok and (inside or statistics.median(t) < min(o))
        print('n = %d: this median - other median = %+.3f us; this median is %s the other library\'s min-max range'
              % (n, statistics.median(t) - statistics.median(o), 'inside' if inside else 'BELOW' if statistics.median(t) < min(o) else 'ABOVE'))
    print()
    print('accepted' if ok else 'NOT accepted: the new median lies above the other library\'s range')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
