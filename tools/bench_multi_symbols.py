#!/usr/bin/env python3
"""The symbols of a whole model in one launch (MultiTensorSymbols, qd_multi_uniform_symbols_u8) against what save_compressed does
without it: the per-tensor loop over qd_uniform_f32 with its level output, at the same bucket sizes.

    python tools/bench_multi_symbols.py [--out profiles/multi_symbols_wrn16_22.json] [--reps 7] [--lib OTHER_libqd_hip.so]

The 60 WRN-16-22 parameter tensors (harness.kernel_bench.model_shapes), s = 16.  Two groups:
    per_channel   bucket_size = per_channel_bucket_sizes(tensors): one scale pair per output channel
    equal_256     bucket_size = [256] * 60
each with
    (a) one_launch   qd_multi_uniform_symbols_u8: 4 B read + 1 B written per element, 8 B per bucket
    (b) loop         qd_uniform_f32(x_i, <scratch>, n_i, b_i, 16, alpha, beta, sym_i, ...) per tensor, as _save calls it: 4 B read,
                     4 B of an fp32 result nobody reads and 1 B written per element, 60 launches
All in ONE process: HIP events on the launch stream around a few back-to-back sweeps (wall time, launch overhead included: that
is what the one launch removes), the rows taken in turn `reps` times over (interleaved), median / min / max of the repetitions
recorded.  The record says per group whether the one-launch median lies below the loop's with disjoint min-max ranges -- the
expectation the sibling launches were held to -- and gives the ratio; nothing is gated here.  For equal_256 it adds GB/s over
5 N + 8 buckets bytes and, as context, the level-histogram row of a benchmark record (--detail: a 4-B-read pass of the same kind).
--lib: measure another build of the library (plain symbol stores: kSymNT in csrc/qd_multi_symbols.hip)."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)


def timed(forms, reps):
    import torch
    for _, fn, iters in forms:                                           # warm-up: code objects, allocator, clocks
        for _ in range(2 * iters):
            fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    samples = {name: [] for name, _, _ in forms}
    for _ in range(reps):
        for name, fn, iters in forms:
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            samples[name].append(e0.elapsed_time(e1) / iters * 1e3)
    us = {name: {'median': round(statistics.median(s), 2), 'min': round(min(s), 2), 'max': round(max(s), 2)} for name, s in samples.items()}
    a, b = us['one_launch'], us['loop']
    return {'us': us, 'loop_over_one_launch': round(b['median'] / a['median'], 3),
            'ranges_overlap': a['max'] >= b['min'] and b['max'] >= a['min'],
            'one_launch_below_with_disjoint_ranges': a['median'] < b['median'] and a['max'] < b['min']}


def measure(reps, detail):
    import torch
    from harness import kernel_bench
    from quantized_distillation_amd import _lib
    from quantized_distillation_amd.multi_tensor import MultiTensorSymbols, per_channel_bucket_sizes
    dev = torch.device('cuda:0')
    lib = _lib.load()
    shapes = [tuple(int(d) for d in s) for s in kernel_bench.model_shapes('wrn')]
    gen = torch.Generator(device=dev).manual_seed(0)
    ws = [torch.randn(s, device=dev, generator=gen) * 0.05 for s in shapes]
    flat = [w.view(-1) for w in ws]
    n_all = sum(w.numel() for w in ws)
    syms = [torch.empty(w.numel(), dtype=torch.uint8, device=dev) for w in ws]
    scratch = torch.empty(max(w.numel() for w in ws), device=dev)
    wsp = _lib.workspace(dev)
    st = _lib.stream_ptr(dev)
    groups = {}
    for name, sizes in (('per_channel', per_channel_bucket_sizes(ws)), ('equal_256', [256] * len(ws))):
        one = MultiTensorSymbols(flat, 16, sizes, symbols=syms)
        ab = [torch.empty(max(one.buckets_total, 1), device=dev) for _ in range(2)]
        first = [4 * sum(a.numel() for a in one.alpha[:i]) for i in range(len(ws))]      # byte offset of every tensor's first bucket

        def loop(sizes=sizes, first=first, ab=ab):
            for x, sym, b, off in zip(flat, syms, sizes, first):
                lib.qd_uniform_f32(x.data_ptr(), scratch.data_ptr(), x.numel(), b, 16, ab[0].data_ptr() + off, ab[1].data_ptr() + off,
                                   sym.data_ptr(), None, 0, 0.0, 0, 0, wsp.data_ptr(), wsp.numel(), st)
        loop()
        one.encode()
        torch.cuda.synchronize()
        assert torch.equal(ab[0][:one.buckets_total], one._flat[0][:one.buckets_total]), 'the two forms disagree'
        g = timed([('one_launch', lambda one=one: one.encode(check_pointers=False), 10), ('loop', loop, 3)], reps)
        g['entry_points'] = [one.entry_point, 'qd_uniform_f32']
        g['buckets'] = one.buckets_total
        nbytes = 5 * n_all + 8 * one.buckets_total
        g['one_launch_bytes'] = nbytes
        g['one_launch_GBps'] = round(nbytes / g['us']['one_launch']['median'] / 1e3, 1)
        groups[name] = g
    context = None
    if detail and os.path.exists(detail):
        rows = json.load(open(detail)).get('roofline', {}).get('kernels', [])
        context = next((r for r in rows if str(r.get('name', '')).startswith('LVH')), None)
    return {'what': 'tools/bench_multi_symbols.py: 60 WRN-16-22 tensors, s = 16; one_launch: qd_multi_uniform_symbols_u8 (5 B per element); '
                    'loop: qd_uniform_f32 with its level output per tensor, the fp32 result into a scratch tensor (9 B per element, 60 '
                    'launches): what save_compressed does without the one launch; HIP events around back-to-back sweeps (wall, launch '
                    'overhead included), median / min / max of %d interleaved repetitions in one process, microseconds per sweep over all '
                    'tensors; GB/s over 5 N + 8 buckets bytes' % reps,
            'device': torch.cuda.get_device_name(0), 'library': os.path.relpath(_lib.LIB_PATH, ROOT) if _lib.LIB_PATH.startswith(ROOT + os.sep) else 'another build (--lib)',
            'tensors': len(shapes), 'elements': n_all, 'reps': reps, 'groups': groups,
            'context_level_histogram_row': context, 'context_from': os.path.relpath(detail, ROOT) if context else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'multi_symbols_wrn16_22.json'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--detail', default=os.path.join(ROOT, 'profiles', 'r06_bench_detail_default.json'))
    ap.add_argument('--lib', default=None)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error('--reps: at least 5')
    if args.lib:
        from quantized_distillation_amd import _lib
        _lib.LIB_PATH = os.path.abspath(args.lib)
    record = measure(args.reps, args.detail)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    for name, g in record['groups'].items():
        print('%-12s %s' % (name, '   '.join('%s %.2f us [%.2f .. %.2f]' % (k, v['median'], v['min'], v['max']) for k, v in g['us'].items())))
        print('%-12s %s' % ('', '   '.join('%s: %s' % (k, v) for k, v in g.items() if k not in ('us', 'entry_points'))))
    return 0


if __name__ == '__main__':
    sys.exit(main())
