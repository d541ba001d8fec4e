#!/usr/bin/env python3
"""One launch with a level count per tensor (MultiTensorQuantizer / MultiTensorSTE with a sequence s) against the per-tensor
loop at the same level counts, and against the scalar-s one launch on the same tensors.

    python tools/bench_multi_levels.py [--out profiles/multi_levels_wrn16_22.json] [--reps 7]

The 60 WRN-16-22 parameter tensors (harness.kernel_bench.model_shapes), s = 256 for the first and the last tensor and 16 / 4
alternating in between ("8 bits first and last").  Three groups -- the quantizer at bucket 256, the quantizer without buckets,
the bucket-aware STE backward at bucket 256 -- and three rows in each:
    (a) mixed_one_launch   the sequence s: qd_multi_uniform_levels_f32 / ..._global_levels_f32 / qd_multi_ste_backward_levels_f32
    (b) loop               uniformQuantization(t_i, s_i, ...) / ste_bucket_backward(w_i, g_i, bucket, s_i) per tensor
    (c) scalar_one_launch  s = 16 for every tensor: the existing entry point and kernel, the like-for-like ceiling of (a) --
                           both move the same bytes
All in ONE process: HIP events on the launch stream around a few back-to-back calls (wall time of the calls, launch overhead
included: that is what the one launch removes), the rows taken in turn `reps` times over (interleaved: clock drift and host
neighbours hit all of them), median / min / max of the repetitions recorded.  Recorded, not gated: the record says whether the
median of (a) lies inside the min-max spread of (c) and gives the ratios.
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)


def level_counts(n):
    return [256 if i in (0, n - 1) else (16, 4)[i % 2] for i in range(n)]


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
    a, b, c = us['mixed_one_launch'], us['loop'], us['scalar_one_launch']
    return {'us': us, 'loop_over_mixed': round(b['median'] / a['median'], 2), 'mixed_over_scalar': round(a['median'] / c['median'], 3),
            'mixed_median_inside_the_scalar_spread': c['min'] <= a['median'] <= c['max'],
            'ranges_overlap': a['max'] >= c['min'] and c['max'] >= a['min']}


def measure(reps):
    import numpy as np
    import torch
    import quantization
    from harness import kernel_bench
    from quantized_distillation_amd import ste
    from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer, MultiTensorSTE
    dev = torch.device('cuda:0')
    sizes = [int(np.prod(s)) for s in kernel_bench.model_shapes('wrn')]
    s_list = level_counts(len(sizes))
    gen = torch.Generator(device=dev).manual_seed(0)
    ws = [torch.randn(n, device=dev, generator=gen) * 0.05 for n in sizes]
    grads = [torch.randn(n, device=dev, generator=gen) for n in sizes]
    outs = [torch.empty(n, device=dev) for n in sizes]
    groups = {}
    for name, bucket in (('quantize_bucket_256', 256), ('quantize_no_buckets', None)):
        mixed = MultiTensorQuantizer(ws, s_list, bucket, outputs=outs)
        scalar = MultiTensorQuantizer(ws, 16, bucket, outputs=outs)

        def loop(bucket=bucket):
            for w, s in zip(ws, s_list):
                quantization.uniformQuantization(w, s, bucket_size=bucket)
        groups[name] = timed([('mixed_one_launch', lambda m=mixed: m.quantize(check_pointers=False), 10), ('loop', loop, 3),
                              ('scalar_one_launch', lambda m=scalar: m.quantize(check_pointers=False), 10)], reps)
        groups[name]['entry_points'] = [mixed.entry_point, scalar.entry_point]
    mixed = MultiTensorSTE(ws, grads, s_list, 256, outs=outs)
    scalar = MultiTensorSTE(ws, grads, 16, 256, outs=outs)

    def loop_ste():
        for w, g, o, s in zip(ws, grads, outs, s_list):
            ste.ste_bucket_backward(w, g, 256, s, out=o)
    groups['ste_bucket_256'] = timed([('mixed_one_launch', lambda: mixed.backward(check_pointers=False), 10), ('loop', loop_ste, 3),
                                      ('scalar_one_launch', lambda: scalar.backward(check_pointers=False), 10)], reps)
    groups['ste_bucket_256']['entry_points'] = [mixed.entry_point, scalar.entry_point]
    return {'what': 'tools/bench_multi_levels.py: 60 WRN-16-22 tensors, s = 256 first and last, 16 / 4 alternating in between; HIP events '
                    'around back-to-back calls (wall, launch overhead included), median / min / max of %d interleaved repetitions in '
                    'one process, microseconds per sweep over all tensors' % reps,
            'device': torch.cuda.get_device_name(0), 'tensors': len(sizes), 'elements': sum(sizes), 'level_counts': s_list, 'reps': reps,
            'groups': groups}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'multi_levels_wrn16_22.json'))
    ap.add_argument('--reps', type=int, default=7)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error('--reps: at least 5')
    record = measure(args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    for name, g in record['groups'].items():
        print('%-22s mixed %8.2f us  loop %8.2f us  scalar %8.2f us   loop / mixed %.2f   mixed / scalar %.3f   inside the scalar spread: %s'
              % (name, g['us']['mixed_one_launch']['median'], g['us']['loop']['median'], g['us']['scalar_one_launch']['median'],
                 g['loop_over_mixed'], g['mixed_over_scalar'], g['mixed_median_inside_the_scalar_spread']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
