#!/usr/bin/env python3
"""The one-launch quantizer writing fp16 / bf16 outputs (MultiTensorQuantizer(out_dtype=...)) against what the fp32-only package
offered for the same result: the fp32 one launch into fp32 shadows followed by a cast into the 16-bit tensors.

    python tools/bench_multi_out16.py [--out profiles/multi_out16_wrn16_22.json] [--reps 7]

The 60 WRN-16-22 parameter tensors (harness.kernel_bench.model_shapes), s = 16, at bucket 256 and without buckets, for bf16
and fp16.  Three rows in each of the four groups:
    (a) out16_one_launch      qd_multi_uniform_out16_f32 / qd_multi_uniform_global_out16_f32: 4 B read + 2 B written per element
    (b) fp32_launch_then_cast the fp32 one launch into fp32 shadows (4 + 4 B), then torch._foreach_copy_ into the 16-bit tensors
                              (4 + 2 B): 14 B per element and one more launch -- the same 16-bit result
    (c) fp32_one_launch       the fp32 one launch alone (8 B per element): recorded, the yardstick of the stores
(without buckets every row reads the input twice: 4 B per element more.)
All in ONE process: HIP events on the launch stream around a few back-to-back calls (wall time of the calls, launch overhead
included), the rows taken in turn `reps` times over (interleaved: clock drift and host neighbours hit all of them), median /
min / max of the repetitions recorded.
The gate: in every group (a) is faster than (b) with no overlap of their min-max ranges -- the reason the path exists.  The exit
status is 1 when it does not hold.  (a) against (c) is recorded, not gated.
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

ROWS = ('out16_one_launch', 'fp32_launch_then_cast', 'fp32_one_launch')


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
    a, b, c = (us[r] for r in ROWS)
    return {'us': us, 'cast_path_over_out16': round(b['median'] / a['median'], 3), 'out16_over_fp32': round(a['median'] / c['median'], 3),
            'gate_out16_faster_than_the_cast_path_without_overlap': a['max'] < b['min'],
            'out16_faster_than_fp32_without_overlap': a['max'] < c['min']}


def measure(reps):
    import numpy as np
    import torch
    from harness import kernel_bench
    from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer
    dev = torch.device('cuda:0')
    sizes = [int(np.prod(s)) for s in kernel_bench.model_shapes('wrn')]
    gen = torch.Generator(device=dev).manual_seed(0)
    ws = [torch.randn(n, device=dev, generator=gen) * 0.05 for n in sizes]
    shadows = [torch.empty(n, device=dev) for n in sizes]
    groups = {}
    for dtype, dname in ((torch.bfloat16, 'bf16'), (torch.float16, 'fp16')):
        outs16 = [torch.empty(n, dtype=dtype, device=dev) for n in sizes]
        for bname, bucket in (('bucket_256', 256), ('no_buckets', None)):
            direct = MultiTensorQuantizer(ws, 16, bucket, outputs=outs16)
            fp32 = MultiTensorQuantizer(ws, 16, bucket, outputs=shadows)

            def then_cast(fp32=fp32, outs16=outs16):
                fp32.quantize(check_pointers=False)
                torch._foreach_copy_(outs16, shadows)
            direct.quantize()
            want = [o.clone() for o in outs16]
            then_cast()
            torch.cuda.synchronize()
            same = all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(want, outs16))
            g = timed([(ROWS[0], lambda m=direct: m.quantize(check_pointers=False), 10), (ROWS[1], then_cast, 10),
                       (ROWS[2], lambda m=fp32: m.quantize(check_pointers=False), 10)], reps)
            g['entry_points'] = [direct.entry_point, fp32.entry_point]
            g['both_paths_give_the_same_bits'] = same
            groups['%s_%s' % (dname, bname)] = g
    return {'what': 'tools/bench_multi_out16.py: 60 WRN-16-22 tensors, s = 16; HIP events around back-to-back calls (wall, launch overhead '
                    'included), median / min / max of %d interleaved repetitions in one process, microseconds per sweep over all '
                    'tensors' % reps,
            'device': torch.cuda.get_device_name(0), 'tensors': len(sizes), 'elements': sum(sizes), 'reps': reps, 'groups': groups,
            'gate_holds': all(g['gate_out16_faster_than_the_cast_path_without_overlap'] for g in groups.values())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'multi_out16_wrn16_22.json'))
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
        print('%-16s out16 %8.2f us  fp32 + cast %8.2f us  fp32 %8.2f us   cast path / out16 %.3f   out16 / fp32 %.3f   gate: %s   same bits: %s'
              % (name, g['us'][ROWS[0]]['median'], g['us'][ROWS[1]]['median'], g['us'][ROWS[2]]['median'], g['cast_path_over_out16'],
                 g['out16_over_fp32'], g['gate_out16_faster_than_the_cast_path_without_overlap'], g['both_paths_give_the_same_bits']))
    print('gate holds: %s' % record['gate_holds'])
    return 0 if record['gate_holds'] else 1


if __name__ == '__main__':
    sys.exit(main())
