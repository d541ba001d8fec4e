#!/usr/bin/env python3
"""The one-launch STE backward reading fp16 / bf16 gradients (MultiTensorSTE with 16-bit grads) against what the fp32-only
package offered for the same result: widen the gradients into an fp32 buffer, then the fp32 one launch in place.

    python tools/bench_multi_ste_in16.py [--out profiles/multi_ste_in16_wrn16_22.json] [--reps 7]

The 60 WRN-16-22 parameter tensors (harness.kernel_bench.model_shapes), bucket 256, s = 16, for bf16 and fp16.  Three rows in
each group:
    (a) in16_one_launch        qd_multi_ste_backward_in16_f32 into fp32 outs: 4 (x) + 2 (g) B read, 4 B written per element
    (b) widen_then_fp32_launch torch._foreach_copy_ of the 16-bit gradients into an fp32 buffer (2 + 4 B), then the fp32
                               MultiTensorSTE in place (4 + 4 + 4 B): 18 B per element and one more launch -- the same result
    (c) fp32_one_launch        the fp32 MultiTensorSTE in place alone (12 B per element): recorded, not gated
All in ONE process: HIP events on the launch stream around a few back-to-back calls (wall time of the calls, launch overhead
included), the rows taken in turn `reps` times over (interleaved: clock drift and host neighbours hit all of them), median /
min / max of the repetitions recorded.  The tool first checks that (a) and (b) give the same bits.
The gate: in both formats (a)'s max is below (b)'s min -- no overlap of the ranges, the reason the path exists.  The exit status
is 1 when it does not hold.  (a) against (c) is recorded, not gated.
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

ROWS = ('in16_one_launch', 'widen_then_fp32_launch', 'fp32_one_launch')


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
    return {'us': us, 'widen_path_over_in16': round(b['median'] / a['median'], 3), 'in16_over_fp32': round(a['median'] / c['median'], 3),
            'gate_in16_faster_than_the_widen_path_without_overlap': a['max'] < b['min'],
            'in16_faster_than_fp32_without_overlap': a['max'] < c['min']}


def measure(reps):
    import numpy as np
    import torch
    from harness import kernel_bench
    from quantized_distillation_amd.multi_tensor import MultiTensorSTE
    dev = torch.device('cuda:0')
    sizes = [int(np.prod(s)) for s in kernel_bench.model_shapes('wrn')]
    gen = torch.Generator(device=dev).manual_seed(0)
    ws = [torch.randn(n, device=dev, generator=gen) * 0.05 for n in sizes]
    g32 = [torch.randn(n, device=dev, generator=gen) * 0.01 for n in sizes]
    outs = [torch.empty(n, device=dev) for n in sizes]                   # (a)'s fp32 master gradients
    wide = [torch.empty(n, device=dev) for n in sizes]                   # (b)'s and (c)'s fp32 buffer, run in place
    groups = {}
    for dtype, dname in ((torch.bfloat16, 'bf16'), (torch.float16, 'fp16')):
        g16 = [g.to(dtype) for g in g32]
        direct = MultiTensorSTE(ws, g16, 16, 256, outs=outs)
        fp32 = MultiTensorSTE(ws, wide, 16, 256)

        def widen_then(fp32=fp32, g16=g16):
            torch._foreach_copy_(wide, g16)
            fp32.backward(check_pointers=False)
        direct.backward()
        want = [o.clone() for o in outs]
        widen_then()
        torch.cuda.synchronize()
        same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(want, wide))
        g = timed([(ROWS[0], lambda m=direct: m.backward(check_pointers=False), 10), (ROWS[1], widen_then, 10),
                   (ROWS[2], lambda m=fp32: m.backward(check_pointers=False), 10)], reps)
        g['entry_points'] = [direct.entry_point, fp32.entry_point]
        g['both_paths_give_the_same_bits'] = same
        groups['%s_bucket_256' % dname] = g
    return {'what': 'tools/bench_multi_ste_in16.py: 60 WRN-16-22 tensors, bucket 256, s = 16; HIP events around back-to-back calls (wall, '
                    'launch overhead included), median / min / max of %d interleaved repetitions in one process, microseconds per sweep '
                    'over all tensors' % reps,
            'device': torch.cuda.get_device_name(0), 'tensors': len(sizes), 'elements': sum(sizes), 'reps': reps, 'groups': groups,
            'both_paths_give_the_same_bits': all(g['both_paths_give_the_same_bits'] for g in groups.values()),
            'gate_holds': all(g['gate_in16_faster_than_the_widen_path_without_overlap'] for g in groups.values())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'multi_ste_in16_wrn16_22.json'))
    ap.add_argument('--reps', type=int, default=7)
    args = ap.parse_args()
    if args.reps < 7:
        ap.error('--reps: at least 7')
    record = measure(args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    for name, g in record['groups'].items():
        print('%-16s in16 %8.2f us  widen + fp32 %8.2f us  fp32 %8.2f us   widen path / in16 %.3f   in16 / fp32 %.3f   gate: %s   same bits: %s'
              % (name, g['us'][ROWS[0]]['median'], g['us'][ROWS[1]]['median'], g['us'][ROWS[2]]['median'], g['widen_path_over_in16'],
                 g['in16_over_fp32'], g['gate_in16_faster_than_the_widen_path_without_overlap'], g['both_paths_give_the_same_bits']))
    print('same bits: %s   gate holds: %s' % (record['both_paths_give_the_same_bits'], record['gate_holds']))
    return 0 if record['gate_holds'] and record['both_paths_give_the_same_bits'] else 1


if __name__ == '__main__':
    sys.exit(main())
