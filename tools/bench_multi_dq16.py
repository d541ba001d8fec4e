#!/usr/bin/env python3
"""The one-launch differentiable-quantization sweeps on a 16-bit student (MultiTensorDiffQuant with fp16 / bf16 outputs and
gradients) against what the fp32-only package offered for the same result: fp32 shadows and a cast around each sweep.

    python tools/bench_multi_dq16.py [--out profiles/multi_dq16_wrn16_22.json] [--reps 7] [--parent-results FILE]

The 60 WRN-16-22 parameter tensors (harness.kernel_bench.model_shapes), bf16 and fp16, 4 and 16 points per tensor.
Forward at bucket 256 and without buckets, three rows:
    (i)   out16_one_launch       qd_multi_nearest_out16_f32: 4 (u) B read, 2 (q) + 1 (idx) B written per element
    (ii)  fp32_launch_then_cast  qd_multi_nearest_f32 into fp32 shadows (9 B), then torch._foreach_copy_ into the 16-bit tensors
                                 (4 + 2 B): 15 B per element and a launch more -- the same result
    (iii) fp32_one_launch        qd_multi_nearest_f32 alone (9 B): recorded, not gated
Backward at bucket 256, three rows:
    (i)   in16_one_launch        qd_multi_point_grad_in16_f32: 2 (g) + 1 (idx) B read per element
    (ii)  widen_then_fp32_launch torch._foreach_copy_ of the 16-bit gradients into fp32 buffers (2 + 4 B), then
                                 qd_multi_point_grad_f32 (5 B): 11 B per element and a launch more -- the same result
    (iii) fp32_one_launch        qd_multi_point_grad_f32 alone (5 B): recorded, not gated
All in ONE process: HIP events on the launch stream around a few back-to-back calls (wall time of the calls, launch overhead
included), the rows of a group taken in turn `reps` times over (interleaved: clock drift and host neighbours hit all of them),
median / min / max of the repetitions recorded.  Before a group is timed the tool checks that (i) and (ii) give the same bits.
The gate: in every group (i)'s max is below (ii)'s min -- no overlap of the ranges.  The exit status is 1 when it does not hold
or the bits differ.  (i) against (iii) is recorded, not gated.

--parent-results: the RESULT lines of the parent commit's `tools/bench_multi_dq.py --config B,K` taken on the same machine in the
same session (one per line); the record then says for every fp32 row whether its median lies inside the parent's min-max.
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

FWD_ROWS = ('out16_one_launch', 'fp32_launch_then_cast', 'fp32_one_launch')
BWD_ROWS = ('in16_one_launch', 'widen_then_fp32_launch', 'fp32_one_launch')
POINTS = (4, 16)
ITERS = 10


def timed(forms, reps):
    import torch
    for _, fn in forms:                                                  # warm-up: code objects, allocator, clocks
        for _ in range(2 * ITERS):
            fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    samples = {name: [] for name, _ in forms}
    for _ in range(reps):
        for name, fn in forms:
            e0.record()
            for _ in range(ITERS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            samples[name].append(e0.elapsed_time(e1) / ITERS * 1e3)
    us = {name: {'median': round(statistics.median(s), 2), 'min': round(min(s), 2), 'max': round(max(s), 2)} for name, s in samples.items()}
    a, b, c = (us[name] for name, _ in forms)
    return {'us': us, 'composed_over_16bit': round(b['median'] / a['median'], 3), '16bit_over_fp32': round(a['median'] / c['median'], 3),
            'gate_16bit_faster_than_the_composed_path_without_overlap': a['max'] < b['min'],
            '16bit_faster_than_fp32_without_overlap': a['max'] < c['min']}


def same16(a, b):
    import torch
    return all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(a, b))


def measure(reps):
    import numpy as np
    import torch
    from harness import kernel_bench
    from quantized_distillation_amd.multi_tensor import MultiTensorDiffQuant
    dev = torch.device('cuda:0')
    sizes = [int(np.prod(s)) for s in kernel_bench.model_shapes('wrn')]
    gen = torch.Generator(device=dev).manual_seed(0)
    ws = [torch.randn(n, device=dev, generator=gen) for n in sizes]
    g32 = [torch.randn(n, device=dev, generator=gen) for n in sizes]
    q32 = [torch.empty(n, device=dev) for n in sizes]                    # (ii)'s and (iii)'s fp32 shadow of the weights
    wide = [torch.empty(n, device=dev) for n in sizes]                   # (ii)'s and (iii)'s fp32 shadow of the gradients
    groups = {}
    for dtype, dname in ((torch.bfloat16, 'bf16'), (torch.float16, 'fp16')):
        g16 = [g.to(dtype) for g in g32]
        q16 = [torch.empty(n, dtype=dtype, device=dev) for n in sizes]  # (i)'s outputs
        cast = [torch.empty(n, dtype=dtype, device=dev) for n in sizes] # (ii)'s outputs
        for k in POINTS:
            pts = torch.sort(torch.rand(len(sizes), k, device=dev, generator=gen), dim=1)[0].contiguous()
            gp16, gp32 = torch.empty(len(sizes), k, device=dev), torch.empty(len(sizes), k, device=dev)
            for bucket in (256, None):
                direct = MultiTensorDiffQuant(ws, q16, g16, k, bucket)
                fp32 = MultiTensorDiffQuant(ws, q32, wide, k, bucket)

                def launch_then_cast(fp32=fp32, pts=pts):
                    fp32.forward(pts)
                    torch._foreach_copy_(cast, q32)

                def widen_then_launch(fp32=fp32, g16=g16, gp32=gp32):
                    torch._foreach_copy_(wide, g16)
                    fp32.backward(out=gp32)
                direct.forward(pts)
                launch_then_cast()
                torch.cuda.synchronize()
                same = same16(q16, cast) and all(torch.equal(a, b) for a, b in zip(direct.indices, fp32.indices))
                g = timed([(FWD_ROWS[0], lambda m=direct, p=pts: m.forward(p)), (FWD_ROWS[1], launch_then_cast),
                           (FWD_ROWS[2], lambda m=fp32, p=pts: m.forward(p))], reps)
                g['entry_points'] = [direct.entry_point, fp32.entry_point]
                g['both_paths_give_the_same_bits'] = same
                g['one_launch_gbps'] = round(sum(sizes) * 7 / g['us'][FWD_ROWS[0]]['median'] / 1e3, 1)
                groups['%s_k%d_forward_%s' % (dname, k, 'bucket_256' if bucket else 'no_buckets')] = g
                if bucket is None:
                    continue
                direct.backward(out=gp16)
                widen_then_launch()
                torch.cuda.synchronize()
                same = torch.equal(gp16.view(torch.int32), gp32.view(torch.int32)) and bool(torch.isfinite(gp16).all())
                g = timed([(BWD_ROWS[0], lambda m=direct, o=gp16: m.backward(out=o)), (BWD_ROWS[1], widen_then_launch),
                           (BWD_ROWS[2], lambda m=fp32, o=gp32: m.backward(out=o))], reps)
                g['entry_points'] = [direct.entry_point, fp32.entry_point]
                g['both_paths_give_the_same_bits'] = same
                g['one_launch_gbps'] = round(sum(sizes) * 3 / g['us'][BWD_ROWS[0]]['median'] / 1e3, 1)
                groups['%s_k%d_backward_bucket_256' % (dname, k)] = g
    return {'what': 'tools/bench_multi_dq16.py: 60 WRN-16-22 tensors; HIP events around back-to-back calls (wall, launch overhead '
                    'included), median / min / max of %d interleaved repetitions in one process, microseconds per sweep over all '
                    'tensors; one_launch_gbps: 7 (forward) / 3 (backward) bytes per element over the 16-bit launch\'s median' % reps,
            'device': torch.cuda.get_device_name(0), 'tensors': len(sizes), 'elements': sum(sizes), 'reps': reps, 'groups': groups,
            'both_paths_give_the_same_bits': all(g['both_paths_give_the_same_bits'] for g in groups.values()),
            'gate_holds': all(g['gate_16bit_faster_than_the_composed_path_without_overlap'] for g in groups.values())}


def against_parent(record, path):
    """The fp32 rows against the parent commit's one-launch figures: {configuration: {sweep: {...}}}."""
    parent = {}
    with open(path) as f:
        for line in f:
            if line.startswith('RESULT '):
                r = json.loads(line[7:])
                parent[(r['bucket_size'], r['points'])] = r['us']
    out = {}
    for name, g in record['groups'].items():
        _, k, sweep, rest = name.split('_', 3)
        key = (256 if rest == 'bucket_256' else None, int(k[1:]))
        if key not in parent:
            continue
        p = parent[key]['one_launch_' + sweep]
        mine = g['us']['fp32_one_launch']
        out[name] = {'parent_one_launch_us': p, 'fp32_one_launch_us': mine, 'median_inside_the_parents_min_max': p['min'] <= mine['median'] <= p['max']}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'multi_dq16_wrn16_22.json'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--parent-results')
    args = ap.parse_args()
    if args.reps < 7:
        ap.error('--reps: at least 7')
    record = measure(args.reps)
    if args.parent_results:
        record['fp32_rows_against_the_parent_commit'] = against_parent(record, args.parent_results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    for name, g in record['groups'].items():
        a, b, c = (g['us'][r] for r in (FWD_ROWS if '_forward_' in name else BWD_ROWS))
        print('%-32s 16-bit %8.2f (%.2f-%.2f) us  composed %8.2f (%.2f-%.2f) us  fp32 %8.2f us   composed / 16-bit %.3f   16-bit / fp32 %.3f   '
              'gate: %s   same bits: %s' % (name, a['median'], a['min'], a['max'], b['median'], b['min'], b['max'], c['median'],
                                            g['composed_over_16bit'], g['16bit_over_fp32'],
                                            g['gate_16bit_faster_than_the_composed_path_without_overlap'], g['both_paths_give_the_same_bits']))
    for name, r in record.get('fp32_rows_against_the_parent_commit', {}).items():
        print('%-32s fp32 %8.2f us, parent %.2f-%.2f us: inside: %s' % (name, r['fp32_one_launch_us']['median'], r['parent_one_launch_us']['min'],
                                                                        r['parent_one_launch_us']['max'], r['median_inside_the_parents_min_max']))
    print('same bits: %s   gate holds: %s' % (record['both_paths_give_the_same_bits'], record['gate_holds']))
    return 0 if record['gate_holds'] and record['both_paths_give_the_same_bits'] else 1


if __name__ == '__main__':
    sys.exit(main())
