#!/usr/bin/env python3
"""One-launch differentiable quantization (MultiTensorDiffQuant) against the per-tensor loop it replaces, by geometry.

    python tools/bench_multi_dq.py [--out profiles/multi_dq_geometry.json] [--reps 7]

For each configuration (bucket_size, points per tensor) on the WRN-16-22 parameter shapes (harness.kernel_bench.model_shapes)
the forward and the backward sweep are timed in both forms IN THE SAME PROCESS: the one launch (qd_multi_nearest_f32 /
qd_multi_point_grad_f32) and the loop over nonUniformQuantization_variable.forward / .backward, one call per tensor (code this
path does not touch).  HIP events on the launch stream around a few back-to-back calls; the four timings are taken in turn,
`reps` times over (interleaved, so a drift of the clocks or a neighbour on the host hits all four), and the median, min and
max repetition are recorded.  The floor: the one-launch form is not slower than the loop (medians; where the min-max ranges
overlap the record says so).

Every configuration runs in a child process of its own under a time limit; the first one that fails ends the run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

CONFIGS = [(256, 16), (None, 16), (100, 16), (256, 128), (256, 256)]      # (256, 16): the tuned baseline
TUNED = {(256, 16), (None, 16)}                                            # (None, 16): forward only
CHILD_LIMIT_S = 300


def measure(bucket, k, reps):
    import numpy as np
    import torch
    import quantization
    from harness import kernel_bench
    from quantized_distillation_amd.multi_tensor import MultiTensorDiffQuant
    dev = torch.device('cuda:0')
    sizes = [int(np.prod(s)) for s in kernel_bench.model_shapes('wrn')]
    gen = torch.Generator(device=dev).manual_seed(0)
    ws = [torch.randn(n, device=dev, generator=gen) for n in sizes]
    grads = [torch.randn(n, device=dev, generator=gen) for n in sizes]
    outs = [torch.empty(n, device=dev) for n in sizes]
    pts = torch.sort(torch.rand(len(sizes), k, device=dev, generator=gen), dim=1)[0]
    rows = [pts[i].contiguous() for i in range(len(sizes))]
    mt = MultiTensorDiffQuant(ws, outs, grads, k, bucket)
    fns = [quantization.nonUniformQuantization_variable(bucket_size=bucket, pre_process_tensors=True, tensor=w) for w in ws]
    gp = torch.empty(len(sizes), k, device=dev)

    def loop_forward():
        for fn, p in zip(fns, rows):
            fn.forward(None, p)

    def loop_backward():
        for fn, g in zip(fns, grads):
            fn.backward(g)

    forms = [('one_launch_forward', lambda: mt.forward(pts), 10), ('loop_forward', loop_forward, 3),
             ('one_launch_backward', lambda: mt.backward(out=gp), 10), ('loop_backward', loop_backward, 3)]
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
    rec = {'bucket_size': bucket, 'points': k, 'tensors': len(sizes), 'elements': sum(sizes), 'reps': reps,
           'tuned': 'yes' if (bucket, k) == (256, 16) else 'forward only' if (bucket, k) in TUNED else 'functional, not tuned',
           'device': torch.cuda.get_device_name(0), 'us': {}}
    for name, s in samples.items():
        rec['us'][name] = {'median': round(statistics.median(s), 2), 'min': round(min(s), 2), 'max': round(max(s), 2)}
    for sweep in ('forward', 'backward'):
        one, loop = rec['us']['one_launch_' + sweep], rec['us']['loop_' + sweep]
        rec[sweep] = {'loop_over_one_launch': round(loop['median'] / one['median'], 2),
                      'not_slower_than_the_loop': one['median'] <= loop['median'],
                      'ranges_overlap': one['max'] >= loop['min'] and loop['max'] >= one['min']}
    # bytes the sweep has to move: forward u in, q + index out; backward gradient + index in
    rec['forward']['one_launch_gbps'] = round(sum(sizes) * 9 / rec['us']['one_launch_forward']['median'] / 1e3, 1)
    rec['backward']['one_launch_gbps'] = round(sum(sizes) * 5 / rec['us']['one_launch_backward']['median'] / 1e3, 1)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'multi_dq_geometry.json'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--config', help='(child) bucket,k -- bucket 0 = None')
    args = ap.parse_args()
    if args.reps < 5:
        ap.error('--reps: at least 5')
    if args.config:
        b, k = (int(v) for v in args.config.split(','))
        print('RESULT ' + json.dumps(measure(b or None, k, args.reps)))
        return 0
    results = []
    for bucket, k in CONFIGS:
        cmd = [sys.executable, os.path.abspath(__file__), '--reps', str(args.reps), '--config', '%d,%d' % (bucket or 0, k)]
        try:
            r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            print('configuration %r ran into its %d s limit: stopping' % ((bucket, k), CHILD_LIMIT_S))
            return 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
        if r.returncode != 0 or not line:
            print(r.stdout[-4000:])
            print('configuration %r failed (rc %d): stopping' % ((bucket, k), r.returncode))
            return 1
        results.append(json.loads(line[0][7:]))
        print(json.dumps(results[-1]), flush=True)
    base = next(r for r in results if (r['bucket_size'], r['points']) == (256, 16))
    flat = next(r for r in results if (r['bucket_size'], r['points']) == (None, 16))
    record = {'what': 'tools/bench_multi_dq.py: WRN-16-22 shape list, HIP events, median of %d interleaved repetitions, microseconds per '
                      'sweep over all tensors' % args.reps,
              'configurations': results,
              'forward_none_over_256_at_16_points': round(flat['us']['one_launch_forward']['median'] /
                                                          base['us']['one_launch_forward']['median'], 3),
              'floor_holds': all(r[s]['not_slower_than_the_loop'] for r in results for s in ('forward', 'backward'))}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    print('forward, no buckets / bucket 256 at 16 points: %.3f; floor holds: %s' % (record['forward_none_over_256_at_16_points'],
                                                                                   record['floor_holds']))
    return 0 if record['floor_holds'] else 1


if __name__ == '__main__':
    sys.exit(main())
