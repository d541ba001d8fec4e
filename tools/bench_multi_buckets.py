#!/usr/bin/env python3
"""One launch with a bucket size per tensor (MultiTensorQuantizer / MultiTensorSTE with a sequence bucket_size) against the
per-tensor loop at the same bucket sizes, and -- at equal entries -- against the scalar-bucket one launch.

    python tools/bench_multi_buckets.py [--out profiles/multi_buckets_wrn16_22.json] [--reps 7]

The 60 WRN-16-22 parameter tensors (harness.kernel_bench.model_shapes), s = 16.  Two questions, the quantizer and the
bucket-aware STE backward each:
    per_channel   bucket_size = per_channel_bucket_sizes(tensors): one scale pair per output channel, one bucket for a bias or
                  a batch-norm vector.
                  (a) one_launch   qd_multi_uniform_buckets_f32 / qd_multi_ste_backward_buckets_f32
                  (b) loop         uniformQuantization(t_i, 16, bucket_size=b_i) / ste_bucket_backward(w_i, g_i, b_i, 16) per
                                   tensor: the code a user has without this entry point
    equal_256     bucket_size = [256] * 60 through the new entry point against bucket_size = 256 through the existing one: the
                  same bytes, the same tiles -- the price of choosing the register body at run time.
                  (a) one_launch   the sequence   (c) scalar_one_launch   the scalar
All in ONE process: HIP events on the launch stream around a few back-to-back calls (wall time of the calls, launch overhead
included: that is what the one launch removes), the rows taken in turn `reps` times over (interleaved: clock drift and host
neighbours hit all of them), median / min / max of the repetitions recorded.  The record says for per_channel whether the
one-launch median is below the loop's with disjoint min-max ranges, and gives every ratio; nothing is gated here.
"""
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
    a, other = us['one_launch'], [n for n in us if n != 'one_launch'][0]
    b = us[other]
    return {'us': us, '%s_over_one_launch' % other: round(b['median'] / a['median'], 3),
            'ranges_overlap': a['max'] >= b['min'] and b['max'] >= a['min'],
            'one_launch_below_with_disjoint_ranges': a['median'] < b['median'] and a['max'] < b['min']}


def measure(reps):
    import torch
    import quantization
    from harness import kernel_bench
    from quantized_distillation_amd import ste
    from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer, MultiTensorSTE, per_channel_bucket_sizes
    dev = torch.device('cuda:0')
    shapes = [tuple(int(d) for d in s) for s in kernel_bench.model_shapes('wrn')]
    gen = torch.Generator(device=dev).manual_seed(0)
    ws = [torch.randn(s, device=dev, generator=gen) * 0.05 for s in shapes]
    grads = [torch.randn(s, device=dev, generator=gen) for s in shapes]
    outs = [torch.empty(s, device=dev) for s in shapes]
    per_channel = per_channel_bucket_sizes(ws)
    groups = {}

    one = MultiTensorQuantizer(ws, 16, per_channel, outputs=outs)

    def loop_q():
        for w, b in zip(ws, per_channel):
            quantization.uniformQuantization(w, 16, bucket_size=b)
    groups['quantize_per_channel'] = timed([('one_launch', lambda: one.quantize(check_pointers=False), 10), ('loop', loop_q, 3)], reps)
    groups['quantize_per_channel']['entry_points'] = [one.entry_point]

    one_ste = MultiTensorSTE(ws, grads, 16, per_channel, outs=outs)

    def loop_ste():
        for w, g, o, b in zip(ws, grads, outs, per_channel):
            ste.ste_bucket_backward(w, g, b, 16, out=o)
    groups['ste_per_channel'] = timed([('one_launch', lambda: one_ste.backward(check_pointers=False), 10), ('loop', loop_ste, 3)], reps)
    groups['ste_per_channel']['entry_points'] = [one_ste.entry_point]

    seq, scalar = MultiTensorQuantizer(ws, 16, [256] * len(ws), outputs=outs), MultiTensorQuantizer(ws, 16, 256, outputs=outs)
    groups['quantize_equal_256'] = timed([('one_launch', lambda: seq.quantize(check_pointers=False), 10),
                                          ('scalar_one_launch', lambda: scalar.quantize(check_pointers=False), 10)], reps)
    groups['quantize_equal_256']['entry_points'] = [seq.entry_point, scalar.entry_point]
    seq_ste, scalar_ste = MultiTensorSTE(ws, grads, 16, [256] * len(ws), outs=outs), MultiTensorSTE(ws, grads, 16, 256, outs=outs)
    groups['ste_equal_256'] = timed([('one_launch', lambda: seq_ste.backward(check_pointers=False), 10),
                                     ('scalar_one_launch', lambda: scalar_ste.backward(check_pointers=False), 10)], reps)
    groups['ste_equal_256']['entry_points'] = [seq_ste.entry_point, scalar_ste.entry_point]
    return {'what': 'tools/bench_multi_buckets.py: 60 WRN-16-22 tensors, s = 16; per_channel: bucket_size = elements per output channel '
                    '(the whole tensor for vectors); equal_256: [256] * 60 against the scalar 256; HIP events around back-to-back calls '
                    '(wall, launch overhead included), median / min / max of %d interleaved repetitions in one process, microseconds '
                    'per sweep over all tensors' % reps,
            'device': torch.cuda.get_device_name(0), 'tensors': len(shapes), 'elements': sum(w.numel() for w in ws),
            'per_channel_bucket_sizes': per_channel, 'reps': reps, 'groups': groups}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'multi_buckets_wrn16_22.json'))
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
        print('%-22s %s' % (name, '   '.join('%s %.2f us [%.2f .. %.2f]' % (k, v['median'], v['min'], v['max']) for k, v in g['us'].items())))
        print('%-22s %s' % ('', '   '.join('%s: %s' % (k, v) for k, v in g.items() if k not in ('us', 'entry_points'))))
    return 0


if __name__ == '__main__':
    sys.exit(main())
