#!/usr/bin/env python3
"""Stochastic-rounding quantization of a whole model: the per-tensor loop against the one-launch MultiTensorQuantizer, on the 60
WRN-16-22 parameter tensors (harness/kernel_bench.model_shapes('wrn'), 82.7 M weights), 16 levels, bucket 256, out of place.
Not part of bench.py.

    timeout -k 10 900 python tools/bench_multi_stochastic.py --out profiles/multi_stochastic_wrn16_22.json [--no-steps]

Four figures from ONE process, HIP events around CALLS_PER_BATCH consecutive calls, the forms alternating batch by batch on
rotating buffer sets (no set is still in the 256 MiB last-level cache when it comes round again):
    (a) loop            uniformQuantization(t, 16, bucket_size=256, stochastic_rounding=True) per tensor -- code this commit does
                        not touch, so it is also the parent commit's figure
    (b) one_launch      MultiTensorQuantizer(stochastic_rounding=True).quantize(), seed by value and seed in device memory
                        (the latter includes the add_ that advances the seed word)
    (c) deterministic   the existing one-launch call (qd_multi_uniform_f32)
    (d) k1s             ONE tensor of the same total size through uniformQuantization(stochastic_rounding=True)
Rates are 8 B per element (read fp32, write fp32) over wall time, against the 8 TB/s HBM peak: wall time of back-to-back
launches, so launch gaps count; not a kernel-only share.  Then steps/s of DistillTrainer(stochastic_rounding=True) on the CIFAR
student, mode 'multi' against 'per_tensor', eager and (multi only: the loop's seed is a launch argument) captured."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import quantization  # noqa: E402
from harness import kernel_bench, models  # noqa: E402
from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
BYTES_PER_ELEM = 8
BUCKET, LEVELS = 256, 16
SETS = 3                            # rotating (masters, shadows) sets of 2 x 331 MB
CALLS_PER_BATCH, BATCHES, WARMUP_BATCHES = 10, 12, 3       # 120 timed calls per form


def spread(samples):
    s = sorted(samples)
    return {'median': statistics.median(s), 'min': s[0], 'max': s[-1], 'n': len(s)}


def timed_batch(fn, i0):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(CALLS_PER_BATCH):
        fn(i0 + i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / CALLS_PER_BATCH        # us per call


def quantize_forms(dev):
    from harness.flat import FlatLayout
    layout = FlatLayout(kernel_bench.model_shapes('wrn'))
    n = layout.total
    gen = torch.Generator(device=dev).manual_seed(0)
    masters, shadows = [], []
    for _ in range(SETS):
        masters.append(torch.randn(n, device=dev, generator=gen) * 0.05)
        shadows.append(torch.empty(n, device=dev))
    xs = [layout.views(m) for m in masters]
    qs = [layout.views(s) for s in shadows]
    by_value = [MultiTensorQuantizer(x, LEVELS, BUCKET, outputs=q, stochastic_rounding=True) for x, q in zip(xs, qs)]
    on_device = [MultiTensorQuantizer(x, LEVELS, BUCKET, outputs=q, stochastic_rounding=True, seed_on_device=True) for x, q in zip(xs, qs)]
    plain = [MultiTensorQuantizer(x, LEVELS, BUCKET, outputs=q) for x, q in zip(xs, qs)]
    keep = [None]

    def loop(i):
        for x in xs[i % SETS]:
            keep[0] = quantization.uniformQuantization(x, LEVELS, bucket_size=BUCKET, stochastic_rounding=True)[0]

    def k1s(i):
        keep[0] = quantization.uniformQuantization(masters[i % SETS], LEVELS, bucket_size=BUCKET, stochastic_rounding=True)[0]

    forms = [('a_loop_per_tensor_stochastic', loop),
             ('b_one_launch_stochastic_seed_by_value', lambda i: by_value[i % SETS].quantize(check_pointers=False)),
             ('b_one_launch_stochastic_seed_on_device', lambda i: on_device[i % SETS].quantize(check_pointers=False)),
             ('c_one_launch_deterministic', lambda i: plain[i % SETS].quantize(check_pointers=False)),
             ('d_k1s_one_tensor_stochastic', k1s)]
    # same bits first: a speed comparison of two different results is worthless
    from quantization import quant_functions as qf
    start = qf._STOCHASTIC_CALLS[0]
    want = [quantization.uniformQuantization(x, LEVELS, bucket_size=BUCKET, stochastic_rounding=True)[0] for x in xs[0]]
    qf._STOCHASTIC_CALLS[0] = start
    got = by_value[0].quantize()
    same = all(torch.equal(a.view(-1).view(torch.int32), b.view(-1).view(torch.int32)) for a, b in zip(want, got))
    del want
    times = {name: [] for name, _fn in forms}
    i = 0
    for b in range(WARMUP_BATCHES + BATCHES):                  # alternating: every form sees the same clocks and neighbours
        for name, fn in forms:
            t = timed_batch(fn, i)
            i += CALLS_PER_BATCH
            if b >= WARMUP_BATCHES:
                times[name].append(t)
    floor_us = BYTES_PER_ELEM * n / HBM_BYTES_PER_S * 1e6
    rec = {'tensors': len(xs[0]), 'elements': n, 'bucket': BUCKET, 'levels': LEVELS, 'in_place': False,
           'one_launch_equals_loop_bitwise': bool(same),
           'timing': 'HIP events around %d consecutive calls, %d batches per form after %d warm-up batches, the forms alternating, %d '
                     'rotating buffer sets of %.0f MB' % (CALLS_PER_BATCH, BATCHES, WARMUP_BATCHES, SETS, 8e-6 * n),
           'hbm_floor_us (8 B/element at 8 TB/s)': floor_us, 'wall_us_per_model': {}, 'wall_fraction_of_hbm_peak': {}}
    for name, _fn in forms:
        rec['wall_us_per_model'][name] = spread(times[name])
        rec['wall_fraction_of_hbm_peak'][name] = floor_us / statistics.median(times[name])
    med = {k: v['median'] for k, v in rec['wall_us_per_model'].items()}
    rec['one_launch_faster_than_loop_by_more_than_the_spread'] = bool(
        max(times['b_one_launch_stochastic_seed_by_value'] + times['b_one_launch_stochastic_seed_on_device']) < min(times['a_loop_per_tensor_stochastic']))
    rec['b_rate_over_d_rate'] = {'seed_by_value': med['d_k1s_one_tensor_stochastic'] / med['b_one_launch_stochastic_seed_by_value'],
                                 'seed_on_device': med['d_k1s_one_tensor_stochastic'] / med['b_one_launch_stochastic_seed_on_device']}
    rec['b_rate_over_c_rate'] = med['c_one_launch_deterministic'] / med['b_one_launch_stochastic_seed_by_value']
    return rec


def steps_per_sec(dev):
    from harness.distill import DistillTrainer, synthetic_batch
    out = {}
    batch, warmup, steps, reps = 64, 10, 100, 5
    for name, mode, captured in (('multi_eager', 'multi', False), ('per_tensor_eager', 'per_tensor', False), ('multi_captured', 'multi', True)):
        torch.manual_seed(0)
        tr = DistillTrainer(models.student(), models.teacher(), dev, num_bits=4, bucket_size=BUCKET, mode=mode, stochastic_rounding=True)
        batches = [synthetic_batch(batch, dev, seed=i) for i in range(2)]
        if captured:
            tr.capture(*batches[0])
        step = lambda i: tr.step(*batches[i % 2])               # (after capture(): the graphs' replay)  # noqa: E731
        for i in range(warmup):
            step(i)
        torch.cuda.synchronize()
        rates = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                step(i)
            torch.cuda.synchronize()
            rates.append(steps / (time.perf_counter() - t0))
        out[name] = {'batch': batch, 'steps_per_rep': steps, 'steps_per_sec': spread(rates), 'tensors': len(tr.params),
                     'captured': tr._graph_fb is not None, 'final_loss_finite': bool(torch.isfinite(step(0)))}
        del tr
        torch.cuda.empty_cache()
    return out


def main():
    out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    dev = torch.device('cuda:0')
    rec = {'model': 'WRN-16-22 parameter list', 'device': torch.cuda.get_device_name(0)}
    rec.update(quantize_forms(dev))
    print(json.dumps(rec))
    if '--no-steps' not in sys.argv:
        torch.cuda.empty_cache()
        rec['cifar_student_trainer_stochastic_rounding'] = steps_per_sec(dev)
        print(json.dumps(rec['cifar_student_trainer_stochastic_rounding']))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'w') as fh:
            json.dump(rec, fh, indent=1)
        print('wrote', out_path)


if __name__ == '__main__':
    main()
