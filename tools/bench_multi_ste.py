#!/usr/bin/env python3
"""The bucket-aware STE backward (K7) of a whole model: the per-tensor loop against one MultiTensorSTE launch, on the WRN-16-22
parameter list (harness/models.py: 60 tensors, 82.7 M weights), bucket 256, 16 levels, in place.  Not part of bench.py.

    timeout -k 10 900 python tools/bench_multi_ste.py --steps-only --out STEPS.json
        steps/s of DistillTrainer(mode='multi', backprop_quantization_style='complicated') on the CIFAR student and on WRN-16-22.
        Uses the trainer only, so the same file runs in a checkout of the PARENT commit (there the trainer still loops).
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ste -- python tools/bench_multi_ste.py --trace
        a run of its own for the kernel-only times: TRACE_REPS times the loop, then TRACE_REPS times the one launch.
    timeout -k 10 900 python tools/bench_multi_ste.py --kernel-stats DIR --parent-steps STEPS.json --out profiles/multi_ste_wrn16_22.json
        wall time by HIP events of (a) the loop and (b) the one launch, alternating batches on rotating buffer sets, the trainer's
        steps/s at this commit, plus what the two files above hold; one JSON record.
"""
import csv
import glob
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from harness import models  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
BYTES_PER_ELEM = 12                 # read x, read g, write out
BUCKET, LEVELS = 256, 16
SETS = 3                            # rotating (x, g) sets of 2 x 331 MB each: no set is still in the 256 MiB last-level cache when reused
CALLS_PER_BATCH, BATCHES, WARMUP_BATCHES = 10, 15, 3
TRACE_REPS = 10


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def spread(samples):
    s = sorted(samples)
    return {'median': statistics.median(s), 'min': s[0], 'max': s[-1], 'n': len(s)}


def wrn_sets(dev):
    """SETS x (list of weight tensors, list of gradient tensors) with the WRN-16-22 shapes, each list views of one flat buffer
    (the trainer's layout)."""
    from harness.flat import FlatLayout
    with torch.device('meta'):
        shapes = [tuple(p.shape) for p in models.WideResNet(16, 22).parameters()]
    layout = FlatLayout(shapes)
    gen = torch.Generator(device=dev).manual_seed(0)
    sets = []
    for _ in range(SETS):
        fx = torch.randn(layout.total, device=dev, generator=gen) * 0.05
        fg = torch.randn(layout.total, device=dev, generator=gen) * 1e-3
        sets.append((layout.views(fx), layout.views(fg)))
    return sets, sum(int(torch.Size(s).numel()) for s in shapes)


def make_calls(sets):
    from quantized_distillation_amd import ste
    from quantized_distillation_amd.multi_tensor import MultiTensorSTE
    multis = [MultiTensorSTE(xs, gs, LEVELS, BUCKET) for xs, gs in sets]

    def loop(i):                                           # harness/distill.py's backward_quant() before the one-launch path
        xs, gs = sets[i % SETS]
        for x, g in zip(xs, gs):
            ste.ste_bucket_backward(x, g, BUCKET, LEVELS, out=g)

    def one(i):
        multis[i % SETS].backward(check_pointers=False)

    return loop, one


def timed_batch(fn, i0):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(CALLS_PER_BATCH):
        fn(i0 + i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / CALLS_PER_BATCH        # us per call


def wall(dev):
    sets, n = wrn_sets(dev)
    loop, one = make_calls(sets)
    # same bits first: a speed comparison of two different results is worthless
    xs, gs = sets[0]
    a = [g.clone() for g in gs]
    for x, g in zip(xs, a):
        from quantized_distillation_amd import ste
        ste.ste_bucket_backward(x, g, BUCKET, LEVELS, out=g)
    keep = [g.clone() for g in gs]
    one(0)
    same = all(torch.equal(p.view(-1).view(torch.int32), q.view(-1).view(torch.int32)) for p, q in zip(a, gs))
    for g, k in zip(gs, keep):
        g.copy_(k)
    ta, tb, i = [], [], 0
    for b in range(WARMUP_BATCHES + BATCHES):                  # alternating: both see the same clocks and neighbours
        for fn, acc in ((loop, ta), (one, tb)):
            t = timed_batch(fn, i)
            i += CALLS_PER_BATCH
            if b >= WARMUP_BATCHES:
                acc.append(t)
    return {'tensors': len(xs), 'elements': n, 'bucket': BUCKET, 'levels': LEVELS, 'in_place': True,
            'one_launch_equals_loop_bitwise': bool(same),
            'timing': 'HIP events around %d consecutive calls, %d batches each after %d warm-up batches, the two forms alternating, '
                      '%d rotating buffer sets of %.0f MB' % (CALLS_PER_BATCH, BATCHES, WARMUP_BATCHES, SETS, 8e-6 * n),
            'wall_us_per_model_loop': spread(ta), 'wall_us_per_model_one_launch': spread(tb),
            'wall_difference_us_median': statistics.median(ta) - statistics.median(tb),
            'one_launch_below_loop_by_more_than_the_spread': bool(max(tb) < min(ta))}


def trace(dev):
    sets, _n = wrn_sets(dev)
    loop, one = make_calls(sets)
    for i in range(3):
        loop(i); one(i)
    torch.cuda.synchronize()
    for i in range(TRACE_REPS):
        loop(i)
    torch.cuda.synchronize()
    for i in range(TRACE_REPS):
        one(i)
    torch.cuda.synchronize()
    print(json.dumps({'trace_reps': TRACE_REPS, 'warmup_reps': 3}))


def kernel_stats(stats_dir, n):
    """Per-model kernel time of both forms from rocprofv3's kernel trace of a --trace run (3 warm-up + TRACE_REPS calls each)."""
    per = {}
    for f in glob.glob(os.path.join(stats_dir, '**', '*kernel_trace.csv'), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name = row.get('Kernel_Name', '')
                if 'k_ste_backward' in name or 'k_multi_ste' in name:
                    key = 'one_launch' if 'k_multi_ste' in name else 'loop'
                    per.setdefault(key, []).append((int(row['Start_Timestamp']), int(row['End_Timestamp']) - int(row['Start_Timestamp']), name))
    if not per.get('loop') or not per.get('one_launch'):
        return {'error': 'no kernel trace of both forms under %s' % stats_dir}
    calls = 3 + TRACE_REPS
    out = {'source': 'rocprofv3 --kernel-trace --stats, a run of its own (bench_multi_ste.py --trace): %d calls of each form, the first 3 '
                     'not counted' % calls}
    for key, rows in per.items():
        rows.sort()
        per_call = len(rows) // calls
        assert per_call * calls == len(rows), (key, len(rows))
        timed = rows[3 * per_call:]
        sums = [sum(d for _s, d, _n in timed[c * per_call:(c + 1) * per_call]) * 1e-3 for c in range(TRACE_REPS)]
        out[key] = {'kernels_of_this_library_per_call': per_call, 'kernel_us_per_model': spread(sums),
                    'kernel_names': sorted(set(re.search(r'k_\w+(<[^>]*>)?', nm).group(0) for _s, _d, nm in timed))}
    floor_us = BYTES_PER_ELEM * n / HBM_BYTES_PER_S * 1e6
    out['hbm_floor_us (12 B/element at 8 TB/s)'] = floor_us
    out['one_launch_fraction_of_hbm_peak'] = floor_us / out['one_launch']['kernel_us_per_model']['median']
    out['loop_fraction_of_hbm_peak (sum of its kernels)'] = floor_us / out['loop']['kernel_us_per_model']['median']
    return out


def steps_per_sec(dev):
    from harness.distill import DistillTrainer, synthetic_batch
    out = {}
    for name, student, batch, warmup, steps, reps in (('cifar_student', models.student, 64, 10, 100, 5),
                                                      ('wrn_16_22', lambda: models.WideResNet(16, 22), 32, 4, 10, 3)):
        torch.manual_seed(0)
        tr = DistillTrainer(student(), models.teacher(), dev, num_bits=4, bucket_size=BUCKET, mode='multi',
                            backprop_quantization_style='complicated')
        batches = [synthetic_batch(batch, dev, seed=i) for i in range(2)]
        t0 = time.perf_counter()
        for i in range(warmup):
            tr.step(*batches[i % 2])
        torch.cuda.synchronize()
        warm = time.perf_counter() - t0
        rates = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                tr.step(*batches[i % 2])
            torch.cuda.synchronize()
            rates.append(steps / (time.perf_counter() - t0))
        out[name] = {'batch': batch, 'steps_per_rep': steps, 'steps_per_sec': spread(rates), 'warmup_s': round(warm, 1),
                     'one_launch_ste': hasattr(tr, 'mt_ste'), 'tensors': len(tr.params), 'final_loss_finite': bool(torch.isfinite(tr.step(*batches[0])))}
        del tr
        torch.cuda.empty_cache()
    return out


def main():
    dev = torch.device('cuda:0')
    out_path = arg('--out')
    if '--trace' in sys.argv:
        return trace(dev)
    if '--steps-only' in sys.argv:
        rec = {'trainer': "DistillTrainer(mode='multi', backprop_quantization_style='complicated'), eager, one GPU", 'configs': steps_per_sec(dev)}
    else:
        rec = {'model': 'WRN-16-22', 'device': torch.cuda.get_device_name(0)}
        rec.update(wall(dev))
        if arg('--kernel-stats'):
            rec['kernel_only'] = kernel_stats(arg('--kernel-stats'), rec['elements'])
        rec['trainer_steps_per_sec_this_commit'] = steps_per_sec(dev)
        if arg('--parent-steps'):
            with open(arg('--parent-steps')) as fh:
                rec['trainer_steps_per_sec_parent_commit (same lease, the run before this one)'] = json.load(fh)['configs']
    print(json.dumps(rec))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'w') as fh:
            json.dump(rec, fh, indent=1)
        print('wrote', out_path)


if __name__ == '__main__':
    main()
