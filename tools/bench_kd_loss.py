#!/usr/bin/env python3
"""The distillation loss, forward + backward, from one call of libqd_loss.so (quantized_distillation_amd.kd_loss: qdl_kd_loss_f32, two
launches, and the multiply by the upstream gradient) next to what the harness runs by default -- harness.models.word_kd_loss /
models.kd_loss as chains of torch operations with autograd behind them.

    python tools/bench_kd_loss.py [--out profiles/kd_loss.json]

The method of tools/bench_packed_gen.py (timed() and Rotating of tools/bench_packed_layers.py are used as they are): HIP events around
`iters` back-to-back forward + backward passes, every pass on the next of `copies` copies of its logits, median [min .. max] of `reps`
interleaved repetitions in ONE process, microseconds per pass.  word_kd_loss at [3136, 10000] and [3136, 32768] (a tenth of the targets
padding, batch 64), kd_loss at [128, 10] and [256, 1000].  GB/s: 12 bytes per element -- student and teacher read, gradient written --
over the fused pass's time, the upstream multiply included in the time and not in the bytes.  Before anything is timed the fused loss
and gradient are held to the torch chain.  Nothing is gated on the times: the ratios are reported as they are."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from bench_packed_layers import Rotating, timed  # noqa: E402

WORD_SHAPES = ((3136, 10000), (3136, 32768))
KD_SHAPES = ((128, 10), (256, 1000))
BATCH, PAD = 64, 1


def measure(reps, copies, iters):
    import torch
    from harness import models
    from quantized_distillation_amd import kd_loss
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    forms, keys, keep = [], [], []

    def passes(loss_fn, students, teacher, target, **kw):
        def one(i):
            students[i].grad = None
            loss_fn(students[i], teacher, target, **kw).backward()
        return Rotating(one, copies)

    for word, shapes in ((True, WORD_SHAPES), (False, KD_SHAPES)):
        fused, plain, kw = (kd_loss.fused_word_kd_loss, models.word_kd_loss, dict(batch=BATCH)) if word else (kd_loss.fused_kd_loss, models.kd_loss, {})
        for rows, cols in shapes:
            students = [(torch.randn(rows, cols, device=dev) * 3.0).requires_grad_(True) for _ in range(copies)]
            teacher = torch.randn(rows, cols, device=dev) * 3.0
            target = torch.randint(0, cols, (rows,), device=dev)
            if word:
                target[torch.rand(rows, device=dev) < 0.1] = PAD
            keep += [students, teacher, target]
            got, want = fused(students[0], teacher, target, **kw), plain(students[0], teacher, target, **kw)
            (g_got,), (g_want,) = torch.autograd.grad(got, students[0]), torch.autograd.grad(want, students[0])
            err = abs(got.item() - want.item()) / (abs(want.item()) + 1.0), float((g_got - g_want).abs().max() / g_want.abs().max())
            if not (err[0] <= 1e-5 and err[1] <= 1e-4):
                raise SystemExit('[%d, %d]: the fused loss and the torch chain disagree (loss %.3g, gradient %.3g): not timing a wrong result' % (rows, cols, *err))
            key = '%s [%d, %d]' % (plain.__name__, rows, cols)
            keys.append((key, rows * cols))
            forms += [(key + ' fused', passes(fused, students, teacher, target, **kw), iters), (key + ' torch', passes(plain, students, teacher, target, **kw), iters)]
    torch.cuda.synchronize()
    us = timed(forms, reps)
    table = {}
    for key, n in keys:
        f, t = us[key + ' fused'], us[key + ' torch']
        table[key] = {'fused_us': f, 'torch_us': t, 'torch_over_fused': round(t['median'] / f['median'], 3), 'fused_gb_per_s_at_12_bytes_per_element': round(12.0 * n / f['median'] / 1e3, 1),
                      'verdict': 'ahead' if f['median'] < t['median'] else 'behind: functional, not tuned'}
    return {'what': 'tools/bench_kd_loss.py: forward + backward of the fused distillation loss (qdl_kd_loss_f32, libqd_loss.so, two launches, and grad * grad_output) against '
                    'harness.models.word_kd_loss / kd_loss as torch chains with autograd; HIP events around %d back-to-back passes (wall, launch and Python overhead included), '
                    'each on the next of %d copies of the student logits, median / min / max of %d interleaved repetitions in one process, microseconds per pass; GB/s = 12 bytes per '
                    'element over the fused median; nothing is gated' % (iters, copies, reps),
            'device': torch.cuda.get_device_name(0), 'reps': reps, 'copies': copies, 'iters': iters, 'rows': table}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kd_loss.json'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--copies', type=int, default=3)
    ap.add_argument('--iters', type=int, default=8)
    args = ap.parse_args()
    if args.reps < 5 or args.copies < 1 or args.iters < 1:
        ap.error('--reps: at least 5; --copies, --iters: at least 1')
    record = measure(args.reps, args.copies, args.iters)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    for key, r in record['rows'].items():
        print('%-32s fused %9.2f [%.2f .. %.2f]  torch %9.2f [%.2f .. %.2f]  torch / fused %.3f  %.1f GB/s  %s'
              % (key, r['fused_us']['median'], r['fused_us']['min'], r['fused_us']['max'], r['torch_us']['median'], r['torch_us']['min'], r['torch_us']['max'],
                 r['torch_over_fused'], r['fused_gb_per_s_at_12_bytes_per_element'], r['verdict']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
