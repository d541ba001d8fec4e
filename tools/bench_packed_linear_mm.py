#!/usr/bin/env python3
"""The batched Linear layer from packed weights (qdm_linear_packed_f32, libqd_infer_mm.so: fp32 MFMA) next to the decode-time
entry point on the same call (qdi_linear_packed_f32, libqd_infer.so) and to torch on the unpacked fp32 weights.

    python tools/bench_packed_linear_mm.py [--out profiles/packed_linear_mm.json] [--error-out profiles/packed_linear_mm_error.txt]

The method of tools/bench_packed_layers.py (its timed() and Rotating are used as they are): W [4096, 4096] and [32768, 512],
bucket 256, s = 2^b at 2 / 4 / 8 bits, m = 8 ... 256 rows of x; HIP events around `iters` back-to-back calls, every call on the
next of `copies` copies of its weight, median [min .. max] of `reps` interleaved repetitions in ONE process, microseconds per
call.  Before anything is timed every result of either library is held to the float64 product at the timed size
(|y - y64| <= 1e-6 sum |terms|); the worst ratio seen is part of the record.
ONE gate (exit status 1): at m = 64, on both shapes and at every width, the new call's median lies below the existing entry
point's and the two ranges do not overlap.  The ratio to torch and the smallest m at which the new call wins are reported."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from bench_packed_layers import BUCKET, Rotating, timed  # noqa: E402

SHAPES = ((4096, 4096), (32768, 512))
MS = (8, 16, 32, 64, 128, 256)
GATE_M = 64


def measure(reps, widths, copies, iters):
    import torch
    import torch.nn.functional as F
    from quantized_distillation_amd import _infer, _infer_mm, _lib, codec
    dev = torch.device('cuda:0')
    old, new = _infer.load().qdi_linear_packed_f32, _infer_mm.load().qdm_linear_packed_f32
    st = _lib.stream_ptr(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    forms, keys, keep, errors = [], [], [], {}
    for rows, cols in SHAPES:
        W = torch.randn(rows, cols, device=dev, generator=gen) * 0.05
        for b in widths:
            s = 1 << b
            pks = [codec.pack_uniform(W, s, BUCKET, b) for _ in range(copies)]
            ws = [pk.unpack() for pk in pks]                               # the fp32 baseline reads the same values
            keep += [pks, ws]
            for m in MS:
                x = torch.randn(m, cols, device=dev, generator=gen)
                y = torch.empty(m, rows, device=dev)
                keep += [x, y]

                def packed_call(i, fn, pks=pks, rows=rows, cols=cols, s=s, b=b, x=x, m=m, y=y):
                    pk = pks[i]
                    return fn(pk.packed.data_ptr(), pk.alpha.data_ptr(), pk.beta.data_ptr(), rows, cols, BUCKET, s, b, x.data_ptr(), m, None,
                              y.data_ptr(), st)

                key = 'linear %dx%d bits %d m %d' % (rows, cols, b, m)
                y64 = x.double() @ ws[0].double().T
                mag = x.double().abs() @ ws[0].double().abs().T
                for name, fn in (('mm', new), ('rowwise', old)):
                    y.fill_(float('nan'))
                    if packed_call(0, fn) != 0:
                        raise SystemExit('%s: the %s call was refused' % (key, name))
                    ratio = float(((y.double() - y64).abs() / mag).max())
                    if not ratio <= 1e-6:
                        raise SystemExit('%s %s: |y - y64| / sum|terms| = %.3g > 1e-6: not timing a wrong result' % (key, name, ratio))
                    errors[key + ' ' + name] = ratio
                del y64, mag
                keys.append((key, rows, cols, b, m))
                forms += [(key + ' mm', Rotating(lambda i, c=packed_call: c(i, new), copies), iters),
                          (key + ' rowwise', Rotating(lambda i, c=packed_call: c(i, old), copies), iters),
                          (key + ' torch', Rotating(lambda i, ws=ws, x=x: F.linear(x, ws[i]), copies), iters)]
    torch.cuda.synchronize()
    us = timed(forms, reps)
    table, gate, wins_from = {}, [], {}
    for key, rows, cols, b, m in keys:
        n, r, t = us[key + ' mm'], us[key + ' rowwise'], us[key + ' torch']
        wins = n['median'] < r['median'] and n['max'] < r['min']
        table[key] = {'mm_us': n, 'rowwise_us': r, 'torch_fp32_us': t, 'rowwise_over_mm': round(r['median'] / n['median'], 2),
                      'torch_over_mm': round(t['median'] / n['median'], 2), 'mm_wins_ranges_apart': wins,
                      'mm_TFLOPs': round(2.0 * m * rows * cols / n['median'] / 1e6, 2)}
        if m == GATE_M and not wins:
            gate.append(key)
        if not wins:
            wins_from['%dx%d bits %d' % (rows, cols, b)] = None            # a later loss: the run of wins starts again
        elif wins_from.get('%dx%d bits %d' % (rows, cols, b)) is None:
            wins_from['%dx%d bits %d' % (rows, cols, b)] = m
    return {'what': 'tools/bench_packed_linear_mm.py: qdm_linear_packed_f32 (mm: fp32 MFMA, libqd_infer_mm.so) against qdi_linear_packed_f32 '
                    '(rowwise: libqd_infer.so) on the same call and torch.nn.functional.linear on the unpacked fp32 weights; bucket %d, '
                    's = 2^b; HIP events around %d back-to-back calls (wall, launch overhead included), each call on the next of %d copies '
                    'of its weight, median / min / max of %d interleaved repetitions in one process, microseconds per call' % (BUCKET, iters, copies, reps),
            'device': torch.cuda.get_device_name(0), 'reps': reps, 'copies': copies, 'iters': iters,
            'gate': 'at m = %d the mm median is below the rowwise median and the ranges do not overlap' % GATE_M, 'gate_failures': gate,
            'smallest_m_from_which_mm_wins': wins_from,
            'worst_error_over_sum_abs_terms': {'mm': max(v for k, v in errors.items() if k.endswith(' mm')),
                                               'rowwise': max(v for k, v in errors.items() if k.endswith(' rowwise'))},
            'error_over_sum_abs_terms': errors, 'rows': table}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'packed_linear_mm.json'))
    ap.add_argument('--error-out', default=os.path.join(ROOT, 'profiles', 'packed_linear_mm_error.txt'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--bits', default='2,4,8')
    ap.add_argument('--copies', type=int, default=6)
    ap.add_argument('--iters', type=int, default=24)
    args = ap.parse_args()
    if args.reps < 5 or args.copies < 1 or args.iters < 1:
        ap.error('--reps: at least 5; --copies, --iters: at least 1')
    record = measure(args.reps, [int(b) for b in args.bits.split(',')], args.copies, args.iters)
    for path in (args.out, args.error_out):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    with open(args.error_out, 'w') as f:
        f.write('error / sum|terms| against the float64 product, at the timed sizes (tools/bench_packed_linear_mm.py); bound 1e-6\n')
        f.write('worst: mm %.3g  rowwise %.3g\n' % (record['worst_error_over_sum_abs_terms']['mm'], record['worst_error_over_sum_abs_terms']['rowwise']))
        for k, v in record['error_over_sum_abs_terms'].items():
            f.write('%-48s %.3g\n' % (k, v))
    for key, r in record['rows'].items():
        print('%-34s mm %8.2f [%.2f .. %.2f]  rowwise %8.2f [%.2f .. %.2f]  torch %8.2f [%.2f .. %.2f]  rowwise / mm %.2f  torch / mm %.2f  %.2f TFLOP/s'
              % (key, r['mm_us']['median'], r['mm_us']['min'], r['mm_us']['max'], r['rowwise_us']['median'], r['rowwise_us']['min'],
                 r['rowwise_us']['max'], r['torch_fp32_us']['median'], r['torch_fp32_us']['min'], r['torch_fp32_us']['max'],
                 r['rowwise_over_mm'], r['torch_over_mm'], r['mm_TFLOPs']))
    print('smallest m from which mm wins:', record['smallest_m_from_which_mm_wins'])
    if record['gate_failures']:
        print('GATE FAILED at:', record['gate_failures'])
        return 1
    print('gate passed: mm below rowwise at m = %d everywhere, ranges apart' % GATE_M)
    return 0


if __name__ == '__main__':
    sys.exit(main())
