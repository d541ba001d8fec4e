#!/usr/bin/env python3
"""nn.Conv2d from packed weights (qdc_conv2d_packed_f32, libqd_infer_conv.so: implicit GEMM on fp32 MFMA) next to the only way
to run that layer from packed weights without it -- qd_unpack_uniform_f32 (PackedUniform.unpack) followed by F.conv2d -- and to
F.conv2d alone on the unpacked fp32 weights.

    python tools/bench_packed_conv.py [--out profiles/packed_conv.json] [--error-out profiles/packed_conv_error.txt]

The method of tools/bench_packed_linear_mm.py (timed() and Rotating of tools/bench_packed_layers.py are used as they are): HIP
events around `iters` back-to-back calls, every call on the next of `copies` copies of its weight, median [min .. max] of
`reps` interleaved repetitions in ONE process, microseconds per call.  Shapes: three WideResNet-shaped layers at batch 128
(4 bits) and the 7 x 7 stride-2 stem at batch 32 (2 / 4 / 8 bits); bucket 256, s = 2^b.  Before anything is timed the first
two images of every result are held to the float64 product with the unfolded input (|y - y64| <= 1e-6 sum |terms|); the ratio
is part of the record.  Nothing is gated: the ratios are reported as they are."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from bench_packed_layers import BUCKET, Rotating, timed  # noqa: E402

# (name, cout, cin, k, stride, pad, batch, h = w, widths)
SHAPES = (('wrn 3x3', 160, 160, 3, 1, 1, 128, 32, (4,)), ('wrn 3x3 stride 2', 320, 160, 3, 2, 1, 128, 32, (4,)),
          ('wrn shortcut 1x1 stride 2', 320, 160, 1, 2, 0, 128, 32, (4,)), ('stem 7x7 stride 2', 64, 3, 7, 2, 3, 32, 224, (2, 4, 8)))


def measure(reps, copies, iters):
    import torch
    import torch.nn.functional as F
    from quantized_distillation_amd import _infer_conv, _lib, codec
    dev = torch.device('cuda:0')
    conv = _infer_conv.load().qdc_conv2d_packed_f32
    st = _lib.stream_ptr(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    forms, keys, keep, errors = [], [], [], {}
    for name, cout, cin, k, stride, pad, batch, hw, widths in SHAPES:
        W = torch.randn(cout, cin * k * k, device=dev, generator=gen) * 0.05
        x = torch.randn(batch, cin, hw, hw, device=dev, generator=gen)
        o = (hw + 2 * pad - k) // stride + 1
        y = torch.empty(batch, cout, o, o, device=dev)
        keep += [x, y]
        for b in widths:
            s = 1 << b
            pks = [codec.pack_uniform(W, s, BUCKET, b) for _ in range(copies)]
            ws = [pk.unpack().view(cout, cin, k, k) for pk in pks]         # the fp32 baseline reads the same values
            keep += [pks, ws]

            def packed_call(i, pks=pks, cout=cout, cin=cin, k=k, s=s, b=b, x=x, batch=batch, hw=hw, stride=stride, pad=pad, y=y):
                pk = pks[i]
                return conv(pk.packed.data_ptr(), pk.alpha.data_ptr(), pk.beta.data_ptr(), cout, cin, k, k, BUCKET, s, b, x.data_ptr(), batch,
                            hw, hw, stride, stride, pad, pad, None, y.data_ptr(), st)

            key = '%s [%d, %d, %d, %d] batch %d at %dx%d bits %d' % (name, cout, cin, k, k, batch, hw, hw, b)
            y.fill_(float('nan'))
            if packed_call(0) != 0:
                raise SystemExit('%s: the call was refused' % key)
            cols = F.unfold(x[:2].double(), k, padding=pad, stride=stride)                     # [2, K, o o]
            w64 = ws[0].reshape(cout, -1).double()
            y64, mag = w64 @ cols, w64.abs() @ cols.abs()
            ratio = float(((y[:2].reshape(2, cout, -1).double() - y64).abs() / mag).max())
            if not ratio <= 1e-6:
                raise SystemExit('%s: |y - y64| / sum|terms| = %.3g > 1e-6: not timing a wrong result' % (key, ratio))
            errors[key] = ratio
            del cols, y64, mag
            keys.append((key, 2.0 * batch * o * o * cout * cin * k * k))
            forms += [(key + ' packed', Rotating(packed_call, copies), iters),
                      (key + ' unpack+conv', Rotating(lambda i, pks=pks, x=x, sh=(cout, cin, k, k), stride=stride, pad=pad:
                                                       F.conv2d(x, pks[i].unpack().view(sh), None, stride, pad), copies), iters),
                      (key + ' torch', Rotating(lambda i, ws=ws, x=x, stride=stride, pad=pad: F.conv2d(x, ws[i], None, stride, pad), copies), iters)]
    torch.cuda.synchronize()
    us = timed(forms, reps)
    table = {}
    for key, flop in keys:
        p, u, t = us[key + ' packed'], us[key + ' unpack+conv'], us[key + ' torch']
        behind = p['median'] > u['median']
        table[key] = {'packed_us': p, 'unpack_then_conv2d_us': u, 'torch_fp32_us': t,
                      'unpack_then_conv2d_over_packed': round(u['median'] / p['median'], 3), 'torch_over_packed': round(t['median'] / p['median'], 3),
                      'packed_TFLOPs': round(flop / p['median'] / 1e6, 2), 'verdict': 'functional, not tuned' if behind else 'ahead of unpack + conv2d'}
    return {'what': 'tools/bench_packed_conv.py: qdc_conv2d_packed_f32 (packed: implicit GEMM on fp32 MFMA, libqd_infer_conv.so) against '
                    'PackedUniform.unpack() + torch.nn.functional.conv2d (MIOpen) and against conv2d alone on the unpacked fp32 weights; bucket %d, '
                    's = 2^b; HIP events around %d back-to-back calls (wall, launch overhead included), each call on the next of %d copies of its '
                    'weight, median / min / max of %d interleaved repetitions in one process, microseconds per call; nothing is gated'
                    % (BUCKET, iters, copies, reps),
            'device': torch.cuda.get_device_name(0), 'reps': reps, 'copies': copies, 'iters': iters,
            'worst_error_over_sum_abs_terms': max(errors.values()), 'error_over_sum_abs_terms': errors, 'rows': table}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'packed_conv.json'))
    ap.add_argument('--error-out', default=os.path.join(ROOT, 'profiles', 'packed_conv_error.txt'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--copies', type=int, default=3)
    ap.add_argument('--iters', type=int, default=6)
    args = ap.parse_args()
    if args.reps < 5 or args.copies < 1 or args.iters < 1:
        ap.error('--reps: at least 5; --copies, --iters: at least 1')
    record = measure(args.reps, args.copies, args.iters)
    for path in (args.out, args.error_out):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    with open(args.error_out, 'w') as f:
        f.write('error / sum|terms| against the float64 product on the first two images, at the timed sizes (tools/bench_packed_conv.py); bound 1e-6\n')
        f.write('worst: %.3g\n' % record['worst_error_over_sum_abs_terms'])
        for k, v in record['error_over_sum_abs_terms'].items():
            f.write('%-72s %.3g\n' % (k, v))
    for key, r in record['rows'].items():
        print('%-66s packed %9.2f [%.2f .. %.2f]  unpack + conv2d %9.2f [%.2f .. %.2f]  conv2d %9.2f [%.2f .. %.2f]  (unpack + conv2d) / packed %.3f  '
              'conv2d / packed %.3f  %.2f TFLOP/s  %s'
              % (key, r['packed_us']['median'], r['packed_us']['min'], r['packed_us']['max'], r['unpack_then_conv2d_us']['median'],
                 r['unpack_then_conv2d_us']['min'], r['unpack_then_conv2d_us']['max'], r['torch_fp32_us']['median'], r['torch_fp32_us']['min'],
                 r['torch_fp32_us']['max'], r['unpack_then_conv2d_over_packed'], r['torch_over_packed'], r['packed_TFLOPs'], r['verdict']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
