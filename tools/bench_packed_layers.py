#!/usr/bin/env python3
"""Linear and Embedding from packed weights (libqd_infer.so) next to torch on the unpacked fp32 weights: what does a layer cost
when it reads bits / 8 bytes per weight?  Reported, not gated.

    python tools/bench_packed_layers.py [--out profiles/packed_layers.json] [--reps 7] [--bits 2,4,8] [--copies 6]

Rows (all in ONE process, the method of tools/bench_codec_bits.py):
    linear     W [32768, 512] (a vocabulary projection) and [4096, 4096], m = 1 and 8 rows of x, bucket 256, s = 2^b:
               qdi_linear_packed_f32 against torch.nn.functional.linear on PackedUniform.unpack() of the same weight
    embedding  W [32768, 512], 4096 indices: qdi_embedding_packed_f32 against torch.nn.functional.embedding on the same
HIP events on the launch stream around `iters` back-to-back calls (wall time, launch overhead included), the rows taken in turn
`reps` times over (interleaved), median / min / max of the repetitions in microseconds per call.  Every call of a row takes
the NEXT of `copies` copies of its weight (packed and fp32 alike), so that a weight is not simply served by the cache the call
before left it in: six fp32 copies of either shape are 384 MiB, more than the 256 MiB of Infinity Cache; six packed copies
are 12 ... 96 MiB and stay in it -- which is part of what a small weight buys.  --copies 1 measures both fully cache-resident.
GB/s is over the algorithmic bytes of the packed call: packed + alpha + beta + x (or idx) + y (or out).  Before anything is
timed, every packed result is held to the fp32 one at the timed size (the bound of tests/packed_layer_cases.py)."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

LINEAR_SHAPES = ((32768, 512), (4096, 4096))
MS = (1, 8)
EMB_SHAPE = (32768, 512)
EMB_COUNT = 4096
BUCKET = 256


def timed(forms, reps):
    import torch
    for _, fn, iters in forms:                                           # warm-up: code objects, allocator, clocks, torch's algorithm choice
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
    return {name: {'median': round(statistics.median(s), 2), 'min': round(min(s), 2), 'max': round(max(s), 2)} for name, s in samples.items()}


class Rotating(object):
    """fn(i) called with i = 0, 1, ..., copies - 1, 0, ..."""

    def __init__(self, fn, copies):
        self.fn, self.copies, self.i = fn, copies, 0

    def __call__(self):
        self.i = (self.i + 1) % self.copies
        return self.fn(self.i)


def measure(reps, widths, copies, iters):
    import torch
    import torch.nn.functional as F
    from quantized_distillation_amd import _infer, _lib, codec
    dev = torch.device('cuda:0')
    lib = _infer.load()
    st = _lib.stream_ptr(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    forms, meta, keep = [], {}, []

    def held(y, x, w, tag):
        y64 = x.double() @ w.double().T
        mag = x.double().abs() @ w.double().abs().T
        ratio = float(((y.double() - y64).abs() / mag).max())
        if not ratio <= 1e-6:
            raise SystemExit('%s: |y - y64| / sum|terms| = %.3g > 1e-6: not timing a wrong result' % (tag, ratio))
        return ratio

    worst = 0.0
    for rows, cols in LINEAR_SHAPES:
        W = torch.randn(rows, cols, device=dev, generator=gen) * 0.05
        for b in widths:
            s = 1 << b
            pks = [codec.pack_uniform(W, s, BUCKET, b) for _ in range(copies)]
            ws = [pk.unpack() for pk in pks]                               # the fp32 baseline reads the same values
            keep += [pks, ws]
            for m in MS:
                x = torch.randn(m, cols, device=dev, generator=gen)
                y = torch.empty(m, rows, device=dev)

                def packed_call(i, pks=pks, rows=rows, cols=cols, s=s, b=b, x=x, m=m, y=y):
                    pk = pks[i]
                    return lib.qdi_linear_packed_f32(pk.packed.data_ptr(), pk.alpha.data_ptr(), pk.beta.data_ptr(), rows, cols, BUCKET, s, b,
                                                     x.data_ptr(), m, None, y.data_ptr(), st)

                def torch_call(i, ws=ws, x=x):
                    return F.linear(x, ws[i])
                if packed_call(0) != 0:
                    raise SystemExit('qdi_linear_packed_f32 refused [%d, %d] at %d bits' % (rows, cols, b))
                worst = max(worst, held(y, x, ws[0], 'linear [%d, %d] %d bits m %d' % (rows, cols, b, m)))
                key = 'linear %dx%d bits %d m %d' % (rows, cols, b, m)
                n = rows * cols
                meta[key] = {'bytes': n * b // 8 + 8 * (n // BUCKET) + 4 * m * cols + 4 * m * rows, 'fp32_bytes': 4 * n + 4 * m * cols + 4 * m * rows}
                forms += [(key + ' packed', Rotating(packed_call, copies), iters), (key + ' torch', Rotating(torch_call, copies), iters)]
    rows, cols = EMB_SHAPE
    W = torch.randn(rows, cols, device=dev, generator=gen) * 0.05
    idx = torch.randint(0, rows, (EMB_COUNT,), device=dev, generator=gen)
    out = torch.empty(EMB_COUNT, cols, device=dev)
    for b in widths:
        s = 1 << b
        pks = [codec.pack_uniform(W, s, BUCKET, b) for _ in range(copies)]
        ws = [pk.unpack() for pk in pks]
        keep += [pks, ws]

        def packed_call(i, pks=pks, s=s, b=b):
            pk = pks[i]
            return lib.qdi_embedding_packed_f32(pk.packed.data_ptr(), pk.alpha.data_ptr(), pk.beta.data_ptr(), rows, cols, BUCKET, s, b,
                                                idx.data_ptr(), EMB_COUNT, out.data_ptr(), st)

        def torch_call(i, ws=ws):
            return F.embedding(idx, ws[i])
        if packed_call(0) != 0:
            raise SystemExit('qdi_embedding_packed_f32 refused at %d bits' % b)
        if not torch.equal(out.view(torch.int32), F.embedding(idx, ws[0]).view(torch.int32)):
            raise SystemExit('embedding at %d bits differs from the unpacked table: not timing a wrong result' % b)
        key = 'embedding %dx%d count %d bits %d' % (rows, cols, EMB_COUNT, b)
        touched = EMB_COUNT * cols                                         # weights the lookup needs (repeats counted once each time)
        meta[key] = {'bytes': touched * b // 8 + 8 * (touched // BUCKET) + 8 * EMB_COUNT + 4 * touched, 'fp32_bytes': 8 * touched + 8 * EMB_COUNT}
        forms += [(key + ' packed', Rotating(packed_call, copies), iters), (key + ' torch', Rotating(torch_call, copies), iters)]
    torch.cuda.synchronize()
    us = timed(forms, reps)
    table = {}
    for key, mt in meta.items():
        p, t = us[key + ' packed'], us[key + ' torch']
        table[key] = {'packed_us': p, 'torch_fp32_us': t, 'torch_over_packed': round(t['median'] / p['median'], 2),
                      'algorithmic_bytes': mt['bytes'], 'packed_GBps': round(mt['bytes'] / p['median'] / 1e3, 1),
                      'fp32_bytes': mt['fp32_bytes'], 'torch_GBps': round(mt['fp32_bytes'] / t['median'] / 1e3, 1)}
    return {'what': 'tools/bench_packed_layers.py: qdi_linear_packed_f32 / qdi_embedding_packed_f32 (bucket %d, s = 2^b) against '
                    'torch.nn.functional.linear / embedding on the unpacked fp32 weights; HIP events around %d back-to-back calls (wall, launch '
                    'overhead included), each call on the next of %d copies of its weight, median / min / max of %d interleaved repetitions '
                    'in one process, microseconds per call; GB/s over the algorithmic bytes' % (BUCKET, iters, copies, reps),
            'device': torch.cuda.get_device_name(0), 'reps': reps, 'copies': copies, 'iters': iters,
            'worst_linear_error_over_sum_abs_terms': worst, 'rows': table}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'packed_layers.json'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--bits', default='2,4,8')
    ap.add_argument('--copies', type=int, default=6)
    ap.add_argument('--iters', type=int, default=24)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error('--reps: at least 5')
    if args.copies < 1 or args.iters < 1:
        ap.error('--copies, --iters: at least 1')
    record = measure(args.reps, [int(b) for b in args.bits.split(',')], args.copies, args.iters)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    for key, r in record['rows'].items():
        print('%-44s packed %8.2f us [%.2f .. %.2f] %7.1f GB/s   torch fp32 %8.2f us [%.2f .. %.2f]   torch / packed %.2f'
              % (key, r['packed_us']['median'], r['packed_us']['min'], r['packed_us']['max'], r['packed_GBps'],
                 r['torch_fp32_us']['median'], r['torch_fp32_us']['min'], r['torch_fp32_us']['max'], r['torch_over_packed']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
