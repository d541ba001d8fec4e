#!/usr/bin/env python3
"""The packed codec at every width it has, 1 ... 8 bits per level index: what do the widths whose elements straddle bytes
(3, 5, 6, 7) cost next to the four that do not?

    python tools/bench_codec_bits.py [--out profiles/codec_bits.json] [--reps 7] [--bits 1,2,...] [--lib OTHER_libqd_hip.so]
                                     [--parent PARENT_RECORD.json]

64 Mi fp32 elements, bucket 256, s = 2^b levels.  For every width three rows:
    pack         qd_pack_uniform_f32     4 B read + b / 8 B written per element (+ 8 B per bucket)
    pack_levels  qd_pack_levels_u8       1 B read + b / 8 B written
    unpack       qd_unpack_uniform_f32   b / 8 B read + 4 B written
All in ONE process (the method of tools/bench_multi_symbols.py): HIP events on the launch stream around a few back-to-back calls
(wall time, launch overhead included), the rows taken in turn `reps` times over (interleaved), median / min / max of the
repetitions in microseconds per call.  Nothing is gated.  What to read it against: pack is bound by its 4 B read per
element, so a width between two others should land between their times; the record says per new width and row whether its
median lies between the 2-bit and the 8-bit median of the same run.
--lib: measure another build of the library (only the widths it accepts: --bits 4,8 for a build before the new widths);
--parent: the record of such a run, carried in the output under 'parent' next to this build's times at the same widths."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

N = 64 << 20
BUCKET = 256
ROWS = ('pack', 'pack_levels', 'unpack')


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
    return {name: {'median': round(statistics.median(s), 2), 'min': round(min(s), 2), 'max': round(max(s), 2)} for name, s in samples.items()}


def measure(reps, widths):
    import torch
    from quantized_distillation_amd import _lib
    dev = torch.device('cuda:0')
    lib = _lib.load()
    st = _lib.stream_ptr(dev)
    nb = N // BUCKET
    x = torch.randn(N, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    y = torch.empty(N, device=dev)
    alpha, beta = torch.empty(nb, device=dev), torch.empty(nb, device=dev)
    forms, keep = [], []
    for b in widths:
        s = 1 << b
        nbytes = int(lib.qd_packed_bytes(N, b))
        packed = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        lev = torch.randint(0, s, (N,), dtype=torch.uint8, device=dev)
        keep += [packed, lev]

        def pack(b=b, s=s, packed=packed):
            return lib.qd_pack_uniform_f32(x.data_ptr(), N, BUCKET, s, b, packed.data_ptr(), alpha.data_ptr(), beta.data_ptr(), st)

        def pack_levels(b=b, packed=packed, lev=lev):
            return lib.qd_pack_levels_u8(lev.data_ptr(), N, b, packed.data_ptr(), st)

        def unpack(b=b, s=s, packed=packed):
            return lib.qd_unpack_uniform_f32(packed.data_ptr(), N, BUCKET, s, b, alpha.data_ptr(), beta.data_ptr(), y.data_ptr(), st)
        for fn in (pack_levels, pack, unpack):                               # (unpack reads what pack wrote, alpha / beta included)
            rc = fn()
            if rc != 0:
                raise SystemExit('%s at %d bits returned %d: this build of the library does not take the width' % (fn.__name__, b, rc))
        forms += [('pack %d' % b, pack, 5), ('pack_levels %d' % b, pack_levels, 5), ('unpack %d' % b, unpack, 5)]
    torch.cuda.synchronize()
    us = timed(forms, reps)
    table = {str(b): {row: us['%s %d' % (row, b)] for row in ROWS} for b in widths}
    for b in widths:
        t = table[str(b)]
        t['pack_GBps'] = round(N * (4 + b / 8.0) / t['pack']['median'] / 1e3, 1)
        t['unpack_GBps'] = round(N * (4 + b / 8.0) / t['unpack']['median'] / 1e3, 1)
    between = None
    if all(str(b) in table for b in (2, 8)):
        between = {str(b): {row: min(table['2'][row]['median'], table['8'][row]['median']) <= table[str(b)][row]['median']
                            <= max(table['2'][row]['median'], table['8'][row]['median']) for row in ROWS}
                   for b in widths if b in (3, 5, 6, 7)}
    return {'what': 'tools/bench_codec_bits.py: %d fp32 elements, bucket %d, s = 2^b; qd_pack_uniform_f32 / qd_pack_levels_u8 / '
                    'qd_unpack_uniform_f32 per width b; HIP events around 5 back-to-back calls (wall, launch overhead included), median / '
                    'min / max of %d interleaved repetitions in one process, microseconds per call; GB/s over (4 + b / 8) N bytes' % (N, BUCKET, reps),
            'device': torch.cuda.get_device_name(0),
            'library': os.path.relpath(_lib.LIB_PATH, ROOT) if _lib.LIB_PATH.startswith(ROOT + os.sep) else 'another build (--lib)',
            'elements': N, 'bucket': BUCKET, 'reps': reps, 'us': table,
            'median_between_the_2_bit_and_the_8_bit_median': between}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'codec_bits.json'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--bits', default='1,2,3,4,5,6,7,8')
    ap.add_argument('--lib', default=None)
    ap.add_argument('--parent', default=None)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error('--reps: at least 5')
    widths = [int(b) for b in args.bits.split(',')]
    if args.lib:
        from quantized_distillation_amd import _lib
        _lib.LIB_PATH = os.path.abspath(args.lib)
    record = measure(args.reps, widths)
    if args.parent:
        with open(args.parent) as f:
            p = json.load(f)
        record['parent'] = {'what': 'the same rows of the parent commit\'s library (before the widths 3, 5, 6 and 7), built apart and measured by '
                                    'this tool in a process of its own in the same session on the same device', 'device': p['device'],
                            'reps': p['reps'], 'us': p['us']}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    for b, t in record['us'].items():
        print('%s bits   %s' % (b, '   '.join('%s %.2f us [%.2f .. %.2f]' % (row, t[row]['median'], t[row]['min'], t[row]['max']) for row in ROWS)))
    for b, t in record.get('parent', {}).get('us', {}).items():
        print('%s bits (parent)   %s' % (b, '   '.join('%s %.2f us [%.2f .. %.2f]' % (row, t[row]['median'], t[row]['min'], t[row]['max']) for row in ROWS)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
