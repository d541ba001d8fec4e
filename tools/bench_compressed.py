#!/usr/bin/env python3
"""Huffman-coded checkpoints on the WRN-16-22 parameter list (harness/models.py): encode / decode times, decode throughput
against the 8 TB/s HBM peak, and file bytes against the reference's size formula.  Not part of bench.py.

    timeout -k 10 600 python tools/bench_compressed.py [--out FILE.json]     (one JSON line per configuration on stdout;
                                                                            --out also writes the whole record to FILE.json)

Kernel times of qd_huffman_encode's three kernels and the single decode kernel come from rocprofv3 when the tool runs
under it (rocprofv3 --kernel-trace --stats ... -- python tools/bench_compressed.py); the tool itself times save / load
with HIP events around the library calls only (the file I/O is outside the timed region)."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from harness import models  # noqa: E402
from quantized_distillation_amd import compressed as C  # noqa: E402
from quantized_distillation_amd import _lib  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    best = None
    for _ in range(reps):
        torch.cuda.synchronize()
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        t = ev[0].elapsed_time(ev[1]) * 1e-3
        best = t if best is None else min(best, t)
    return best


def main():
    out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    params = [p.data.to(dev) for p in models.WideResNet(16, 22).parameters()]
    ts = {'p%d' % i: t for i, t in enumerate(params)}
    n = sum(t.numel() for t in params)
    rec = {'model': 'WRN-16-22', 'tensors': len(params), 'elements': n, 'runs': []}
    tmp = tempfile.mkdtemp()
    for label, kw in (('uniform_s16_b256', dict(s=16, bucket_size=256)),
                      ('nonuniform_k4_b256', dict(points=[[0.0, 0.3, 0.7, 1.0]], bucket_size=256))):
        path = os.path.join(tmp, label + '.qd')
        rep = C.save_compressed(path, ts, **kw)
        f = C._parse(open(path, 'rb').read())
        data = open(path, 'rb').read()
        outs = C.load_compressed(path, device=dev)
        # decode only: the sections already on the device, one launch (compressed._decode without the raw copies)
        torch.cuda.synchronize()
        t_load = timed(lambda: C._decode(f, data, outs, dev), 5)
        t_save = timed(lambda: C.save_compressed(path, ts, **kw), 3)
        bitstream = rep['sections']['bitstream']
        moved = bitstream + rep['sections']['chunk_offsets'] + rep['sections']['alpha_beta'] + 4 * n
        rec['runs'].append({'config': label, 'coding': rep['coding'], 'mean_bit_length': rep['mean_bit_length'],
                            'file_bytes': rep['file_bytes'], 'reference_bytes': rep['reference_size_mb'] * 1e6,
                            'file_over_reference': rep['file_bytes'] / (rep['reference_size_mb'] * 1e6),
                            'sections': rep['sections'], 'save_wall_s': t_save, 'load_call_wall_s': t_load,
                            'decode_bytes_moved': moved, 'hbm_floor_s': moved / HBM_BYTES_PER_S})
        print(json.dumps(rec['runs'][-1]))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'w') as fh:
            json.dump(rec, fh, indent=1)
        print('wrote', out_path)


if __name__ == '__main__':
    main()
