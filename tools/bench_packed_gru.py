#!/usr/bin/env python3
"""GRU steps from packed weights (qdg_gru_cell_packed_f32, libqd_infer_gru.so: both products on fp32 MFMA as two sums, gates in the
same launch) next to the only way to run these layers from packed weights without it -- PackedUniform.unpack() of both weights
followed by torch's fp32 GRU -- and to torch alone on the unpacked fp32 weights.

    python tools/bench_packed_gru.py [--out profiles/packed_gru.json] [--error-out profiles/packed_gru_error.txt]

The method of tools/bench_packed_lstm.py (timed() and Rotating of tools/bench_packed_layers.py are used as they are): HIP events
around `iters` back-to-back calls, every call on the next of `copies` copies of its weights, median [min .. max] of `reps`
interleaved repetitions in ONE process, microseconds per call.  Shapes, at 2 / 4 / 8 bits, bucket 256, s = 2^b: the decoder
cells of the translation student with rnn_type GRU, (1500, 1000) + (1500, 500) and (1500, 500) + (1500, 500), at batch 1, 16 and
64 (one PackedGRUCell call), and its encoder nn.GRU(500, 500, 2) at T = 50, batch 64 (one PackedGRU call: per layer one batched
Linear and 50 steps).  Before anything is timed every cell result is held to float64: gi and gh to 1e-6 sum |terms|, h' to the
float64 epilogue of the call's own gates (units of 2^-24 (|h| + 1)); the figures go to --error-out.  Nothing is gated on the
times: the ratios are reported as they are."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from bench_packed_layers import BUCKET, Rotating, timed  # noqa: E402

CELLS = ((1000, 500), (500, 500))            # (input, hidden) of the decoder's two cells
BATCHES = (1, 16, 64)
WIDTHS = (2, 4, 8)
ENCODER = (500, 500, 2, 50, 64)              # input, hidden, layers, T, batch
H_BOUND = 40.2                               # 4 x what the fp32 reference formulas reach (tests/test_hip_packed_gru.py)


def held(lib, pc, x, h, st, key):
    """The cell call with its gates, against float64: (gi and gh error / sum|terms|, h' error in the unit above, sigma of gi + gh)."""
    import torch
    H = pc.hidden_size
    gates, h1 = torch.empty(x.shape[0], 2, 3 * H, device=x.device), torch.empty_like(h)
    rc = lib.qdg_gru_cell_packed_f32(*pc._weight_args(pc.ih), *pc._weight_args(pc.hh), H, pc.input_size, x.data_ptr(), None, h.data_ptr(), x.shape[0],
                                     pc.ih.bias.data_ptr(), pc.hh.bias.data_ptr(), h1.data_ptr(), gates.data_ptr(), st)
    if rc != 0:
        raise SystemExit('%s: the call was refused (%d)' % (key, rc))
    ratio = 0.0
    for got, part, act in ((gates[:, 0], pc.ih, x), (gates[:, 1], pc.hh, h)):
        w, a, b = part._weight().double(), act.double(), part.bias.double()
        ratio = max(ratio, float(((got.double() - (a @ w.T + b)).abs() / (a.abs() @ w.abs().T + b.abs())).max()))
    if not ratio <= 1e-6:
        raise SystemExit('%s: |gates - float64| / sum|terms| = %.3g > 1e-6: not timing a wrong result' % (key, ratio))
    a, b = gates[:, 0].double().view(-1, 3, H), gates[:, 1].double().view(-1, 3, H)
    z = torch.sigmoid(a[:, 1] + b[:, 1])
    h64 = (1.0 - z) * torch.tanh(a[:, 2] + torch.sigmoid(a[:, 0] + b[:, 0]) * b[:, 2]) + z * h.double()
    hu = float(((h1.double() - h64).abs() / (h.double().abs() + 1)).max()) * 2.0 ** 24
    if not hu <= H_BOUND:
        raise SystemExit("%s: h' error %.2f units: beyond %.1f, not timing a wrong result" % (key, hu, H_BOUND))
    return ratio, hu, float((a + b).std())


def measure(reps, copies, iters, seq_iters):
    import torch
    from torch import nn
    from quantized_distillation_amd import _infer_gru, _lib, packed_layers
    dev = torch.device('cuda:0')
    lib = _infer_gru.load()
    st = _lib.stream_ptr(dev)
    torch.manual_seed(0)
    forms, keys, keep, errors = [], [], [], {}
    with torch.no_grad():
        for inp, hid in CELLS:
            cell = nn.GRUCell(inp, hid).to(dev)
            for b in WIDTHS:
                pcs = [packed_layers.PackedGRUCell.from_gru_cell(cell, 1 << b, BUCKET, b) for _ in range(copies)]
                fps = [pc.unpack() for pc in pcs]                          # the fp32 baseline reads the same values
                keep += [pcs, fps]
                for batch in BATCHES:
                    x, h = torch.randn(batch, inp, device=dev) * 3, torch.randn(batch, hid, device=dev) * 2
                    key = 'cell (%d, %d) + (%d, %d) batch %d bits %d' % (3 * hid, inp, 3 * hid, hid, batch, b)
                    errors[key] = held(lib, pcs[0], x, h, st, key)
                    keys.append(key)
                    forms += [(key + ' packed', Rotating(lambda i, pcs=pcs, x=x, h=h: pcs[i](x, h), copies), iters),
                              (key + ' unpack+torch', Rotating(lambda i, pcs=pcs, x=x, h=h: torch._VF.gru_cell(
                                  x, h, pcs[i].ih._weight(), pcs[i].hh._weight(), pcs[i].ih.bias, pcs[i].hh.bias), copies), iters),
                              (key + ' torch', Rotating(lambda i, fps=fps, x=x, h=h: fps[i](x, h), copies), iters)]
        inp, hid, layers, T, batch = ENCODER
        gru = nn.GRU(inp, hid, layers).to(dev)
        x = torch.randn(T, batch, inp, device=dev)
        for b in WIDTHS:
            pgs = [packed_layers.PackedGRU.from_gru(gru, 1 << b, BUCKET, b) for _ in range(copies)]
            fps = [pg.unpack() for pg in pgs]
            keep += [pgs, fps]
            key = 'encoder GRU(%d, %d, %d) T %d batch %d bits %d' % (inp, hid, layers, T, batch, b)
            got, want = pgs[0](x)[0], fps[0].double()(x.double())[0]
            fps[0].float()
            diff = float((got.double() - want).abs().max())
            if not diff <= 1e-5:
                raise SystemExit('%s: |output - float64 nn.GRU| = %.3g > 1e-5: not timing a wrong result' % (key, diff))
            errors[key] = diff

            def unpack_then_gru(i, pgs=pgs, x=x, hid=hid, layers=layers, batch=batch):
                flat = [t for cl in pgs[i].cells for t in (cl.ih._weight(), cl.hh._weight(), cl.ih.bias, cl.hh.bias)]
                return torch._VF.gru(x, x.new_zeros(layers, batch, hid), flat, True, layers, 0.0, False, False, False)
            keys.append(key)
            forms += [(key + ' packed', Rotating(lambda i, pgs=pgs, x=x: pgs[i](x), copies), seq_iters),
                      (key + ' unpack+torch', Rotating(unpack_then_gru, copies), seq_iters),
                      (key + ' torch', Rotating(lambda i, fps=fps, x=x: fps[i](x), copies), seq_iters)]
        torch.cuda.synchronize()
        us = timed(forms, reps)
    table = {}
    for key in keys:
        p, u, t = us[key + ' packed'], us[key + ' unpack+torch'], us[key + ' torch']
        table[key] = {'packed_us': p, 'unpack_then_torch_us': u, 'torch_fp32_us': t, 'unpack_then_torch_over_packed': round(u['median'] / p['median'], 3),
                      'torch_over_packed': round(t['median'] / p['median'], 3),
                      'verdict': 'functional, not tuned: behind unpack + torch' if p['median'] > u['median'] else 'ahead of unpack + torch'}
    return {'what': 'tools/bench_packed_gru.py: PackedGRUCell / PackedGRU (packed: qdg_gru_cell_packed_f32, libqd_infer_gru.so; the encoder also '
                    'qdm_linear_packed_f32) against PackedUniform.unpack() of every weight + torch\'s fp32 gru_cell / gru and against torch alone on '
                    'the unpacked fp32 weights; bucket %d, s = 2^b; HIP events around back-to-back calls (%d of a cell, %d of the encoder; wall, launch '
                    'and Python overhead included), each call on the next of %d copies of its weights, median / min / max of %d interleaved '
                    'repetitions in one process, microseconds per call; nothing is gated' % (BUCKET, iters, seq_iters, copies, reps),
            'device': torch.cuda.get_device_name(0), 'reps': reps, 'copies': copies, 'iters': iters, 'seq_iters': seq_iters, 'errors': errors, 'rows': table}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'packed_gru.json'))
    ap.add_argument('--error-out', default=os.path.join(ROOT, 'profiles', 'packed_gru_error.txt'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--copies', type=int, default=3)
    ap.add_argument('--iters', type=int, default=24)
    ap.add_argument('--seq-iters', type=int, default=2)
    args = ap.parse_args()
    if args.reps < 5 or args.copies < 1 or args.iters < 1 or args.seq_iters < 1:
        ap.error('--reps: at least 5; --copies, --iters, --seq-iters: at least 1')
    record = measure(args.reps, args.copies, args.iters, args.seq_iters)
    for path in (args.out, args.error_out):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    cells = {k: v for k, v in record['errors'].items() if k.startswith('cell')}
    with open(args.error_out, 'w') as f:
        f.write('qdg_gru_cell_packed_f32 against float64 at the timed sizes (tools/bench_packed_gru.py), cell mode, x Gaussian sigma 3, h sigma 2\n')
        f.write("gi, gh: error / sum|terms|, bound 1e-6; h': error against the float64 epilogue of the call's own fp32 gi and gh, in units of\n")
        f.write("2^-24 (|h| + 1), bound %.1f (4 x what the fp32 reference formulas reach; tests/test_hip_packed_gru.py)\n" % H_BOUND)
        f.write("worst: gates %.3g   h' %.2f\n" % tuple(max(v[i] for v in cells.values()) for i in range(2)))
        for k, (ratio, hu, sigma) in cells.items():
            f.write("%-52s gates %.3g (sigma %.2f)   h' %.2f\n" % (k, ratio, sigma, hu))
        for k, v in record['errors'].items():
            if k not in cells:
                f.write('%-52s |output - float64 nn.GRU of the unpacked weights| %.3g (a wiring check, bound 1e-5)\n' % (k, v))
    for key, r in record['rows'].items():
        print('%-52s packed %9.2f [%.2f .. %.2f]  unpack + torch %9.2f [%.2f .. %.2f]  torch %9.2f [%.2f .. %.2f]  (unpack + torch) / packed %.3f  '
              'torch / packed %.3f  %s'
              % (key, r['packed_us']['median'], r['packed_us']['min'], r['packed_us']['max'], r['unpack_then_torch_us']['median'],
                 r['unpack_then_torch_us']['min'], r['unpack_then_torch_us']['max'], r['torch_fp32_us']['median'], r['torch_fp32_us']['min'],
                 r['torch_fp32_us']['max'], r['unpack_then_torch_over_packed'], r['torch_over_packed'], r['verdict']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
