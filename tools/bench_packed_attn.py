#!/usr/bin/env python3
"""One global-attention step of the translation student's decoder from packed weights (PackedGlobalAttention: qda_attn_context_f32 and
qda_attn_out_packed_f32, libqd_infer_attn.so, two launches) next to what the parent commit offers -- the seven-call composition
bmm, masked_fill, softmax, bmm, cat, PackedLinear, tanh -- and to the same composition with torch's fp32 Linear on the unpacked weight.

    python tools/bench_packed_attn.py [--out profiles/packed_attn.json] [--error-out profiles/packed_attn_error.txt]

The method of tools/bench_packed_gru.py (timed() and Rotating of tools/bench_packed_layers.py are used as they are): HIP events around
`iters` back-to-back steps, every step on the next of `copies` copies of its weights, median [min .. max] of `reps` interleaved
repetitions in ONE process, microseconds per step.  Shape: dim 500, S 50, the `dot` form over the memory, lengths between S / 2 and S,
batch 1 / 16 / 64, 2 / 4 / 8 bits, bucket 256, s = 2^b.  Before anything is timed every result is held to float64 on the CPU: align and
ctx to 4 x what the fp32 torch composition reaches there on the same inputs, pre to 1e-6 sum |terms|, attn_h to 4 x torch's fp32 tanh of
the call's own pre; the figures are appended to --error-out.  Nothing is gated on the times: the ratios are reported as they are."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from bench_packed_layers import BUCKET, Rotating, timed  # noqa: E402

DIM, S = 500, 50
BATCHES = (1, 16, 64)
WIDTHS = (2, 4, 8)
U = 2.0 ** -24


def composition(linear, x, memory, mask):
    """The seven calls around `linear` ([ctx ; x] -> dim): what a decoder step runs without the fused kernels."""
    import torch
    align = torch.softmax(torch.bmm(memory, x.unsqueeze(2)).squeeze(2).masked_fill(mask, float('-inf')), dim=1)
    return torch.tanh(linear(torch.cat([torch.bmm(align.unsqueeze(1), memory).squeeze(1), x], dim=1))), align


def held(lib, att, x, memory, lengths, st, key):
    """The two C calls with pre asked for, against float64 on the CPU; the figures, each next to its bound."""
    import torch
    batch = x.shape[0]
    align, ctx, attn_h, pre = (torch.empty(batch, n, device=x.device) for n in (S, DIM, DIM, DIM))
    o = att.out
    rcs = (lib.qda_attn_context_f32(x.data_ptr(), memory.data_ptr(), memory.data_ptr(), lengths.data_ptr(), batch, S, DIM, align.data_ptr(), ctx.data_ptr(), st),
           lib.qda_attn_out_packed_f32(o.packed.data_ptr(), o.alpha.data_ptr(), o.beta.data_ptr(), o.bucket_size or 0, o.s, o.bits, DIM, ctx.data_ptr(),
                                       x.data_ptr(), batch, o.bias.data_ptr(), attn_h.data_ptr(), pre.data_ptr(), st))
    if rcs != (0, 0):
        raise SystemExit('%s: a call was refused %r' % (key, rcs))
    mask = (torch.arange(S)[None, :] >= lengths.cpu()[:, None])
    ref = {}
    for dtype in (torch.float32, torch.float64):
        mem = memory.cpu().to(dtype).masked_fill(mask[:, :, None], 0.0)
        a = torch.softmax(torch.bmm(mem, x.cpu().to(dtype).unsqueeze(2)).squeeze(2).masked_fill(mask, float('-inf')), dim=1)
        ref[dtype] = (a.double(), torch.bmm(a.unsqueeze(1), mem).squeeze(1).double(), torch.bmm(a.unsqueeze(1), mem.abs()).squeeze(1).double())
    a64, c64, mag = ref[torch.float64]
    units = lambda a, c: (float((a.double().cpu() - a64).abs().max()) / U, float(((c.double().cpu() - c64).abs() / mag).max()) / U)  # noqa: E731
    got, base = units(align, ctx), units(*ref[torch.float32][:2])
    w, cx = o._weight().double(), torch.cat([ctx, x], dim=1).double()
    ratio = float(((pre.double() - (cx @ w.T + o.bias.double())).abs() / (cx.abs() @ w.abs().T + o.bias.double().abs())).max())
    t64 = torch.tanh(pre.double().cpu())
    tanh, tanh_base = float((attn_h.double().cpu() - t64).abs().max()) / U, float((torch.tanh(pre.cpu()).double() - t64).abs().max()) / U
    if not (got[0] <= 4 * base[0] and got[1] <= 4 * base[1] and ratio <= 1e-6 and tanh <= 4 * tanh_base):
        raise SystemExit('%s: align %.2f (fp32 torch %.2f), ctx %.2f (%.2f), pre %.3g, tanh %.2f (%.2f): beyond a bound, not timing a wrong result'
                         % (key, got[0], base[0], got[1], base[1], ratio, tanh, tanh_base))
    return {'align': got[0], 'align_fp32_torch': base[0], 'ctx': got[1], 'ctx_fp32_torch': base[1], 'pre': ratio, 'tanh': tanh, 'tanh_fp32_torch': tanh_base}


def measure(reps, copies, iters):
    import torch
    from torch import nn
    from quantized_distillation_amd import _infer_attn, _lib, packed_layers
    dev = torch.device('cuda:0')
    lib = _infer_attn.load()
    st = _lib.stream_ptr(dev)
    torch.manual_seed(0)
    forms, keys, keep, errors = [], [], [], {}
    lin = nn.Linear(2 * DIM, DIM).to(dev)
    with torch.no_grad():
        for b in WIDTHS:
            atts = [packed_layers.PackedGlobalAttention.from_linears(lin, None, 1 << b, BUCKET, b) for _ in range(copies)]
            pls = [packed_layers.PackedLinear(a.out.as_packed_uniform(), a.out.bias, batched_from=16) for a in atts]   # the parent's best per batch
            fps = [a.unpack()[0] for a in atts]                            # the fp32 baseline reads the same values
            keep += [atts, pls, fps]
            for batch in BATCHES:
                x = torch.randn(batch, DIM, device=dev) * 2.0 / DIM ** 0.5
                memory = torch.randn(batch, S, DIM, device=dev)
                lengths = torch.randint(S // 2, S + 1, (batch,), device=dev)
                mask = torch.arange(S, device=dev)[None, :] >= lengths[:, None]
                key = 'dim %d S %d batch %d bits %d' % (DIM, S, batch, b)
                errors[key] = held(lib, atts[0], x, memory, lengths, st, key)
                keys.append(key)
                forms += [(key + ' packed', Rotating(lambda i, atts=atts, x=x, m=memory, n=lengths: atts[i](x, m, n), copies), iters),
                          (key + ' composition', Rotating(lambda i, pls=pls, x=x, m=memory, k=mask: composition(pls[i], x, m, k), copies), iters),
                          (key + ' torch', Rotating(lambda i, fps=fps, x=x, m=memory, k=mask: composition(fps[i], x, m, k), copies), iters)]
        torch.cuda.synchronize()
        us = timed(forms, reps)
    table = {}
    for key in keys:
        p, c, t = us[key + ' packed'], us[key + ' composition'], us[key + ' torch']
        behind = [n for n, v in (('the PackedLinear composition', c), ('torch fp32', t)) if p['median'] > v['median']]
        table[key] = {'packed_us': p, 'packed_linear_composition_us': c, 'torch_fp32_us': t, 'composition_over_packed': round(c['median'] / p['median'], 3),
                      'torch_over_packed': round(t['median'] / p['median'], 3),
                      'verdict': 'functional, not tuned: behind ' + ' and '.join(behind) if behind else 'ahead of both'}
    return {'what': 'tools/bench_packed_attn.py: PackedGlobalAttention (dot form; qda_attn_context_f32 + qda_attn_out_packed_f32, libqd_infer_attn.so) against '
                    'bmm, masked_fill, softmax, bmm, cat, PackedLinear(batched_from=16), tanh and against the same seven calls with nn.Linear on the '
                    'unpacked fp32 weight; the mask of the compositions is made once outside the timed step; bucket %d, s = 2^b; HIP events around %d '
                    'back-to-back steps (wall, launch and Python overhead included), each on the next of %d copies of its weights, median / min / max of '
                    '%d interleaved repetitions in one process, microseconds per step; nothing is gated' % (BUCKET, iters, copies, reps),
            'device': torch.cuda.get_device_name(0), 'reps': reps, 'copies': copies, 'iters': iters, 'errors': errors, 'rows': table}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'packed_attn.json'))
    ap.add_argument('--error-out', default=os.path.join(ROOT, 'profiles', 'packed_attn_error.txt'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--copies', type=int, default=3)
    ap.add_argument('--iters', type=int, default=24)
    args = ap.parse_args()
    if args.reps < 5 or args.copies < 1 or args.iters < 1:
        ap.error('--reps: at least 5; --copies, --iters: at least 1')
    record = measure(args.reps, args.copies, args.iters)
    for path in (args.out, args.error_out):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    with open(args.error_out, 'a') as f:                                 # below the test shapes' figures, which are written by hand
        f.write('\nAt the timed sizes (tools/bench_packed_attn.py), against float64 on the CPU; in brackets what fp32 torch reaches there on the same inputs,\n')
        f.write('a quarter of the bound.  align: 2^-24; ctx: 2^-24 sum_s align_s |v_s|; pre: error / sum|terms|, bound 1e-6; tanh: 2^-24 against the float64 tanh of pre\n')
        for k, e in record['errors'].items():
            f.write('%-32s align %.2f (%.2f)   ctx %.2f (%.2f)   pre %.3g   tanh %.2f (%.2f)\n'
                    % (k, e['align'], e['align_fp32_torch'], e['ctx'], e['ctx_fp32_torch'], e['pre'], e['tanh'], e['tanh_fp32_torch']))
    for key, r in record['rows'].items():
        print('%-32s packed %8.2f [%.2f .. %.2f]  composition %8.2f [%.2f .. %.2f]  torch %8.2f [%.2f .. %.2f]  composition / packed %.3f  torch / packed %.3f  %s'
              % (key, r['packed_us']['median'], r['packed_us']['min'], r['packed_us']['max'], r['packed_linear_composition_us']['median'],
                 r['packed_linear_composition_us']['min'], r['packed_linear_composition_us']['max'], r['torch_fp32_us']['median'], r['torch_fp32_us']['min'],
                 r['torch_fp32_us']['max'], r['composition_over_packed'], r['torch_over_packed'], r['verdict']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
