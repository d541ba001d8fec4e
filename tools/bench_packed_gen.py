#!/usr/bin/env python3
"""The end of a decoder step from the packed generator weight (PackedGenerator: qdn_generator_packed_f32, libqd_infer_gen.so, two
launches) next to what the parent commit offers -- PackedLinear(batched_from=8), torch.log_softmax, torch.topk -- and to the same
composition with torch's fp32 Linear on the unpacked weight.

    python tools/bench_packed_gen.py [--out profiles/packed_gen.json]

The method of tools/bench_packed_attn.py (timed() and Rotating of tools/bench_packed_layers.py are used as they are): HIP events around
`iters` back-to-back calls, every call on the next of `copies` copies of its weights, median [min .. max] of `reps` interleaved
repetitions in ONE process, microseconds per call.  Shapes [10000, 500] and [32768, 512], m 5 / 64 / 320, 4 bits, bucket 256, k = 5,
with and without the [m, V] log-probs (without them the composition still has to write and read its logits).  Before anything is
timed the fused call is held to the composition on the same weight: its top-k words carry the composition's top-k log-probs, log-probs within 1e-5 (|log p| + 1).
Nothing is gated on the times: the ratios are reported as they are."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from bench_packed_layers import BUCKET, Rotating, timed  # noqa: E402

SHAPES = ((10000, 500), (32768, 512))
MS = (5, 64, 320)
BITS, K = 4, 5


def composition(linear, x, log_probs):
    """What a decoder step runs without the fused kernels; without log_probs the caller keeps only lse and the top k."""
    import torch
    logp = torch.log_softmax(linear(x), dim=-1)
    top = torch.topk(logp, K, dim=-1)
    return (logp if log_probs else None), top.values, top.indices


def measure(reps, copies, iters):
    import torch
    from torch import nn
    from quantized_distillation_amd import packed_layers
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    forms, keys, keep = [], [], []
    with torch.no_grad():
        for V, dim in SHAPES:
            lin = nn.Linear(dim, V).to(dev)
            gens = [packed_layers.PackedGenerator.from_linear(lin, 1 << BITS, BUCKET, BITS) for _ in range(copies)]
            pls = [packed_layers.PackedLinear(g.as_packed_uniform(), g.bias, batched_from=8) for g in gens]
            fps = [g.unpack() for g in gens]                               # the fp32 baseline reads the same values
            keep += [gens, pls, fps]
            for m in MS:
                x = torch.randn(m, dim, device=dev) * 4.0
                out, (ref_logp, ref_val, ref_idx) = gens[0](x, topk=K), composition(pls[0], x, True)
                err = float(((out.log_probs - ref_logp).abs() / (ref_logp.abs() + 1.0)).max())
                # the composition's logits have another summation order below batched_from: a near-tie may swap, the log-probs may not differ
                if float((ref_logp.gather(1, out.top_indices) - ref_val).abs().max()) > 1e-4 or ref_idx.shape != out.top_indices.shape or err > 1e-5:
                    raise SystemExit('[%d, %d] m %d: the fused call and the composition disagree (log-prob error %.3g): not timing a wrong result' % (V, dim, m, err))
                for lp in (True, False):
                    key = '[%d, %d] m %d %s' % (V, dim, m, 'log-probs and top-%d' % K if lp else 'top-%d only' % K)
                    keys.append(key)
                    forms += [(key + ' packed', Rotating(lambda i, gens=gens, x=x, lp=lp: gens[i](x, topk=K, log_probs=lp), copies), iters),
                              (key + ' composition', Rotating(lambda i, pls=pls, x=x, lp=lp: composition(pls[i], x, lp), copies), iters),
                              (key + ' torch', Rotating(lambda i, fps=fps, x=x, lp=lp: composition(fps[i], x, lp), copies), iters)]
        torch.cuda.synchronize()
        us = timed(forms, reps)
    table = {}
    for key in keys:
        p, c, t = us[key + ' packed'], us[key + ' composition'], us[key + ' torch']
        behind = [n for n, v in (('the PackedLinear composition', c), ('torch fp32', t)) if p['median'] > v['median']]
        table[key] = {'packed_us': p, 'packed_linear_composition_us': c, 'torch_fp32_us': t, 'composition_over_packed': round(c['median'] / p['median'], 3),
                      'torch_over_packed': round(t['median'] / p['median'], 3), 'verdict': 'behind ' + ' and '.join(behind) if behind else 'ahead of both'}
    return {'what': 'tools/bench_packed_gen.py: PackedGenerator (qdn_generator_packed_f32, libqd_infer_gen.so, two launches) against PackedLinear(batched_from=8) + '
                    'torch.log_softmax + torch.topk and against the same three calls with nn.Linear on the unpacked fp32 weight; %d bits, bucket %d, k = %d; HIP events '
                    'around %d back-to-back calls (wall, launch and Python overhead included), each on the next of %d copies of its weights, median / min / max of %d '
                    'interleaved repetitions in one process, microseconds per call; nothing is gated' % (BITS, BUCKET, K, iters, copies, reps),
            'device': torch.cuda.get_device_name(0), 'reps': reps, 'copies': copies, 'iters': iters, 'rows': table}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'packed_gen.json'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--copies', type=int, default=3)
    ap.add_argument('--iters', type=int, default=16)
    args = ap.parse_args()
    if args.reps < 5 or args.copies < 1 or args.iters < 1:
        ap.error('--reps: at least 5; --copies, --iters: at least 1')
    record = measure(args.reps, args.copies, args.iters)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    for key, r in record['rows'].items():
        print('%-46s packed %9.2f [%.2f .. %.2f]  composition %9.2f [%.2f .. %.2f]  torch %9.2f [%.2f .. %.2f]  composition / packed %.3f  torch / packed %.3f  %s'
              % (key, r['packed_us']['median'], r['packed_us']['min'], r['packed_us']['max'], r['packed_linear_composition_us']['median'],
                 r['packed_linear_composition_us']['min'], r['packed_linear_composition_us']['max'], r['torch_fp32_us']['median'], r['torch_fp32_us']['min'],
                 r['torch_fp32_us']['max'], r['composition_over_packed'], r['torch_over_packed'], r['verdict']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
