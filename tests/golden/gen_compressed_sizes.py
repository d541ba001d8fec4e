#!/usr/bin/env python3
"""Generate tests/golden/compressed_sizes.json by RUNNING the reference's size accounting.

    python tests/golden/gen_compressed_sizes.py REFERENCE_DIR

REFERENCE_DIR is a checkout of antspy/quantized_distillation; its package is imported unmodified, the way gen_golden.py
imports it.  For a few seeded small models it records get_huffman_encoding_mean_bit_length
(quantization/help_functions.py:175-232) and get_size_quantized_model (helpers/functions.py:226-262).  The inputs are
0.05 * randn from the CPU generator with the recorded seed, so any machine rebuilds the same tensors
(tests/test_compressed_host.py, tests/test_hip_compressed.py: `model_tensors`).
"""
import json
import os
import sys

import torch

if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], 'quantization')):
    sys.exit('usage: gen_compressed_sizes.py REFERENCE_DIR (a checkout of antspy/quantized_distillation)')
REF = os.path.abspath(sys.argv[1])
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path = [REF] + [p for p in sys.path if os.path.abspath(p or '.') != os.path.abspath(os.path.join(HERE, '..', '..'))]
import quantization as refq                      # noqa: E402
import quantization.help_functions as refqhf     # noqa: E402
from helpers import functions as reff            # noqa: E402

assert os.path.abspath(refq.__file__).startswith(REF), refq.__file__
torch.set_num_threads(1)

MODELS = {
    'convnet_small': [(16, 3, 5, 5), (16,), (32, 16, 5, 5), (32,), (10, 800), (10,)],
    'ragged': [(1000,), (77,), (3, 333), (4097,), (5,)],
    'mlp': [(256, 784), (256,), (128, 256), (128,), (10, 128), (10,)],
}
CASES = [
    dict(model='convnet_small', seed=1, s=16, bucket_size=256, quantize_first_last=True),
    dict(model='convnet_small', seed=2, s=4, bucket_size=None, quantize_first_last=False),
    dict(model='ragged', seed=3, s=256, bucket_size=64, quantize_first_last=True),
    dict(model='mlp', seed=4, s=8, bucket_size=100, quantize_first_last=True),
    dict(model='mlp', seed=5, points=[0.0, 0.3, 0.7, 1.0], bucket_size=256, quantize_first_last=True),
    dict(model='ragged', seed=6, points=[0.0, 0.1, 0.2, 0.5, 0.8, 0.9, 0.95, 1.0], bucket_size=None, quantize_first_last=False),
]


def model_tensors(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [0.05 * torch.randn(*s, generator=g) for s in shapes]


class Holder(torch.nn.Module):
    def __init__(self, ts):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(t) for t in ts])


def main():
    out = []
    for case in CASES:
        ts = model_tensors(MODELS[case['model']], case['seed'])
        m = Holder(ts)
        b = case['bucket_size']
        if 'points' in case:
            pts = torch.tensor(case['points'])
            fn = lambda p: refq.nonUniformQuantization(p, pts, bucket_size=b)     # noqa: E731
            kind, bits = 'nonUniform', (len(case['points']) - 1).bit_length()
        else:
            fn = lambda p: refq.uniformQuantization(p, case['s'], bucket_size=b)   # noqa: E731
            kind, bits = 'uniform', (case['s'] - 1).bit_length()
        params = list(m.parameters())
        qparams = params if case['quantize_first_last'] else params[1:-1]
        mean_bits = refqhf.get_huffman_encoding_mean_bit_length(iter(qparams), fn, kind, s=2 ** bits)
        size_mb = reff.get_size_quantized_model(m, bits, fn, b, kind, case['quantize_first_last'])
        rec = dict(case, shapes=MODELS[case['model']], mean_bit_length=float(mean_bits), size_mb=float(size_mb))
        out.append(rec)
        print(rec['model'], rec['seed'], mean_bits, size_mb)
    with open(os.path.join(HERE, 'compressed_sizes.json'), 'w') as f:
        json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
