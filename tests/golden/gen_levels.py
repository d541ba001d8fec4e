#!/usr/bin/env python3
"""Generate tests/golden/levels.json by RUNNING the reference on the level ladder of tests/level_cases.py.

Run in the authoring container only (it needs the reference checkout gen_golden.py names, which does not exist on the GPU
box):

    python tests/golden/gen_levels.py

The reference package is imported unmodified through gen_golden.py and called through its public API; nothing of it is copied
here.  Two run-time substitutions, both of gen_golden.py's kind (attributes patched for the duration of a call, no source
edited or stored):
  * uniformQuantization_variable.backward is gen_golden.patched_backward() (the two shape fixes of SURVEY.md 8c);
  * for the stochastic cases `torch.rand` is replaced by a function that returns the Philox draws of the case's seed
    (oracle_np.philox4x32_7_uniform) laid out in the bucket view the reference asks for, so that
    `probabilities = s*tensor`, `floor_`, `div_`, `(currRand <= probabilities).float()*1/s` are pinned op for op.

The file holds data only: per case its parameters (tests/level_cases.py: fixture_cases) and the SHA-256 of the little-endian
fp32 bytes of q, alpha and beta, one after the other (of the output for an STE case; an options case also keeps the
reference's fp32 mean), and the Huffman mean code lengths of a three-tensor model.  No tensor is stored."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G          # noqa: E402  (puts the reference first on sys.path and imports its `quantization`)

ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.append(os.path.join(ROOT, 'tests'))
sys.path.append(ROOT)           # behind the reference: `oracle` comes from here, `quantization` stays the reference's
import level_cases as L         # noqa: E402

refq, refqhf = G.refq, G.refqhf
assert os.path.abspath(refq.__file__).startswith(G.REF), refq.__file__
torch.set_num_threads(1)


def flat(t):
    return t.detach().numpy().reshape(-1)


class philox_rand(object):
    """`with philox_rand(seed, n):` -- torch.rand(size) returns the draws of the n real elements in a tensor of `size`
    (row-major: the bucket view), 0.0 in the padding."""

    def __init__(self, seed, n):
        self.seed, self.n, self.calls = seed, n, 0

    def __enter__(self):
        self.real = torch.rand
        torch.rand = self
        return self

    def __exit__(self, *a):
        torch.rand = self.real

    def __call__(self, size):
        self.calls += 1
        total = int(np.prod(tuple(size)))
        r = np.zeros(total, np.float32)
        r[:self.n] = L.padded_draws(self.seed, self.n, None)
        return torch.from_numpy(r).view(*size)


def run_case(c, backward):
    x, n, bucket = L.case_input(c)
    xt = torch.from_numpy(x.copy())
    s = c['s']
    if c['kind'] == 'ste':
        fn = refq.uniformQuantization_variable(s, bucket_size=bucket)
        fn.forward(xt)
        return dict(out=flat(backward(fn, torch.from_numpy(L.case_gradient(c).copy()))))
    if c['kind'] == 'stoch':
        with philox_rand(c['seed'], n) as rnd:
            q, sf = refq.uniformQuantization(xt, s, stochastic_rounding=True, bucket_size=bucket)
        assert rnd.calls == 1
    else:
        q, sf = refq.uniformQuantization(xt, s, bucket_size=bucket, **(L.OPTIONS if c['kind'] == 'opt' else {}))
    assert np.array_equal(xt.numpy(), x), 'the reference wrote its input'
    r = dict(q=flat(q), alpha=flat(sf.alpha), beta=flat(sf.beta))
    if c['kind'] == 'opt':
        r['mean'] = float(sf.mean_tensor)
        # the input is built so that every summation order gives the correctly rounded mean: one reference bit pattern
        assert np.float32(r['mean']) == L.exact_mean(x), (c, r['mean'], L.exact_mean(x))
    return r


def main():
    backward = G.patched_backward()
    cases = []
    for c in L.fixture_cases():
        c = dict(c)
        r = run_case(c, backward)
        c['sha256'] = L.result_digest(c['kind'], r)
        if c['kind'] == 'opt':
            c['mean'] = float(np.float32(r['mean']))      # the reference's fp32 mean, exactly (a float64 holds every float32)
        cases.append(c)
    huffman = []
    for s in L.HUFFMAN_S:
        model = [torch.from_numpy(t.copy()) for t in L.huffman_model(s)]
        bits = refqhf.get_huffman_encoding_mean_bit_length(iter(model), lambda p: refq.uniformQuantization(p, s, bucket_size=256),
                                                           'uniform', s)
        huffman.append(dict(s=s, mean_bit_length=float(bits)))
    doc = dict(about='reference results on the level ladder: tests/golden/gen_levels.py, tests/level_cases.py', cases=cases,
               huffman=huffman)
    with open(L.FIXTURE, 'w') as f:
        f.write('{\n"about": %s,\n"huffman": %s,\n"cases": [\n' % (json.dumps(doc['about']), json.dumps(huffman, sort_keys=True)))
        f.write(',\n'.join(json.dumps(c, sort_keys=True, separators=(',', ':')) for c in cases))
        f.write('\n]\n}\n')
    print('levels.json: %d cases, %d bytes' % (len(cases), os.path.getsize(L.FIXTURE)))


if __name__ == '__main__':
    main()
