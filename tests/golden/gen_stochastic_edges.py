"""Finds (seed, element) pairs at which the stochastic-rounding generator draws exactly 0.0 -- the one draw at which the
reference's `rand <= probabilities` (quant_functions.py:187) moves an element that sits exactly ON a level one level up --
and writes them to tests/golden/stochastic_edges.json.  Data only: seeds, element indices, the 32-bit word behind each draw.

A draw is the top 24 bits of a Philox4x32-7 word (oracle/oracle_np.py: philox4x32_7_words), so it is 0.0 once in 2^24
draws.  The scan walks seeds BASE, BASE + 1, ... over the elements 0..4095 of each (2^12 seeds cover 2^24 draws) until it
has WANT pairs; tests/test_stochastic_host.py recomputes every recorded draw.  CPU only, a few seconds:

    python tests/golden/gen_stochastic_edges.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle_np as onp  # noqa: E402

BASE = 0x5EED00000000          # (a seed with a non-zero high key word)
ELEMENTS = 4096
WANT = 6
BATCH = 2048                   # seeds per vectorised call


def main():
    blocks = np.arange(ELEMENTS // 4, dtype=np.uint64)[None, :]
    pairs, first = [], BASE
    while len(pairs) < WANT:
        seeds = np.arange(first, first + BATCH, dtype=np.uint64)[:, None]
        words = onp.philox4x32((blocks, 0, 0x51ed270b, 0x2545f491),
                               (seeds & np.uint64(0xFFFFFFFF), seeds >> np.uint64(32)), 7)
        words = np.stack(np.broadcast_arrays(*words), axis=2).reshape(BATCH, ELEMENTS)
        for si, e in zip(*np.nonzero(words < 256)):
            pairs.append(dict(seed=int(first + si), element=int(e), word=int(words[si, e])))
        first += BATCH
    pairs = pairs[:WANT]
    for p in pairs:                                                    # the same through the per-seed function the tests use
        assert onp.philox4x32_7_uniform(p['seed'], p['element'] + 1)[p['element']] == 0.0
    out = dict(generator='philox4x32-7, counter (element >> 2, 0, 0x51ed270b, 0x2545f491), key = seed, word = element & 3',
               base_seed=BASE, elements=ELEMENTS, seeds_scanned=first - BASE, pairs=pairs)
    path = os.path.join(ROOT, 'tests', 'golden', 'stochastic_edges.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print('wrote', path, 'after', first - BASE, 'seeds:', pairs)


if __name__ == '__main__':
    main()
