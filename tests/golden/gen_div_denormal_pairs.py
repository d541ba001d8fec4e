"""Writes tests/golden/div_denormal_pairs.json: fp32 pairs (n, alpha) INSIDE the stated range of the bucket-invariant division
(csrc/qd_common.h: alpha in [2^-60, 2^100], n >= 2^-100) whose quotient is DENORMAL and on which the shortcut
    y = RN(1 / alpha);  q = RN(n y);  r = fma(-alpha, q, n);  u = fma(r, y, q)
differs from the IEEE quotient RN(n / alpha) -- the reason for the `alpha 2^-120` clause of scale_fast_ok.  CPU only.

Candidates come from a float64 emulation of the three operations (every product of two fp32 values is exact in float64; the
last sum may round twice, so it only proposes); every pair that is written has been re-derived in exact rational arithmetic
by tools/div_invariant_check.py:div_invariant_exact, which tests/test_host_logic.py repeats on the committed file.

    python tests/golden/gen_div_denormal_pairs.py        # deterministic: rewrites the same file
"""
import json
import os
import sys
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import div_invariant_check as dic  # noqa: E402

OUT = os.path.join(HERE, 'div_denormal_pairs.json')
# the pairs of the issue that introduced this fixture: (n bits, alpha bits)
NAMED = [(0x25FFFFFF, 0x702AAAAA), (0x2D800001, 0x6DC00000), (0x1380FDE1, 0x53C00000), (0x18AA2AE5, 0x58C00000)]
NASTY = np.array([0x7FFFFF, 0x7FFFFE, 0, 1, 2, 0x400000, 0x3FFFFF, 0x555555, 0x2AAAAA, 0x7FF000, 0x400001, 0x600000, 0x200000],
                 dtype=np.uint32)
PER_EXPONENT = 3
QUOTIENT_EXPONENTS = range(-149, -126)


def in_domain(nb, ab):
    n, a = dic.f32_fraction(nb), dic.f32_fraction(ab)
    return Fraction(2) ** -60 <= a <= Fraction(2) ** 100 and n >= Fraction(2) ** -100


def differs(nb, ab):
    """-> (shortcut, IEEE quotient) as Fractions when they differ and the pair is in the domain, else None."""
    if not in_domain(nb, ab):
        return None
    u, want = dic.div_invariant_exact(dic.f32_fraction(nb), dic.f32_fraction(ab))
    return (u, want) if u != want else None


def quotient_exponent(want):
    """floor(log2) of a positive Fraction."""
    e = want.numerator.bit_length() - want.denominator.bit_length()
    return e - 1 if want < Fraction(2) ** e else e


def propose(rng, qe, count):
    """`count` * 3 (n bits, alpha bits) with n / alpha next to a rounding tie (k + 1/2) 2^-149 of the denormal grid, 2^qe <=
    k 2^-149 < 2^(qe+1) -- where the shortcut's q = RN(n y) and the true quotient can fall on different sides -- filtered by
    the float64 emulation's verdict."""
    lo_ea = max(-60, -100 - qe)                                    # n >= 2^-100
    ea = rng.randint(lo_ea, 100, size=count)
    ma = np.where(rng.rand(count) < 0.5, NASTY[rng.randint(len(NASTY), size=count)],
                  rng.randint(0, 1 << 23, size=count).astype(np.uint32)).astype(np.uint32)
    ab = ((ea + 127).astype(np.uint32) << np.uint32(23)) | ma
    k = rng.randint(1 << (qe + 149), 1 << (qe + 150), size=count).astype(np.float64)
    a = ab.view(np.float32).astype(np.float64)
    mid = ((k + 0.5) * a * 2.0 ** -149).astype(np.float32)         # (the product is exact in float64: 24 + 24 bits)
    nb = np.concatenate([mid.view(np.int32) + np.int32(d) for d in (-1, 0, 1)]).astype(np.int32).view(np.uint32)
    ab = np.concatenate([ab, ab, ab])
    n, a = nb.view(np.float32).astype(np.float64), ab.view(np.float32).astype(np.float64)
    y = (1.0 / a).astype(np.float32).astype(np.float64)
    q = (n * y).astype(np.float32).astype(np.float64)
    r = (n - a * q).astype(np.float32).astype(np.float64)
    u = (q + r * y).astype(np.float32)
    want = (n / a).astype(np.float32)                              # (may round twice as well: a proposal only)
    near = u.view(np.int32) != want.view(np.int32)
    return nb[near], ab[near]


def main():
    rng = np.random.RandomState(20240)
    pairs, seen = [], set()

    def add(nb, ab, origin, only=None):
        d = differs(int(nb), int(ab))
        if d is None or (int(nb), int(ab)) in seen:
            return None
        u, want = d
        e = quotient_exponent(want) if want else -150
        if only is not None and e != only:
            return None
        seen.add((int(nb), int(ab)))
        pairs.append({'n_bits': '0x%08x' % int(nb), 'alpha_bits': '0x%08x' % int(ab), 'quotient_exponent': e,
                      'shortcut': float(u), 'ieee': float(want), 'origin': origin})
        return e
    for nb, ab in NAMED:
        assert add(nb, ab, 'issue') is not None, (hex(nb), hex(ab))
    for qe in QUOTIENT_EXPONENTS:
        have = 0
        for _ in range(8):                             # (-149 and -127 stay empty: nothing turned up in 40 rounds either)
            nb, ab = propose(rng, qe, 20000)
            for i in range(nb.size):
                if have < PER_EXPONENT and add(nb[i], ab[i], 'search', only=qe) == qe:
                    have += 1
            if have >= PER_EXPONENT:
                break
        print('quotient exponent %d: %d pairs' % (qe, have))
    pairs.sort(key=lambda p: (p['quotient_exponent'], p['n_bits'], p['alpha_bits']))
    with open(OUT, 'w') as f:
        json.dump({'doc': 'fp32 (n, alpha) with alpha in [2^-60, 2^100], n >= 2^-100, a denormal quotient, and '
                          'fma(fma(-alpha, RN(n y), n), y, RN(n y)) != RN(n / alpha) for y = RN(1 / alpha); '
                          'written by tests/golden/gen_div_denormal_pairs.py',
                   'pairs': pairs}, f, indent=1)
        f.write('\n')
    print('%d pairs -> %s' % (len(pairs), OUT))


if __name__ == '__main__':
    main()
