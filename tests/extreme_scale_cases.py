"""Named fp32 inputs on and around the domain of the bucket-invariant division (csrc/qd_common.h: div_alpha<true>,
fastdiv_ok, scale_fast_ok), for tests/test_hip_extreme_scales.py and its CPU-tensor twin in tests/test_host_parity.py.

  * pair buckets: one bucket per (n, alpha) of tests/golden/div_denormal_pairs.json -- alpha in range, n >= 2^-100, a DENORMAL
    quotient on which the shortcut and the IEEE division differ -- of the shape
        x[0] = beta (the minimum), x[5] = alpha (the maximum), x[100] = n + beta, two level-0 fillers alpha 2^-10, the rest beta
    so that alpha_x == alpha_q == alpha, beta_q == beta and n / alpha is computed by every kernel that consumes the quotient;
  * boundary buckets: alpha exactly 2^-60 / 2^100 and their neighbouring floats on both sides, with numerators 2^-100, its
    neighbours, alpha 2^-120, values next to every rounding boundary of 4 / 16 / 256 levels;
  * the families of test_quantize_bit_exact_at_extreme_scales (tiny / huge / denormal / mixed per bucket / constant /
    alpha < 1e-10), a few dozen buckets each;
every bucketed tensor with a ragged tail.  Everything is a function of (bucket, seed): no state, nothing written."""
import json
import os

import numpy as np

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
PAIRS_JSON = os.path.join(HERE, 'golden', 'div_denormal_pairs.json')
G_PAIR = 2.0 ** 100                 # the incoming gradient at a pair's element: lifts a denormal quotient to 2^-49 .. 2^-26


def f32(bits):
    return np.array([bits], dtype=np.uint32).view(F32)[0]


def up(v):
    return np.nextafter(F32(v), F32(np.inf))


def down(v):
    return np.nextafter(F32(v), F32(-np.inf))


_PAIRS = []


def pairs():
    """[(n, alpha)] as np.float32, in the fixture's order."""
    if not _PAIRS:
        with open(PAIRS_JSON) as f:
            _PAIRS.extend((f32(int(p['n_bits'], 16)), f32(int(p['alpha_bits'], 16))) for p in json.load(f)['pairs'])
    return list(_PAIRS)


def positions(size):
    """(index of the minimum, of the maximum, of the pair's numerator) inside a bucket of `size` elements."""
    return 0, (5 if size > 8 else 2), (100 if size > 100 else size - 3)


def pair_beta(n):
    """An exactly representable beta != 0 with (n + beta) and (n + beta) - beta exact: four ulps of n below zero.  It is so far
    below alpha that max - beta rounds to alpha itself."""
    return F32(-4.0) * np.spacing(n)


def pair_bucket(size, n, alpha, with_beta):
    beta = pair_beta(n) if with_beta else F32(0.0)
    x = np.full(size, beta, dtype=F32)
    pmin, pmax, pn = positions(size)
    x[pmax] = alpha
    x[pn] = F32(np.float64(n) + np.float64(beta))
    assert np.float64(x[pn]) == np.float64(n) + np.float64(beta) and F32(x[pn] - beta) == n and F32(alpha - beta) == alpha
    if size > 16:
        x[7] = x[11] = alpha * F32(2.0 ** -10)              # level 0 for every s <= 256, a normal quotient
    return x


def pair_tensor(bucket, with_beta=False, tail=7):
    """One bucket per pair and a short last bucket (`tail` elements) that holds the first pair again."""
    ps = pairs()
    parts = [pair_bucket(bucket, n, a, with_beta) for n, a in ps]
    if tail:
        parts.append(pair_bucket(tail, ps[0][0], ps[0][1], with_beta))
    return np.concatenate(parts)


def pair_positions(bucket, total):
    """Flat indices of (the pairs' elements, the minima, the maxima) of pair_tensor(bucket) with `total` elements."""
    pn, pmin, pmax = [], [], []
    for lo in range(0, total, bucket):
        a, b, c = positions(min(bucket, total - lo))
        pmin.append(lo + a), pmax.append(lo + b), pn.append(lo + c)
    return np.array(pn), np.array(pmin), np.array(pmax)


def pair_gradient(bucket, total, dense, seed=0):
    """dense=False: zero but G_PAIR at each pair's element -- the bucket sum has ONE term, so its order cannot matter and the
    result is comparable bit for bit.  dense=True: N(0, 1) everywhere, 2^125 (1 + U) at the pair's element -- the largest
    weight fp32 allows: a quotient wrong by one denormal ulp is an error of 2^-24 .. 2^-23 -- and 2^-10 N(0, 1) at the two
    touched positions, so that the sum of the magnitudes errlog.check_ste measures against is about 2^-8 + |g u|."""
    pn, _, _ = pair_positions(bucket, total)
    if not dense:
        g = np.zeros(total, dtype=F32)
        g[pn] = F32(G_PAIR)
        return g
    rng = np.random.RandomState(seed + bucket)
    g = rng.randn(total).astype(F32)
    g[pn] = (2.0 ** 125 * (1.0 + rng.rand(pn.size))).astype(F32)
    _, pmin, pmax = pair_positions(bucket, total)
    g[pmin] *= F32(2.0 ** -10)                              # the two touched positions: check_ste adds |g| there to the scale
    g[pmax] *= F32(2.0 ** -10)
    return g


# ------------------------------------------------------------------------------------------------ alpha on the boundaries
LO, HI = F32(2.0 ** -60), F32(2.0 ** 100)
BOUNDARY_ALPHAS = [('2^-60', LO), ('below 2^-60', down(LO)), ('above 2^-60', up(LO)),
                   ('2^100', HI), ('below 2^100', down(HI)), ('above 2^100', up(HI))]


def boundary_bucket(rng, size, alpha, shifted):
    """min = beta, max = beta + alpha exactly (beta = 0, or beta = alpha: 2 alpha and 2 alpha - alpha are exact), inside:
    random fractions, values next to the rounding boundaries (k + 1/2) / (s - 1) of 4 / 16 / 256 levels, and -- beta = 0 -- the
    numerators 2^-100, its neighbours and alpha 2^-120."""
    a64 = np.float64(alpha)
    beta = a64 if shifted else 0.0
    vals = list(rng.rand(size) * a64)
    for s in (4, 16, 256):
        for k in rng.randint(0, s - 1, size=3):
            mid = F32((k + 0.5) / (s - 1) * a64)
            vals[int(rng.randint(size))] = np.float64(mid)
            vals[int(rng.randint(size))] = np.float64(up(mid))
            vals[int(rng.randint(size))] = np.float64(down(mid))
    x = (np.array(vals[:size]) + beta).astype(F32)
    if not shifted:
        tiny = [F32(2.0 ** -100), up(2.0 ** -100), down(2.0 ** -100), F32(a64 * 2.0 ** -120), F32(0.0)]
        for j, v in enumerate(tiny):
            if 20 + j < size:
                x[20 + j] = v
    x = np.clip(x, F32(beta), F32(beta + a64))
    pmin, pmax, _ = positions(size)
    x[pmin], x[pmax] = F32(beta), F32(beta + a64)
    assert F32(x.max() - x.min()) == alpha
    return x


def boundary_tensor(bucket, reps=3, tail=19, seed=0):
    """reps x (six alphas x {beta = 0, beta = alpha}) buckets -- 36 for reps = 3 -- and a ragged tail on alpha = 2^-60."""
    rng = np.random.RandomState(1000 + seed + bucket)
    parts = [boundary_bucket(rng, bucket, a, sh) for _ in range(reps) for _, a in BOUNDARY_ALPHAS for sh in (False, True)]
    if tail:
        parts.append(boundary_bucket(rng, tail, LO, False))
    return np.concatenate(parts)


def single_bucket_cases(n, seed=0):
    """bucket_size=None: the whole tensor is one bucket, so one tensor per boundary alpha (beta = alpha for the two below)."""
    for i, (name, a) in enumerate(BOUNDARY_ALPHAS):
        yield 'alpha ' + name, boundary_bucket(np.random.RandomState(2000 + seed + i), n, a, name.startswith('below'))


def families(bucket, nbuckets=24, tail=5, seed=0):
    """The families of test_quantize_bit_exact_at_extreme_scales at a few dozen buckets."""
    rng = np.random.RandomState(3000 + seed + bucket)
    n = nbuckets * bucket + tail
    base = rng.randn(n).astype(F32)
    scales = [1.0, 2.0 ** -58, 2.0 ** -61, 1e-30, 1e-37, 1e-39, 1e-43, 2.0 ** 99, 2.0 ** 101, 3e37]
    per = np.repeat(np.array(scales * nbuckets)[:nbuckets + 1], bucket)[:n]
    yield 'mixed scale per bucket', (base.astype(np.float64) * per).astype(F32)
    yield 'tiny 2^-61', (base * F32(2.0 ** -61)).astype(F32)
    yield 'huge 3e37', (base * F32(3e37)).astype(F32)
    yield 'zeros next to denormals', np.where(rng.rand(n) < 0.7, 0.0, base * 1e-41).astype(F32)
    const = (base * F32(2.0 ** -59) + F32(3.0)).astype(F32)
    const[bucket:2 * bucket] = F32(0.25)
    yield 'offset 3 + 2^-59, one constant bucket', const
    yield 'alpha < 1e-10', (np.abs(base) * F32(1e-36) + F32(1.0)).astype(F32)


def cases(bucket, n=None, seed=0):
    """Every named case at one bucket size; bucket None: single-bucket tensors of n elements."""
    if bucket is None:
        for name, x in single_bucket_cases(n, seed):
            yield name, x
        rng = np.random.RandomState(seed + n)
        yield 'tiny 2^-61', (rng.randn(n) * 2.0 ** -61).astype(F32)
        yield 'alpha < 1e-10', (np.abs(rng.randn(n)) * 1e-36 + 1.0).astype(F32)
        return
    yield 'pairs', pair_tensor(bucket)
    yield 'pairs + beta', pair_tensor(bucket, with_beta=True)
    yield 'boundary alphas', boundary_tensor(bucket, seed=seed)
    for name, x in families(bucket, seed=seed):
        yield name, x
