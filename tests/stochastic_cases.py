"""Cases of the stochastic-rounding branch of qd_uniform_f32 (include/qd_hip.h; quant_functions.py:174-187 of the reference),
shared by tests/test_stochastic_host.py (libqd_host.so and the oracle, no GPU) and tests/test_hip_stochastic.py (libqd_hip.so,
and device against host bit for bit).  A plain helper module: no fixtures, nothing runs on import.

What the cases are built to decide, and random data never does:
  * `rnd <= p` BY EQUALITY.  A draw is a multiple of 2^-24, so an input can be made whose probability p equals its own draw
    bit for bit (threshold_input): with alpha = 1, beta = 0 and s - 1 a power of two, t = x (s - 1) and p = t - floor(t) are
    exact.  `<` instead of `<=`, `1 - rnd`, a 23-bit or half-offset conversion of the word, a wrong word order or a wrong
    draw altogether flip such elements; so does a p formed after a contraction of t - floor(t).
  * `rnd == 0.0` at `p == 0` (edge_input): an element exactly on a level moves one level up, the bucket's maximum to level
    s, one past the top.  tests/golden/stochastic_edges.json lists (seed, element) pairs whose draw is 0.0.
  * the level index at that edge: saturated at s - 1 (include/qd_hip.h), the neighbouring bytes untouched.
  * independence of the up / down decisions between neighbouring elements, the words of a block, bucket rows and the seeds
    successive calls use (stream_statistics): z-scores against the exact Bernoulli variance of the probabilities used.
`python tests/stochastic_cases.py` prints the z-scores of the oracle's generator (profiles/stochastic_streams.txt)."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                  # (run as a script: `python tests/stochastic_cases.py`)
    sys.path.insert(0, ROOT)
from oracle import oracle_np as onp  # noqa: E402
from quantized_distillation_amd import _lib  # noqa: E402

F32 = np.float32
SEED = 0x0DDBA11C0FFEE123                 # the fixed seed S of the threshold cases (check_seed_conditions holds it to them)
SENTINEL = 0xEE                           # around the level-index output

# (n, bucket) of tests/test_hip_parity.py::test_stochastic_rounding_bit_exact_on_every_kernel_path: vector, chunk, chunk-any,
# lane-group, block-per-bucket, single bucket (small, fused / three-launch), global
SHAPES = [(10007, 256), (10007, 64), (10007, 100), (10007, 33), (10007, 7), (10007, 1000), (70001, 2048), (70001, 4096),
          (70001, 20000), (10007, None), (300001, None), (10007, 3), (10007, 513), (4096, 128), (50, 256)]
OFFSET_SHAPES = [(10007, 256), (10007, None)]          # run on views 1..3 floats into a 16-byte granule as well
SHAPE_IDS = ['n%d-b%s' % s for s in SHAPES]


def rows_of(n, bucket):
    """[(lo, hi)] of the buckets of an n-element tensor (help_functions.py:67-94; padding repeats the last element)."""
    nb, row, _ = onp.bucket_geometry(n, bucket)
    return [(b * row, min((b + 1) * row, n)) for b in range(nb)]


def plant_unit_range(x, n, bucket, rng, avoid=()):
    """One exact 0.0 and one exact 1.0 per bucket at seeded positions (never at `avoid`): alpha = 1, beta = 0 exactly.
    Returns the boolean mask of the planted elements."""
    planted = np.zeros(n, bool)
    avoid = set(avoid)
    for lo, hi in rows_of(n, bucket):
        free = [i for i in rng.permutation(np.arange(lo, hi)) if i not in avoid][:2]
        assert len(free) == 2, 'a bucket needs room for its 0 and its 1'
        x[free[0]], x[free[1]] = 0.0, 1.0
        planted[free] = True
    return planted


def draws(seed, n):
    return onp.philox4x32_7_uniform(seed, n)


def padded_draws(seed, n, bucket):
    _, _, padded = onp.bucket_geometry(n, bucket)
    r = np.zeros(padded, F32)
    r[:n] = draws(seed, n)
    return r


def oracle(x, s, seed, bucket):
    """The reference formula fed with the generator's draws; q, lev and up flattened to the n real elements."""
    n = x.size
    r = onp.uniform_quantize_stochastic(x, s, padded_draws(seed, n, bucket), bucket)
    return dict(q=r['q'].reshape(-1), lev=r['lev'].reshape(-1)[:n].astype(np.uint8), up=r['up'].reshape(-1)[:n],
                alpha=r['alpha'].reshape(-1), beta=r['beta'].reshape(-1))


def level_value(level_floor, up, s):
    """q of an element of a bucket with alpha = 1, beta = 0 in the reference's operation order (:183,187,142-148):
    floor / (s - 1), plus 1 / (s - 1) where the draw decided `up`, times alpha, plus beta, plus the mean (0)."""
    sm1 = F32(s - 1)
    w = (np.asarray(level_floor, F32) / sm1).astype(F32)
    inc = (np.asarray(up).astype(F32) * F32(1.0) / sm1).astype(F32)
    w = (w + inc).astype(F32)
    return ((w * F32(1.0)).astype(F32) + F32(0.0)).astype(F32) + F32(0.0)


# ------------------------------------------------------------------------------------------------ the two libraries at the C ABI
class Library(object):
    """qd_uniform_f32 of one library with the seed given directly.  kind: 'host' (libqd_host.so, CPU tensors) or 'hip'."""

    def __init__(self, kind):
        self.kind = kind
        self.lib = _lib.host() if kind == 'host' else _lib.load()
        self.device = torch.device('cpu' if kind == 'host' else 'cuda:0')

    def uniform(self, x, bucket, s, seed, want_lev=True, offset=0, stochastic=1):
        """-> dict(q, alpha, beta, lev) as numpy arrays.  offset: x and q start `offset` floats into their allocations."""
        n = x.size
        nb = len(rows_of(n, bucket))
        xb = torch.zeros(n + 4, dtype=torch.float32)
        xb[offset:offset + n] = torch.from_numpy(np.ascontiguousarray(x, dtype=F32))
        xb = xb.to(self.device)
        qb = torch.full((n + 4,), 777.0, dtype=torch.float32, device=self.device)
        ab = torch.full((2, nb), 777.0, dtype=torch.float32, device=self.device)
        lev = torch.full((n + 8,), SENTINEL, dtype=torch.uint8, device=self.device)          # [4, 4 + n) is the output
        xv, qv, lv = xb[offset:offset + n], qb[offset:offset + n], lev[4:4 + n]
        if self.kind == 'hip':
            ws = _lib.workspace(self.device)
            tail = (ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        else:
            tail = (None, 0, None)
        rc = self.lib.qd_uniform_f32(xv.data_ptr(), qv.data_ptr(), n, bucket or 0, s, ab[0].data_ptr(), ab[1].data_ptr(),
                                     lv.data_ptr() if want_lev else None, None, 0, 0.0, stochastic, ctypes.c_uint64(seed),
                                     *tail)
        assert rc == 0, (rc, n, bucket, s)
        if self.kind == 'hip':
            torch.cuda.synchronize()
        qh, levh = qb.cpu().numpy(), lev.cpu().numpy()
        assert np.all(np.delete(qh, np.arange(offset, offset + n)) == F32(777.0)), 'q written outside [0, n)'
        assert np.all(levh[:4] == SENTINEL) and np.all(levh[4 + n:] == SENTINEL), 'level_idx written outside [0, n)'
        if not want_lev:
            assert np.all(levh == SENTINEL)
        return dict(q=qh[offset:offset + n].copy(), alpha=ab[0].cpu().numpy(), beta=ab[1].cpu().numpy(),
                    lev=levh[4:4 + n].copy() if want_lev else None)

    def set_fused_mode(self, mode):
        """qd_set_single_fused_mode of the device library (the host library has one path); returns the previous mode."""
        return self.lib.qd_set_single_fused_mode(mode) if self.kind == 'hip' else mode


def same_outputs(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k], equal_nan=True) for k in ('q', 'alpha', 'beta', 'lev'))


# ------------------------------------------------------------------------------------------------ every element on its threshold
def threshold_input(kind, n, bucket, s, seed=SEED):
    """-> (x, planted mask, threshold mask, expected level of the threshold elements).  s - 1 must be a power of two.
    'A': x = d / (s - 1): p == d bit for bit, `d <= p` holds by equality: level 1.
    'B': x = nextafter(d, -inf) / (s - 1) for d > 0: p is the next float below the draw: level 0.
    'C': x = (l + d) / (s - 1) with seeded l in 0..s-2 where the draw's low log2(s - 1) bits are clear (l + d is then exact
         in fp32 and so is t - floor(t)), l = 0 elsewhere: level l + 1, up to the top level s - 1."""
    sm1 = s - 1
    bits = sm1.bit_length() - 1
    assert sm1 == 1 << bits
    d = draws(seed, n)
    rng = np.random.RandomState(n * 31 + (bucket or 0) + ord(kind))
    if kind == 'A':
        x, thr, want = d / F32(sm1), np.ones(n, bool), np.ones(n, np.int64)
    elif kind == 'B':
        x, thr, want = np.nextafter(d, F32(-np.inf)) / F32(sm1), d > 0, np.zeros(n, np.int64)
        x = np.where(thr, x, F32(0.0)).astype(F32)
    else:
        word24 = np.round(d.astype(np.float64) * 16777216.0).astype(np.int64)
        clear = (word24 & (sm1 - 1)) == 0
        l = np.where(clear, rng.randint(0, sm1, n), 0)
        x, thr, want = (l.astype(F32) + d) / F32(sm1), np.ones(n, bool), l + 1
        assert np.array_equal((l.astype(F32) + d).astype(np.float64), l + d.astype(np.float64)), 'l + d must be exact'
    x = x.astype(F32)
    assert np.array_equal(x.astype(np.float64) * sm1, (x * F32(sm1)).astype(np.float64))      # t = x (s - 1) is exact
    planted = plant_unit_range(x, n, bucket, rng)
    return x, planted, thr & ~planted, want


def check_seed_conditions(seed=SEED):
    """A condition of the cases, checked on the CPU: apart from the planted 0 and 1 at least 99 % of the elements of A and B
    are threshold elements, and in C at least 20 % sit on a level above 0 with their draw on the threshold."""
    for n, bucket in SHAPES:
        for kind in 'AB':
            _, planted, thr, _ = threshold_input(kind, n, bucket, 5, seed)
            assert thr.sum() >= 0.99 * (~planted).sum(), (kind, n, bucket)
        _, planted, thr, want = threshold_input('C', n, bucket, 5, seed)
        d = draws(seed, n)
        clear = (np.round(d.astype(np.float64) * 16777216.0).astype(np.int64) & 3) == 0
        assert (clear & thr).sum() >= 0.20 * (~planted).sum(), ('C', n, bucket)
        assert len(set(want[clear & thr])) == 4                                  # levels 1, 2, 3 and the top level 4


def check_threshold(lib, n, bucket, s, kinds='ABC', offset=0, seed=SEED):
    """Runs the threshold cases of one shape on `lib`; returns the outputs (for a comparison between libraries)."""
    outs = []
    for kind in kinds:
        x, planted, thr, want = threshold_input(kind, n, bucket, s, seed)
        got = lib.uniform(x, bucket, s, seed, want_lev=s <= 256, offset=offset)
        tag = (lib.kind, kind, n, bucket, s, offset)
        assert np.all(got['alpha'] == F32(1.0)) and np.all(got['beta'] == F32(0.0)), tag
        ref = oracle(x, s, seed, bucket)
        # the closed form first, so that the oracle cannot drift with the kernel: level `want`, by equality
        low = (want[thr] - 1).astype(F32) if kind != 'B' else np.zeros(int(thr.sum()), F32)
        value = level_value(low, kind != 'B', s)
        bad = np.flatnonzero(got['q'][thr] != value)
        assert bad.size == 0, (tag, 'threshold elements on the wrong level', bad.size, np.flatnonzero(thr)[bad[:5]])
        assert np.array_equal(ref['q'][thr], value) and np.array_equal(ref['lev'][thr], want[thr]), (tag, 'the oracle')
        assert np.array_equal(got['q'], ref['q']), tag
        if got['lev'] is not None:
            assert np.array_equal(got['lev'][thr], want[thr].astype(np.uint8)), tag
            assert np.array_equal(got['lev'], ref['lev']), tag
        outs.append(got)
    return outs


# ------------------------------------------------------------------------------------------------ rnd == 0.0 at p == 0
def edge_pairs():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stochastic_edges.json')) as f:
        return json.load(f)['pairs']


EDGE_GEOMETRIES = [(4500, 256), (4500, 100), (4500, 8192), (4500, None), (20000, None)]     # 8192: one bucket of n < bucket
EDGE_IDS = ['n%d-b%s' % g for g in EDGE_GEOMETRIES]


def interior_level(s):
    """A level l in 1..s-3 whose x = l / (s - 1) scales back to exactly l: t = x (s - 1) == l, p == 0."""
    sm1 = F32(s - 1)
    for l in range(max(1, (s - 1) // 3), s - 2):
        x = F32(l) / sm1
        if F32(x * sm1) == F32(l):
            return l, x
    raise AssertionError(s)


def edge_input(where, element, n, bucket, s, seed):
    """Seeded values in [1/8, 7/8], one exact 0.0 and 1.0 per bucket, and `element` -- whose draw under `seed` is 0.0 --
    placed on a level: 'max' = the 1.0 of its bucket, 'min' = the 0.0, 'mid' = an interior level.  -> (x, level it sits on)"""
    rng = np.random.RandomState(element + s)
    x = (0.125 + 0.75 * rng.rand(n)).astype(F32)
    plant_unit_range(x, n, bucket, rng, avoid=(element,))
    lo, hi = [r for r in rows_of(n, bucket) if r[0] <= element < r[1]][0]
    if where == 'mid':
        l, x[element] = interior_level(s)
        return x, l
    old = F32(1.0) if where == 'max' else F32(0.0)
    at = lo + int(np.flatnonzero(x[lo:hi] == old)[0])
    x[at], x[element] = F32(0.5), old                        # the bucket keeps exactly one 0 and one 1
    return x, (s - 1 if where == 'max' else 0)


def check_edges(lib, n, bucket, s, want_lev):
    """Every recorded pair, at the bucket's maximum, its minimum and an interior level: one level up, even past the top."""
    outs = []
    for pair in edge_pairs():
        seed, e = pair['seed'], pair['element']
        assert draws(seed, e + 1)[e] == 0.0
        for where in ('max', 'min', 'mid'):
            x, l = edge_input(where, e, n, bucket, s, seed)
            got = lib.uniform(x, bucket, s, seed, want_lev=want_lev)
            tag = (lib.kind, where, pair, n, bucket, s)
            assert np.all(got['alpha'] == F32(1.0)) and np.all(got['beta'] == F32(0.0)), tag
            value = level_value(l, True, s)[()]
            assert value > F32(l) / F32(s - 1) and (where != 'max' or value > F32(1.0)), tag           # past the top at 'max'
            assert got['q'][e] == value, (tag, got['q'][e], value)
            ref = oracle(x, s, seed, bucket)
            assert ref['q'][e] == value and ref['up'][e], (tag, 'the oracle')
            assert np.array_equal(got['q'], ref['q']), tag
            if want_lev:
                # saturated at s - 1 (include/qd_hip.h); with s = 256 an unsaturated 256 would be stored as 0 and, in the
                # packed stores of the device, carry into the next element's byte
                assert got['lev'][e] == min(l + 1, s - 1), (tag, got['lev'][e])
                assert np.array_equal(got['lev'], ref['lev']), (tag, np.flatnonzero(got['lev'] != ref['lev'])[:8])
            # the deterministic branch leaves the element on its level: the one-level move IS the stochastic `<=`
            det = lib.uniform(x, bucket, s, seed, want_lev=want_lev, stochastic=0)
            assert det['q'][e] == level_value(l, False, s)[()], tag
            outs.append(got)
    return outs


# ------------------------------------------------------------------------------------------------ independent streams
STREAM_N = 1 << 18
STREAM_SEED = 0x51A7157C5EED0001
STREAM_BUCKET = 256
Z_BOUND = 6.0            # standard deviations of the exact null variance: a false alarm of about 2e-9 per statistic
Z_FINDING = 4.0          # above this for the ORACLE's own decisions: a finding about the generator, not a bound to widen


def stream_input():
    """x_i = p_i from a seeded uniform, with one exact 0 and 1 in every row of 256 (so alpha = 1, beta = 0 both for the one
    bucket of bucket_size=None and for bucket 256); s = 2 makes p = x and the output 0 or 1.  -> (x, mask of the p_i)"""
    rng = np.random.RandomState(2024)
    x = rng.rand(STREAM_N).astype(F32)
    x = np.where(x >= F32(1.0), F32(0.5), x)
    planted = np.zeros(STREAM_N, bool)
    x[3::STREAM_BUCKET], x[200::STREAM_BUCKET] = 0.0, 1.0
    planted[3::STREAM_BUCKET] = planted[200::STREAM_BUCKET] = True
    return x, ~planted


def oracle_decisions(seed, x):
    return draws(seed, x.size) <= x


def _z_pairs(r_a, r_b, v_a, v_b):
    """z of sum r_a r_b with r = up - p: under independence its terms have mean 0 and variance v_a v_b, v = p (1 - p)."""
    return float(np.sum(r_a * r_b) / np.sqrt(np.sum(v_a * v_b)))


def stream_statistics(up, up_next, up_far, up_rows, x, use):
    """up, up_next, up_far: decisions (bool [n]) at seeds S, S + 1 and S + 2^32 with one bucket; up_rows: at S with bucket 256.
    -> ordered {name: z}.  Every statistic is a sum of N bounded terms that are independent under the null hypothesis, divided
    by the square root of its exact variance computed from the p_i used; planted elements take no part (`use`)."""
    p = x.astype(np.float64)
    v = p * (1.0 - p)

    def res(u):
        return np.where(use, u.astype(np.float64) - p, 0.0)
    vv = np.where(use, v, 0.0)
    r, z = res(up), {}
    for b in range(10):                                              # the up-rate of a band of p against the band's mean p
        sel = use & (p >= b / 10.0) & (p < (b + 1) / 10.0)
        z['band %d/10 up-rate' % b] = float(r[sel].sum() / np.sqrt(v[sel].sum()))
    for lag in (1, 2, 4):
        z['element i, i + %d' % lag] = _z_pairs(r[:-lag], r[lag:], vv[:-lag], vv[lag:])
    r4, v4 = r.reshape(-1, 4), vv.reshape(-1, 4)
    for a in range(4):
        for c in range(a + 1, 4):
            z['block words %d, %d' % (a, c)] = _z_pairs(r4[:, a], r4[:, c], v4[:, a], v4[:, c])
    rr = res(up_rows)
    last, first = np.arange(STREAM_BUCKET - 1, x.size - 1, STREAM_BUCKET), np.arange(STREAM_BUCKET, x.size, STREAM_BUCKET)
    z['last of row r, first of row r + 1'] = _z_pairs(rr[last], rr[first], vv[last], vv[first])
    z['call k, k + 1 (seeds S, S + 1)'] = _z_pairs(r, res(up_next), vv, vv)
    z['seeds S, S + 2^32'] = _z_pairs(r, res(up_far), vv, vv)
    return z


def oracle_stream_statistics():
    x, use = stream_input()
    d = [oracle_decisions(s, x) for s in (STREAM_SEED, STREAM_SEED + 1, STREAM_SEED + (1 << 32))]
    return stream_statistics(d[0], d[1], d[2], d[0], x, use)


def library_decisions(lib, seed, x, bucket):
    got = lib.uniform(x, bucket, 2, seed, want_lev=False)
    assert np.all(got['alpha'] == F32(1.0)) and np.all(got['beta'] == F32(0.0))
    assert np.all((got['q'] == 0.0) | (got['q'] == 1.0) | (got['q'] == 2.0))      # (2: the planted 1 under a zero draw)
    return got['q'] >= 1.0


def check_streams(lib):
    x, use = stream_input()
    seeds = (STREAM_SEED, STREAM_SEED + 1, STREAM_SEED + (1 << 32))
    d = [library_decisions(lib, s, x, None) for s in seeds]
    rows = library_decisions(lib, STREAM_SEED, x, STREAM_BUCKET)
    for s, got in zip(seeds + (STREAM_SEED,), d + [rows]):
        assert np.array_equal(got[use], oracle_decisions(s, x)[use]), (lib.kind, hex(s))
    z = stream_statistics(d[0], d[1], d[2], rows, x, use)
    worst = max(z, key=lambda k: abs(z[k]))
    assert abs(z[worst]) <= Z_BOUND, (lib.kind, worst, z[worst])
    return z


def format_statistics(z):
    lines = ['Stochastic rounding: independence of the up / down decisions (tests/stochastic_cases.py: stream_statistics).',
             'Oracle generator (Philox4x32-7), n = 2^18, s = 2, x_i = p_i, seeds S = 0x%X, S + 1, S + 2^32.' % STREAM_SEED,
             'z = statistic / sqrt(exact null variance from the p_i used); the tests bound |z| at %.0f, and |z| > %.0f here'
             % (Z_BOUND, Z_FINDING), 'would be a finding about the generator or the seed schedule.', '']
    lines += ['%-40s z = %+.3f' % (k, v) for k, v in z.items()]
    lines += ['', 'largest |z| = %.3f' % max(abs(v) for v in z.values())]
    return '\n'.join(lines) + '\n'


# ------------------------------------------------------------------------------------------------ through the Python API
def check_api_sequence(device):
    """Two successive calls after torch.manual_seed: the oracle at the seeds next_stochastic_seed announces, different from
    each other, and the same again after the same torch.manual_seed with the call counter where it was."""
    import quantization
    import quantization.quant_functions as qf
    is_host = torch.device(device).type == 'cpu'
    x = np.random.RandomState(77).randn(10007).astype(F32)
    xt = torch.from_numpy(x).to(device)
    runs = []
    start = qf._STOCHASTIC_CALLS[0]
    try:
        for _ in range(2):
            torch.manual_seed(1234)
            qf._STOCHASTIC_CALLS[0] = start
            seq = []
            for call in range(2):
                seed = qf.next_stochastic_seed(peek=True, host=is_host)
                q, _ = quantization.uniformQuantization(xt, 16, bucket_size=256, stochastic_rounding=True)
                assert np.array_equal(q.cpu().numpy(), oracle(x, 16, seed, 256)['q']), (device, call)
                seq.append((seed, q.cpu()))
            assert seq[1][0] == (seq[0][0] + 1) & 0xFFFFFFFFFFFFFFFF and not torch.equal(seq[0][1], seq[1][1])
            runs.append(seq)
    finally:
        qf._STOCHASTIC_CALLS[0] = max(qf._STOCHASTIC_CALLS[0], start + 2)
    for a, b in zip(*runs):
        assert a[0] == b[0] and torch.equal(a[1], b[1]), 'not reproducible after torch.manual_seed'


if __name__ == '__main__':
    print(format_statistics(oracle_stream_statistics()), end='')
