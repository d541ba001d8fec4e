"""The non-finite cases shared by tests/test_hip_nonfinite.py (device), tests/test_nonfinite_host.py (CPU tensors),
tests/test_oracle_golden.py, tests/test_compressed_host.py and tests/test_hip_host_agreement.py: access to
tests/golden/nonfinite_paths.npz (tests/golden/gen_golden.py: run_nonfinite_paths), the inputs it was generated from, a
bit-for-bit comparison that takes a NaN for a NaN, and the model of the compressed-checkpoint cases."""
import numpy as np
import torch

from conftest import load_golden

PATTERNS = ('nan_full', 'nan_last', 'pinf', 'ninf', 'both', 'inf_bucket', 'ends')


def plant(base, pattern, bucket):
    """tests/golden/gen_golden.py: plant_nonfinite, on a numpy copy."""
    x = np.array(base, dtype=np.float32, copy=True)
    n = x.size
    if pattern == 'nan_full':
        x[300] = np.nan
    elif pattern == 'nan_last':
        x[n - 10] = np.nan
    elif pattern == 'pinf':
        x[700] = np.inf
    elif pattern == 'ninf':
        x[1500] = -np.inf
    elif pattern == 'both':
        x[1030], x[1040] = np.inf, -np.inf
    elif pattern == 'inf_bucket':
        row = bucket or 256
        x[2 * row:3 * row] = np.inf
    elif pattern == 'ends':
        x[0], x[n - 1] = np.nan, np.nan
    else:
        raise ValueError(pattern)
    return x


def same(got, want):
    """Bit for bit: equal shapes and values, NaN where NaN is expected, infinities of the expected sign."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    return got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def _bname(bucket):
    return 'b%s' % ('none' if bucket is None else bucket)


def expand(v, bucket, n):
    """Per-bucket values repeated over the elements of their bucket, unpadded."""
    v = np.asarray(v, np.float32).reshape(-1)
    return np.repeat(v, bucket)[:n] if (bucket is not None and n >= bucket) else np.full(n, v[0], np.float32)


class Paths(object):
    """tests/golden/nonfinite_paths.npz.  The file stacks the seven patterns of a (k, bucket) and leaves out what one fp32
    operation per reference op derives from what it holds (the generator checked each against the reference's result):
    q = points[idx] * alpha + beta, and the pre-processed path's indices / values, which equal the plain function's."""

    def __init__(self):
        g = load_golden('nonfinite_paths.npz')
        self.z, self.meta = g.z, g.meta
        self.base, self.g = self.z['base'], self.z['g']
        assert tuple(self.meta['patterns']) == PATTERNS

    def pts(self, k):
        return self.z['pts_k%d' % k]

    def scale(self, i):
        c = self.meta['scale'][i]
        j, b = PATTERNS.index(c['pattern']), _bname(c['bucket'])
        return dict(c, x=plant(self.base, c['pattern'], c['bucket']), u=self.z['u_' + b][j].reshape(c['u_shape']),
                    alpha=self.z['alpha_' + b][j].reshape(c['alpha_shape']), beta=self.z['beta_' + b][j].reshape(c['alpha_shape']),
                    back=self.z['back_' + b][j])

    def nearest(self, i):
        c = self.meta['cases'][i]
        assert 'raises' not in c
        j, b, k = PATTERNS.index(c['pattern']), _bname(c['bucket']), c['k']
        sc = self.scale([(m['bucket'], m['pattern']) for m in self.meta['scale']].index((c['bucket'], c['pattern'])))
        idx = self.z['idx_k%d_%s' % (k, b)][j].astype(np.int64)
        n = idx.size
        with np.errstate(invalid='ignore'):
            q = ((self.pts(k)[idx] * expand(sc['alpha'], c['bucket'], n)).astype(np.float32)
                 + expand(sc['beta'], c['bucket'], n)).astype(np.float32)
        return dict(c, x=sc['x'], pts=self.pts(k), idx=idx, q=q, alpha=sc['alpha'], beta=sc['beta'], gp=self.z['gp_k%d_%s' % (k, b)][j])

    def grad(self, i):
        c = self.meta['grads'][i]
        b = _bname(c['bucket'])
        gg = self.g.copy()
        for pos, v in c['plant']:
            gg[pos] = np.float32(float(v))
        return dict(c, g=gg, idx=self.z['fin_idx_' + b].astype(np.int64), alpha=self.z['fin_alpha_' + b],
                    gp=self.z['fin_gp_' + b][i % 3])


_paths = []


def G():
    if not _paths:
        _paths.append(Paths())
    return _paths[0]


def nonfinite_model():
    """Three tensors: one with a NaN bucket, one with a +inf bucket, one with a -inf bucket (and finite buckets around them)."""
    rng = np.random.RandomState(21)
    a, b, c = (rng.randn(n).astype(np.float32) * 0.1 for n in (3000, 1025, 700))
    a[300], b[1024], c[5] = np.nan, np.inf, -np.inf
    return {'nan': torch.from_numpy(a).view(30, 100), 'pinf': torch.from_numpy(b), 'ninf': torch.from_numpy(c)}
