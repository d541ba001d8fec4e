"""The device-independent non-finite cases of tests/test_hip_nonfinite.py on CPU tensors (libqd_host.so): the goldens of
tests/golden/nonfinite_paths.npz through K4 / K5 / K6, K2 / K3 and K8, the C-ABI cases of K3 and K6, the per-tensor half of
the neighbour-isolation lists and the oracle comparison of K7 -- the same test bodies, `DEV` switched -- and the arg indices
of a bucket that holds a NaN, host library against both oracles and torch."""
import numpy as np
import pytest
import torch

import quantization
import test_hip_nonfinite as N
from nonfinite_cases import G, PATTERNS, plant
from oracle import oracle_c as oc
from oracle import oracle_np as onp
from quantized_distillation_amd import _lib, ste


@pytest.fixture(autouse=True)
def _on_cpu(monkeypatch):
    _lib.host()
    oc.build()
    monkeypatch.setattr(N, 'DEV', 'cpu')


@pytest.mark.parametrize('bucket', [256, 100, None])
@pytest.mark.parametrize('k', [2, 4, 16])
def test_nearest_point_and_point_gradient_goldens(k, bucket):
    N.test_nearest_point_and_point_gradient_goldens(k, bucket)


def test_point_gradient_of_a_finite_tensor_under_a_nonfinite_gradient():
    N.test_point_gradient_of_a_finite_tensor_under_a_nonfinite_gradient()


def test_point_gradient_with_a_nan_bucket_alpha_through_the_c_abi():
    N.test_point_gradient_with_a_nan_bucket_alpha_through_the_c_abi()


@pytest.mark.parametrize('bucket', [256, 100, None])
def test_scale_down_and_inverse_goldens(bucket):
    N.test_scale_down_and_inverse_goldens(bucket)


def test_inverse_scaling_propagates_nonfinite_alpha_beta_and_u():
    N.test_inverse_scaling_propagates_nonfinite_alpha_beta_and_u()


def test_training_loop_epilogues_golden():
    N.test_training_loop_epilogues_golden()


@pytest.mark.parametrize('value', [np.nan, np.inf, -np.inf], ids=['nan', 'pinf', 'ninf'])
@pytest.mark.parametrize('bucket', [256, 100, None])
def test_per_tensor_calls_on_neighbouring_views_are_isolated(bucket, value):
    N.test_per_tensor_calls_on_neighbouring_views_are_isolated(bucket, value)


@pytest.mark.parametrize('value', [np.nan, np.inf, -np.inf], ids=['nan', 'pinf', 'ninf'])
@pytest.mark.parametrize('bucket', [256, 100])
def test_ste_backward_of_the_isolation_lists_against_the_oracle(bucket, value):
    """K7 of the host library on every tensor of the isolation lists through the check the device test applies to K7m."""
    for name, sizes, ti, pos in N.isolation_lists():
        xs = N.isolation_inputs(sizes, 11)
        xs[ti][pos] = value
        gs = N.isolation_inputs(sizes, 12)
        for j, (x, g) in enumerate(zip(xs, gs)):
            out = ste.ste_bucket_backward(torch.from_numpy(x), torch.from_numpy(g), bucket, 16)
            N.check_ste_against_oracle(out.numpy(), x, g, 16, bucket, (name, j))


@pytest.mark.parametrize('bucket', [256, 100, None])
def test_arg_indices_of_a_bucket_that_holds_a_nan(bucket):
    """idx_min_rows / idx_max_rows: a bucket that holds a NaN reports the position of its FIRST NaN for both (torch.min / max
    propagate it) -- the host library, the C oracle at 1 and at several threads, the numpy oracle and torch itself agree.  The
    NaN sits away from the bucket's start, behind the true minimum and maximum, twice in one bucket, and (the golden inputs)
    next to infinities."""
    rng = np.random.RandomState(3)
    inputs = [plant(G().base, pat, bucket) for pat in PATTERNS]
    x = rng.randn(3000).astype(np.float32)
    x[44], x[300 + 7], x[300 + 90], x[2999] = np.nan, np.nan, np.nan, np.nan
    x[10], x[20] = -50.0, 50.0
    inputs += [x, np.array([np.nan, np.inf], np.float32), np.array([1.0, -np.inf, np.nan, np.inf, np.nan], np.float32)]
    big = rng.randn(70001).astype(np.float32)                          # the C oracle's OpenMP path (bucket None)
    big[60000], big[65000] = np.nan, np.nan
    inputs.append(big)
    for x in inputs:
        t = torch.from_numpy(x)
        q, sf = quantization.uniformQuantization(t, 16, bucket_size=bucket)
        imin, imax = sf.idx_min_rows.numpy().reshape(-1), sf.idx_max_rows.numpy().reshape(-1)
        rows = onp.bucketize(x, bucket)
        rows = torch.from_numpy(np.ascontiguousarray(rows)).view(1, -1) if bucket is None else torch.from_numpy(np.ascontiguousarray(rows))
        tmin, tmax = rows.min(dim=1)[1].numpy(), rows.max(dim=1)[1].numpy()
        assert np.array_equal(imin, tmin) and np.array_equal(imax, tmax), (x.size, bucket, imin, tmin)
        with np.errstate(invalid='ignore'):
            r = onp.uniform_quantize(x, 16, bucket)
        assert np.array_equal(r['imin'].reshape(-1), tmin) and np.array_equal(r['imax'].reshape(-1), tmax), (x.size, bucket)
        before = oc.max_threads()
        try:
            for th in (1, 4):
                oc.set_threads(th)
                c = oc.uniform_quantize(x, 16, bucket)
                assert np.array_equal(c['imin'], tmin) and np.array_equal(c['imax'], tmax), (x.size, bucket, th, c['imin'], tmin)
                assert np.array_equal(c['q'], q.numpy(), equal_nan=True)
                assert np.array_equal(oc.scale_down(x, bucket)['imin'], tmin) and np.array_equal(oc.scale_down(x, bucket)['imax'], tmax)
        finally:
            oc.set_threads(before)
        nanrow = np.isnan(rows.numpy()).any(axis=1)
        first = np.isnan(rows.numpy()).argmax(axis=1)
        assert np.array_equal(imin[nanrow], first[nanrow]) and np.array_equal(imax[nanrow], first[nanrow])
