"""GPU parity tests: the HIP path (through the `quantization` API and the C ABI) against the
golden vectors produced by the reference and against the CPU oracle.

Bar: bit-exact for q, alpha, beta, arg indices, level indices and point indices; tolerance only
where an fp32 summation order is involved (mean, point gradient, 'complicated' STE sum)."""
import os

import numpy as np
import pytest
import torch

import quantization
import quantization.help_functions as qhf
from oracle import oracle_c as oc
from oracle import oracle_np as onp
from quantized_distillation_amd import _lib

import errlog

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    _lib.load()
    oc.build()


def level_flips(q, q_ref, alpha_ref, s, bucket):
    """(number of elements of q that sit on another quantization level than q_ref, largest |q - q_ref| among the others).
    Two outputs of the same element differ by a last-bit effect (the mean's rounding, carried through x - m + m) or by a
    whole level, alpha / (s - 1): half a level separates the two."""
    q, q_ref = np.asarray(q, np.float64).reshape(-1), np.asarray(q_ref, np.float64).reshape(-1)
    a = np.asarray(alpha_ref, np.float64).reshape(-1)
    n = q.size
    per_elem = np.repeat(a, bucket)[:n] if (bucket is not None and n >= bucket and a.size > 1) else np.full(n, a[0])
    d = np.abs(q - q_ref)
    flipped = d > 0.5 * per_elem / (s - 1)
    rest = d[~flipped]
    return int(flipped.sum()), float(rest.max()) if rest.size else 0.0


def test_subtract_mean_where_the_last_bit_of_the_mean_flips_levels():
    """subtract_mean=True (ref: quant_functions.py:66-70,148) on inputs where every element sits on a rounding boundary of the
    level computation (tests/golden/gen_golden.py run_mean_options).  The reference's mean is torch's fp32 CPU sum, which
    changes with the thread count (the golden holds its runs at 1 / 2 / 4 / 8 threads: up to 4 distinct means per case, and
    outputs that differ from EACH OTHER by whole levels on thousands of elements).  So there is no reference bit pattern to
    hit; what is defined and checked: the device mean is the correctly rounded mean, the output is bit-identical to the
    oracle given that mean, the oracle given any of the reference's means reproduces that reference run bit for bit
    (tests/test_oracle_golden.py), and where the device's mean EQUALS one of the reference's, so does the output."""
    import conftest
    G = conftest.load_golden('mean_options.npz')
    equal_runs = flips_seen = 0
    for i, c in enumerate(G.meta):
        x = G.arr('m', i, 'x')
        q, sf = quantization.uniformQuantization(dev(x), c['s'], bucket_size=c['bucket'], subtract_mean=True)
        m = np.float32(float(sf.mean_tensor))
        assert m == np.float32(x.astype(np.float64).sum() / x.size), (i, c)
        ref = onp.uniform_quantize(x, c['s'], c['bucket'], False, True, mean=float(m))
        assert np.array_equal(host(q), ref['q']) and np.array_equal(host(sf.alpha).reshape(-1), ref['alpha'].reshape(-1)), (i, c)
        for th in c['q_stored_for_threads']:
            m_ref = np.float32(c['mean_by_threads'][str(th)])
            q_ref = G.arr('m', i, 'q_t%d' % th)
            if m_ref == m:
                equal_runs += 1
                assert np.array_equal(host(q), q_ref), (i, th)
            else:
                flips, worst = level_flips(host(q), q_ref, host(sf.alpha), c['s'], c['bucket'])
                flips_seen += flips
                assert worst <= 1e-6 * float(np.abs(x).max()), (i, th, worst)
                assert abs(float(m) - float(m_ref)) <= 8 * np.spacing(np.float32(abs(m))), (i, th)     # the reference's means: 1-4 ulps around it
    assert equal_runs >= 3                        # some reference runs do land on the correctly rounded mean
    assert flips_seen > 0                         # ... and the others differ by whole levels: the cases are adversarial


# ------------------------------------------------------------------------------ uniform (K1/K1g/K2/K3)
def test_uniform_golden(golden_uniform):
    G = golden_uniform
    for i, c in enumerate(G.meta):
        x = G.arr('u', i, 'x')
        tag = 'case %d %r' % (i, c)
        xd = dev(x)
        q, sf = quantization.uniformQuantization(xd, c['s'], bucket_size=c['bucket'], max_element=c['max_element'],
                                                 subtract_mean=c['subtract_mean'])
        assert torch.equal(xd.cpu(), torch.from_numpy(x)), 'input modified: ' + tag
        assert q.shape == xd.shape and q.dtype == torch.float32 and q.device == xd.device
        assert list(sf.expected_tensor_size) == c['expected_tensor_size'], tag
        assert sf.original_tensor_length == c['original_tensor_length'] and tuple(sf.original_tensor_size) == x.shape
        assert tuple(sf.alpha.shape) == G.arr('u', i, 'alpha').shape, tag
        if c['subtract_mean']:
            m = float(sf.mean_tensor)
            errlog.check_mean('qd_mean_f32 vs the reference fp32 mean (golden)', m, c['mean'], float(np.abs(x).mean()), tag, n_terms=x.size)
            # the device mean is the correctly rounded one (float64 accumulation, one rounding); the reference's fp32 sum is
            # 0-2 ulps away from it depending on torch's thread count (tests/golden/mean_options.npz)
            assert np.float32(m) == np.float32(x.astype(np.float64).sum() / x.size), tag
            # everything downstream of the mean is bit-exact given the mean the device computed
            ref = onp.uniform_quantize(x, c['s'], c['bucket'], c['max_element'], True, mean=m)
            assert np.array_equal(host(q), ref['q']), tag
            assert np.array_equal(host(sf.alpha).reshape(-1), ref['alpha'].reshape(-1)), tag
            # ... and DIRECTLY against the reference's output: no element on another level, values within 1e-6 max|x|
            flips, worst = level_flips(host(q), G.arr('u', i, 'q'), G.arr('u', i, 'alpha'), c['s'], c['bucket'])
            assert flips == 0, (tag, 'elements on another level than the reference put them', flips)
            assert worst <= 1e-6 * float(np.abs(x).max()), (tag, worst)
            continue
        assert np.array_equal(host(q), G.arr('u', i, 'q')), tag
        assert np.array_equal(host(sf.alpha), G.arr('u', i, 'alpha')), tag
        assert np.array_equal(host(sf.beta), G.arr('u', i, 'beta')), tag
        assert np.array_equal(host(sf.idx_min_rows), G.arr('u', i, 'imin')), tag
        assert np.array_equal(host(sf.idx_max_rows), G.arr('u', i, 'imax')), tag
        assert sf.idx_min_rows.dtype == torch.int64


def test_scale_down_and_inverse_golden(golden_uniform):
    G = golden_uniform
    for i, c in enumerate(G.meta):
        if c['subtract_mean']:
            continue
        x = G.arr('u', i, 'x')
        sf = quantization.ScalingFunction('linear', c['max_element'], False, c['bucket'])
        u = sf.scale_down(dev(x))
        tag = 'case %d %r' % (i, c)
        assert np.array_equal(host(u), G.arr('u', i, 'u')), tag            # padded bucket layout, bit-exact
        assert np.array_equal(host(sf.alpha), G.arr('u', i, 'alpha')), tag
        assert np.array_equal(host(sf.idx_max_rows), G.arr('u', i, 'imax')), tag
        back = sf.inv_scale_down(u)
        ref = onp.inv_scale_down(G.arr('u', i, 'u'), G.arr('u', i, 'alpha'), G.arr('u', i, 'beta'), 0.0, x.size, x.shape)
        assert np.array_equal(host(back), ref), tag
        with pytest.raises(ValueError):
            sf.inv_scale_down(torch.zeros(u.numel() + 1, device=DEV))


def test_roundtrip_golden(golden_misc):
    G = golden_misc
    for i, c in enumerate(G.meta['roundtrip']):
        sf = quantization.ScalingFunction('linear', False, False, c['bucket'])
        u = sf.scale_down(dev(G.z['rt%d_x' % i]))
        assert np.array_equal(host(u), G.z['rt%d_u' % i])
        assert np.array_equal(host(sf.inv_scale_down(u)), G.z['rt%d_back' % i])


def test_level_index_output_via_c_abi(golden_uniform):
    """The integer path: uint8 level index rint(u*(s-1)) straight from the C ABI, bit-exact."""
    G = golden_uniform
    lib = _lib.load()
    for i, c in enumerate(G.meta):
        if c['subtract_mean'] or c['max_element'] is not False or c['s'] > 256:
            continue
        x = G.arr('u', i, 'x')
        n = x.size
        xd = dev(x).view(-1)
        q = torch.empty_like(xd)
        lev = torch.full((n + 3,), 255, dtype=torch.uint8, device=DEV)[:n]
        ws = _lib.workspace(xd.device)
        _lib.check(lib.qd_uniform_f32(xd.data_ptr(), q.data_ptr(), n, c['bucket'] or 0, c['s'], None, None,
                                      lev.data_ptr(), None, 0, 0.0, 0, 0, ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
        want = G.arr('u', i, 'lev').reshape(-1)[:n]
        assert np.array_equal(host(lev).astype(np.int32), want), (i, c)
        assert np.array_equal(host(q), G.arr('u', i, 'q').reshape(-1)), (i, c)


def test_modify_in_place_and_views():
    x = torch.randn(5000, generator=torch.Generator().manual_seed(3))
    ref = onp.uniform_quantize(x.numpy(), 16, 256)['q']
    xd = x.to(DEV)
    q, sf = quantization.uniformQuantization(xd, 16, bucket_size=256, modify_in_place=True)
    assert q.data_ptr() == xd.data_ptr() and np.array_equal(host(xd), ref)
    # arg indices were taken before the overwrite
    assert np.array_equal(host(sf.idx_min_rows).reshape(-1), onp.scale_down(x.numpy(), 256)['imin'].reshape(-1))
    # misaligned view (4-byte aligned base): generic path
    big = torch.zeros(5001, device=DEV)
    big[1:] = x.to(DEV)
    q, _ = quantization.uniformQuantization(big[1:], 16, bucket_size=256)
    assert np.array_equal(host(q), ref)
    q, _ = quantization.uniformQuantization(big[1:], 16)
    assert np.array_equal(host(q), onp.uniform_quantize(x.numpy(), 16, None)['q'])
    # non-contiguous input is accepted (made contiguous)
    m = torch.randn(64, 48, generator=torch.Generator().manual_seed(4))
    q, _ = quantization.uniformQuantization(m.to(DEV).t(), 4, bucket_size=256)
    assert np.array_equal(host(q), onp.uniform_quantize(m.t().contiguous().numpy(), 4, 256)['q'])
    # empty tensor
    q, sf = quantization.uniformQuantization(torch.empty(0, device=DEV), 16, bucket_size=256)
    assert q.numel() == 0


@pytest.mark.parametrize('bucket', [256, 1024, 100, 33, 250, 513, 1000, 5000, None])
def test_nonuniform_modify_in_place_on_every_kernel_family(bucket):
    """nonUniformQuantization(modify_in_place=True): the kernel writes over its input (round 2 quantized out of place and
    copied back: +8 B/element) -- vector, chunk, chunk_any, one-wave-per-bucket and single-bucket kernels, ragged tails,
    a tensor small enough for the one-launch single-bucket kernel (which in-place calls must not take): values and int64
    indices bit-identical to the out-of-place call and to the C oracle, arg indices taken before the overwrite.
    ref: quant_functions.py:243-290."""
    rng = np.random.RandomState(11 + (bucket or 0))
    pts = np.array([0.0, 0.25, 0.6, 1.0], np.float32)
    for n in (70001, 300000 + 3, 1 << 20):
        x = rng.randn(n).astype(np.float32)
        want = oc.nonuniform_quantize(x, pts, bucket)
        xd = dev(x)
        q0, i0, sf0 = quantization.nonUniformQuantization(xd, dev(pts), bucket_size=bucket)
        assert np.array_equal(host(xd), x), 'out of place: the input is untouched'
        imin0, imax0 = sf0.idx_min_rows.clone(), sf0.idx_max_rows.clone()          # (lazy: read before xd is overwritten)
        q1, i1, sf1 = quantization.nonUniformQuantization(xd, dev(pts), bucket_size=bucket, modify_in_place=True)
        assert q1.data_ptr() == xd.data_ptr()
        assert np.array_equal(host(q1), want['q']) and np.array_equal(host(i1), want['idx']), (bucket, n)
        assert torch.equal(q0, q1) and torch.equal(i0, i1)
        assert torch.equal(sf0.alpha, sf1.alpha) and torch.equal(sf0.beta, sf1.beta)
        assert torch.equal(imin0, sf1.idx_min_rows) and torch.equal(imax0, sf1.idx_max_rows)
    with pytest.raises(ValueError):
        quantization.nonUniformQuantization(dev(rng.randn(64, 48).astype(np.float32)).t(), dev(pts), bucket_size=bucket, modify_in_place=True)


@pytest.mark.parametrize('bucket', [64, 128, 256, 512, 1024, 2048, 4096, 100, 3, None])
def test_uniform_random_sweep_vs_c_oracle(bucket):
    rng = np.random.RandomState(11)
    for n in (1, 63, 64, 1000, 4097, 70001, 262144 + 5):
        for s in (2, 16, 256):
            x = (rng.randn(n) * rng.choice([0.05, 1.0, 30.0])).astype(np.float32)
            q, sf = quantization.uniformQuantization(dev(x), s, bucket_size=bucket)
            r = oc.uniform_quantize(x, s, bucket)
            assert np.array_equal(host(q), r['q']), (n, s, bucket)
            assert np.array_equal(host(sf.alpha).reshape(-1), r['alpha']), (n, s, bucket)
            assert np.array_equal(host(sf.beta).reshape(-1), r['beta']), (n, s, bucket)
            assert np.array_equal(host(sf.idx_min_rows).reshape(-1), r['imin']), (n, s, bucket)
            assert np.array_equal(host(sf.idx_max_rows).reshape(-1), r['imax']), (n, s, bucket)


@pytest.mark.parametrize('bucket', [33, 50, 7, 250, 511, 100, 1000, 513])
def test_uniform_chunk_kernels_many_chunks_per_wave(bucket):
    """16.7 M elements: many chunks per LAUNCH -- thousands of blocks of the chunk kernels, more than are resident at once --
    stochastic branch too (the draw is indexed by element).  Not several chunks per wave: the grid has a wave per chunk (bucket
    33: about 4 237 blocks for 8 473 chunks), so each wave's loop runs once here; the later trips of that loop are
    tests/test_hip_grid_trips.py's, under qd_set_grid_cap."""
    n = (1 << 24) + 12345
    x = (torch.randn(n, generator=torch.Generator().manual_seed(bucket)) * 0.3).numpy()
    q, sf = quantization.uniformQuantization(dev(x), 16, bucket_size=bucket)
    r = oc.uniform_quantize(x, 16, bucket)
    assert np.array_equal(host(q), r['q'])
    assert np.array_equal(host(sf.alpha).reshape(-1), r['alpha']) and np.array_equal(host(sf.beta).reshape(-1), r['beta'])
    seed = quantization.quant_functions.next_stochastic_seed(peek=True)
    qs, _ = quantization.uniformQuantization(dev(x), 16, bucket_size=bucket, stochastic_rounding=True)
    rand = np.zeros(onp.bucket_geometry(n, bucket)[2], np.float32)
    rand[:n] = onp.philox4x32_7_uniform(seed, n)
    want = onp.uniform_quantize_stochastic(x, 16, rand, bucket)
    assert np.array_equal(host(qs), want['q'])


@pytest.mark.parametrize('bucket', [257, 300, 449, 511, 513, 600, 770, 1000, 1001, 1023, 1500, 1700, 2000, 2049, 3000, 3500, 4093, 5000,
                                    6000, 6145, 8000, 8190, 8200, 10001, 16384, 20000, 32768, 32769])
def test_uniform_wave_per_bucket_any_size(bucket):
    """Bucket sizes above 256 that are not one of the vector sizes: one wave per bucket on the aligned float4s that touch
    it (k_bucket_wave_any).  Tensor ends at, just after and well after a bucket boundary (the last buckets go to the tail
    path when their final float4 would cross the end of the tensor); deterministic, stochastic, clamp + mean, level
    indices; q, alpha, beta bit-exact against the C oracle."""
    from quantized_distillation_amd import codec
    rng = np.random.RandomState(bucket)
    for extra in (0, 1, 2, 3, bucket // 2, bucket - 1):
        n = bucket * 37 + extra
        x = (rng.randn(n) * rng.choice([0.05, 1.0, 30.0])).astype(np.float32)
        for s_ in (16, 256):
            q, sf = quantization.uniformQuantization(dev(x), s_, bucket_size=bucket)
            r = oc.uniform_quantize(x, s_, bucket)
            assert np.array_equal(host(q), r['q']), (n, s_)
            assert np.array_equal(host(sf.alpha).reshape(-1), r['alpha']) and np.array_equal(host(sf.beta).reshape(-1), r['beta'])
            assert np.array_equal(host(sf.idx_min_rows).reshape(-1), r['imin']), (n, s_)
    n = bucket * 301 + 2
    x = rng.randn(n).astype(np.float32)
    x[5] = np.nan                                                    # poisons bucket 0 only
    xd = dev(x)
    q, sf = quantization.uniformQuantization(xd, 16, bucket_size=bucket)
    r = oc.uniform_quantize(x, 16, bucket)
    assert np.array_equal(host(q), r['q'], equal_nan=True) and np.array_equal(host(sf.alpha).reshape(-1), r['alpha'], equal_nan=True)
    x[5] = 0.25
    xd = dev(x)
    seed = quantization.quant_functions.next_stochastic_seed(peek=True)
    qs, _ = quantization.uniformQuantization(xd, 16, bucket_size=bucket, stochastic_rounding=True)
    rand = np.zeros(onp.bucket_geometry(n, bucket)[2], np.float32)
    rand[:n] = onp.philox4x32_7_uniform(seed, n)
    assert np.array_equal(host(qs), onp.uniform_quantize_stochastic(x, 16, rand, bucket)['q'])
    q, sf = quantization.uniformQuantization(xd, 4, bucket_size=bucket, max_element=0.7, subtract_mean=True)
    r = onp.uniform_quantize(x, 4, bucket, 0.7, True, mean=float(sf.mean_tensor))
    assert np.array_equal(host(q), r['q']) and np.array_equal(host(sf.alpha).reshape(-1), r['alpha'].reshape(-1))
    h = codec.level_histogram(xd, 16, bucket)
    assert np.array_equal(host(h), np.bincount(oc.uniform_quantize(x, 16, bucket)['lev'], minlength=16))


def test_few_buckets_of_a_large_bucket_size():
    """Tensors with too few buckets to fill one chunk of the chunk kernels fall through to the lane-group kernels
    (k_bucket_groups<MODE, 64>: a wave per bucket, two passes): every mode, bit-exact against the C oracle."""
    rng = np.random.RandomState(77)
    pts = np.array([0.0, 0.25, 0.7, 1.0], np.float32)
    for n, bucket in ((700, 300), (900, 400), (1300, 260), (1001, 500)):
        x = rng.randn(n).astype(np.float32)
        xd = dev(x)
        for s_ in (16, 4):
            q, sf = quantization.uniformQuantization(xd, s_, bucket_size=bucket)
            r = oc.uniform_quantize(x, s_, bucket)
            assert np.array_equal(host(q), r['q']) and np.array_equal(host(sf.alpha).reshape(-1), r['alpha']), (n, bucket, s_)
        sfn = quantization.ScalingFunction('linear', False, False, bucket)
        u = sfn.scale_down(xd)
        assert np.array_equal(host(u).reshape(-1)[:n], oc.scale_down(x, bucket)['u']), (n, bucket)
        qn, idx, _ = quantization.nonUniformQuantization(xd, dev(pts), bucket_size=bucket)
        rn = oc.nonuniform_quantize(x, pts, bucket)
        assert np.array_equal(host(qn), rn['q']) and np.array_equal(host(idx), rn['idx']), (n, bucket)


@pytest.mark.parametrize('bucket', [33, 255, 300, 506, 509, 511, 513, 1000, 1001, 1017, 1023, 2000, 2048, 3001, 4000, 4096, 5000, 8190, 12000,
                                    30000])
def test_other_modes_at_chunk_sizes(bucket):
    """scale_down and nonUniformQuantization at bucket sizes of the chunk kernels (with and without the lead-in to the
    128-byte line): bit-exact against the C oracle."""
    rng = np.random.RandomState(bucket)
    for n in (bucket * 41 + 3, bucket * 64, bucket * 300 + bucket // 2, bucket * 7 + 1):
        x = rng.randn(n).astype(np.float32)
        xd = dev(x)
        pts = np.array([0.0, 0.3, 0.6, 1.0], np.float32)
        q, idx, sf = quantization.nonUniformQuantization(xd, dev(pts), bucket_size=bucket)
        r = oc.nonuniform_quantize(x, pts, bucket)
        assert np.array_equal(host(q), r['q']) and np.array_equal(host(idx), r['idx']), (bucket, n)
        sfn = quantization.ScalingFunction('linear', False, False, bucket)
        u = sfn.scale_down(xd)
        r2 = oc.scale_down(x, bucket)
        assert np.array_equal(host(u).reshape(-1)[:n], r2['u']), (bucket, n)
        assert np.array_equal(host(sfn.alpha).reshape(-1), r2['alpha']), (bucket, n)
        if n % bucket:                                               # padding = the scaled last element
            assert np.all(host(u).reshape(-1)[n:] == host(u).reshape(-1)[n - 1])
        # K3 at the same bucket size (float4 stream with a per-element bucket choice): bit-exact against the oracle's
        # inverse of the oracle's u
        back = sfn.inv_scale_down(u)
        nbk = -(-n // bucket)
        u_pad = np.concatenate([r2['u'], np.full(nbk * bucket - n, r2['u'][-1], np.float32)]).reshape(nbk, bucket)
        want_back = onp.inv_scale_down(u_pad, r2['alpha'].reshape(nbk, 1), r2['beta'].reshape(nbk, 1), 0.0, n, (n,))
        assert np.array_equal(host(back).reshape(-1), np.asarray(want_back, np.float32).reshape(-1)), (bucket, n, 'inv_scale_down')
        # the pre-processed forward (u resident, midpoint rule, 64 points: the grid-narrowed search) and the point gradient
        pts64 = np.sort(rng.rand(64)).astype(np.float32)
        fn = quantization.nonUniformQuantization_variable(bucket_size=bucket, pre_process_tensors=True, tensor=xd)
        qm = fn.forward(None, dev(pts64))
        rm = oc.nonuniform_quantize(x, pts64, bucket, 'midpoint')
        assert np.array_equal(host(qm), rm['q']) and np.array_equal(host(fn.savedForBackward['indices']), rm['idx']), (bucket, n)
        g = rng.randn(n).astype(np.float32)
        _, gp = fn.backward(dev(g))
        want, absum = oc.point_grad(g, rm['idx'], rm['alpha'], bucket, 64)
        errlog.check_sum('K6 point gradient, any-bucket-size kernel (k = 64)', host(gp), want, absum, (bucket, n), n_terms=n)
        assert torch.equal(gp, fn.backward(dev(g))[1]), 'same inputs, same bits (no atomics on any K6 path)'


@pytest.mark.parametrize('off', [1, 2, 3])
def test_views_at_every_4_byte_offset(off):
    """Tensor views that start 4, 8 or 12 bytes into a 16-byte granule (x[1:], x[2:], x[3:] of an allocation) go through the
    same 16-byte-access kernels as aligned tensors -- the hardware needs dword alignment only -- and give the same bits as
    the oracle and as the same call on an aligned copy: every kernel family of uniformQuantization (vector, chunk,
    chunk_any, one-wave-per-bucket, no buckets small / large), stochastic rounding, in place on the misaligned view,
    scale_down + inverse, nonUniformQuantization, the pre-processed forward + point gradient, the bucket-aware STE, clamp /
    truncated-STE."""
    from quantized_distillation_amd import ste
    import quantization.quant_functions as qf
    rng = np.random.RandomState(off)

    def view(a):
        buf = torch.empty(a.size + 8, dtype=torch.float32, device=DEV)
        v = buf[off:off + a.size]
        v.copy_(torch.from_numpy(a))
        assert v.data_ptr() % 16 == 4 * off
        return v

    for bucket in (256, 64, 1024, 100, 33, 7, 1000, 513, 5000, None):
        for n in ((70001, 1 << 21) if bucket in (256, None) else (70001,)):
            x = rng.randn(n).astype(np.float32)
            g = rng.randn(n).astype(np.float32)
            xd, xa, gd, ga = view(x), dev(x), view(g), dev(g)
            assert xa.data_ptr() % 16 == 0
            tag = (off, bucket, n)
            q, sf = quantization.uniformQuantization(xd, 16, bucket_size=bucket)
            r = oc.uniform_quantize(x, 16, bucket)
            assert np.array_equal(host(q), r['q']), tag
            assert np.array_equal(host(sf.alpha).reshape(-1), r['alpha']) and np.array_equal(host(sf.idx_min_rows).reshape(-1), r['imin']), tag
            qf._STOCHASTIC_CALLS[0] = 1000 + n % 97                      # the same draws for both calls
            qs, _ = quantization.uniformQuantization(xd, 16, bucket_size=bucket, stochastic_rounding=True)
            qf._STOCHASTIC_CALLS[0] = 1000 + n % 97
            qs_a, _ = quantization.uniformQuantization(xa, 16, bucket_size=bucket, stochastic_rounding=True)
            assert torch.equal(qs, qs_a) and not torch.equal(qs, q), tag
            y = view(x)                                                   # in place on a misaligned view
            qi, _ = quantization.uniformQuantization(y, 16, bucket_size=bucket, modify_in_place=True)
            assert qi.data_ptr() == y.data_ptr() and np.array_equal(host(y), r['q']), tag
            sfn, sfa = (quantization.ScalingFunction('linear', False, False, bucket) for _ in range(2))
            u, ua = sfn.scale_down(xd), sfa.scale_down(xa)
            assert torch.equal(u, ua) and np.array_equal(host(u).reshape(-1)[:n], oc.scale_down(x, bucket)['u']), tag
            assert torch.equal(sfn.inv_scale_down(u), sfa.inv_scale_down(ua)), tag
            pts = np.sort(rng.rand(8)).astype(np.float32)
            qn, idx, _ = quantization.nonUniformQuantization(xd, dev(pts), bucket_size=bucket)
            rn = oc.nonuniform_quantize(x, pts, bucket)
            assert np.array_equal(host(qn), rn['q']) and np.array_equal(host(idx), rn['idx']), tag
            fn = quantization.nonUniformQuantization_variable(bucket_size=bucket, pre_process_tensors=True, tensor=xd)
            fa = quantization.nonUniformQuantization_variable(bucket_size=bucket, pre_process_tensors=True, tensor=xa)
            qm, qma = fn.forward(None, dev(pts)), fa.forward(None, dev(pts))
            assert torch.equal(qm, qma) and np.array_equal(host(qm), oc.nonuniform_quantize(x, pts, bucket, 'midpoint')['q']), tag
            gp, gpa = fn.backward(gd)[1], fa.backward(ga)[1]
            wantv, absv = oc.point_grad(g, oc.nonuniform_quantize(x, pts, bucket, 'midpoint')['idx'],
                                        oc.nonuniform_quantize(x, pts, bucket, 'midpoint')['alpha'], bucket, len(pts))
            errlog.check_sum('K6 point gradient on a view at a 4-byte offset', host(gp), wantv, absv, tag, n_terms=g.size)
            errlog.check_sum('K6 point gradient (aligned twin of the view)', host(gpa), wantv, absv, tag, n_terms=g.size)
            if bucket is not None:
                assert torch.equal(ste.ste_bucket_backward(xd, gd, bucket, 16), ste.ste_bucket_backward(xa, ga, bucket, 16)), tag
    w = rng.randn(50001).astype(np.float32) * 1.5
    g = rng.randn(50001).astype(np.float32)
    wd, gd = view(w), view(g)
    ste.truncated_ste_(gd, wd)
    assert np.array_equal(host(gd), np.where(np.abs(w) > 1, 0.0, g).astype(np.float32))
    ste.clamp_(wd)
    assert np.array_equal(host(wd), np.clip(w, -1, 1))


def test_uniform_big_checksums_from_reference(golden_big):
    for c in golden_big:
        if c['op'] != 'uniform':
            continue
        x = torch.randn(c['n'], generator=torch.Generator().manual_seed(c['seed']))
        q, _ = quantization.uniformQuantization(x.to(DEV), c['s'], bucket_size=c['bucket'])
        qh = host(q)
        s1, s2 = oc.checksum(qh)
        assert abs(s1 - c['sum_q']) <= 1e-9 * c['sum_q2'] and abs(s2 - c['sum_q2']) <= 1e-9 * c['sum_q2'], c
        assert [float(v) for v in qh[:5]] == c['q_head'] and [float(v) for v in qh[-3:]] == c['q_tail']


def test_headline_size_properties_and_oracle():
    """BASELINE.json's workload: 64 Mi fp32, 4-bit, bucket 256.  Full bit-exact comparison with
    the C oracle plus size-independent properties (idempotence, level membership)."""
    n = 64 * 1024 * 1024
    x = torch.randn(n, generator=torch.Generator().manual_seed(0))
    xd = x.to(DEV)
    q, sf = quantization.uniformQuantization(xd, 16, bucket_size=256)
    q2, _ = quantization.uniformQuantization(q, 16, bucket_size=256)
    assert torch.equal(q, q2), 'Q(Q(x)) != Q(x)'
    # every output is one of the 16 levels of its bucket: (q - beta)/alpha*15 is an integer
    lev = torch.round((q.view(-1, 256) - sf.beta) / sf.alpha * 15)
    assert float(lev.min()) == 0.0 and float(lev.max()) == 15.0
    assert torch.equal(q.view(-1, 256).min(dim=1, keepdim=True)[0], sf.beta)
    r = oc.uniform_quantize(x.numpy(), 16, 256, want_idx=False, want_lev=False)
    assert np.array_equal(host(q), r['q'])
    assert np.array_equal(host(sf.alpha).reshape(-1), r['alpha'])
    # same tensor without buckets, and a ragged length
    qg, _ = quantization.uniformQuantization(xd, 16)
    assert np.array_equal(host(qg), oc.uniform_quantize(x.numpy(), 16, None, want_idx=False, want_lev=False)['q'])
    xr = xd[:n - 239]
    qr, _ = quantization.uniformQuantization(xr, 4, bucket_size=256)
    assert np.array_equal(host(qr), oc.uniform_quantize(x.numpy()[:n - 239], 4, 256, want_idx=False, want_lev=False)['q'])


def test_stochastic_rounding_statistics():
    """In-kernel counter-based RNG cannot be bit-matched to torch's host RNG (the reference draws
    torch.rand on the host, quant_functions.py:185-186): check the statistics instead."""
    torch.manual_seed(5)
    n = 1 << 20
    x = torch.rand(n, generator=torch.Generator().manual_seed(6))
    x[0], x[1] = 0.0, 1.0
    xd = x.to(DEV)
    s = 4
    q, _ = quantization.uniformQuantization(xd, s, stochastic_rounding=True)
    qh, xh = host(q).astype(np.float64), x.numpy().astype(np.float64)
    t = xh * (s - 1)
    lo, hi = np.floor(t) / (s - 1), np.ceil(t) / (s - 1)
    assert np.all((np.abs(qh - lo) < 1e-6) | (np.abs(qh - hi) < 1e-6)), 'not one of the two neighbouring levels'
    assert abs((qh - xh).mean()) < 3e-4, 'stochastic rounding must be unbiased'
    up = np.abs(qh - hi) < 1e-6
    frac = t - np.floor(t)
    sel = (frac > 0.2) & (frac < 0.3)
    assert abs(up[sel].mean() - frac[sel].mean()) < 0.01
    q2, _ = quantization.uniformQuantization(xd, s, stochastic_rounding=True)
    assert not torch.equal(q, q2), 'successive calls must use different random streams'
    qb, _ = quantization.uniformQuantization(xd, s, stochastic_rounding=True, bucket_size=256)
    assert abs((host(qb).astype(np.float64) - xh).mean()) < 3e-4


def test_stochastic_rounding_bit_exact_on_every_kernel_path():
    """The stochastic branch is defined by (seed, element index) only, so every kernel path -- vector, chunk,
    chunk_any, lane-group, block-per-bucket, single bucket -- must produce the same bits as the oracle's
    restatement of the reference formula (quant_functions.py:174-187) fed with the generator's draws."""
    import quantization.quant_functions as qf
    rng = np.random.RandomState(11)
    cases = [(10007, 256, 16), (10007, 64, 4), (10007, 100, 16), (10007, 33, 4), (10007, 7, 16), (10007, 1000, 4),
             (70001, 2048, 16), (70001, 4096, 4), (70001, 20000, 16), (10007, None, 16), (300001, None, 4),
             (10007, 3, 4), (10007, 513, 16), (4096, 128, 2), (50, 256, 16)]
    for n, bucket, s in cases:
        x = rng.randn(n).astype(np.float32)
        seed = qf.next_stochastic_seed(peek=True)
        q, sf = quantization.uniformQuantization(dev(x), s, stochastic_rounding=True, bucket_size=bucket)
        draws = onp.philox4x32_7_uniform(seed, n)
        nb, row, padded = onp.bucket_geometry(n, bucket)
        rand = np.zeros(padded, np.float32)
        rand[:n] = draws
        want = onp.uniform_quantize_stochastic(x, s, rand, bucket)
        assert np.array_equal(host(q), want['q']), (n, bucket, s)
        assert np.array_equal(host(sf.alpha).reshape(-1), want['alpha'].reshape(-1)), (n, bucket, s)


# ------------------------------------------------------------------------------ non-uniform (K4/K5/K6)
def test_nonuniform_golden(golden_nonuniform):
    G = golden_nonuniform
    for i, c in enumerate(G.meta):
        x, pts = G.arr('n', i, 'x'), G.arr('n', i, 'pts')
        tag = 'case %d %r' % (i, c)
        xd = dev(x)
        q, idx, sf = quantization.nonUniformQuantization(xd, dev(pts), bucket_size=c['bucket'])
        assert idx.dtype == torch.int64 and idx.shape == xd.shape
        assert np.array_equal(host(idx), G.arr('n', i, 'idx')), tag
        assert np.array_equal(host(q), G.arr('n', i, 'q')), tag
        assert np.array_equal(host(sf.alpha), G.arr('n', i, 'alpha')), tag
        # list of python floats and CPU tensor of points are accepted too
        q_l, idx_l, _ = quantization.nonUniformQuantization(xd, [float(v) for v in pts], bucket_size=c['bucket'])
        assert torch.equal(q_l, q) and torch.equal(idx_l, idx)
        # the one-byte index form (index_dtype=torch.uint8, an opt-in): same values, same indices after .long()
        if c['k'] <= 256:
            q8, idx8, sf8 = quantization.nonUniformQuantization(xd, dev(pts), bucket_size=c['bucket'], index_dtype=torch.uint8)
            assert idx8.dtype == torch.uint8 and idx8.shape == xd.shape, tag
            assert torch.equal(idx8.long(), idx) and torch.equal(q8, q) and torch.equal(sf8.alpha, sf.alpha), tag
        # pre-processed variable: midpoint rule, first and second query, gradients
        fn = quantization.nonUniformQuantization_variable(bucket_size=c['bucket'], pre_process_tensors=True, tensor=xd)
        qp = fn.forward(None, dev(pts))
        assert np.array_equal(host(qp), G.arr('n', i, 'q_pre')), tag
        assert np.array_equal(host(fn.savedForBackward['indices']), G.arr('n', i, 'idx_pre')), tag
        assert fn.savedForBackward['indices'].dtype == torch.int64 and fn.savedForBackward['numPoints'] == c['k']
        g = G.arr('n', i, 'g')
        gin, gp = fn.backward(dev(g))
        assert gin.data_ptr() == gin.data_ptr() and np.array_equal(host(gin), g)
        want, absum = onp.point_grad(g, G.arr('n', i, 'idx_pre'), G.arr('n', i, 'alpha'), c['bucket'], c['k'])
        errlog.check_sum('K6 point gradient vs float64 oracle (golden cases)', host(gp), want, absum, tag, n_terms=g.size)
        errlog.check_sum("K6 point gradient vs the reference's own fp32 gradPointTensor (golden)", host(gp), G.arr('n', i, 'gp'), absum, tag,
                         n_terms=g.size)
        qp2 = fn.forward(None, dev(G.arr('n', i, 'pts2')))
        assert np.array_equal(host(qp2), G.arr('n', i, 'q_pre2')), tag
        assert np.array_equal(host(fn.savedForBackward['indices']), G.arr('n', i, 'idx_pre2')), tag
        # non-preprocessed variable = the plain function
        fn2 = quantization.nonUniformQuantization_variable(bucket_size=c['bucket'])
        assert torch.equal(fn2.forward(xd, dev(pts)), q)
        _, gp2 = fn2.backward(dev(g))
        want2, absum2 = onp.point_grad(g, G.arr('n', i, 'idx'), G.arr('n', i, 'alpha'), c['bucket'], c['k'])
        errlog.check_sum('K6 point gradient vs float64 oracle (golden cases)', host(gp2), want2, absum2, tag, n_terms=g.size)


@pytest.mark.parametrize('k', [2, 4, 16, 33, 256, 1000])
def test_nonuniform_random_vs_c_oracle(k):
    rng = np.random.RandomState(k)
    for n, bucket in [(100003, 256), (100003, None), (5000, 100), (1 << 20, 256), (300, 256)]:
        x = rng.randn(n).astype(np.float32)
        pts = np.sort(rng.rand(k)).astype(np.float32)
        for mode in ('distance', 'midpoint'):
            r = oc.nonuniform_quantize(x, pts, bucket, mode)
            if mode == 'distance':
                q, idx, sf = quantization.nonUniformQuantization(dev(x), dev(pts), bucket_size=bucket)
                if k <= 256:
                    q8, idx8, _ = quantization.nonUniformQuantization(dev(x), dev(pts), bucket_size=bucket, index_dtype=torch.uint8)
                    assert idx8.dtype == torch.uint8 and torch.equal(idx8.long(), idx) and torch.equal(q8, q), (n, bucket, k)
                else:
                    with pytest.raises(ValueError, match='256'):
                        quantization.nonUniformQuantization(dev(x), dev(pts), bucket_size=bucket, index_dtype=torch.uint8)
            else:
                fn = quantization.nonUniformQuantization_variable(bucket_size=bucket, pre_process_tensors=True, tensor=dev(x))
                q = fn.forward(None, dev(pts))
                idx = fn.savedForBackward['indices']
                g = rng.randn(n).astype(np.float32)
                _, gp = fn.backward(dev(g))
                want, absum = oc.point_grad(g, r['idx'], r['alpha'], bucket, k)
                errlog.check_sum('K6 point gradient vs float64 oracle (k = %d)' % k, host(gp), want, absum, (n, bucket, k), n_terms=n)
                # determinism: same inputs, same bits -- on every path (registers, LDS columns, turn token, any-bucket-size)
                _, gp_again = fn.backward(dev(g))
                assert torch.equal(gp, gp_again), (n, bucket, k)
            assert np.array_equal(host(idx), r['idx']), (n, bucket, mode)
            assert np.array_equal(host(q), r['q']), (n, bucket, mode)
            assert np.bincount(host(idx).reshape(-1), minlength=k).sum() == n


@pytest.mark.parametrize('bucket,k', [(100, 4), (100, 600), (1000, 4), (1000, 600), (100, 64), (100, 100), (33, 16), (256, 600),
                                      (None, 700), (256, 1024), (1000, 1024), (100, 128), (1000, 256), (7, 16), (5, 4), (6, 200),
                                      (3, 16), (2, 4), (256, 100), (None, 100), (256, 300), (None, 300)])
def test_point_gradient_deterministic_and_within_1e6_on_every_path(bucket, k):
    """qd_point_grad_f32 promises a deterministic two-stage reduction on EVERY path (include/qd_hip.h).  Round 2's path for
    non-power-of-two buckets, k > 512 and misaligned index pointers used float LDS atomics, whose order is not fixed; it
    now runs on lane-private columns like the fast path.  20 launches each -- uint8 and int64 indices, aligned and
    misaligned index pointers -- must give bit-identical grad_points, within 1e-6 of sum |g alpha| of the float64 oracle
    (ref: quant_functions.py:493-503)."""
    lib = _lib.load()
    rng = np.random.RandomState(k * 7 + (bucket or 1))
    n = 700001
    g = rng.randn(n).astype(np.float32)
    idx = rng.randint(0, k, size=n).astype(np.int64)
    nb = 1 if bucket is None else (n + bucket - 1) // bucket
    alpha = (np.abs(rng.randn(nb)) + 0.1).astype(np.float32)
    want, absum = oc.point_grad(g, idx, alpha, bucket, k)
    gd, ad = dev(g), dev(alpha)
    ws = torch.empty(lib.qd_workspace_bytes(), dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    variants = [('int64', dev(idx), 8, 0)]
    pad = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    pad[1:] = dev(idx)
    variants.append(('int64 at +8 bytes', pad[1:], 8, 0))                 # index pointer not 16-byte aligned
    if k <= 256:
        variants.append(('uint8', dev(idx.astype(np.uint8)), 1, 0))
        p8 = torch.zeros(n + 1, dtype=torch.uint8, device=DEV)
        p8[1:] = dev(idx.astype(np.uint8))
        variants.append(('uint8 at +1 byte', p8[1:], 1, 0))
    for name, it, ib, _ in variants:
        outs = []
        for rep in range(20):
            out = torch.full((k,), float('nan'), device=DEV)
            _lib.check(lib.qd_point_grad_f32(gd.data_ptr(), it.data_ptr(), ib, ad.data_ptr(), n, bucket or 0, k, out.data_ptr(),
                                             ws.data_ptr(), ws.numel(), st))
            outs.append(out)
        torch.cuda.synchronize()
        for o in outs[1:]:
            assert torch.equal(o, outs[0]), (bucket, k, name, 'run-to-run difference')
        errlog.check_sum('K6 point gradient, every path (bucket %s, k = %d)' % (bucket, k), host(outs[0]), want, absum,
                         (bucket, k, name), n_terms=n)


@pytest.mark.parametrize('bucket,k', [(100, 4), (7, 16), (1000, 64), (4097, 128), (100, 256), (33, 4), (256, 16)])
def test_point_gradient_long_streams_at_any_bucket_size(bucket, k):
    """The float4 kernels of K6 walk the buckets of a lane's stream incrementally at non-power-of-two bucket sizes (one
    division per lane, then (bucket, offset) advanced per load; qd_reductions.hip BucketWalk).  8 Mi + 5 elements give every
    lane 16 and more steps of that walk, with the padded last bucket and a scalar tail; the alphas differ by orders of
    magnitude between neighbouring buckets so that a float4 given the wrong bucket cannot hide inside the tolerance
    (ref: quant_functions.py:493-503)."""
    lib = _lib.load()
    rng = np.random.RandomState(k * 11 + bucket)
    n = (1 << 23) + 5
    g = rng.randn(n).astype(np.float32)
    idx = rng.randint(0, k, size=n).astype(np.uint8 if k <= 256 else np.int64)
    nb = (n + bucket - 1) // bucket
    alpha = (10.0 ** rng.randint(-3, 4, size=nb)).astype(np.float32)
    want, absum = oc.point_grad(g, idx.astype(np.int64), alpha, bucket, k)
    gd, ad = dev(g), dev(alpha)
    ws = torch.empty(lib.qd_workspace_bytes(), dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    for name, it, ib in (('uint8', dev(idx), 1), ('int64', dev(idx.astype(np.int64)), 8)):
        outs = []
        for rep in range(3):
            out = torch.full((k,), float('nan'), device=DEV)
            _lib.check(lib.qd_point_grad_f32(gd.data_ptr(), it.data_ptr(), ib, ad.data_ptr(), n, bucket, k, out.data_ptr(),
                                             ws.data_ptr(), ws.numel(), st))
            outs.append(out)
        torch.cuda.synchronize()
        assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0]), (bucket, k, name, 'run-to-run difference')
        errlog.check_sum('K6 point gradient, long streams (bucket %d, k = %d)' % (bucket, k), host(outs[0]), want, absum,
                         (bucket, k, name), n_terms=n)


@pytest.mark.parametrize('k', [33, 64, 65, 200, 256, 1000])
def test_fine_cell_table_with_crowded_and_degenerate_points(k):
    """Above 32 points the pre-processed forward (midpoint rule) answers an element from a 2048-cell table when its cell holds
    at most one midpoint and searches inside the cell otherwise (qd_points.h).  Point sets that stress exactly that:
    all points inside ONE cell, a bell-shaped crowd (what a percentile initialisation produces), duplicates, points ON cell
    boundaries j / 2048, points outside [0, 1]; values on boundaries, on midpoints, below 0, above 1, +-inf and NaN.  Every
    call here is pre-scaled, so what qd_transform_plan names for it is k_nearest_prescaled_stream (every bucket size with more
    than one bucket -- 256, 1000, 100, 33, 5000, and 256 on 700 elements -- and every indices-only call) and k_single_apply
    (one bucket, 200003 and 50000 elements, with q).  The bucket kernels -- vector, one wave per bucket, chunk, lane groups,
    generic -- meet such point sets, under both rules, in tests/test_hip_nearest_ties.py.  Indices and values bit-identical to numpy's
    count of midpoints <= u (ref: quant_functions.py:531-563)."""
    lib = _lib.load()
    rng = np.random.RandomState(k)
    sets = {
        'one cell': np.sort(0.5 + rng.rand(k) / 4096.0),
        'bell': np.sort(np.clip(0.5 + 0.11 * rng.randn(k), 0.0, 1.0)),
        'duplicates': np.sort(np.repeat(rng.rand((k + 3) // 4), 4)[:k]),
        'on boundaries': np.sort(rng.choice(2049, size=k, replace=k > 2049) / 2048.0),
        'outside': np.sort(np.concatenate([[-0.5, -1e-3], rng.rand(k - 4), [1.0 + 1e-3, 1.7]])),
        'uniform': np.sort(rng.rand(k)),
    }
    n = 200003
    u = rng.rand(n).astype(np.float32)
    u[:2049] = (np.arange(2049) / 2048.0).astype(np.float32)                  # every cell boundary
    u[3000:3008] = [-1.0, -0.0, 2.0, np.inf, -np.inf, np.nan, 1.0, 0.0]
    ws = torch.empty(lib.qd_workspace_bytes(), dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    for name, pts64 in sets.items():
        pts = pts64.astype(np.float32)
        mid = (pts[:-1] + (pts[1:] - pts[:-1]) / np.float32(2.0)).astype(np.float32)          # :533, fp32
        uu = u.copy()
        uu[4000:4000 + mid.size] = mid                                                         # values ON midpoints: ties go up
        want_idx = np.searchsorted(mid, uu, side='right').astype(np.int64)         # (a NaN orders last: k - 1, as in the reference)
        want_q = pts[want_idx]
        pd, ud = dev(pts), dev(uu)
        for bucket, nn in ((256, n), (1000, n), (100, n), (33, n), (0, n), (0, 50000), (256, 700), (5000, n)):
            nb = lib.qd_num_buckets(nn, bucket)
            ab = torch.ones(2, nb, device=DEV)
            ab[1].zero_()
            for idx_bytes, dt in ((8, torch.int64), (1, torch.uint8)):
                if idx_bytes == 1 and k > 256:
                    continue
                q = torch.full((nn,), float('nan'), device=DEV)
                idx = torch.full((nn,), 77, dtype=dt, device=DEV)
                _lib.check(lib.qd_nearest_point_f32(ud.data_ptr(), 1, pd.data_ptr(), k, 1, q.data_ptr(), idx.data_ptr(), idx_bytes, nn, bucket,
                                                    ab[0].data_ptr(), ab[1].data_ptr(), None, 0, 0.0, ws.data_ptr(), ws.numel(), st))
                got_i = host(idx).astype(np.int64)
                assert np.array_equal(got_i, want_idx[:nn]), (k, name, bucket, nn, idx_bytes, np.flatnonzero(got_i != want_idx[:nn])[:5])
                assert np.array_equal(host(q), want_q[:nn], equal_nan=True), (k, name, bucket, nn, idx_bytes)
                # indices only (q == NULL, include/qd_hip.h): the same indices, nothing else written
                idx2 = torch.full((nn,), 77, dtype=dt, device=DEV)
                rc = lib.qd_nearest_point_f32(ud.data_ptr(), 1, pd.data_ptr(), k, 1, None, idx2.data_ptr(), idx_bytes, nn, bucket,
                                              ab[0].data_ptr(), ab[1].data_ptr(), None, 0, 0.0, ws.data_ptr(), ws.numel(), st)
                _lib.check(rc)
                assert torch.equal(idx2, idx), (k, name, bucket, nn, idx_bytes, 'indices only')
    # indices only is refused where the stream kernel cannot serve it, and without an index output
    pd, ud = dev(np.array([0.0, 1.0], np.float32)), dev(np.zeros(64, np.float32))
    ab = torch.ones(2, 64, device=DEV)
    i8 = torch.zeros(64, dtype=torch.int64, device=DEV)
    for args in ((1, None, i8.data_ptr(), 8, 3, 0), (1, None, None, 8, 64, 0), (0, None, i8.data_ptr(), 8, 64, 0), (1, None, i8.data_ptr(), 8, 64, 2)):
        prescaled, qp, ip, ib, nn, bucket = args
        assert lib.qd_nearest_point_f32(ud.data_ptr(), prescaled, pd.data_ptr(), 2, 1, qp, ip, ib, nn, bucket, ab[0].data_ptr(), ab[1].data_ptr(),
                                        None, 0, 0.0, ws.data_ptr(), ws.numel(), st) == -1, args


def test_search_sorted_handle_query():
    """SearchSorted(tensor).query(points) (quant_functions.py:509-573): int64 indices by the midpoint rule.  The kernel writes
    indices only (no throw-away q) when the tensor has at least 4 elements and a 16-byte aligned base; tiny tensors and views
    at an odd offset take the form with a scratch q."""
    from quantization.quant_functions import SearchSorted
    rng = np.random.RandomState(0)
    for n, off in ((10000, 0), (1 << 20, 0), ((1 << 20) + 3, 0), (5, 0), (3, 0), (1, 0), (10000, 1), (4099, 3), (70001, 4)):
        base = rng.rand(n + off).astype(np.float32)
        x = base[off:]
        for pts in (np.array([0.0, 0.3, 0.31, 0.9], dtype=np.float32), np.sort(rng.rand(100)).astype(np.float32)):
            idx = SearchSorted(dev(base)[off:]).query(dev(pts))
            assert idx.dtype == torch.int64 and idx.numel() == n
            assert np.array_equal(host(idx), onp.assign_midpoint(x, pts)), (n, off, pts.size)


def test_init_points_and_huffman_golden(golden_misc):
    G = golden_misc
    for i, c in enumerate(G.meta['init_points']):
        sf = quantization.ScalingFunction('linear', False, False, c['bucket'], False)
        p = qhf.initialize_quantization_points(dev(G.z['ip%d_x' % i]), sf, c['k'])
        assert p.device == dev(np.zeros(1, np.float32)).device and np.array_equal(host(p), G.z['ip%d_p' % i]), c
    params = [dev(G.z['hf_p%d' % j]) for j in range(4)]
    for c in G.meta['huffman']:
        if c['kind'] == 'uniform':
            f = lambda t, c=c: quantization.uniformQuantization(t, c['s'], bucket_size=c['bucket'])   # noqa: E731
            got = qhf.get_huffman_encoding_mean_bit_length(iter(params), f, 'uniform', s=c['s'])
        else:
            pts = torch.tensor(c['points'])
            f = lambda t, pts=pts, c=c: quantization.nonUniformQuantization(t, pts, bucket_size=c['bucket'])   # noqa: E731
            got = qhf.get_huffman_encoding_mean_bit_length(iter(params), f, 'nonuniform')
        assert abs(got - c['mean_bit_length']) < 1e-12, (c, got)


# ------------------------------------------------------------------------------ STE variants (K7/K8)
def test_ste_complicated_golden(golden_ste):
    G = golden_ste
    for i, c in enumerate(G.meta):
        x, g = G.arr('s', i, 'x'), G.arr('s', i, 'g')
        fn = quantization.uniformQuantization_variable(c['s'], bucket_size=c['bucket'])
        q = fn.forward(dev(x))
        assert np.array_equal(host(q), G.arr('s', i, 'q'))
        out = fn.backward(dev(g))
        assert fn.saved_for_backward is None
        errlog.check_ste('K7 bucket sum vs float64 oracle (golden cases)', host(out), x, g, c['s'], c['bucket'], (i, c))
        errlog.check_ste("K7 bucket sum vs the (patched) reference's own fp32 output (golden)", host(out), x, g, c['s'], c['bucket'],
                         (i, c), ref_out=G.arr('s', i, 'gout'))
        ref = onp.ste_complicated_backward(x, g, c['s'], c['bucket'])
        # exactly the same positions are touched as in the oracle (the tie rule, integer path)
        assert np.array_equal(host(out) != g, ref != g), (i, c)


def test_ste_complicated_large_vs_c_oracle():
    rng = np.random.RandomState(2)
    for n, bucket, s in [(1 << 20, 256, 16), (100003, 256, 4), (50000, 100, 16), (1 << 19, 256, 256), (1 << 19, 1024, 256),
                         (300001, 512, 64), (200000, 33, 256)]:
        x = rng.randn(n).astype(np.float32)
        if s == 64:
            x += 100.0                                   # beta >> alpha: the terms are differences of nearly equal quotients
        g = rng.randn(n).astype(np.float32)
        fn = quantization.uniformQuantization_variable(s, bucket_size=bucket)
        fn.forward(dev(x))
        out = host(fn.backward(dev(g)))
        ref = oc.ste_complicated_backward(x, g, s, bucket)
        assert np.array_equal(out != g, ref != g)
        errlog.check_ste('K7 bucket sum vs float64 oracle (large, s = %d)' % s, out, x, g, s, bucket, (n, s, bucket))


def test_truncated_ste_kernels():
    rng = np.random.RandomState(3)
    w = (rng.randn(100001) * 0.8).astype(np.float32)
    g = rng.randn(100001).astype(np.float32)
    wd, gd = dev(w), dev(g)
    lib = _lib.lib_for(wd)                       # the library of the tensors' device (tests/test_host_parity.py runs this on CPU tensors)
    _lib.check(lib.qd_truncated_ste_f32(wd.data_ptr(), gd.data_ptr(), w.size, 1.0, _lib.stream_for(wd)))
    assert np.array_equal(host(gd), onp.truncated_ste_mask(w, g))
    _lib.check(lib.qd_clamp_f32(wd.data_ptr(), w.size, 1.0, _lib.stream_for(wd)))
    assert np.array_equal(host(wd), np.clip(w, -1.0, 1.0))


# ------------------------------------------------------------------------------ multi-tensor K1
def test_multi_tensor_matches_per_tensor():
    from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer
    g = torch.Generator().manual_seed(9)
    shapes = [(500, 1600), (50, 75, 5, 5), (50,), (10,), (1,), (257,), (256,), (50, 50, 5, 5), (3, 3), (1025,)]
    for bucket in (256, 128, 100, None):
        masters = [torch.randn(*s, generator=g).to(DEV) for s in shapes]
        mt = MultiTensorQuantizer(masters, 16, bucket)
        outs = mt.quantize()
        for m, o in zip(masters, outs):
            want, _ = quantization.uniformQuantization(m, 16, bucket_size=bucket)
            assert torch.equal(o, want), (bucket, tuple(m.shape))
            assert np.array_equal(host(o), onp.uniform_quantize(host(m), 16, bucket)['q'])
        # masters untouched; a second call after an update sees the new values
        masters[0].mul_(0.5)
        outs = mt.quantize()
        assert torch.equal(outs[0], quantization.uniformQuantization(masters[0], 16, bucket_size=bucket)[0])


def test_c_abi_argument_errors():
    lib = _lib.load()
    x = torch.zeros(16, device=DEV)
    assert lib.qd_uniform_f32(x.data_ptr(), x.data_ptr(), 16, 4, 1, None, None, None, None, 0, 0.0, 0, 0, None, 0,
                              _lib.stream_ptr()) == -1          # levels < 2
    assert lib.qd_uniform_f32(None, x.data_ptr(), 16, 4, 16, None, None, None, None, 0, 0.0, 0, 0, None, 0,
                              _lib.stream_ptr()) == -1          # null input
    big = torch.zeros(100000, device=DEV)
    assert lib.qd_uniform_f32(big.data_ptr(), big.data_ptr(), 100000, 0, 16, None, None, None, None, 0, 0.0, 0, 0,
                              None, 0, _lib.stream_ptr()) == -2  # global path needs the workspace
    with pytest.raises(RuntimeError):
        _lib.check(-2)


def test_beyond_int32_elements():
    """Maximum sizes: a tensor with more than 2^31 elements (8.6 GB in, 8.6 GB out) exercises the
    64-bit indexing of every path.  Checked by a size-independent property: quantizing the whole
    tensor equals quantizing bucket-aligned pieces, and the pieces are checked against the C
    oracle on sampled windows."""
    n = (1 << 31) + 256 * 3 + 17                    # ragged, > INT32_MAX
    free, _ = torch.cuda.mem_get_info()
    if free < 3 * n * 4 + (4 << 30):
        pytest.skip('not enough free HBM for the 2^31-element test')
    x = torch.empty(n, device=DEV)
    piece = 1 << 28
    g = torch.Generator(device=DEV).manual_seed(7)
    for lo in range(0, n, piece):
        x[lo:lo + piece].normal_(generator=g)
    q, sf = quantization.uniformQuantization(x, 16, bucket_size=256)
    assert sf.alpha.shape == ((n + 255) // 256, 1)
    # windows at the start, across the 2^31 boundary and the ragged tail, against the oracle
    for lo in (0, (1 << 31) - 256 * 4, n - (n % 256) - 256 * 2):
        hi = min(n, lo + 256 * 8)
        want = oc.uniform_quantize(host(x[lo:hi]), 16, 256, want_idx=False, want_lev=False)['q']
        assert np.array_equal(host(q[lo:hi]), want), lo
    # whole == pieces (bucket-aligned split)
    cut = (1 << 31) + 256
    qa, _ = quantization.uniformQuantization(x[:cut], 16, bucket_size=256)
    assert torch.equal(qa, q[:cut])
    del qa
    qb, _ = quantization.uniformQuantization(x[cut:], 16, bucket_size=256)
    assert torch.equal(qb, q[cut:])
    del qb, q
    # un-bucketed path (global reduce + apply) and the nearest-point path on the same tensor
    qg, sfg = quantization.uniformQuantization(x, 4)
    mn, mx = x.min(), x.max()
    assert float(sfg.beta) == float(mn) and float(sfg.alpha) == float(mx - mn)
    assert torch.equal(qg[-5:], quantization.uniformQuantization(x, 4)[0][-5:])
    lev = torch.round((qg[-1000:] - sfg.beta) / sfg.alpha * 3)
    assert float(lev.min()) >= 0 and float(lev.max()) <= 3
    del qg
    pts = torch.tensor([0.0, 0.4, 0.6, 1.0], device=DEV)
    fn = quantization.nonUniformQuantization_variable(bucket_size=256, pre_process_tensors=True, tensor=x)
    qn = fn.forward(None, pts)
    idx = fn.savedForBackward.raw_indices()
    assert idx.dtype == torch.uint8 and idx.numel() == n
    hist = torch.bincount(idx[-100000:].long(), minlength=4)
    assert int(hist.sum()) == 100000
    lo = (1 << 31) - 512
    r = oc.nonuniform_quantize(host(x[lo:lo + 2048]), host(pts), 256, 'midpoint')
    assert np.array_equal(host(qn[lo:lo + 2048]), r['q']) and np.array_equal(host(idx[lo:lo + 2048]).astype(np.int64), r['idx'])
    gsum = fn.backward(torch.ones_like(x))[1]
    # sum over bins of grad = sum_i alpha_bucket(i) (g = 1): compare with 256 * sum(alpha) minus the ragged remainder
    al = fn.scaling_function.alpha.view(-1).double()
    want = float(al[:-1].sum() * 256 + al[-1] * (n % 256))
    assert abs(float(gsum.double().sum()) - want) <= 1e-5 * want


def test_beyond_int32_elements_at_a_bucket_size_that_is_not_a_power_of_two():
    """Maximum sizes, second half: more than 2^31 elements at bucket 100 -- the stream kernels of the pre-processed forward
    (K5) and of inv_scale_down (K3) take their 64-bit division branch there, the chunk kernel of scale_down (K2) and the
    bucket walk of the point gradient (K6) index past 2^31.  Windows around the 2^31-st element and at the ragged tail
    against the oracle; the point gradient through sum_j grad_j = sum_i alpha_bucket(i) for g = 1."""
    bucket = 100
    n = (1 << 31) + bucket * 7 + 13
    free, _ = torch.cuda.mem_get_info()
    if free < 5 * n * 4 + (4 << 30):
        pytest.skip('not enough free HBM for the 2^31-element test')
    x = torch.empty(n, device=DEV)
    piece = 1 << 28
    g = torch.Generator(device=DEV).manual_seed(11)
    for lo in range(0, n, piece):
        x[lo:lo + piece].normal_(generator=g)
    pts = torch.tensor([0.0, 0.3, 0.55, 1.0], device=DEV)
    fn = quantization.nonUniformQuantization_variable(bucket_size=bucket, pre_process_tensors=True, tensor=x)
    qn = fn.forward(None, pts)
    idx = fn.savedForBackward.raw_indices()
    assert idx.dtype == torch.uint8 and idx.numel() == n and qn.numel() == n
    first_after = ((1 << 31) // bucket) * bucket                 # the bucket that straddles element 2^31
    windows = (0, first_after - bucket * 3, n - (n % bucket) - bucket * 4)
    for lo in windows:
        hi = min(n, lo + bucket * 8)
        r = oc.nonuniform_quantize(host(x[lo:hi]), host(pts), bucket, 'midpoint')
        assert np.array_equal(host(qn[lo:hi]), r['q']), lo
        assert np.array_equal(host(idx[lo:hi]).astype(np.int64), r['idx']), lo
    del qn
    # K2 -> K3 on the same tensor: inv_scale_down(scale_down(x)) against the oracle's round trip on the windows
    sf = quantization.ScalingFunction('linear', False, False, bucket)
    u = sf.scale_down(x)
    back = sf.inv_scale_down(u)
    for lo in windows:
        hi = min(n, lo + bucket * 8)
        ro = onp.scale_down(host(x[lo:hi]), bucket)
        assert np.array_equal(host(u.view(-1)[lo:hi]), ro['u'].reshape(-1)[:hi - lo]), lo
        want = onp.inv_scale_down(ro['u'], ro['alpha'], ro['beta'], 0.0, hi - lo, (hi - lo,))
        assert np.array_equal(host(back.view(-1)[lo:hi]), want), lo
    del u, back
    gsum = fn.backward(torch.ones_like(x))[1]
    al = fn.scaling_function.alpha.view(-1).double()
    want = float(al[:-1].sum() * bucket + al[-1] * (n % bucket))
    assert abs(float(gsum.double().sum()) - want) <= 1e-5 * want


# ------------------------------------------------------------------------------ packed codec + histograms
@pytest.mark.parametrize('s,bits', [(2, 1), (4, 2), (3, 2), (16, 4), (9, 4), (256, 8), (16, 8)])
def test_pack_unpack_roundtrip(s, bits):
    from quantized_distillation_amd import codec
    rng = np.random.RandomState(s)
    for n, bucket in [(256 * 40, 256), (100003, 256), (70001, 64), (5 * 2048 + 7, 2048), (300, 256), (1 << 22, 512), (128 * 33 + 5, 128),
                      (1024 * 9 + 3, 1024),
                      (100003, 100), (100003, 33), (70001, 1000), (1 << 20, 513), (100003, None), (777, None), (5000, 3),
                      (100003, 4096), (50, 256)]:      # any bucket size: quantize with level indices + pack them
        x = rng.randn(n).astype(np.float32)
        xd = dev(x)
        pk = codec.pack_uniform(xd, s, bucket, bits=bits)
        ref = oc.uniform_quantize(x, s, bucket)
        # packed bytes == numpy packing of the oracle's level indices (little endian inside a byte)
        lev = ref['lev'].astype(np.uint64)
        epb = 8 // bits
        pad = (-n) % epb
        levp = np.concatenate([lev, np.zeros(pad, np.uint64)]).reshape(-1, epb)
        want = np.zeros(levp.shape[0], np.uint64)
        for c in range(epb):
            want |= levp[:, c] << np.uint64(c * bits)
        assert np.array_equal(host(pk.packed), want.astype(np.uint8)), (n, bucket)
        assert np.array_equal(host(pk.alpha), ref['alpha']) and np.array_equal(host(pk.beta), ref['beta'])
        # decode == uniformQuantization, bit for bit
        y = pk.unpack()
        q, _ = quantization.uniformQuantization(xd, s, bucket_size=bucket)
        assert torch.equal(y, q) and np.array_equal(host(y), ref['q'])
        # size = what helpers/functions.py:255-259 charges: bits*N/8 + 8 bytes per bucket
        assert pk.nbytes == (n * bits + 7) // 8 + 8 * (1 if (bucket is None or n < bucket) else -(-n // bucket))


def test_unpack_at_every_alignment():
    """qd_unpack_uniform_f32 on outputs / packed streams that start 4 bytes into a 16-byte granule, sizes around whole KiB of
    packed data: the same bits as the aligned call and as uniformQuantization."""
    from quantized_distillation_amd import codec
    lib = _lib.load()
    rng = np.random.RandomState(11)
    for s, bits in ((16, 4), (4, 2), (2, 1), (200, 8)):
        chunk = 64 * 128 // bits
        for n in (chunk, chunk * 5, chunk * 5 + 4, chunk * 7 + 1001, chunk - 4):
            for bucket in (16, 256, 2048):                         # (16: packed through the level-index path, decoded by these kernels)
                x = rng.randn(n).astype(np.float32)
                pk = codec.pack_uniform(dev(x), s, bucket, bits=bits)
                want = host(pk.unpack())
                assert np.array_equal(want, oc.uniform_quantize(x, s, bucket)['q']), (s, bits, n, bucket)
                # output 4 bytes into a 16-byte granule: the narrow form does everything
                ybuf = torch.empty(n + 8, device=DEV)
                y = ybuf[1:n + 1]
                _lib.check(lib.qd_unpack_uniform_f32(pk.packed.data_ptr(), n, bucket, s, bits, pk.alpha.data_ptr(), pk.beta.data_ptr(),
                                                     y.data_ptr(), _lib.stream_ptr()))
                assert np.array_equal(host(y), want), (s, bits, n, bucket)
                # packed stream 4 bytes into a granule
                pbuf = torch.empty(pk.packed.numel() + 16, dtype=torch.uint8, device=DEV)
                pbuf[4:4 + pk.packed.numel()].copy_(pk.packed)
                y2 = torch.empty(n, device=DEV)
                _lib.check(lib.qd_unpack_uniform_f32(pbuf.data_ptr() + 4, n, bucket, s, bits, pk.alpha.data_ptr(), pk.beta.data_ptr(),
                                                     y2.data_ptr(), _lib.stream_ptr()))
                assert np.array_equal(host(y2), want), (s, bits, n, bucket)


def test_level_histogram_and_device_huffman(golden_misc):
    from quantized_distillation_amd import codec
    rng = np.random.RandomState(1)
    for n, s, bucket in [(100003, 16, 256), (1 << 20, 4, None), (5000, 256, 256), (77, 2, 256), (64 * 3001 + 9, 16, 64), (128 * 700, 4, 128),
                         (512 * 333 + 100, 256, 512), (1024 * 100 + 1, 16, 1024), (2048 * 77 + 2047, 2, 2048), (5, 16, 2048), ((1 << 22) + 3, 16, 256),
                         (100003, 16, 100)]:
        x = rng.randn(n).astype(np.float32)
        want = np.bincount(oc.uniform_quantize(x, s, bucket)['lev'], minlength=s)
        h = codec.level_histogram(dev(x), s, bucket)        # one pass at the vector bucket sizes (qd_level_histogram_f32), levels + count elsewhere
        assert h.dtype == torch.int64 and np.array_equal(host(h), want), (n, s, bucket)
        if n > 8:
            assert np.array_equal(host(codec.level_histogram(dev(x)[1:], s, bucket)),
                                  np.bincount(oc.uniform_quantize(x[1:], s, bucket)['lev'], minlength=s)), (n, s, bucket, 'view at +4 B')
    # a bucket that holds a NaN: both forms count its elements as level 0 (what the uint8 level output stores for them)
    x = rng.randn(256 * 50).astype(np.float32)
    x[256 * 7 + 3] = np.nan
    h_fused, h_two = host(codec.level_histogram(dev(x), 16, 256)), host(codec.level_histogram(dev(np.concatenate([[0.0], x]).astype(np.float32))[1:], 16, 256))
    assert np.array_equal(h_fused, h_two) and h_fused.sum() == x.size
    idx = rng.randint(0, 200, size=1 << 21).astype(np.uint8)
    assert np.array_equal(host(codec.histogram_u8(dev(idx), 256)), np.bincount(idx, minlength=256))
    assert np.array_equal(host(codec.histogram_u8(dev(idx[3:]), 256)), np.bincount(idx[3:], minlength=256))   # unaligned
    # many k (register duplicates, skipped symbols >= k, every flush geometry), sizes around the resident grid
    for k in (1, 2, 3, 16, 17, 64, 65, 100, 255, 256):
        for n in (1, 15, 16, 4099, (1 << 22) + 5):
            idx = rng.randint(0, 256, size=n).astype(np.uint8)
            if k < 256:
                idx[::3] = rng.randint(0, k, size=len(idx[::3]))
            want = np.bincount(idx, minlength=256)[:k]
            assert np.array_equal(host(codec.histogram_u8(dev(idx), k)), want), (k, n)
    # the entry point without a workspace (global atomics on a zeroed histogram) counts the same
    idx = rng.randint(0, 100, size=(1 << 21) + 3).astype(np.uint8)
    idx_d, out = dev(idx), torch.empty(128, dtype=torch.int64, device=DEV)
    for k in (4, 16, 100, 128):
        _lib.check(_lib.load().qd_histogram_u8(idx_d.data_ptr(), idx_d.numel(), k, out.data_ptr(), _lib.stream_ptr()))
        assert np.array_equal(host(out)[:k], np.bincount(idx, minlength=256)[:k]), k
    runs = np.repeat(np.arange(7, dtype=np.uint8), 100000)                  # long runs: all four bytes of a word equal
    assert np.array_equal(host(codec.histogram_u8(dev(runs), 256)), np.bincount(runs, minlength=256))
    # same Huffman mean code length as the reference computed through its digitize path
    G = golden_misc
    params = [dev(G.z['hf_p%d' % j]) for j in range(4)]
    for c in G.meta['huffman']:
        if c['kind'] == 'uniform':
            got = codec.huffman_mean_bit_length_uniform(params, c['s'], c['bucket'])
            assert abs(got - c['mean_bit_length']) < 1e-12, (c, got)


def test_histogram_of_4_5_billion_symbols():
    """4.5 G symbols (past 2^32): 64-bit totals, uint32 per-block counters that one block cannot overflow in one launch.
    A periodic pattern gives the expected counts without a host pass."""
    from quantized_distillation_amd import codec
    reps = 18_000_000
    x = torch.arange(251, dtype=torch.uint8, device=DEV).repeat(reps)      # 4.5 GB
    h = codec.histogram_u8(x, 256)
    want = torch.zeros(256, dtype=torch.int64)
    want[:251] = reps
    assert torch.equal(h.cpu(), want)
    h = codec.histogram_u8(x[1:], 256)                                       # unaligned: byte loads
    want[0] -= 1
    assert torch.equal(h.cpu(), want)


def test_counting_kernels_past_2_to_31_elements():
    """The size-accounting kernels on 2^31 + 3 * 256 + 5 fp32 elements (64-bit element indices, uint32 per-block counters):
    a tensor made of one 256-element pattern repeated, so the expected counts are the pattern's counts times the number of
    repetitions (+ the short last bucket), no host pass over 8.6 GB."""
    import quantization.help_functions as qhf
    from quantized_distillation_amd import codec
    rng = np.random.RandomState(3)
    pat = rng.randn(256).astype(np.float32)
    reps = (1 << 23) + 3                                                       # 2^31 + 768 elements in whole buckets
    tail = pat[:5].copy()
    x = torch.cat([dev(pat).repeat(reps), dev(tail)])
    n = x.numel()
    assert n > (1 << 31)
    s = 16
    lev_pat = oc.uniform_quantize(pat, s, 256)['lev']
    lev_tail = oc.uniform_quantize(tail, s, 256)['lev']                         # the short last bucket is scaled on its own
    want = np.bincount(lev_pat, minlength=s).astype(np.int64) * reps + np.bincount(lev_tail, minlength=s)
    assert np.array_equal(host(codec.level_histogram(x, s, 256)), want)                       # one pass (k_level_hist_vec)
    assert np.array_equal(host(codec.level_histogram(x, s, 100)).sum(), n)                    # levels + count form: every element counted
    # the boundary function's counting step on the same tensor: digitize the re-scaled quantized tensor
    q, sf = quantization.uniformQuantization(x, s, bucket_size=256)
    del x
    scaled = sf.scale_down(q).view(-1)[0:sf.original_tensor_length]
    edges = qhf._digitize_edges(s, 1e-5)
    got = host(qhf._device_counts('digitize', scaled, s, torch.from_numpy(edges).to(DEV)))
    qp = oc.uniform_quantize(pat, s, 256)['q']
    qt = oc.uniform_quantize(tail, s, 256)['q']
    want_d = (np.bincount(np.digitize(oc.scale_down(qp, 256)['u'], edges), minlength=s + 1).astype(np.int64) * reps
              + np.bincount(np.digitize(oc.scale_down(qt, 256)['u'], edges), minlength=s + 1))
    assert np.array_equal(got, want_d) and got.sum() == n
    del q, scaled
    idx = torch.arange(7, dtype=torch.int64, device=DEV).repeat((1 << 28) + 1)   # 2^31 / 8 * 7 ... : 1.88 G int64 symbols, 15 GB
    h = host(qhf._device_counts('index', idx, 256))
    assert np.array_equal(h[:7], np.full(7, (1 << 28) + 1)) and h[7:].sum() == 0


# ------------------------------------------------------------------------------ absmax / absnorm (parity unpinned)
@pytest.mark.parametrize('kind', ['absmax', 'absnorm'])
def test_abs_scaling_intended_math(kind):
    """The reference raises for these scaling types on every torch version, so this only checks the
    kernels against the oracle's restatement of the intended math (parity unpinned)."""
    rng = np.random.RandomState(5)
    for n, bucket in [(1000, 256), (5000, None), (257, 256), (100003, 256), (300000, None), (64, 100)]:
        x = rng.randn(n).astype(np.float32)
        x[::97] = 0.0
        xd = dev(x)
        sf = quantization.ScalingFunction(kind, False, False, bucket)
        u = sf.scale_down(xd)
        ref = onp.scale_down_abs(x, bucket, kind)
        nrm = host(sf.norm_scaling).reshape(-1)
        if kind == 'absmax':
            assert np.array_equal(nrm, ref['norm'])
        else:
            assert np.allclose(nrm, ref['norm'], rtol=2e-6, atol=0)
        ref = onp.scale_down_abs(x, bucket, kind, norm=nrm)          # exact given the device's norms
        assert np.array_equal(host(u), ref['u'].reshape(host(u).shape))
        assert np.array_equal(host(sf.tensor_sign), ref['sign'].reshape(host(u).shape))
        back = host(sf.inv_scale_down(u))
        assert np.allclose(back, x, rtol=3e-7, atol=1e-30) and back.shape == x.shape
        q, sf2 = quantization.uniformQuantization(xd, 8, type_of_scaling=kind, bucket_size=bucket)
        nrm2 = host(sf2.norm_scaling).reshape(-1)
        assert np.array_equal(host(q), onp.uniform_quantize_abs(x, 8, bucket, kind, norm=nrm2)['q'])
        assert np.all(host(q)[x == 0] == 0)
    with pytest.raises(ValueError):
        quantization.uniformQuantization_variable(16, type_of_scaling=kind, bucket_size=256).backward(dev(x))


def test_nonfinite_inputs_golden(golden_nonfinite):
    """Reference behaviour on NaN / +-inf inputs (NaN poisons its bucket): every path that computes a
    bucket's min/max -- per-tensor API, scale_down, multi-tensor, codec -- reproduces it."""
    from quantized_distillation_amd import codec
    from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer
    G = golden_nonfinite
    for i, c in enumerate(G.meta):
        x = G.arr('f', i, 'x')
        xd = dev(x)
        q, sf = quantization.uniformQuantization(xd, c['s'], bucket_size=c['bucket'])
        assert np.array_equal(host(q), G.arr('f', i, 'q'), equal_nan=True), (i, c)
        assert np.array_equal(host(sf.alpha), G.arr('f', i, 'alpha'), equal_nan=True), (i, c)
        assert np.array_equal(host(sf.beta), G.arr('f', i, 'beta'), equal_nan=True), (i, c)
        if xd.is_cuda:                               # (multi-tensor launches and the codec exist for device tensors only)
            out = MultiTensorQuantizer([xd], c['s'], c['bucket']).quantize()[0]
            assert np.array_equal(host(out), G.arr('f', i, 'q'), equal_nan=True), (i, c)
        if c['bucket'] == 256 and xd.is_cuda:
            assert np.array_equal(host(codec.pack_uniform(xd, c['s'], 256).alpha), G.arr('f', i, 'alpha').reshape(-1), equal_nan=True)
        sf2 = quantization.ScalingFunction('linear', False, False, c['bucket'])
        u = sf2.scale_down(xd)
        ref = onp.scale_down(x, c['bucket'])
        assert np.array_equal(host(u), ref['u'], equal_nan=True), (i, c)


def test_nonuniform_options_golden(golden_nonuniform_options):
    """max_element / subtract_mean through nonUniformQuantization and the pre-processed variable."""
    G = golden_nonuniform_options
    for i, c in enumerate(G.meta):
        x, pts = G.arr('o', i, 'x'), G.arr('o', i, 'pts')
        xd, pd = dev(x), dev(pts)
        q, idx, sf = quantization.nonUniformQuantization(xd, pd, max_element=c['max_element'],
                                                         subtract_mean=c['subtract_mean'], bucket_size=c['bucket'])
        fn = quantization.nonUniformQuantization_variable(max_element=c['max_element'], subtract_mean=c['subtract_mean'],
                                                          bucket_size=c['bucket'], pre_process_tensors=True, tensor=xd)
        qp = fn.forward(None, pd)
        ip = fn.savedForBackward['indices']
        if c['subtract_mean']:
            m = float(sf.mean_tensor)
            errlog.check_mean('qd_mean_f32 vs the reference fp32 mean (golden)', m, c['mean'], float(np.abs(x).mean()), (i, c), n_terms=x.size)
            r = onp.nonuniform_quantize(x, pts, c['bucket'], 'distance', c['max_element'], True, mean=m)
            assert np.array_equal(host(idx), r['idx']) and np.array_equal(host(q), r['q']), (i, c)
            # directly against the reference's output: the same point for every element, values within 1e-6 max|x|
            assert np.array_equal(host(idx), G.arr('o', i, 'idx')), (i, c, int((host(idx) != G.arr('o', i, 'idx')).sum()))
            assert np.abs(host(q).astype(np.float64) - G.arr('o', i, 'q')).max() <= 1e-6 * float(np.abs(x).max()), (i, c)
            assert np.array_equal(host(ip), G.arr('o', i, 'idx_pre')), (i, c)
            m2 = float(fn.scaling_function.mean_tensor)
            r2 = onp.nonuniform_quantize(x, pts, c['bucket'], 'midpoint', c['max_element'], True, mean=m2)
            assert np.array_equal(host(ip), r2['idx']) and np.array_equal(host(qp), r2['q']), (i, c)
        else:
            assert np.array_equal(host(idx), G.arr('o', i, 'idx')) and np.array_equal(host(q), G.arr('o', i, 'q')), (i, c)
            assert np.array_equal(host(ip), G.arr('o', i, 'idx_pre')) and np.array_equal(host(qp), G.arr('o', i, 'q_pre')), (i, c)


def test_api_calls_under_hipgraph_capture():
    """Every entry point enqueues on the current stream and allocates only through torch, so the drop-in calls
    can be captured in a hipGraph (torch.cuda.CUDAGraph) and replayed on new data in the static input buffers."""
    rng = np.random.RandomState(21)
    n, k = 100003, 16
    x0, x1 = rng.randn(n).astype(np.float32), (rng.randn(n) * 3 + 1).astype(np.float32)
    g0, g1 = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    pts = np.sort(rng.rand(k)).astype(np.float32)
    xs, gs, pd = dev(x0), dev(g0), dev(pts)
    fn = quantization.nonUniformQuantization_variable(bucket_size=256, pre_process_tensors=True, tensor=dev(x0))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                  # warm-up outside the capture (lazy allocations)
        quantization.uniformQuantization(xs, 16, bucket_size=256)
        quantization.uniformQuantization(xs, 16)
        quantization.nonUniformQuantization(xs, pd, bucket_size=256)
        fn.forward(None, pd); fn.backward(gs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        qb, sfb = quantization.uniformQuantization(xs, 16, bucket_size=256)
        qg, _ = quantization.uniformQuantization(xs, 16)
        qn, idx, _ = quantization.nonUniformQuantization(xs, pd, bucket_size=256)
        fn.forward(None, pd)
        _, gp = fn.backward(gs)
    for xv, gv in ((x1, g1), (x0, g0)):
        xs.copy_(dev(xv)); gs.copy_(dev(gv))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(qb), oc.uniform_quantize(xv, 16, 256, want_idx=False, want_lev=False)['q'])
        assert np.array_equal(host(qg), oc.uniform_quantize(xv, 16, None, want_idx=False, want_lev=False)['q'])
        r = oc.nonuniform_quantize(xv, pts, 256, 'distance')
        assert np.array_equal(host(idx), r['idx']) and np.array_equal(host(qn), r['q'])
        rm = oc.nonuniform_quantize(x0, pts, 256, 'midpoint')     # fn was pre-processed on x0: its u is resident
        want, absum = oc.point_grad(gv, rm['idx'], rm['alpha'], 256, k)
        errlog.check_sum('K6 point gradient under hipGraph capture', host(gp), want, absum, k, n_terms=gv.size)


# ------------------------------------------------------------------------------ round-2 boundary fixes
def test_lazy_arg_indices_raise_after_the_source_was_modified():
    """idx_min_rows / idx_max_rows are taken lazily from the tensor given to scale_down (the reference computes them
    eagerly, quant_functions.py:85-90): reading them after an in-place write to that tensor must raise, never
    return indices of the NEW data."""
    x = dev(np.random.RandomState(5).randn(5000).astype(np.float32))
    sf = quantization.ScalingFunction('linear', False, False, 256)
    sf.scale_down(x)
    x.mul_(-1.0)                                   # arg-min and arg-max swap places
    with pytest.raises(RuntimeError, match='modified in place'):
        sf.idx_min_rows
    # untouched source: fine, and equal to the oracle's first-occurrence indices
    y = dev(np.random.RandomState(6).randn(5000).astype(np.float32))
    q, sf2 = quantization.uniformQuantization(y, 16, bucket_size=256)
    want = onp.uniform_quantize(host(y), 16, 256)
    assert np.array_equal(host(sf2.idx_min_rows).reshape(-1), want['imin'].reshape(-1))
    assert np.array_equal(host(sf2.idx_max_rows).reshape(-1), want['imax'].reshape(-1))
    # read first, modify later: the materialised indices stay available
    z = dev(np.random.RandomState(7).randn(5000).astype(np.float32))
    _, sf3 = quantization.uniformQuantization(z, 16, bucket_size=256)
    keep = host(sf3.idx_max_rows).copy()
    z.zero_()
    assert np.array_equal(host(sf3.idx_max_rows), keep)


@pytest.mark.parametrize('n', [16385, 20000, 70001])
def test_nonuniform_single_bucket_of_exactly_bucket_size(n):
    """numel == bucket_size is ONE bucket (help_functions.py:67-94) and takes the single-bucket kernel, which needs
    the reduction scratch above 16 Ki elements (round-1 advisor finding: NULL workspace -> QD_ERR_WORKSPACE_TOO_SMALL)."""
    x = np.random.RandomState(n).randn(n).astype(np.float32)
    pts = np.sort(np.random.RandomState(1).rand(5)).astype(np.float32)
    q, idx, sf = quantization.nonUniformQuantization(dev(x), torch.from_numpy(pts), bucket_size=n)
    want = onp.nonuniform_quantize(x, pts, n)
    assert np.array_equal(host(q), want['q']) and np.array_equal(host(idx), want['idx'])
    fn = quantization.nonUniformQuantization_variable(bucket_size=n, pre_process_tensors=True, tensor=dev(x))
    q2 = fn.forward(None, torch.from_numpy(pts).to(DEV))
    assert np.array_equal(host(q2), onp.nonuniform_quantize(x, pts, n, 'midpoint')['q'])


# ------------------------------------------------------------------------------ one-launch single bucket (k_single_fused)
FUSED_SIZES = [16385, 65536 + 3, 262144, 1 << 20, 800000, 5308416 + 1, 1408 * 1408 * 9]


@pytest.fixture
def fused_mode():
    lib = _lib.load()
    prev = lib.qd_set_single_fused_mode(-1)

    def set_mode(m):
        lib.qd_set_single_fused_mode(m)
    yield set_mode
    lib.qd_set_single_fused_mode(-1)
    assert prev in (0, 1, 2, 3, 4)


@pytest.mark.parametrize('mode', [1, 2, 3, 4, 0],
                         ids=['fused', 'fused-all-give-up', 'fused-every-7th-gives-up', 'fused-one-gives-up', 'three-launch'])
def test_single_bucket_paths_bit_exact(mode, fused_mode):
    """bucket_size=None on every path the library can take for it -- the one-launch register-resident kernel, its
    contention fallback (a block that gives up at the barrier folds the whole tensor itself; all blocks, every 7th
    block, exactly one block) and the three-launch path -- against the C oracle: q, alpha, beta bit-exact, for sizes
    that land on every V variant and with ragged tails."""
    fused_mode(mode)
    for n in FUSED_SIZES:
        x = np.random.RandomState(n % 9973).randn(n).astype(np.float32) * 0.05
        for s in (16, 4):
            want = oc.uniform_quantize(x, s, None, want_idx=False, want_lev=False)
            q, sf = quantization.uniformQuantization(dev(x), s)
            assert np.array_equal(host(q), want['q']), (mode, n, s)
            assert np.array_equal(host(sf.alpha).reshape(-1), want['alpha']) and np.array_equal(host(sf.beta).reshape(-1), want['beta'])
        # clamp + mean, in place, sliced (unaligned base -> never fused), scale_down, non-uniform
        want = oc.uniform_quantize(x, 16, None, max_element=0.08, subtract_mean=True, want_idx=False, want_lev=False)
        q, sf = quantization.uniformQuantization(dev(x), 16, max_element=0.08, subtract_mean=True)
        m = np.float32(host(sf.mean_tensor))
        want_m = oc.uniform_quantize(x, 16, None, max_element=0.08, subtract_mean=True, mean=m, want_idx=False, want_lev=False)
        errlog.check_mean('qd_mean_f32 vs float64 oracle', m, want['mean'], float(np.abs(x).mean()), (mode, n), n_terms=n)
        assert np.array_equal(host(q), want_m['q']), (mode, n, 'clamp+mean')
        xd = dev(x)
        q2, _ = quantization.uniformQuantization(xd, 16, modify_in_place=True)
        assert q2.data_ptr() == xd.data_ptr() and np.array_equal(host(xd), oc.uniform_quantize(x, 16, None, want_idx=False, want_lev=False)['q'])
        big = dev(np.concatenate([np.zeros(1, np.float32), x]))
        q3, _ = quantization.uniformQuantization(big[1:], 16)
        assert np.array_equal(host(q3), oc.uniform_quantize(x, 16, None, want_idx=False, want_lev=False)['q']), (mode, n, 'offset base')
        sfs = quantization.ScalingFunction('linear', False, False, None)
        u = sfs.scale_down(dev(x))
        assert np.array_equal(host(u), oc.scale_down(x, None)['u']), (mode, n, 'scale_down')
        pts = np.array([0.0, 0.3, 0.55, 1.0], np.float32)
        qn, idx, _ = quantization.nonUniformQuantization(dev(x), torch.from_numpy(pts))
        wn = oc.nonuniform_quantize(x, pts, None)
        assert np.array_equal(host(qn), wn['q']) and np.array_equal(host(idx), wn['idx']), (mode, n, 'non-uniform')


def test_single_bucket_fused_nan_stochastic_and_level_output(fused_mode):
    import quantization.quant_functions as qf
    from quantized_distillation_amd import codec
    n = 300001
    x = np.random.RandomState(3).randn(n).astype(np.float32)
    outs = {}
    for mode in (1, 2, 3, 4, 0):
        fused_mode(mode)
        qf._STOCHASTIC_CALLS[0] = 1234                     # same seed on every path
        q, _ = quantization.uniformQuantization(dev(x), 16, stochastic_rounding=True)
        outs[mode] = host(q)
        h = codec.level_histogram(dev(x), 16, None)        # uint8 level side output of the same kernel
        lev = oc.uniform_quantize(x, 16, None, want_idx=False)['lev']
        assert np.array_equal(host(h), np.bincount(lev, minlength=16)), mode
        xn = x.copy()
        xn[n // 2] = np.nan
        qn, sfn = quantization.uniformQuantization(dev(xn), 16)
        assert np.isnan(host(qn)).all() and np.isnan(host(sfn.alpha)).all(), 'one NaN poisons the whole single bucket (as torch.min/max do)'
    for mode in (1, 2, 3, 4):
        assert np.array_equal(outs[mode], outs[0]), 'stochastic draws depend on (seed, element) only'


@pytest.mark.parametrize('mode', [3, 4, 1], ids=['every-7th-gives-up', 'one-gives-up', 'all-meet'])
def test_single_bucket_fused_partial_give_up_two_streams(mode, fused_mode):
    """The realistic contention outcome -- SOME blocks of a launch give up at the grid barrier, the others meet -- over
    240 launches on two streams (120 each, sizes on both V variants, barrier slot sets wrap around several times): every
    output, alpha and beta bit-identical to the three-launch path and to the C oracle.  (Round 2's protocol -- a relaxed
    gave_up counter read by the last block out -- could leave the slice of a block that gave up unwritten; a block that
    gives up now finishes its own slice and depends on nobody.)"""
    sizes = [1 << 20, 262144 + 7, 65536 + 3, 800000]
    xs = [np.random.RandomState(7 + i).randn(n).astype(np.float32) * 0.05 for i, n in enumerate(sizes)]
    xd = [dev(x) for x in xs]
    fused_mode(0)
    ref = [quantization.uniformQuantization(x, 16) for x in xd]
    ref_q = [host(q) for q, _ in ref]
    ref_a = [host(sf.alpha).copy() for _, sf in ref]
    ref_b = [host(sf.beta).copy() for _, sf in ref]
    for i, x in enumerate(xs):
        want = oc.uniform_quantize(x, 16, None, want_idx=False, want_lev=False)
        assert np.array_equal(ref_q[i], want['q']) and np.array_equal(ref_a[i].reshape(-1), want['alpha'])
    fused_mode(mode)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    outs = [[], []]
    for rep in range(120):
        for si, st in enumerate(streams):
            with torch.cuda.stream(st):
                i = (rep + si) % len(sizes)
                q, sf = quantization.uniformQuantization(xd[i], 16)
                outs[si].append((i, q, sf))
    torch.cuda.synchronize()
    for si in range(2):
        for i, q, sf in outs[si]:
            assert np.array_equal(host(q), ref_q[i]), (mode, si, i)
            assert np.array_equal(host(sf.alpha), ref_a[i]) and np.array_equal(host(sf.beta), ref_b[i])
    # through the C ABI with a NaN-poisoned output buffer: every element must be overwritten
    lib = _lib.load()
    ws = torch.empty(lib.qd_workspace_bytes(), dtype=torch.uint8, device=DEV)
    for i, x in enumerate(xd):
        out = torch.full_like(x, float('nan'))
        ab = torch.full((2,), float('nan'), device=DEV)
        for rep in range(10):
            out.fill_(float('nan'))
            rc = lib.qd_uniform_f32(x.data_ptr(), out.data_ptr(), x.numel(), 0, 16, ab.data_ptr(), ab[1:].data_ptr(), None,
                                    None, 0, 0.0, 0, 0, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
            assert rc == 0
            assert np.array_equal(host(out), ref_q[i]), (mode, i, rep)
            assert float(ab[0]) == float(ref_a[i].reshape(-1)[0]) and float(ab[1]) == float(ref_b[i].reshape(-1)[0])


def test_single_bucket_fused_many_launches_in_flight(fused_mode):
    """More one-launch kernels in flight than there are barrier slot sets (64), on four streams: launches that end up
    sharing a slot set overwrite each other's tags, fail their sweeps and take the give-up path -- slower, never wrong,
    never hung."""
    fused_mode(1)
    n = 1 << 20
    xs = [np.random.RandomState(40 + i).randn(n).astype(np.float32) for i in range(4)]
    want = [oc.uniform_quantize(x, 16, None, want_idx=False, want_lev=False)['q'] for x in xs]
    xd = [dev(x) for x in xs]
    streams = [torch.cuda.Stream() for _ in range(4)]
    torch.cuda.synchronize()
    results = [[] for _ in range(4)]
    for rep in range(48):
        for i, st in enumerate(streams):
            with torch.cuda.stream(st):
                results[i].append(quantization.uniformQuantization(xd[i], 16)[0])
    torch.cuda.synchronize()
    for i in range(4):
        for q in results[i]:
            assert np.array_equal(host(q), want[i])


# ------------------------------------------------------------------------------ bucket-invariant division (round 2)
def test_division_by_bucket_invariant_alpha():
    """Device-side proof slice: 1.2 * 10^8 adversarial (n, alpha) pairs (six families of 2 * 10^7: the quantizer's own domain,
    wide exponents, all-ones / near-power-of-two significands, near-exact quotients around level values, the edges of the
    stated ranges, small normal quotients down to 2^-120 -- what scale_down adds) through the very inline function the kernels use (qd_selftest_div_invariant, csrc/qd_selftest.hip)
    against the IEEE quotient: 0 mismatches required.  tools/div_invariant_check.py --pairs 1e9 is the long run
    (docs/history/profiles/r03_div_invariant.txt).  ref: quant_functions.py:106-107."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import div_invariant_check as dic
    bad, rows = dic.run_device(20_000_000, seed=5, verbose=False)
    for fam, name, tested, nbad, skipped, first in rows:
        assert tested >= 10_000_000, (fam, name, tested, skipped)        # the generators stay inside the domain
        assert nbad == 0, (fam, name, nbad, hex(first))
    assert bad == 0


@pytest.mark.parametrize('bucket', [256, 64, 512, 100, 36, 33, 50, 7, 1000])
def test_quantize_bit_exact_at_extreme_scales(bucket):
    """The quantize kernels divide by the bucket's alpha through y = RN(1/alpha) and two FMAs when alpha is in
    [2^-60, 2^100] (exact there, qd_common.h) and by IEEE division otherwise; numerators below 2^-100 only ever
    yield level 0.  Exercise both sides of every boundary: tiny / huge / denormal scales, buckets that mix them,
    constant buckets, zeros next to denormals -- q, alpha, beta bit-exact against the C oracle for 16 and 4 levels,
    deterministic, plus the stochastic branch against the Philox restatement."""
    import quantization.quant_functions as qf
    rng = np.random.RandomState(bucket)
    n = 40 * 2048 + 3
    base = rng.randn(n).astype(np.float32)
    scales = [1.0, 1e-3, 2.0 ** -58, 2.0 ** -61, 2.0 ** -70, 1e-30, 1e-37, 1e-39, 1e-43, 2.0 ** 99, 2.0 ** 101, 1e30, 3e37]
    cases = [(base * np.float32(sc)).astype(np.float32) for sc in scales]
    mixed = base.copy()
    per = np.repeat(np.array(scales * 400, dtype=np.float64)[: (n + 255) // 256], 256)[:n]
    mixed = (mixed.astype(np.float64) * per).astype(np.float32)              # a different scale every 256 elements
    cases.append(mixed)
    sparse = np.where(rng.rand(n) < 0.7, 0.0, base * 1e-41).astype(np.float32)   # zeros next to denormals
    cases.append(sparse)
    tinyspread = (np.abs(base) * np.float32(1e-36) + np.float32(1.0)).astype(np.float32)   # alpha < 1e-10 -> 1, constant-ish
    cases.append(tinyspread)
    offset = (base * np.float32(2.0 ** -59) + np.float32(3.0)).astype(np.float32)
    cases.append(offset)
    for ci, x in enumerate(cases):
        for s in (16, 4, 256):
            want = oc.uniform_quantize(x, s, bucket, want_idx=False, want_lev=False)
            q, sf = quantization.uniformQuantization(dev(x), s, bucket_size=bucket)
            got = host(q)
            assert np.array_equal(got, want['q'], equal_nan=True), (bucket, ci, s, int(np.sum(got != want['q'])))
            assert np.array_equal(host(sf.alpha).reshape(-1), want['alpha'], equal_nan=True)
        seed = qf.next_stochastic_seed(peek=True, host=not dev(x[:1]).is_cuda)
        qs, _ = quantization.uniformQuantization(dev(x), 16, stochastic_rounding=True, bucket_size=bucket)
        nb, row, padded = onp.bucket_geometry(n, bucket)
        rand = np.zeros(padded, np.float32)
        rand[:n] = onp.philox4x32_7_uniform(seed, n)
        ws = onp.uniform_quantize_stochastic(x, 16, rand, bucket)
        assert np.array_equal(host(qs), ws['q'], equal_nan=True), (bucket, ci, 'stochastic')


@pytest.mark.parametrize('bucket', [256, 64, 1024, 100, 33])
def test_scale_down_bit_exact_at_extreme_scales(bucket):
    """scale_down RETURNS u = (x - beta) / alpha, so where its vector kernel divides through y = RN(1/alpha) and two FMAs
    (buckets whose alpha is in [2^-60, 2^100] and whose nonzero numerators are all >= max(2^-100, alpha 2^-120): a normal
    quotient; qd_bucket_vec_kernels.h vec_bucket, qd_common.h scale_fast_ok) every BIT of u must equal the IEEE quotient of quant_functions.py:106-107.
    Buckets on both sides of each condition: numerators below 2^-100, denormal quotients (where the shortcut can differ in
    the last bit and must not be taken), quotients at the 2^-120 threshold, tiny / huge / mixed scales, zeros next to
    denormals, constant buckets -- u, alpha, beta compared as bit patterns with the numpy oracle."""
    rng = np.random.RandomState(bucket + 17)
    n = 64 * 1024 + 5
    base = rng.randn(n).astype(np.float32)
    scales = [1.0, 1e-3, 2.0 ** -58, 2.0 ** -61, 1e-30, 1e-37, 1e-39, 2.0 ** 99, 2.0 ** 101, 1e30]
    cases = [(base * np.float32(sc)).astype(np.float32) for sc in scales]
    per = np.repeat(np.array(scales * 400, dtype=np.float64)[: (n + 255) // 256], 256)[:n]
    cases.append((base.astype(np.float64) * per).astype(np.float32))       # a different scale every 256 elements
    # one large element per bucket-ish stretch over tiny ones: numerators 2^-130 .. 2^-80 under alpha = 2^e, e = -10 .. 60
    # -> quotients from deep in the denormal range up to small normal ones, on both sides of both thresholds
    tiny = (np.abs(base).astype(np.float64) + 0.5) * (2.0 ** rng.randint(-130, -80, size=n))
    big_at = rng.rand(n) < 1.0 / 40
    tiny[big_at] = 2.0 ** rng.randint(-10, 60, size=int(big_at.sum()))
    tiny[rng.rand(n) < 0.2] = 0.0
    cases.append(tiny.astype(np.float32))
    exact = np.zeros(n, np.float64)                                          # quotients exactly AT the 2^-120 threshold
    exact[:] = 2.0 ** -100 * rng.randint(0, 5, size=n)
    exact[::37] = 2.0 ** 20
    cases.append(exact.astype(np.float32))
    cases.append(np.where(rng.rand(n) < 0.7, 0.0, base * 1e-41).astype(np.float32))   # zeros next to denormals
    cases.append((np.abs(base) * np.float32(1e-36) + np.float32(1.0)).astype(np.float32))   # alpha < 1e-10 -> 1
    for ci, x in enumerate(cases):
        want = onp.scale_down(x, bucket)
        sf = quantization.ScalingFunction('linear', False, False, bucket)
        u = host(sf.scale_down(dev(x))).reshape(-1)
        wu = want['u'].reshape(-1)
        assert u.size == wu.size
        nan = np.isnan(wu)
        assert np.array_equal(np.isnan(u), nan), (bucket, ci)
        diff = (u.view(np.uint32) != wu.view(np.uint32)) & ~nan
        assert not diff.any(), (bucket, ci, int(diff.sum()), u[diff][:4], wu[diff][:4])
        assert np.array_equal(host(sf.alpha).reshape(-1).view(np.uint32), want['alpha'].reshape(-1).view(np.uint32)), (bucket, ci)
        assert np.array_equal(host(sf.beta).reshape(-1).view(np.uint32), want['beta'].reshape(-1).view(np.uint32)), (bucket, ci)


def test_multi_tensor_bit_exact_at_extreme_scales():
    from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer
    rng = np.random.RandomState(5)
    xs = [(rng.randn(4096 + 77 * i) * sc).astype(np.float32) for i, sc in
          enumerate([1.0, 2.0 ** -59, 2.0 ** -62, 1e-38, 1e-42, 2.0 ** 100, 2.0 ** 102, 1e-3])]
    mt = MultiTensorQuantizer([dev(x) for x in xs], 16, 256)
    for x, q in zip(xs, mt.quantize()):
        assert np.array_equal(host(q), oc.uniform_quantize(x, 16, 256, want_idx=False, want_lev=False)['q'], equal_nan=True)
