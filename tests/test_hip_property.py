"""Property-based GPU parity (hypothesis): random sizes, bucket sizes, level counts, value
distributions and options, HIP path vs the C oracle, bit-exact."""
import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

import quantization
from oracle import oracle_c as oc

import errlog

import os

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SOAK = int(os.environ.get('QD_SOAK', '1'))        # QD_SOAK=10 multiplies the number of examples (soak runs)

buckets = st.sampled_from([None, 256, 256, 64, 128, 512, 1024, 2048, 4096, 100, 7, 1, 33, 1000, 4, 12, 36, 300, 2000, 8192, 8196, 5, 50, 250, 511, 513, 3, 1001, 1023, 450, 509, 770, 3000, 5003, 8190])
sizes = st.one_of(st.integers(1, 5000), st.integers(5000, 300000))
levels = st.sampled_from([2, 3, 4, 7, 16, 16, 255, 256, 1000])

# the default run draws a fixed example sequence (the same cases on every box); soak runs explore
settings.register_profile('qd', derandomize=(SOAK == 1), database=None)
settings.load_profile('qd')


NONFINITE = 9                                     # the `kind` of make() that plants NaN / +-inf


def make(n, seed, kind):
    rng = np.random.RandomState(seed)
    if kind == 0:
        x = rng.randn(n)
    elif kind == 1:
        x = rng.randn(n) * 1e-3 + 5.0
    elif kind == 2:
        x = rng.randint(-4, 5, size=n).astype(np.float64)          # ties everywhere
    elif kind == 3:
        x = np.full(n, 0.25)                                       # alpha guard
    elif kind == 4:
        x = rng.standard_cauchy(n)                                 # heavy tails / huge ranges
    elif kind == 5:
        x = rng.rand(n) * 1e-30                                    # tiny magnitudes (alpha < 1e-10 -> 1)
    elif kind == 6:
        # any power-of-two scale: both sides of the bucket-invariant-division range [2^-60, 2^100], denormals, near-overflow
        with np.errstate(over='ignore', under='ignore'):
            x = np.ldexp(rng.randn(n), int(rng.randint(-148, 122)))
    elif kind == 7:
        # a different scale every few hundred elements (buckets of one wave fall on both sides of the range)
        with np.errstate(over='ignore', under='ignore'):
            e = np.repeat(rng.randint(-140, 120, size=n // 97 + 1), 97)[:n]
            x = np.ldexp(rng.randn(n), e)
    elif kind == NONFINITE:
        # NaN, +inf and -inf at seeded positions, the first and the last element among them; no nan_to_num below
        x = rng.randn(n)
        where = np.unique(np.concatenate([[0, n - 1], rng.randint(0, n, size=4)]))
        x[where] = np.array([np.nan, np.inf, -np.inf])[rng.randint(0, 3, size=where.size)]
        x[0] = np.nan if n < 3 else x[0]
        return x.astype(np.float32)
    else:
        x = np.where(rng.rand(n) < 0.6, 0.0, rng.randn(n) * 1e-40) + (rng.rand(n) < 0.001) * 1.0   # zeros, denormals, a few ones
    return np.nan_to_num(x.astype(np.float32), nan=0.0, posinf=3e38, neginf=-3e38)


@settings(max_examples=60 * SOAK, deadline=None, suppress_health_check=list(HealthCheck))
@given(n=sizes, bucket=buckets, s=levels, seed=st.integers(0, 2 ** 31 - 1), kind=st.integers(0, 9),
       clamp=st.sampled_from([False, False, 0.5, 2.0]))
def test_uniform_matches_oracle(n, bucket, s, seed, kind, clamp):
    x = make(n, seed, kind)
    q, sf = quantization.uniformQuantization(torch.from_numpy(x).to(DEV), s, bucket_size=bucket, max_element=clamp)
    r = oc.uniform_quantize(x, s, bucket, max_element=clamp)
    assert np.array_equal(q.cpu().numpy(), r['q'], equal_nan=True)
    assert np.array_equal(sf.alpha.cpu().numpy().reshape(-1), r['alpha'], equal_nan=True)
    assert np.array_equal(sf.beta.cpu().numpy().reshape(-1), r['beta'], equal_nan=True)
    assert np.array_equal(sf.idx_min_rows.cpu().numpy().reshape(-1), r['imin'])
    assert np.array_equal(sf.idx_max_rows.cpu().numpy().reshape(-1), r['imax'])


@settings(max_examples=40 * SOAK, deadline=None, suppress_health_check=list(HealthCheck))
@given(n=sizes, bucket=buckets, k=st.sampled_from([1, 2, 3, 4, 5, 16, 17, 64, 200, 600]), seed=st.integers(0, 2 ** 31 - 1),
       kind=st.integers(0, 3), dup=st.booleans())
def test_nonuniform_matches_oracle(n, bucket, k, seed, kind, dup):
    x = make(n, seed, kind)
    rng = np.random.RandomState(seed ^ 0x5bd1)
    pts = np.sort(rng.rand(k)).astype(np.float32)
    if dup and k > 2:
        pts[1] = pts[0]
        pts[-1] = pts[-2]
    xd, pd = torch.from_numpy(x).to(DEV), torch.from_numpy(pts).to(DEV)
    q, idx, sf = quantization.nonUniformQuantization(xd, pd, bucket_size=bucket)
    r = oc.nonuniform_quantize(x, pts, bucket, 'distance')
    assert np.array_equal(idx.cpu().numpy(), r['idx']) and np.array_equal(q.cpu().numpy(), r['q'])
    fn = quantization.nonUniformQuantization_variable(bucket_size=bucket, pre_process_tensors=True, tensor=xd)
    qm = fn.forward(None, pd)
    rm = oc.nonuniform_quantize(x, pts, bucket, 'midpoint')
    assert np.array_equal(fn.savedForBackward['indices'].cpu().numpy(), rm['idx'])
    assert np.array_equal(qm.cpu().numpy(), rm['q'])
    g = rng.randn(n).astype(np.float32)
    _, gp = fn.backward(torch.from_numpy(g).to(DEV))
    want, absum = oc.point_grad(g, rm['idx'], rm['alpha'], bucket, k)
    errlog.check_sum('K6 point gradient, property soak (any n / bucket / k)', gp.cpu().numpy(), want, absum, (n, bucket, k, seed), n_terms=n)


@settings(max_examples=30 * SOAK, deadline=None, suppress_health_check=list(HealthCheck))
@given(n=sizes, bucket=st.sampled_from([64, 128, 256, 256, 512, 1024, 2048, None, 100, 33, 7, 3, 1000, 513, 4096, 5003]),
       sb=st.sampled_from([(2, 1), (3, 2), (4, 2), (9, 4), (16, 4), (16, 8), (256, 8)]),
       seed=st.integers(0, 2 ** 31 - 1), kind=st.sampled_from([0, 1, 2, 3, 4, 5, NONFINITE]))
def test_pack_unpack_matches_quantizer(n, bucket, sb, seed, kind):
    from quantized_distillation_amd import codec
    s, bits = sb
    x = make(n, seed, kind)
    xd = torch.from_numpy(x).to(DEV)
    pk = codec.pack_uniform(xd, s, bucket, bits=bits)
    q, _ = quantization.uniformQuantization(xd, s, bucket_size=bucket)
    assert np.array_equal(pk.unpack().cpu().numpy(), q.cpu().numpy(), equal_nan=True)
    r = oc.uniform_quantize(x, s, bucket)
    assert np.array_equal(codec.level_histogram(xd, s, bucket).cpu().numpy(), np.bincount(r['lev'], minlength=s))


@settings(max_examples=30 * SOAK, deadline=None, suppress_health_check=list(HealthCheck))
@given(n=sizes, bucket=st.sampled_from([64, 128, 256, 512, 1024, 100, 7]), s=st.sampled_from([2, 4, 16, 256]),
       seed=st.integers(0, 2 ** 31 - 1), kind=st.integers(0, 3))
def test_ste_backward_matches_oracle(n, bucket, s, seed, kind):
    x = make(n, seed, kind)
    g = np.random.RandomState(seed ^ 77).randn(n).astype(np.float32)
    fn = quantization.uniformQuantization_variable(s, bucket_size=bucket)
    fn.forward(torch.from_numpy(x).to(DEV))
    out = fn.backward(torch.from_numpy(g).to(DEV)).cpu().numpy()
    ref = oc.ste_complicated_backward(x, g, s, bucket)
    errlog.check_ste('K7 bucket sum, property soak', out, x, g, s, bucket, (n, bucket, s, seed, kind))
    atol = 1e-6 * (np.abs(g).mean() + 1e-30) * min(bucket, n) + 1e-30          # "clearly visible" threshold below
    # tie rule: only the first arg-min / arg-max of each bucket of the QUANTIZED tensor may be touched.  (A
    # correction below half an ulp of g leaves g unchanged, and whether it does depends on the summation
    # order, so "touched" is compared as a subset plus the positions whose correction is clearly visible.)
    q = oc.uniform_quantize(x, s, bucket)['q']
    row = min(bucket, n)
    nb = -(-n // row)
    qp = np.concatenate([q, np.full(nb * row - n, q[-1], np.float32)]).reshape(nb, row)
    base = np.arange(nb) * row
    allowed = np.zeros(nb * row, bool)
    allowed[base + qp.argmin(1)] = True
    allowed[base + qp.argmax(1)] = True
    assert not np.any((out != g) & ~allowed[:n])
    visible = np.abs(ref - g) > 4 * atol + 4 * np.spacing(np.abs(g))
    assert np.all((out != g)[visible])


@settings(max_examples=25 * SOAK, deadline=None, suppress_health_check=list(HealthCheck))
@given(sizes_=st.lists(st.one_of(st.integers(1, 300), st.integers(300, 70000)), min_size=1, max_size=12),
       bucket=st.sampled_from([None, 256, 256, 64, 128, 100, 7, 1024]), s=st.sampled_from([2, 4, 16, 256]),
       seed=st.integers(0, 2 ** 31 - 1), kind=st.integers(0, 6), misalign=st.booleans())
def test_multi_tensor_matches_oracle(sizes_, bucket, s, seed, kind, misalign):
    """One launch over a random set of tensors (carved out of one flat buffer, optionally at odd element
    offsets so that some bases are not 16-byte aligned) == the oracle on each tensor."""
    from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer
    kinds = (0, 1, 2, 3, 4, 5, NONFINITE)
    xs = [make(n, seed + 13 * i, kinds[(kind + i) % 7]) for i, n in enumerate(sizes_)]
    gap = 3 if misalign else 0
    total = sum(n + gap for n in sizes_)
    flat_in = torch.zeros(total, device=DEV)
    flat_out = torch.full((total,), 777.0, device=DEV)
    ins, outs, off = [], [], 0
    for x in xs:
        off += gap
        ins.append(flat_in[off:off + x.size]); outs.append(flat_out[off:off + x.size])
        ins[-1].copy_(torch.from_numpy(x))
        off += x.size
    mt = MultiTensorQuantizer(ins, s, bucket, outputs=outs)
    mt.quantize()
    for x, o in zip(xs, outs):
        r = oc.uniform_quantize(x, s, bucket, want_idx=False, want_lev=False)
        assert np.array_equal(o.cpu().numpy(), r['q'], equal_nan=True)
    if gap:                                                            # nothing written between the tensors
        keep = torch.ones(total, dtype=torch.bool)
        off = 0
        for x in xs:
            off += gap
            keep[off:off + x.size] = False
            off += x.size
        assert bool((flat_out.cpu()[keep] == 777.0).all())


@settings(max_examples=25 * SOAK, deadline=None, suppress_health_check=list(HealthCheck))
@given(n=sizes, bucket=buckets, s=levels, seed=st.integers(0, 2 ** 31 - 1), kind=st.integers(0, 2),
       clamp=st.sampled_from([False, 0.5, 2.0]))
def test_uniform_subtract_mean_matches_oracle(n, bucket, s, seed, kind, clamp):
    """subtract_mean=True: the mean is a float64-accumulated device reduction (qd_mean_f32); the oracle is given
    the device's mean so that the comparison of everything downstream stays bit-exact, and the mean itself
    is checked against numpy's float64 mean to 1 ulp-ish."""
    x = make(n, seed, kind)
    xd = torch.from_numpy(x).to(DEV)
    q, sf = quantization.uniformQuantization(xd, s, bucket_size=bucket, subtract_mean=True, max_element=clamp)
    mean = float(sf.mean_tensor)
    ref_mean = float(np.float32(x.astype(np.float64).mean()))
    errlog.check_mean('qd_mean_f32, property soak', mean, x.astype(np.float64).mean(), float(np.abs(x.astype(np.float64)).mean()),
                      (n, seed, kind), n_terms=n)
    r = oc.uniform_quantize(x, s, bucket, max_element=clamp, subtract_mean=True, mean=mean, want_idx=False, want_lev=False)
    assert np.array_equal(q.cpu().numpy(), r['q'])
    assert np.array_equal(sf.alpha.cpu().numpy().reshape(-1), r['alpha'])
    assert np.array_equal(sf.beta.cpu().numpy().reshape(-1), r['beta'])


@settings(max_examples=40 * SOAK, deadline=None, suppress_health_check=list(HealthCheck))
@given(n=sizes, bucket=buckets, s=st.sampled_from([2, 4, 16, 16, 255, 256]), seed=st.integers(0, 2 ** 31 - 1), kind=st.integers(0, 8),
       off=st.sampled_from([0, 0, 1, 3]))
def test_level_and_digitize_histograms_match_numpy(n, bucket, s, seed, kind, off):
    """The counting kernels of the size accounting (round 4): the level histogram of a tensor (one pass at the vector bucket
    sizes, levels + count elsewhere) against the C oracle's levels, and the digitize + histogram of the re-scaled quantized
    tensor against np.digitize with the reference's float64 edges (quantization/help_functions.py:213-223)."""
    import quantization.help_functions as qhf
    from quantized_distillation_amd import codec
    x = make(n + off, seed, kind)[off:]
    xd = torch.from_numpy(make(n + off, seed, kind)).to(DEV)[off:]
    h = codec.level_histogram(xd, s, bucket)
    assert np.array_equal(h.cpu().numpy(), np.bincount(oc.uniform_quantize(x, s, bucket)['lev'], minlength=s))
    q, sf = quantization.uniformQuantization(xd, s, bucket_size=bucket)
    scaled = sf.scale_down(q).view(-1)[0:sf.original_tensor_length]
    edges = qhf._digitize_edges(s, 1e-5)
    got = qhf._device_counts('digitize', scaled, s, torch.from_numpy(edges).to(DEV))
    want = np.bincount(np.digitize(scaled.cpu().numpy(), edges), minlength=s + 1)
    assert np.array_equal(got.cpu().numpy(), want)
