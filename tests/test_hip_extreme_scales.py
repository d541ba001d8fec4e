"""The bucket-invariant division (csrc/qd_common.h: y = RN(1 / alpha) once per bucket, two FMAs per element) on every path
that consumes it, at the inputs where it can be wrong (tests/extreme_scale_cases.py):

  * where the QUOTIENT is consumed -- scale_down (K2), the one-pass re-scale + digitize histogram, and the 'complicated' STE
    backward (K7, K7m) -- buckets that hold a pair (n, alpha) of tests/golden/div_denormal_pairs.json: alpha in range, n >=
    2^-100, a denormal quotient on which the shortcut differs from the IEEE division.  Only the `alpha 2^-120` clause of
    scale_fast_ok keeps the shortcut away from them;
  * where only the LEVEL is consumed, alpha exactly on 2^-60 and 2^100 and one float to either side, on every site that
    chooses between the two forms by fastdiv_ok.

Every comparison is on bits, against oracle_np / oracle_c (IEEE divisions); the one tolerance is errlog's for the fp32 bucket
sum of K7 with a dense gradient.  The tests that work on any tensor run again on CPU tensors in tests/test_host_parity.py
(libqd_host.so divides by IEEE: that run also proves inputs and expectations right)."""
import numpy as np
import pytest
import torch

import quantization
import quantization.help_functions as qhf
import quantization.quant_functions as qf
from oracle import oracle_c as oc
from oracle import oracle_np as onp
from quantized_distillation_amd import _lib, ste

import errlog
import extreme_scale_cases as C
import test_hip_parity as P

pytestmark = pytest.mark.gpu

REGISTER_BUCKETS = [64, 256, 1024]          # ste_vec_tile: 16 lanes per bucket (64, 256) and 64 (1024)
WAVE_BUCKETS = [33, 100, 1000]              # ste_wave_bucket
LEVELS = [4, 16, 256]
TIE_MODES = ['reference', 'true_arg']


@pytest.fixture(scope='module', autouse=True)
def _need_library():
    oc.build()


def dev(a):
    return P.dev(a)                         # P.DEV at the time of the call: 'cuda:0', or 'cpu' under tests/test_host_parity.py


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).reshape(-1).view(np.uint32)


def assert_same_bits(got, want, tag):
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    assert got.shape == want.shape, tag
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), tag
    diff = (bits(got) != bits(want)) & ~nan
    assert not diff.any(), (tag, int(diff.sum()), np.flatnonzero(diff)[:4], got[diff][:4], want[diff][:4])


_ORACLE = {}


def ste_oracle(bucket, s, tie_mode, with_beta):
    """(x, g, expected out) of the one-term-per-bucket case: computed once, shared, never written."""
    key = (bucket, s, tie_mode, with_beta)
    if key not in _ORACLE:
        x = C.pair_tensor(bucket, with_beta)
        g = C.pair_gradient(bucket, x.size, dense=False)
        want = onp.ste_complicated_backward(x, g, s, bucket, tie_mode)
        pn, pmin, pmax = C.pair_positions(bucket, x.size)
        # the case is what it claims to be: S = -g (n / alpha) != 0 lands at the maximum, -S at the minimum, g elsewhere
        assert np.all(want[pmax] != 0) and np.array_equal(want[pmax], -want[pmin]) and np.array_equal(want[pn], g[pn])
        _ORACLE[key] = (x, g, want)
    return _ORACLE[key]


# ---------------------------------------------------------------------------------------------------- K7: the STE backward
@pytest.mark.parametrize('s', LEVELS)
@pytest.mark.parametrize('bucket', REGISTER_BUCKETS + WAVE_BUCKETS)
def test_ste_backward_one_term_per_bucket_is_bit_exact_on_denormal_quotients(bucket, s):
    """g is zero except 2^100 at each pair's element, so every bucket sum is the single term -g (n / alpha): no summation
    order, no tolerance.  uniformQuantization_variable.backward and ste.ste_bucket_backward, both tie modes, beta = 0 and
    beta != 0, against the oracle's IEEE quotient bit for bit."""
    for with_beta in (False, True):
        for tie_mode in TIE_MODES:
            x, g, want = ste_oracle(bucket, s, tie_mode, with_beta)
            fn = quantization.uniformQuantization_variable(s, bucket_size=bucket)
            fn.forward(dev(x))
            assert_same_bits(host(fn.backward(dev(g), tie_mode)), want, ('variable', bucket, s, tie_mode, with_beta))
            out = ste.ste_bucket_backward(dev(x), dev(g), bucket, s, tie_mode=tie_mode)
            assert_same_bits(host(out), want, ('ste_bucket_backward', bucket, s, tie_mode, with_beta))


@pytest.mark.parametrize('s', LEVELS)
@pytest.mark.parametrize('bucket', REGISTER_BUCKETS + WAVE_BUCKETS)
def test_ste_backward_dense_gradient_within_the_bucket_sum_tolerance(bucket, s):
    """A dense gradient on the pair buckets (the pair's element weighted 2^125 .. 2^126: a quotient wrong by one denormal ulp is
    up to 2^-12 of the sum of the magnitudes) and on the boundary-alpha buckets (K7's own forward chooses by fastdiv_ok):
    errlog.check_ste at its own tolerance, both tie modes."""
    for name, x in (('pairs', C.pair_tensor(bucket)), ('pairs + beta', C.pair_tensor(bucket, True)),
                    ('boundary alphas', C.boundary_tensor(bucket))):
        g = C.pair_gradient(bucket, x.size, dense=True) if name != 'boundary alphas' else \
            np.random.RandomState(bucket).randn(x.size).astype(np.float32)
        for tie_mode in TIE_MODES:
            out = host(ste.ste_bucket_backward(dev(x), dev(g), bucket, s, tie_mode=tie_mode))
            ratio = errlog.check_ste('K7 at extreme scales (%s)' % name, out, x, g, s, bucket, (name, bucket, s, tie_mode),
                                     tie_mode=tie_mode)
            print('K7 %s bucket %d s %d %s: error / sum|terms| = %.3g' % (name, bucket, s, tie_mode, ratio))


@pytest.mark.parametrize('bucket', REGISTER_BUCKETS + WAVE_BUCKETS)
def test_multi_tensor_ste_equals_the_per_tensor_call_and_the_oracle(bucket):
    """The same lists through MultiTensorSTE (K7m), with one level count and with a level count per tensor: bit-identical to
    ste.ste_bucket_backward tensor by tensor, and -- the one-term gradients -- to the oracle."""
    from quantized_distillation_amd.multi_tensor import MultiTensorSTE
    for tie_mode in TIE_MODES:
        for levels in (4, 16, 256, [4, 16, 256, 16, 4]):
            per = levels if isinstance(levels, list) else [levels] * 5
            cases = [ste_oracle(bucket, per[0], tie_mode, False), ste_oracle(bucket, per[1], tie_mode, True),
                     ste_oracle(bucket, per[2], tie_mode, False)]
            xs = [c[0] for c in cases] + [C.pair_tensor(bucket, True), C.boundary_tensor(bucket)]
            gs = [c[1] for c in cases] + [C.pair_gradient(bucket, xs[3].size, True), C.pair_gradient(bucket, xs[4].size, True, seed=1)]
            xd, gd = [dev(x) for x in xs], [dev(g) for g in gs]
            outs = [torch.full_like(g, float('nan')) for g in gd]
            mt = MultiTensorSTE(xd, gd, levels, bucket, outs=outs, tie_mode=tie_mode)
            got = mt.backward()
            assert mt.entry_point == ('qd_multi_ste_backward_levels_f32' if isinstance(levels, list) else 'qd_multi_ste_backward_f32')
            for i, (x, g, o) in enumerate(zip(xd, gd, got)):
                want = ste.ste_bucket_backward(x, g, bucket, per[i], tie_mode=tie_mode)
                assert_same_bits(host(o), host(want), ('K7m vs per-tensor', bucket, levels, tie_mode, i))
            for i, c in enumerate(cases):
                assert_same_bits(host(got[i]), c[2], ('K7m vs oracle', bucket, levels, tie_mode, i))


# ------------------------------------------------------------------------------- K2 and the one-pass re-scale + digitize
@pytest.mark.parametrize('bucket', [256, 64, 1024, 100, 33])
def test_scale_down_bit_exact_on_denormal_quotients(bucket):
    """ScalingFunction.scale_down returns u itself: on the pair buckets every bit of u, alpha and beta against oracle_np."""
    for name in ('pairs', 'pairs + beta', 'boundary alphas'):
        x = dict(C.cases(bucket))[name]
        want = onp.scale_down(x, bucket)
        sf = quantization.ScalingFunction('linear', False, False, bucket)
        u = host(sf.scale_down(dev(x)))
        assert_same_bits(u, want['u'], ('u', name, bucket))
        assert_same_bits(host(sf.alpha), want['alpha'], ('alpha', name, bucket))
        assert_same_bits(host(sf.beta), want['beta'], ('beta', name, bucket))
        if name == 'pairs':                                      # the case is what it claims to be
            pn, _, _ = C.pair_positions(bucket, x.size)
            ieee = np.array([n / a for n, a in C.pairs()], np.float32)
            assert np.array_equal(want['u'].reshape(-1)[pn[:-1]], ieee) and np.all(ieee < np.float32(2.0 ** -126)) and np.all(ieee > 0)


def pair_edges():
    """float64 digitize edges at the midpoints between the shortcut's and the IEEE quotient of every pair: whichever of the two
    a kernel computes decides the bin."""
    import json
    with open(C.PAIRS_JSON) as f:
        ps = json.load(f)['pairs']
    return np.unique(np.array([(p['shortcut'] + p['ieee']) / 2 for p in ps], dtype=np.float64))


@pytest.mark.parametrize('bucket', list(qhf.FUSED_DIGITIZE_BUCKETS))
def test_one_pass_rescale_digitize_histogram_on_denormal_quotients(bucket):
    """qd_scale_digitize_histogram_f32 on the pair buckets with an edge between the two candidate quotients of every pair:
    the counters of numpy's digitize of the oracle's u, and of the two-call form (scale_down, then digitize + count)."""
    edges = pair_edges()
    assert 16 <= edges.size <= qhf.DEVICE_HISTOGRAM_MAX_SYMBOLS
    edges_dev = torch.from_numpy(edges).to(P.DEV)
    for with_beta in (False, True):
        x = C.pair_tensor(bucket, with_beta)
        u = onp.scale_down(x, bucket)['u'].reshape(-1)[:x.size]
        want = np.bincount(np.digitize(u, edges), minlength=edges.size + 1)
        assert np.count_nonzero(want) > 16                        # the pairs spread over the bins
        xd = dev(x)
        sf = quantization.ScalingFunction('linear', False, False, bucket_size=bucket)
        got = qhf._fused_rescale_counts(xd, sf, edges.size, edges_dev)
        assert got is not None
        two = qhf._device_counts('digitize', sf.scale_down(xd).view(-1)[0:x.size], edges.size, edges_dev)
        assert np.array_equal(host(got), want), (bucket, with_beta, host(got), want)
        assert np.array_equal(host(two), want), (bucket, with_beta, 'two-call form')


# ------------------------------------------------------------------------------------- level-only consumers, per tensor
def check_k1(x, s, bucket, tag):
    want = oc.uniform_quantize(x, s, bucket, want_idx=False, want_lev=False)
    q, sf = quantization.uniformQuantization(dev(x), s, bucket_size=bucket)
    assert_same_bits(host(q), want['q'], ('q',) + tag)
    assert_same_bits(host(sf.alpha), want['alpha'], ('alpha',) + tag)
    assert_same_bits(host(sf.beta), want['beta'], ('beta',) + tag)


def check_k1_stochastic(x, s, bucket, tag):
    seed = qf.next_stochastic_seed(peek=True, host=not dev(x[:1]).is_cuda)
    q, sf = quantization.uniformQuantization(dev(x), s, stochastic_rounding=True, bucket_size=bucket)
    _, _, padded = onp.bucket_geometry(x.size, bucket)
    rand = np.zeros(padded, np.float32)
    rand[:x.size] = onp.philox4x32_7_uniform(seed, x.size)
    want = onp.uniform_quantize_stochastic(x, s, rand, bucket)
    assert_same_bits(host(q), want['q'], ('stochastic q',) + tag)
    assert_same_bits(host(sf.alpha), want['alpha'], ('stochastic alpha',) + tag)


@pytest.mark.parametrize('bucket', [513, 2049, 5000, 256, 100])
def test_quantize_on_the_alpha_boundaries(bucket):
    """Per-tensor K1 with alpha exactly 2^-60 / 2^100 and one float to either side, at bucket sizes of the wave kernel (513,
    2049; 5000: a bucket spread over several waves) and of the vector / chunk kernels: q, alpha, beta bit-exact for 4, 16 and
    256 levels, deterministic and stochastic (against the Philox restatement)."""
    for name, x in C.cases(bucket):
        if name.startswith('pairs') and bucket > 1024:
            continue
        for s in LEVELS:
            check_k1(x, s, bucket, (name, bucket, s))
            if name in ('boundary alphas', 'pairs', 'mixed scale per bucket'):
                check_k1_stochastic(x, s, bucket, (name, bucket, s))


@pytest.mark.parametrize('n', [1000, 16385])
def test_quantize_without_buckets_on_the_alpha_boundaries(n):
    """bucket_size=None at a size of the one-block kernel and at the smallest of the one-launch kernel."""
    for name, x in C.cases(None, n):
        for s in LEVELS:
            check_k1(x, s, None, (name, n, s))
            check_k1_stochastic(x, s, None, (name, n, s))


@pytest.mark.parametrize('mode', [1, 0], ids=['fused', 'three-launch'])
@pytest.mark.parametrize('n', [16385, 300001])
def test_single_bucket_launchers_on_the_alpha_boundaries(n, mode):
    """The single-bucket launchers (one launch, three launches) at a single-small and a single-large size."""
    lib = _lib.load()
    lib.qd_set_single_fused_mode(mode)
    try:
        for name, x in C.single_bucket_cases(n):
            for s in (16, 4, 256):
                check_k1(x, s, None, (name, n, s, mode))
            check_k1_stochastic(x, 16, None, (name, n, mode))
    finally:
        lib.qd_set_single_fused_mode(-1)


# ----------------------------------------------------------------------------------------- level-only consumers, codec
@pytest.mark.parametrize('bucket', [256, 64, 2048, 100, None])
def test_level_histogram_levels_only_and_pack_on_the_alpha_boundaries(bucket):
    """The kernels of csrc/qd_codec.hip that compute levels without writing q: the level histogram, the levels-only form of
    qd_uniform_f32 (q = NULL), pack -> unpack: counts, level indices, packed bytes, alpha / beta and the decoded values
    against the C oracle."""
    from quantized_distillation_amd import codec
    lib = _lib.load()
    named = list(C.cases(bucket, 3000)) if bucket is None else [(k, v) for k, v in C.cases(bucket) if not k.startswith('pairs')]
    for name, x in named:
        n = x.size
        xd = dev(x)
        for s in LEVELS:
            ref = oc.uniform_quantize(x, s, bucket)
            lev = ref['lev'].reshape(-1)[:n]
            h = codec.level_histogram(xd, s, bucket)
            assert np.array_equal(host(h), np.bincount(lev, minlength=s)), (name, bucket, s, 'histogram')
            if bucket in codec._FUSED_BUCKETS:
                out = torch.full((n,), 255, dtype=torch.uint8, device=xd.device)
                ab = torch.full((2, -(-n // bucket)), float('nan'), device=xd.device)
                ws = _lib.workspace(xd.device)
                _lib.check(lib.qd_uniform_f32(xd.data_ptr(), None, n, bucket, s, ab[0].data_ptr(), ab[1].data_ptr(), out.data_ptr(), None,
                                              0, 0.0, 0, 0, ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
                assert np.array_equal(host(out), lev.astype(np.uint8)), (name, bucket, s, 'levels only')
                assert_same_bits(host(ab[0]), ref['alpha'], (name, bucket, s, 'levels only alpha'))
            bits_ = codec.bits_for_levels(s)
            pk = codec.pack_uniform(xd, s, bucket, bits=bits_)
            assert np.array_equal(host(pk.packed), P_pack(lev, bits_)), (name, bucket, s, 'packed bytes')
            assert_same_bits(host(pk.alpha), ref['alpha'], (name, bucket, s, 'pack alpha'))
            assert_same_bits(host(pk.beta), ref['beta'], (name, bucket, s, 'pack beta'))
            assert_same_bits(host(pk.unpack()), ref['q'], (name, bucket, s, 'unpack'))


def P_pack(lev, nbits):
    """numpy packing of level indices, little endian inside a byte (as tests/test_hip_parity.py::test_pack_unpack_roundtrip)."""
    epb = 8 // nbits
    levp = np.concatenate([lev.astype(np.uint64), np.zeros((-lev.size) % epb, np.uint64)]).reshape(-1, epb)
    want = np.zeros(levp.shape[0], np.uint64)
    for c in range(epb):
        want |= levp[:, c] << np.uint64(c * nbits)
    return want.astype(np.uint8)


# ---------------------------------------------------------------------------- level-only consumers, the one-launch quantizer
def _mt_list(bucket):
    if bucket is None:
        return [x for _, x in C.cases(None, 3000)] + [x for _, x in C.single_bucket_cases(1025, seed=7)]
    return [x for _, x in C.cases(bucket)]


@pytest.mark.parametrize('bucket', [None, 256, 100])
def test_multi_tensor_quantizer_on_the_alpha_boundaries(bucket):
    """MultiTensorQuantizer (K9) without buckets and bucketed; one level count and a level count per tensor; plain, with
    max_element = 2^100 (which clamps the buckets above it ONTO the boundary) and with stochastic rounding against the Philox
    restatement at seed0 + i: q bit-exact against the oracles, and alpha / beta where the launch reports them."""
    from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer
    xs = _mt_list(bucket)
    xd = [dev(x) for x in xs]
    per_tensor = [LEVELS[i % 3] for i in range(len(xs))]
    for levels in (4, 16, 256, per_tensor):
        per = levels if isinstance(levels, list) else [levels] * len(xs)
        for me in (False, 2.0 ** 100):
            mt = MultiTensorQuantizer(xd, levels, bucket, max_element=me)
            for i, (x, q) in enumerate(zip(xs, mt.quantize())):
                want = oc.uniform_quantize(x, per[i], bucket, max_element=me, want_idx=False, want_lev=False)
                assert_same_bits(host(q), want['q'], ('K9', bucket, levels, me, i))
                if bucket is None:
                    assert_same_bits(host(mt.alpha_beta[i]), [want['alpha'].reshape(-1)[0], want['beta'].reshape(-1)[0]],
                                     ('K9 alpha beta', levels, me, i))
            seed0 = 0x5EED0000 + (bucket or 0)
            mt = MultiTensorQuantizer(xd, levels, bucket, stochastic_rounding=True, max_element=me)
            for i, (x, q) in enumerate(zip(xs, mt.quantize(seed=seed0))):
                _, _, padded = onp.bucket_geometry(x.size, bucket)
                rand = np.zeros(padded, np.float32)
                rand[:x.size] = onp.philox4x32_7_uniform(seed0 + i, x.size)
                want = onp.uniform_quantize_stochastic(x, per[i], rand, bucket, max_element=me)
                assert_same_bits(host(q), want['q'], ('K9 stochastic', bucket, levels, me, i))
