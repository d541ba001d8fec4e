"""The level count s on every device path that takes one, at every entry of the ladder of tests/level_cases.py: 2 .. 17
(every length of the ds_bpermute level table and the first computed division), the bit widths 5 .. 8 and their neighbours,
the values around 2^23 and 2^24 where sm1 = (float)(s - 1) fills the significand and then rounds, and 2^31 - 1 where it passes
INT_MAX.  tools/launch_coverage.py counts kernel names; the branch on `p.sm1 <= 15.0f` lives inside one name, so only values
see it.

Everything is compared with the oracle (oracle_np: it takes every s of the ladder), bit for bit; the two exceptions are the
ones the suite already has -- the fp32 bucket sum of K7 with a dense gradient (errlog.check_ste) and the absnorm norm
(abs_cases.BOUND).  tests/test_level_cases_host.py holds the oracle to the reference on the same ladder and runs the shared
checks of level_cases on CPU tensors.  Shapes are the smallest that reach each launcher path (tests/abi_contract.py:
BUCKET_PATHS at the ragged length, SINGLE_SMALL, SINGLE_LARGE, FUSED_MODES, _k1_extra)."""
import numpy as np
import pytest
import torch

import quantization
from oracle import oracle_c as oc
from oracle import oracle_np as onp
from quantized_distillation_amd import _lib, codec, ste
from quantized_distillation_amd import compressed as C
from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer, MultiTensorSTE

import abi_contract as A
import abs_cases as ac
import level_cases as L
import stochastic_cases as SC

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def _built():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    _lib.load()
    oc.build()


def ragged(bucket, nfull):
    """The ragged length of a launcher path: nfull whole buckets and a last bucket of 1 .. 3 elements."""
    return A.lengths(bucket, nfull, 1 + bucket % 3)[1]


# ---------------------------------------------------------------------------------------------------- K1
@pytest.mark.parametrize('bucket,nfull', [(b, f) for b, f, _ in A.BUCKET_PATHS], ids=['b%d-nf%d' % (b, f) for b, f, _ in A.BUCKET_PATHS])
def test_k1_every_bucket_path_on_the_ladder(bucket, nfull):
    """q, alpha, beta of uniformQuantization, deterministic and stochastic (the Philox restatement with the peeked seed)."""
    L.check_k1_ladder(DEV, ragged(bucket, nfull), bucket, 100 + bucket)


@pytest.mark.parametrize('n', [n for n, _ in A.SINGLE_SMALL])
def test_k1_single_bucket_small_on_the_ladder(n):
    L.check_k1_ladder(DEV, n, None, 200)


@pytest.mark.parametrize('n', [A.SINGLE_LARGE[0][0], A.SINGLE_LARGE[1][0]])
def test_k1_single_bucket_large(n):
    """k_single_fused<V = 4> and the reduce + apply pair above kFusedMaxN, at the ends of the ladder and both sides of the table."""
    L.check_k1_ladder(DEV, n, None, 201, ladder=L.SPARSE)


@pytest.mark.parametrize('n,bucket', [(2563, 256), (65 * 33 + 2, 33), (6001, 1000), (1000, None), (70001, None)])
def test_k1_max_element_and_subtract_mean_on_the_ladder(n, bucket):
    L.check_k1_options(DEV, n, bucket, 202)


@pytest.mark.parametrize('mode', [m for m, _ in A.FUSED_MODES])
def test_k1_fused_mode_hooks(mode):
    """qd_set_single_fused_mode: three launches, every / some / one block giving up, at n = 70001."""
    lib = _lib.load()
    prev = lib.qd_set_single_fused_mode(mode)
    try:
        L.check_k1_ladder(DEV, 70001, None, 203, ladder=L.FUSED_S)
    finally:
        lib.qd_set_single_fused_mode(prev)


# ---------------------------------------------------------------------------------------------------- K7
@pytest.mark.parametrize('bucket,nfull', [(64, 10), (256, 10), (1024, 10), (100, 21), (513, 6)])
def test_k7_ste_backward_on_the_ladder(bucket, nfull):
    """qd_ste_bucket_backward_f32: the register tiles (64, 256, 1024) and a wave per bucket (100, 513), both tie modes."""
    L.check_k7(DEV, ragged(bucket, nfull), bucket, 300 + bucket)


# ---------------------------------------------------------------------------------------------------- K9 / K7m
SIZES = (1, 3, 255, 256, 257, 1023, 1025, 2053, 4097)


def model(seed):
    """One tensor per ladder entry, the sizes cycling: the waves of one block belong to tensors on both sides of the table
    and of 2^24."""
    return [L.inputs(SIZES[i % len(SIZES)], seed + i) for i in range(len(L.LADDER))]


def per_tensor(x, s, bucket, **kw):
    return L.host(quantization.uniformQuantization(L.to(DEV, x), s, bucket_size=bucket, **kw)[0])


@pytest.mark.parametrize('bucket', [256, 100, None])
def test_multi_tensor_quantizer_a_level_count_per_tensor(bucket):
    """MultiTensorQuantizer with s = the ladder: plain, max_element and stochastic (tensor i with seed0 + i); tensor i equals
    the per-tensor call at s[i] and the oracle."""
    xs = model(400)
    ts = [L.to(DEV, x) for x in xs]
    s = list(L.LADDER)
    plain = [L.host(q) for q in MultiTensorQuantizer(ts, s, bucket).quantize()]
    clamp = [L.host(q) for q in MultiTensorQuantizer(ts, s, bucket, max_element=0.8).quantize()]
    mq = MultiTensorQuantizer(ts, s, bucket, stochastic_rounding=True)
    seed0 = 0x0123456789ABCDEF
    stoch = [L.host(q) for q in mq.quantize(seed=seed0)]
    assert mq.last_seed == seed0
    hip = SC.Library('hip')
    for i, (x, si) in enumerate(zip(xs, s)):
        tag = (bucket, i, x.size, si)
        L.same_bits(plain[i], onp.uniform_quantize(x, si, bucket)['q'], ('plain',) + tag)
        L.same_bits(plain[i], per_tensor(x, si, bucket), ('plain, per tensor',) + tag)
        L.same_bits(clamp[i], onp.uniform_quantize(x, si, bucket, max_element=0.8)['q'], ('max_element',) + tag)
        L.same_bits(clamp[i], per_tensor(x, si, bucket, max_element=0.8), ('max_element, per tensor',) + tag)
        seed = (seed0 + i) & 0xFFFFFFFFFFFFFFFF
        want = onp.uniform_quantize_stochastic(x, si, L.padded_draws(seed, x.size, bucket), bucket)['q']
        L.same_bits(stoch[i], want, ('stochastic',) + tag)
        L.same_bits(stoch[i], hip.uniform(x, bucket, si, seed, want_lev=False)['q'], ('stochastic, per tensor',) + tag)


@pytest.mark.parametrize('s', [5, 17, 2 ** 31 - 1])
def test_multi_tensor_quantizer_one_level_count(s):
    xs = model(410)[:9]
    ts = [L.to(DEV, x) for x in xs]
    for bucket in (256, 100, None):
        for kw in ({}, dict(max_element=0.8)):
            got = MultiTensorQuantizer(ts, s, bucket, **kw).quantize()
            for i, x in enumerate(xs):
                L.same_bits(L.host(got[i]), onp.uniform_quantize(x, s, bucket, **kw)['q'], (s, bucket, i, tuple(kw)))
        mq = MultiTensorQuantizer(ts, s, bucket, stochastic_rounding=True)
        got = mq.quantize(seed=77)
        for i, x in enumerate(xs):
            want = onp.uniform_quantize_stochastic(x, s, L.padded_draws(77 + i, x.size, bucket), bucket)['q']
            L.same_bits(L.host(got[i]), want, ('stochastic', s, bucket, i))


@pytest.mark.parametrize('bucket', [256, 100])
def test_multi_tensor_ste_a_level_count_per_tensor(bucket):
    """MultiTensorSTE (register tiles at 256, a wave per bucket at 100) with s = the ladder, and with one s: tensor i equals
    ste.ste_bucket_backward at s[i] bit for bit (dense gradients too) and, with one term per bucket, the oracle."""
    xs = model(420)
    ws = [L.to(DEV, x) for x in xs]
    g1 = [L.one_term_gradient(x.size, bucket, 430 + i) for i, x in enumerate(xs)]
    gd = [L.dense_gradient(x.size, 440 + i) for i, x in enumerate(xs)]
    for tie_mode in L.TIE_MODES:
        for name, gs in (('one term', g1), ('dense', gd)):
            for s in (list(L.LADDER), 5, 17, 2 ** 31 - 1):
                outs = [torch.full((x.size,), 777.0, device=DEV) for x in xs]
                MultiTensorSTE(ws, [L.to(DEV, g) for g in gs], s, bucket, outs=outs, tie_mode=tie_mode).backward()
                for i, x in enumerate(xs):
                    si = s[i] if isinstance(s, list) else s
                    tag = (name, bucket, tie_mode, i, x.size, si)
                    one = ste.ste_bucket_backward(ws[i], L.to(DEV, gs[i]), bucket, si, tie_mode=tie_mode)
                    L.same_bits(L.host(outs[i]), L.host(one), ('per tensor',) + tag)
                    if name == 'one term':
                        L.same_bits(L.host(outs[i]), onp.ste_complicated_backward(x, gs[i], si, bucket, tie_mode), ('oracle',) + tag)


# ---------------------------------------------------------------------------------------------------- absmax / absnorm
@pytest.mark.parametrize('n,bucket', [(257, 256), (5000, None)])
@pytest.mark.parametrize('kind', ac.KINDS)
def test_abs_scalings_on_the_ladder(kind, n, bucket):
    """uniformQuantization(type_of_scaling=...) on the smallest bucketed shape of abs_cases.OPTION_SHAPES and a one-wave single
    bucket of abs_cases.SINGLE_LENGTHS: q bit for bit given the norm the device reports, the norm held as tests/test_hip_abs.py
    holds it (absmax: the bits; absnorm: abs_cases.BOUND)."""
    assert (n, bucket) in ac.OPTION_SHAPES or (bucket is None and n in ac.SINGLE_LENGTHS)
    x = ac.random_data(n, 500 + n % 89)
    xd = L.to(DEV, x)
    for s in L.LADDER:
        case = ac._case('levels-%s-n%d-b%s-s%d' % (kind, n, bucket, s), x, bucket, kind, s)
        q, sf = quantization.uniformQuantization(xd, s, type_of_scaling=kind, bucket_size=bucket)
        nrm = L.host(sf.norm_scaling).reshape(-1)
        ac.check_norm(case, nrm)
        assert ac.bits_same(q, ac.expect(case, nrm)['q']), (case.id, 'q')


# ---------------------------------------------------------------------------------------------------- the codec, where a level fits a byte
CODEC_SHAPES = [(2563, 256), (2121, 100), (1000, None)]


def numpy_packing(lev, n, bits):
    """The packing of tests/test_hip_parity.py::test_pack_unpack_roundtrip (little endian inside a byte)."""
    lev = lev.astype(np.uint64)
    epb = 8 // bits
    levp = np.concatenate([lev, np.zeros((-n) % epb, np.uint64)]).reshape(-1, epb)
    want = np.zeros(levp.shape[0], np.uint64)
    for c in range(epb):
        want |= levp[:, c] << np.uint64(c * bits)
    return want.astype(np.uint8)


@pytest.mark.parametrize('n,bucket', CODEC_SHAPES)
def test_codec_on_the_byte_ladder(n, bucket):
    """level_idx of qd_uniform_f32 (and its levels-only form where it exists: bucket 256), pack_uniform, unpack and
    level_histogram against the oracle's levels."""
    lib = _lib.load()
    x = L.inputs(n, 600 + n)
    xd = L.to(DEV, x)
    for s in L.BYTE:
        ref = onp.uniform_quantize(x, s, bucket)
        lev = ref['lev'].reshape(-1)[:n]
        assert lev.min() == 0 and lev.max() == s - 1
        # the level_idx output at the C ABI: A.k1 compares q, alpha, beta and lev with the oracle between guard bands
        A.run_case(A.k1('level_idx s=%d' % s, x, bucket or 0, levels=s, lev_phase=0), lib, DEV, fills=A.FILLS[:1])
        if bucket == 256:
            A.run_case(A.k1('levels only s=%d' % s, x, bucket, levels=s, lev_phase=0, q_null=True), lib, DEV, fills=A.FILLS[:1])
        bits = codec.bits_for_levels(s)
        pk = codec.pack_uniform(xd, s, bucket, bits=bits)
        assert np.array_equal(L.host(pk.packed), numpy_packing(lev, n, bits)), (s, bucket, 'packed bytes')
        L.same_bits(L.host(pk.alpha), ref['alpha'], ('pack alpha', s, bucket))
        L.same_bits(L.host(pk.beta), ref['beta'], ('pack beta', s, bucket))
        q, _ = quantization.uniformQuantization(xd, s, bucket_size=bucket)
        assert torch.equal(pk.unpack(), q), (s, bucket, 'unpack')
        L.same_bits(L.host(q), ref['q'], ('q', s, bucket))
        h = codec.level_histogram(xd, s, bucket)
        assert h.dtype == torch.int64 and np.array_equal(L.host(h), np.bincount(lev, minlength=s)), (s, bucket, 'histogram')


def test_257_levels_do_not_fit_a_byte():
    """level_idx, qd_level_histogram_f32 and qd_pack_uniform_f32 at 257 levels: QD_ERR_INVALID_ARGUMENT, the sentinel-filled
    outputs untouched (A.run_case checks every placed array of a refused call)."""
    lib = _lib.load()
    x = A.data(2563, 256, 50)
    n = x.size
    nb = A.nbuckets(n, 256)
    A.run_case(A.k1('257 levels with level_idx', x, 256, levels=257, lev_phase=0, rc=A.ERR_INVALID), lib, DEV)
    A.run_case(A.k1('257 levels, levels only', x, 256, levels=257, lev_phase=0, q_null=True, rc=A.ERR_INVALID), lib, DEV)
    A.run_case(A.case('histogram of 257 levels', 'qd_level_histogram_f32', [('x', A.inp(x, 0)), ('hist', A.out(A.U64, 257, 0))],
                      [A.Ref('x'), n, 256, 257, A.Ref('hist'), A.WS, A.WSB, A.STREAM], None, rc=A.ERR_INVALID), lib, DEV)
    A.run_case(A.case('pack 257 levels', 'qd_pack_uniform_f32',
                      [('x', A.inp(x, 0)), ('packed', A.out(A.U8, n, 0)), ('alpha', A.out(A.F32, nb, 4)), ('beta', A.out(A.F32, nb, 12))],
                      [A.Ref('x'), n, 256, 257, 8, A.Ref('packed'), A.Ref('alpha'), A.Ref('beta'), A.STREAM], None, rc=A.ERR_INVALID),
               lib, DEV)
    with pytest.raises(ValueError):
        codec.pack_uniform(L.to(DEV, x), 257, 256)


@pytest.mark.parametrize('bucket', [256, 100, None])
def test_compressed_files_with_every_table_length(tmp_path, bucket):
    """save_compressed(s = [2 .. 17]): the same bytes on the device as on the host, and load_compressed gives back the
    per-tensor uniformQuantization."""
    s = list(L.TABLE)
    xs = model(700)[:len(s)]
    dev_ts = {'t%02d' % i: L.to(DEV, x) for i, x in enumerate(xs)}
    host_ts = {k: v.cpu() for k, v in dev_ts.items()}
    pd, ph = str(tmp_path / 'd.qd'), str(tmp_path / 'h.qd')
    C.save_compressed(pd, dev_ts, s=s, bucket_size=bucket)
    C.save_compressed(ph, host_ts, s=s, bucket_size=bucket)
    assert open(pd, 'rb').read() == open(ph, 'rb').read()
    back_d, back_h = C.load_compressed(pd, device=DEV), C.load_compressed(pd, device='cpu')
    for (k, t), si, x in zip(dev_ts.items(), s, xs):
        want = onp.uniform_quantize(x, si, bucket)['q']
        L.same_bits(per_tensor(x, si, bucket), want, ('uniformQuantization', k, si, bucket))
        L.same_bits(L.host(back_d[k]), want, ('decoded on the device', k, si, bucket))
        L.same_bits(L.host(back_h[k]), want, ('decoded on the host', k, si, bucket))


# ---------------------------------------------------------------------------------------------------- device against host
@pytest.mark.parametrize('n,bucket', [(2563, 256), (1000, None)])
def test_device_and_host_library_give_the_same_bits_on_the_ladder(n, bucket):
    hip, cpu = SC.Library('hip'), SC.Library('host')
    x = L.inputs(n, 800 + n)
    for s in L.LADDER:
        for stochastic in (0, 1):
            seed = L.stochastic_seed(s, 3)
            a = hip.uniform(x, bucket, s, seed, want_lev=s <= 256, stochastic=stochastic)
            b = cpu.uniform(x, bucket, s, seed, want_lev=s <= 256, stochastic=stochastic)
            assert SC.same_outputs(a, b), (n, bucket, s, stochastic)
            L.same_bits(a['q'], b['q'], ('q', n, bucket, s, stochastic))


# ---------------------------------------------------------------------------------------------------- the accepted range
def test_out_of_range_s_is_refused_everywhere_before_anything_is_launched(tmp_path):
    """s in {2^31, 2^32, 2^32 + 16} (a float of that value too) and 16.5: ValueError naming [2, 2^31 - 1] at every entry
    point, the tensors a call would write untouched; 16.0 is 16; 2^31 - 1 is accepted."""
    L.check_refusals(DEV, tmp_path)
    with pytest.raises(ValueError, match=L.RANGE_TEXT):
        _lib.glue().uniform(L.to(DEV, L.inputs(1283, 11)), 2 ** 31, 256, False, 0.0, False, 0, False, False)
