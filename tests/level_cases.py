"""The level count `s` as an input axis: the ladder of level counts every uniform path is held to, the cases of the reference
fixture tests/golden/levels.json, and the checks shared by tests/test_level_cases_host.py (oracle_np, oracle_c and libqd_host.so
against the reference's digests, no GPU) and tests/test_hip_levels.py (libqd_hip.so against the oracle and against libqd_host.so).
A plain helper module: no fixtures, nothing runs on import; the product and torch are imported inside the functions that need
them (tests/golden/gen_levels.py imports this module beside the REFERENCE's `quantization` package).

Why a ladder.  Every uniform kernel branches on s at run time inside one kernel name -- `p.sm1 <= 15.0f` selects the
ds_bpermute level table or the computed division (csrc/qd_common.h: qdq_tab / qdq_stochastic_tab) -- and sm1 = (float)(s - 1)
stops being exact above 2^24, reaches 2^31 > INT_MAX at s = 2^31 - 1, and from 2^23 on makes every t = u * sm1 >= 2^22 an
integer or a half-integer (rintf ties on a quarter of the range, a stochastic p of 0 or 0.5).  The accepted range of s is
[2, 2^31 - 1] (include/qd_hip.h next to qd_uniform_f32; _lib.level_count): REFUSED lists what is outside.

Inputs come from np.random.RandomState by (shape, seed) and hold no NaN and no infinity.  Every check takes the device: 'cpu'
(libqd_host.so) or 'cuda:0'."""
import collections
import hashlib
import json
import math
import os

import numpy as np

F32 = np.float32
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'levels.json')

TABLE = tuple(range(2, 18))           # every table length 2 .. 16 (sm1 <= 15: the ds_bpermute table), and 17: the first computed one
MID = (31, 32, 33, 64, 100, 128, 255, 256, 257, 1000, 4096)      # 2^bits for 5, 6, 7, 8 bits and their neighbours; 256 / 257: the uint8 limit
BIG = (
    65535, 65536, 65537,              # s - 1 exact, far below 2^23: no tie beyond the ordinary ones; levels past uint16
    2 ** 23,                          # s - 1 = 2^23 - 1, exact, the last sm1 BELOW 2^23: t has half-integers up to the top
    2 ** 23 + 1,                      # s - 1 = 2^23 exact: sm1 AT 2^23 -- every t >= 2^22 is an integer or a half-integer
    2 ** 23 + 2,                      # s - 1 = 2^23 + 1 exact and odd, sm1 above 2^23
    2 ** 24,                          # s - 1 = 2^24 - 1: the largest odd integer fp32 holds, exact
    2 ** 24 + 1,                      # s - 1 = 2^24 exact: the last exact one before the spacing of fp32 becomes 2
    2 ** 24 + 2,                      # s - 1 = 2^24 + 1: a tie, rounded to even DOWN to 2^24 (the sm1 of the entry above)
    2 ** 24 + 3,                      # s - 1 = 2^24 + 2 exact
    2 ** 24 + 4,                      # s - 1 = 2^24 + 3: a tie, rounded to even UP to 2^24 + 4
    2 ** 31 - 128,                    # s - 1 = 2^31 - 129 rounds up to 2^31 - 128, the largest fp32 <= INT_MAX: sm1 still converts to int
    2 ** 31 - 1,                      # INT_MAX, the top of the range: s - 1 = 2^31 - 2 rounds up to 2^31, sm1 > INT_MAX
)
LADDER = TABLE + MID + BIG
BYTE = tuple(s for s in TABLE + MID if s <= 256)       # level_idx, pack, histogram, compressed files: a level fits a byte
REFUSED = (2 ** 31, 2 ** 32, 2 ** 32 + 16)            # above the range: ValueError, nothing launched (2^32 + 16 once gave 16 levels)
SPARSE = (2, 16, 17, 256, 2 ** 24 + 2, 2 ** 31 - 1)   # the large single-bucket shapes
FUSED_S = (5, 16, 17, 2 ** 31 - 1)                    # the fused-mode hooks; a scalar s of the multi-tensor classes uses (5, 17, 2^31 - 1)
RANGE_TEXT = r'\[2, 2\^31 - 1\]'                      # every refusal names the range

assert len(set(LADDER)) == len(LADDER) == 40 and all(F32(s - 1) <= 15 for s in TABLE[:-1]) and F32(TABLE[-1] - 1) > 15
assert F32(2 ** 24 + 1) == 2 ** 24 and F32(2 ** 24 + 3) == 2 ** 24 + 4 and F32(2 ** 31 - 129) == 2 ** 31 - 128 and F32(2 ** 31 - 2) == 2 ** 31

# the shapes of the reference fixture: bucket 256 with a ragged tail (5 buckets + 3), bucket 100 (7 + 41), no bucket
SHAPES = collections.OrderedDict([('b256', (1283, 256)), ('b100', (741, 100)), ('none', (1000, None))])
OPTIONS = dict(max_element=0.7, subtract_mean=True)
HUFFMAN_S = (3, 5, 17, 100, 1000)
HUFFMAN_SIZES = ((1283,), (40, 25), (741,))            # the three tensors of the Huffman model; quantized with bucket 256
HUFFMAN_TOL = 1e-12                                    # README: the mean code length equals the reference's within 1e-12


# ---------------------------------------------------------------- inputs
def inputs(n, seed):
    return np.random.RandomState(seed).randn(n).astype(F32)


def grid_inputs(n, seed):
    """randn on the grid of 2^-10 plus 0.25: every partial sum of the n <= 4096 elements is exact in fp32 and in float64, so
    the fp32 mean of ANY summation order is the correctly rounded sum / n -- the reference's mean (torch's blocked fp32 sum) and
    qd_mean_f32's (float64, one rounding) are the same float, and subtract_mean has one reference bit pattern."""
    assert n <= 4096
    return (np.round(np.random.RandomState(seed).randn(n) * 1024.0) / 1024.0 + 0.25).astype(F32)


def one_term_gradient(n, bucket, seed):
    """Zero except one element per bucket (a seeded position, a randn value): every bucket sum of the 'complicated' STE is
    its single term -- no summation order, so the backward is comparable bit for bit."""
    rng = np.random.RandomState(seed)
    g = np.zeros(n, F32)
    row = bucket if n >= bucket else n
    for lo in range(0, n, row):
        g[rng.randint(lo, min(lo + row, n))] = F32(rng.randn())
    return g


def dense_gradient(n, seed):
    return np.random.RandomState(seed).randn(n).astype(F32)


def stochastic_seed(s, shape_index):
    return (0x9E3779B97F4A7C15 * s + 0x632BE59BD9B4E019 * (shape_index + 1)) & 0xFFFFFFFFFFFFFFFF


def padded_draws(seed, n, bucket):
    """The Philox draws of the n elements in the padded bucket layout (padding: 0.0; its results are dropped)."""
    from oracle import oracle_np as onp
    _, _, padded = onp.bucket_geometry(n, bucket)
    r = np.zeros(padded, F32)
    r[:n] = onp.philox4x32_7_uniform(seed, n)
    return r


def digest(a, dtype='<f4'):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=dtype).tobytes()).hexdigest()


# ---------------------------------------------------------------- the cases of tests/golden/levels.json
def fixture_cases():
    """The case parameters, in the order of the file: kind 'det' (every shape), 'opt' (max_element + subtract_mean on b256),
    'ste' (the backward of uniformQuantization_variable on b256 / b100, one-term gradients), 'stoch' (every shape, torch.rand
    replaced by the Philox draws of `seed`)."""
    cases = []
    for si, shape in enumerate(SHAPES):
        for li, s in enumerate(LADDER):
            cases.append(dict(kind='det', shape=shape, s=s, x_seed=1000 * (si + 1) + li))
    for li, s in enumerate(LADDER):
        cases.append(dict(kind='opt', shape='b256', s=s, x_seed=5000 + li))
    for si, shape in enumerate(('b256', 'b100')):
        for li, s in enumerate(LADDER):
            cases.append(dict(kind='ste', shape=shape, s=s, x_seed=6000 + 100 * si + li, g_seed=7000 + 100 * si + li))
    for si, shape in enumerate(SHAPES):
        for li, s in enumerate(LADDER):
            cases.append(dict(kind='stoch', shape=shape, s=s, x_seed=8000 + 100 * si + li, seed=stochastic_seed(s, si)))
    return cases


def case_input(c):
    n, bucket = SHAPES[c['shape']]
    return (grid_inputs if c['kind'] == 'opt' else inputs)(n, c['x_seed']), n, bucket


def case_gradient(c):
    n, bucket = SHAPES[c['shape']]
    return one_term_gradient(n, bucket, c['g_seed'])


def huffman_model(s):
    return [inputs(int(np.prod(shape)), 9000 + s + i).reshape(shape) for i, shape in enumerate(HUFFMAN_SIZES)]


def result_digest(kind, r):
    """What the file stores of a result: the SHA-256 of the little-endian fp32 bytes of q, alpha and beta, one after the
    other -- of the output for an STE case."""
    if kind == 'ste':
        return digest(r['out'])
    return digest(np.concatenate([np.asarray(r[k], F32).reshape(-1) for k in ('q', 'alpha', 'beta')]))


def load_fixture():
    with open(FIXTURE) as f:
        doc = json.load(f)
    want = fixture_cases()
    got = [{k: v for k, v in c.items() if k not in ('sha256', 'mean')} for c in doc['cases']]
    assert got == want, 'tests/golden/levels.json was not generated from fixture_cases(): run tests/golden/gen_levels.py'
    return doc


def oracle_result(c, which):
    """The case through oracle_np ('np') or oracle_c ('c'), fed the recorded mean where there is one."""
    from oracle import oracle_c as oc
    from oracle import oracle_np as onp
    x, n, bucket = case_input(c)
    s = c['s']
    if c['kind'] in ('det', 'opt'):
        kw = dict(OPTIONS, mean=c['mean']) if c['kind'] == 'opt' else {}
        r = onp.uniform_quantize(x, s, bucket, **kw) if which == 'np' else oc.uniform_quantize(x, s, bucket, want_idx=False, **kw)
        return dict(q=r['q'], alpha=r['alpha'], beta=r['beta'], mean=r['mean'])
    if c['kind'] == 'stoch':
        rand = padded_draws(c['seed'], n, bucket)
        r = onp.uniform_quantize_stochastic(x, s, rand, bucket) if which == 'np' else oc.uniform_quantize_stochastic(x, s, rand[:n], bucket)
        return dict(q=r['q'], alpha=r['alpha'], beta=r['beta'])
    g = case_gradient(c)
    return dict(out=onp.ste_complicated_backward(x, g, s, bucket) if which == 'np' else oc.ste_complicated_backward(x, g, s, bucket))


def api_result(c, device):
    """The case through the product on `device`: the Python API, and for the stochastic cases the C ABI with the recorded
    seed (the Python API derives its seed from the process counter)."""
    import quantization
    import stochastic_cases as SC
    x, n, bucket = case_input(c)
    s = c['s']
    if c['kind'] in ('det', 'opt'):
        q, sf = quantization.uniformQuantization(to(device, x), s, bucket_size=bucket, **(OPTIONS if c['kind'] == 'opt' else {}))
        return dict(q=host(q), alpha=host(sf.alpha), beta=host(sf.beta), mean=float(sf.mean_tensor))
    if c['kind'] == 'stoch':
        r = SC.Library('host' if str(device) == 'cpu' else 'hip').uniform(x, bucket, s, c['seed'], want_lev=s <= 256)
        return dict(q=r['q'], alpha=r['alpha'], beta=r['beta'])
    fn = quantization.uniformQuantization_variable(s, bucket_size=bucket)
    fn.forward(to(device, x))
    return dict(out=host(fn.backward(to(device, case_gradient(c)))))


# ---------------------------------------------------------------- comparisons
def to(device, a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order='C')).to(device)       # (a copy: the shared inputs are read-only)


def host(t):
    return t.detach().cpu().numpy()


def same_bits(got, want, tag):
    got = np.ascontiguousarray(np.asarray(got, F32)).reshape(-1)
    want = np.ascontiguousarray(np.asarray(want, F32)).reshape(-1)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert not np.isnan(want).any(), (tag, 'the oracle gave a NaN on finite input')
    diff = got.view(np.uint32) != want.view(np.uint32)
    assert not diff.any(), (tag, '%d of %d elements differ, first at %d: %r != %r'
                            % (diff.sum(), diff.size, np.flatnonzero(diff)[0], got[diff][0], want[diff][0]))


def exact_mean(x):
    return F32(math.fsum(np.asarray(x, np.float64).reshape(-1).tolist()) / x.size)


_INPUTS = {}


def shared_input(n, seed):
    """inputs(n, seed), made once per process and never written (the large shapes are shared by the tests that use them)."""
    if (n, seed) not in _INPUTS:
        x = inputs(n, seed)
        x.setflags(write=False)
        _INPUTS[(n, seed)] = x
    return _INPUTS[(n, seed)]


# ---------------------------------------------------------------- K1 through the Python API
def check_k1(device, x, s, bucket, tag, max_element=False, subtract_mean=False):
    """uniformQuantization, deterministic: q, alpha, beta (and a correctly rounded mean) against oracle_np bit for bit."""
    import quantization
    from oracle import oracle_np as onp
    q, sf = quantization.uniformQuantization(to(device, x), s, bucket_size=bucket, max_element=max_element, subtract_mean=subtract_mean)
    mean = None
    if subtract_mean:
        mean = F32(float(sf.mean_tensor))
        assert mean == exact_mean(x), (tag, 'the mean is the correctly rounded one', mean, exact_mean(x))
    want = onp.uniform_quantize(x, s, bucket, max_element=max_element, subtract_mean=subtract_mean, mean=mean)
    same_bits(host(q), want['q'], ('q',) + tuple(tag))
    same_bits(host(sf.alpha), want['alpha'], ('alpha',) + tuple(tag))
    same_bits(host(sf.beta), want['beta'], ('beta',) + tuple(tag))
    return host(q)


def check_k1_stochastic(device, x, s, bucket, tag, max_element=False):
    """uniformQuantization(stochastic_rounding=True) against the Philox restatement with the seed the call is about to draw."""
    import quantization
    import quantization.quant_functions as qf
    from oracle import oracle_np as onp
    seed = qf.next_stochastic_seed(peek=True, host=str(device) == 'cpu')
    q, sf = quantization.uniformQuantization(to(device, x), s, stochastic_rounding=True, bucket_size=bucket, max_element=max_element)
    want = onp.uniform_quantize_stochastic(x, s, padded_draws(seed, x.size, bucket), bucket, max_element=max_element)
    same_bits(host(q), want['q'], ('stochastic q',) + tuple(tag))
    same_bits(host(sf.alpha), want['alpha'], ('stochastic alpha',) + tuple(tag))
    same_bits(host(sf.beta), want['beta'], ('stochastic beta',) + tuple(tag))


def check_k1_ladder(device, n, bucket, seed, ladder=LADDER):
    """One shape on the ladder, deterministic and stochastic."""
    x = shared_input(n, seed)
    for s in ladder:
        check_k1(device, x, s, bucket, (n, bucket, s))
        check_k1_stochastic(device, x, s, bucket, (n, bucket, s))


def check_k1_options(device, n, bucket, seed, ladder=LADDER):
    """max_element + subtract_mean (the options of tests/abi_contract.py: _k1_extra) on the ladder, and max_element with
    stochastic rounding."""
    x = shared_input(n, seed)
    for s in ladder:
        check_k1(device, x, s, bucket, ('mean + clamp', n, bucket, s), max_element=0.8, subtract_mean=True)
        check_k1_stochastic(device, x, s, bucket, ('clamp', n, bucket, s), max_element=0.8)


# ---------------------------------------------------------------- K7 through the Python API
TIE_MODES = ('reference', 'true_arg')


def check_k7(device, n, bucket, seed, ladder=LADDER):
    """uniformQuantization_variable.backward and ste.ste_bucket_backward, both tie modes: one-term-per-bucket gradients bit
    for bit against the oracle, a dense gradient within errlog's bound of the float64 bucket sums (the method of
    tests/test_hip_extreme_scales.py)."""
    import errlog
    import quantization
    from oracle import oracle_np as onp
    from quantized_distillation_amd import ste
    x = shared_input(n, seed)
    g1 = one_term_gradient(n, bucket, seed + 1)
    gd = dense_gradient(n, seed + 2)
    for s in ladder:
        for tie_mode in TIE_MODES:
            want = onp.ste_complicated_backward(x, g1, s, bucket, tie_mode)
            fn = quantization.uniformQuantization_variable(s, bucket_size=bucket)
            fn.forward(to(device, x))
            same_bits(host(fn.backward(to(device, g1), tie_mode)), want, ('K7 variable', n, bucket, s, tie_mode))
            out = ste.ste_bucket_backward(to(device, x), to(device, g1), bucket, s, tie_mode=tie_mode)
            same_bits(host(out), want, ('K7 ste_bucket_backward', n, bucket, s, tie_mode))
            out = ste.ste_bucket_backward(to(device, x), to(device, gd), bucket, s, tie_mode=tie_mode)
            errlog.check_ste('K7 on the level ladder', host(out), x, gd, s, bucket, (n, bucket, s, tie_mode), tie_mode=tie_mode)


# ---------------------------------------------------------------- the accepted range of s
def refusals(device):
    """(name, call) of every entry point that takes a level count and exists for tensors on `device`; call(s, sink) runs it
    with that s and may write only into `sink` (a tensor of varied values the caller compares afterwards) and its clones."""
    import quantization
    import quantization.help_functions as qhf
    from quantized_distillation_amd import codec, ste
    from quantized_distillation_amd.compressed import save_compressed
    from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer, MultiTensorSTE
    cuda = str(device) != 'cpu'
    x = to(device, inputs(1283, 11))
    g = to(device, inputs(1283, 12))
    out = []

    def add(name, fn):
        out.append((name, fn))

    add('uniformQuantization, common path', lambda s, sink: quantization.uniformQuantization(x, s, bucket_size=256))
    add('uniformQuantization, no bucket', lambda s, sink: quantization.uniformQuantization(x, s))
    add('uniformQuantization, stochastic', lambda s, sink: quantization.uniformQuantization(x, s, stochastic_rounding=True, bucket_size=256))
    add('uniformQuantization, options', lambda s, sink: quantization.uniformQuantization(x, s, max_element=0.7, subtract_mean=True, bucket_size=256))
    add('uniformQuantization, in place', lambda s, sink: quantization.uniformQuantization(sink, s, bucket_size=256, modify_in_place=True))
    add('uniformQuantization_variable', lambda s, sink: quantization.uniformQuantization_variable(s, bucket_size=256).forward(x))

    def late(s, sink):                        # s assigned after construction: backward refuses it too
        fn = quantization.uniformQuantization_variable(16, bucket_size=256)
        fn.forward(x)
        fn.s = s
        fn.backward(g)
    add('uniformQuantization_variable.backward', late)
    add('get_huffman_encoding_mean_bit_length', lambda s, sink: qhf.get_huffman_encoding_mean_bit_length(
        iter([x]), lambda p: quantization.uniformQuantization(p, 16, bucket_size=256), 'uniform', s))
    add('ste.ste_bucket_backward', lambda s, sink: ste.ste_bucket_backward(x, g, 256, s, out=sink))
    if cuda:
        add('uniformQuantization, absmax', lambda s, sink: quantization.uniformQuantization(x, s, type_of_scaling='absmax', bucket_size=256))
        add('codec.pack_uniform', lambda s, sink: codec.pack_uniform(x, s, 256, bits=8))
        add('codec.level_histogram', lambda s, sink: codec.level_histogram(x, s, 256))
        add('codec.huffman_mean_bit_length_uniform', lambda s, sink: codec.huffman_mean_bit_length_uniform([x], s, 256))
        add('MultiTensorQuantizer, scalar', lambda s, sink: MultiTensorQuantizer([x, g], s, 256, outputs=[sink, sink.clone()]).quantize())
        add('MultiTensorQuantizer, sequence', lambda s, sink: MultiTensorQuantizer([x, g], [16, s], 256, outputs=[sink, sink.clone()]).quantize())
        add('MultiTensorQuantizer, no bucket', lambda s, sink: MultiTensorQuantizer([x, g], [s, 16], None, outputs=[sink, sink.clone()]).quantize())
        add('MultiTensorSTE, scalar', lambda s, sink: MultiTensorSTE([x, x], [g, g.clone()], s, 256, outs=[sink, sink.clone()]).backward())
        add('MultiTensorSTE, sequence', lambda s, sink: MultiTensorSTE([x, x], [g, g.clone()], [s, 4], 256, outs=[sink, sink.clone()]).backward())
    return x, out, save_compressed


def check_refusals(device, tmp_path):
    """s in REFUSED, 1 and 16.5 raise ValueError naming the range at every entry point, before anything is written (the
    tensor a call would write keeps its sentinel, the input its bits); 16.0 is accepted and is 16."""
    import pytest
    import torch
    import quantization
    from harness.distill import DistillTrainer
    x, calls, save_compressed = refusals(device)
    before = host(x).copy()
    sentinel = to(device, inputs(x.numel(), 13) * F32(3.0) + F32(777.0))
    for name, call in calls:
        for s in REFUSED + (16.5, float(2 ** 32 + 16)):
            sink = sentinel.clone()
            with pytest.raises(ValueError, match=RANGE_TEXT):
                call(s, sink)
            assert torch.equal(sink, sentinel), (name, s, 'a refused call wrote its output')
            assert np.array_equal(host(x), before), (name, s, 'a refused call wrote its input')
    for s in REFUSED:
        with pytest.raises(ValueError):
            save_compressed(str(tmp_path / 'refused.qdz'), {'w': x}, s=s)
        with pytest.raises(ValueError):
            save_compressed(str(tmp_path / 'refused.qdz'), {'w': x, 'v': x}, s=[16, s])
        assert not (tmp_path / 'refused.qdz').exists()
    for bits in (31, 32, 64, [4, 31], [32, 4]):
        with pytest.raises(ValueError, match='num_bits'):
            DistillTrainer(_Boom(), _Boom(), 'cpu', num_bits=bits)
    q16, _ = quantization.uniformQuantization(x, 16, bucket_size=256)
    for kw in (dict(bucket_size=256), dict(bucket_size=256, stochastic_rounding=False, subtract_mean=True)):
        a, _ = quantization.uniformQuantization(x, 16.0, **kw)
        b, _ = quantization.uniformQuantization(x, 16, **kw)
        assert torch.equal(a, b), ('16.0 is 16', kw)
    top, _ = quantization.uniformQuantization(x, 2 ** 31 - 1, bucket_size=256)       # the top of the range is inside it
    assert not torch.equal(top, q16)


class _Boom(object):
    """A model DistillTrainer must not touch before it has refused its arguments."""

    def __getattr__(self, name):
        raise AssertionError('the model was used (%s) before num_bits was refused' % name)
