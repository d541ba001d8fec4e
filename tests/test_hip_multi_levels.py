"""A level count per tensor in the one-launch quantizer and STE (qd_multi_uniform_levels_f32, qd_multi_uniform_global_levels_f32,
qd_multi_ste_backward_levels_f32; MultiTensorQuantizer / MultiTensorSTE with a sequence s) against the yardstick the header
names: the per-tensor call at s_i -- quantization.uniformQuantization / ste.ste_bucket_backward -- bit for bit (int32 views: NaN
payloads count).  The deterministic quantizer results are also held to the C oracle at s_i, the STE results on finite inputs to
K7's bound of the float64 oracle (errlog.check_ste).

The list: about 300 tensors of 0 .. 4096 elements (most of them a tile or less, so a wave's consecutive tiles and the four
waves of a block belong to tensors of different level counts), the level count cycling through LEVELS, one tensor of 1 Mi
elements in the middle, every fifth tensor 4 bytes off a 16-byte boundary, empty tensors first, last and two in a row, one
tensor with a NaN and one with +-inf."""
import numpy as np
import pytest
import torch

import abi_contract as A
import errlog
import quantization
from oracle import oracle_c as oc
from quantization import quant_functions as qf
from quantized_distillation_amd import _lib, compressed, ste
from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer, MultiTensorSTE
from test_hip_multi_stochastic import Carved, counter_at, same_bits
from test_hip_property import make

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
M64 = 0xFFFFFFFFFFFFFFFF
LEVELS = [2, 3, 16, 17, 255, 256, 1000]       # both sides of the 16-level table, the smallest, no power of two, above uint8
SIZE_SET = [0, 1, 5, 255, 256, 257, 1024, 256 * 3 + 7, 4096]
N_TENSORS = 301
BIG, NAN_AT, INF_AT, EMPTY_PAIR = 150, 60, 61, (100, 101)
OPTIONS = {'none': dict(), 'clamp': dict(max_element=0.5), 'stoch': dict(stochastic_rounding=True),
           'stoch_cell': dict(stochastic_rounding=True, seed_on_device=True)}
START = 7000                                   # the process's stochastic call counter both sides start from


def _sizes():
    sizes = [SIZE_SET[(i * 4 + 1) % 9] for i in range(N_TENSORS)]        # (4 and 9 coprime: every size, against every level count)
    sizes[0] = sizes[-1] = 0
    sizes[EMPTY_PAIR[0]] = sizes[EMPTY_PAIR[1]] = 0
    sizes[BIG] = 1 << 20
    sizes[NAN_AT] = sizes[INF_AT] = 4096
    return sizes


SIZES = _sizes()
S_LIST = [LEVELS[i % 7] for i in range(N_TENSORS)]
PHASES = [1 if i % 5 == 2 else 0 for i in range(N_TENSORS)]               # in floats: 4 bytes past a 16-byte boundary
_CACHE = {}


def the_list():
    """(Carved, the pristine flat input): built once, never written."""
    if 'list' not in _CACHE:
        gen = torch.Generator(device=DEV).manual_seed(31)
        xs = [torch.randn(n, device=DEV, generator=gen) for n in SIZES]
        xs[NAN_AT][300] = float('nan')                      # bucket 1 of 16 at bucket 256
        xs[INF_AT][5] = float('inf')
        xs[INF_AT][1000] = float('-inf')
        xs[BIG][512:768] = 0.25                             # a constant bucket: the alpha guard
        c = Carved(SIZES, PHASES, xs)
        _CACHE['list'] = (c, c.flat())
    return _CACHE['list']


def per_tensor(bucket, opt):
    """[(q, ScalingFunction)] of the per-tensor loop at s_i from counter START: computed once per (bucket, options)."""
    key = ('loop', bucket, opt)
    if key not in _CACHE:
        c, pristine = the_list()
        kw = {k: v for k, v in OPTIONS[opt].items() if k != 'seed_on_device'}
        with counter_at(START):
            _CACHE[key] = [quantization.uniformQuantization(x, s, bucket_size=bucket, **kw) for x, s in zip(c.views(pristine), S_LIST)]
            assert qf._STOCHASTIC_CALLS[0] == START + (N_TENSORS if 'stochastic_rounding' in kw else 0)
    return _CACHE[key]


def check_equal(outs, want, what):
    assert len(outs) == len(want)
    for i, (o, w) in enumerate(zip(outs, want)):
        w = w[0] if isinstance(w, tuple) else w
        assert same_bits(o, w.reshape(-1)), '%s: tensor %d (%d elements, s = %d) differs from the per-tensor call' % (what, i, o.numel(), S_LIST[i])


# ---------------------------------------------------------------- the quantizer
@pytest.mark.parametrize('opt', list(OPTIONS))
@pytest.mark.parametrize('bucket', [256, 64, 100, None])
def test_quantizer_equals_the_per_tensor_call_at_each_level_count(bucket, opt):
    c, pristine = the_list()
    want = per_tensor(bucket, opt)
    fx, fq = pristine.clone(), c.flat(filled=False)
    with counter_at(START):
        mt = MultiTensorQuantizer(c.views(fx), S_LIST, bucket, outputs=c.views(fq), **OPTIONS[opt])
        outs = mt.quantize()
    torch.cuda.synchronize()
    assert mt.s == tuple(S_LIST) and mt._levels.dtype == torch.int32 and mt._levels.tolist() == S_LIST
    assert mt.entry_point == ('qd_multi_uniform_global_levels_f32' if bucket is None else 'qd_multi_uniform_levels_f32')
    assert c.untouched_outside(fq), 'the launch wrote outside its outputs'
    assert same_bits(fx, pristine), 'out of place: the inputs are inputs only'
    check_equal(outs, want, (bucket, opt))
    assert bool(torch.isnan(outs[NAN_AT]).any()) and not bool(torch.isnan(outs[NAN_AT + 7]).any())
    if bucket is None:
        for i, (q, sf) in enumerate(want):
            row = torch.stack([sf.alpha.reshape(-1)[0], sf.beta.reshape(-1)[0]]) if q.numel() else \
                torch.tensor([1.0, float('inf')], device=DEV)
            assert same_bits(mt.alpha_beta[i], row), (i, mt.alpha_beta[i], row)
    if 'stochastic_rounding' not in OPTIONS[opt]:           # deterministic: the C oracle at s_i too
        me = OPTIONS[opt].get('max_element', False)
        host = fq.cpu().numpy()
        xin = pristine.cpu().numpy()
        for i, (o, n) in enumerate(zip(c.offsets, SIZES)):
            if n:
                ref = oc.uniform_quantize(xin[o:o + n], S_LIST[i], bucket, max_element=me, want_idx=False, want_lev=False)['q']
                assert A._same(host[o:o + n], ref), (bucket, opt, i, n, S_LIST[i], 'differs from the C oracle')
    else:                                                   # the draws are in use
        det = per_tensor(bucket, 'none')
        assert not same_bits(outs[BIG], det[BIG][0])
    # in place (outputs aliasing the tensors): the same bits
    with counter_at(START):
        mt = MultiTensorQuantizer(c.views(fx), S_LIST, bucket, outputs=c.views(fx), **OPTIONS[opt])
        outs = mt.quantize()
    torch.cuda.synchronize()
    assert c.untouched_outside(fx)
    check_equal(outs, want, (bucket, opt, 'in place'))


@pytest.mark.parametrize('opt', ['none', 'stoch'])
def test_quantizer_at_bucket_128(opt):
    """The one register instantiation the sweep above leaves out (buckets of 128 elements), deterministic and stochastic."""
    c, pristine = the_list()
    want = per_tensor(128, opt)
    fq = c.flat(filled=False)
    with counter_at(START):
        outs = MultiTensorQuantizer(c.views(pristine), S_LIST, 128, outputs=c.views(fq), **OPTIONS[opt]).quantize()
    torch.cuda.synchronize()
    assert c.untouched_outside(fq)
    check_equal(outs, want, (128, opt))


@pytest.mark.parametrize('bucket', [256, None])
def test_entry_i_stays_with_tensor_i_after_a_held_tensor_was_rebound(bucket):
    gen = torch.Generator(device=DEV).manual_seed(4)
    sizes, s_list = [700, 0, 4096, 257, 5000], [256, 16, 4, 17, 2]
    xs = [torch.randn(n, device=DEV, generator=gen) for n in sizes]
    mt = MultiTensorQuantizer(xs, s_list, bucket)
    levels_ptr, table_ptr = mt._levels.data_ptr(), mt._table.data_ptr()
    check_equal_to(mt.quantize(), xs, s_list, bucket)
    fresh = torch.randn(4096 + 1, device=DEV, generator=gen)[1:]        # another storage, 4 bytes off: another tile path too
    xs[2].set_(fresh)
    mt.outputs[3].set_(torch.empty(257, device=DEV))
    outs = mt.quantize()
    assert mt._levels.data_ptr() == levels_ptr and mt._levels.tolist() == s_list, 'the level array is independent of the re-plan'
    assert mt._ptrs == mt._held() and mt._table.data_ptr() != 0 and table_ptr != 0
    assert xs[2].data_ptr() == fresh.data_ptr()
    check_equal_to(outs, xs, s_list, bucket)


def check_equal_to(outs, xs, s_list, bucket):
    torch.cuda.synchronize()
    for i, (o, x, s) in enumerate(zip(outs, xs, s_list)):
        assert same_bits(o, quantization.uniformQuantization(x, s, bucket_size=bucket)[0]), (i, s)


# ---------------------------------------------------------------- the STE backward
class SteList(object):
    """x / g carved like tests/test_hip_multi_ste.py carves them, from a list of numpy arrays."""

    def __init__(self, xs, gs, phases):
        self.c = Carved([x.size for x in xs], phases, [torch.from_numpy(x).to(DEV) for x in xs])
        self.x = self.c.flat()
        self.c.data = [torch.from_numpy(g).to(DEV) for g in gs]
        self.g = self.c.flat()
        self.xs, self.gs = xs, gs


def ste_list(kind):
    """'clean': the sizes of the quantizer's list without its empty / NaN / inf oddities, finite inputs of the four kinds K7's
    oracle bound holds on; 'odd': the list itself (empty tensors, a NaN, +-inf)."""
    if ('ste', kind) not in _CACHE:
        if kind == 'odd':
            c, pristine = the_list()
            xs = [v.cpu().numpy() for v in c.views(pristine)]
            phases = PHASES
        else:
            keep = [i for i, n in enumerate(SIZES) if n and i not in (NAN_AT, INF_AT)]
            xs = [make(SIZES[i], 900 + i, i % 4).astype(np.float32) for i in keep]
            phases = [PHASES[i] for i in keep]
            _CACHE['ste_levels', kind] = [S_LIST[i] for i in keep]
        gs = [np.random.RandomState(i ^ 77).randn(x.size).astype(np.float32) for i, x in enumerate(xs)]
        _CACHE['ste', kind] = SteList(xs, gs, phases)
        _CACHE.setdefault(('ste_levels', kind), S_LIST)
    return _CACHE['ste', kind], _CACHE['ste_levels', kind]


@pytest.mark.parametrize('tie_mode', ['reference', 'true_arg'])
@pytest.mark.parametrize('kind,bucket', [('clean', 256), ('clean', 512), ('clean', 100), ('odd', 256), ('odd', 512), ('odd', 100),
                                         ('clean', 64), ('clean', 128), ('clean', 1024)])       # (the last three: the other register rows)
def test_ste_equals_the_per_tensor_call_at_each_level_count(kind, bucket, tie_mode):
    L, s_list = ste_list(kind)
    c = L.c
    xs = c.views(L.x)
    x_before = L.x.clone()
    # out of place
    flat_multi, flat_loop = c.flat(filled=False), c.flat(filled=False)
    mt = MultiTensorSTE(xs, c.views(L.g), s_list, bucket, outs=c.views(flat_multi), tie_mode=tie_mode)
    outs = mt.backward()
    assert mt.entry_point == 'qd_multi_ste_backward_levels_f32' and mt.s == tuple(s_list)
    want = [ste.ste_bucket_backward(x, g, bucket, s, out=o, tie_mode=tie_mode) if x.numel() else o
            for x, g, o, s in zip(xs, c.views(L.g), c.views(flat_loop), s_list)]
    torch.cuda.synchronize()
    assert same_bits(L.x, x_before) and c.untouched_outside(flat_multi) and c.untouched_outside(flat_loop)
    for i, (o, w) in enumerate(zip(outs, want)):
        assert same_bits(o, w), (kind, bucket, tie_mode, i, o.numel(), s_list[i], int((o.view(torch.int32) != w.view(torch.int32)).sum()))
    assert not same_bits(flat_multi, L.g)
    # in place on the gradient
    g_multi = L.g.clone()
    outs = MultiTensorSTE(xs, c.views(g_multi), s_list, bucket, tie_mode=tie_mode).backward()
    torch.cuda.synchronize()
    assert c.untouched_outside(g_multi)
    for i, (o, w) in enumerate(zip(outs, want)):
        assert same_bits(o, w), (kind, bucket, tie_mode, 'in place', i)
    if kind == 'clean':                                     # finite inputs: K7's bound of the float64 oracle
        host = flat_multi.cpu().numpy()
        for i, (o, x, g) in enumerate(zip(c.offsets, L.xs, L.gs)):
            errlog.check_ste('multi-tensor K7 with a level count per tensor vs float64 oracle', host[o:o + x.size], x, g, s_list[i],
                             bucket, (bucket, tie_mode, i, x.size, s_list[i]), tie_mode=tie_mode)
    else:
        assert bool(torch.isnan(outs[NAN_AT]).any()) and bool(torch.isnan(outs[INF_AT]).any())


# ---------------------------------------------------------------- routing: equal entries are the scalar
def test_a_list_of_equal_entries_takes_the_existing_entry_points():
    c, pristine = the_list()
    xs = c.views(pristine)
    n = len(xs)
    for bucket, kw, name in ((256, {}, 'qd_multi_uniform_f32'), (None, {}, 'qd_multi_uniform_global_f32'),
                             (256, {'max_element': 0.5}, 'qd_multi_uniform_opt_f32'),
                             (None, {'stochastic_rounding': True}, 'qd_multi_uniform_global_opt_f32')):
        a, b = MultiTensorQuantizer(xs, 16, bucket, **kw), MultiTensorQuantizer(xs, [16] * n, bucket, **kw)
        seed = {'seed': 99} if 'stochastic_rounding' in kw else {}
        qa, qb = a.quantize(**seed), b.quantize(**seed)
        assert a.s == 16 and b.s == (16,) * n and a._levels is None and b._levels is None
        assert a.entry_point == b.entry_point == name
        for i, (u, v) in enumerate(zip(qa, qb)):
            assert same_bits(u, v), (bucket, kw, i)
    L, _ = ste_list('clean')
    xs = L.c.views(L.x)
    a = MultiTensorSTE(xs, L.c.views(L.g), 16, 256, outs=L.c.views(L.c.flat(filled=False)))
    b = MultiTensorSTE(xs, L.c.views(L.g), [16] * len(xs), 256, outs=L.c.views(L.c.flat(filled=False)))
    ga, gb = a.backward(), b.backward()
    assert a.entry_point == b.entry_point == 'qd_multi_ste_backward_f32' and b._levels is None and b.s == (16,) * len(xs)
    assert all(same_bits(u, v) for u, v in zip(ga, gb))


# ---------------------------------------------------------------- capture
def _uniform_at(x, s, bucket, seed):
    lib = _lib.load()
    q = torch.empty_like(x)
    if x.numel():
        ws = _lib.workspace(torch.device(DEV))
        _lib.check(lib.qd_uniform_f32(x.data_ptr(), q.data_ptr(), x.numel(), bucket or 0, s, None, None, None, None, 0, 0.0, 1,
                                      seed & M64, ws.data_ptr(), ws.numel(), _lib.stream_ptr(torch.device(DEV))))
    return q


@pytest.mark.parametrize('bucket', [256, None])
def test_a_captured_launch_with_a_mixed_list_draws_anew_at_every_replay(bucket):
    c, pristine = the_list()
    xs = c.views(pristine)[40:110]                          # 70 tensors: every level count, the NaN / inf tensors, the empty pair
    s_list = S_LIST[40:110]
    n = len(xs)
    k = 0x7FFFFFFFFFFFFFF0                                   # the int64 cell wraps to negative on the way
    mt = MultiTensorQuantizer(xs, s_list, bucket, stochastic_rounding=True, seed_on_device=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # warm-up outside the capture
        mt.quantize(check_pointers=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert mt.reseed(k) == k
    torch.cuda.synchronize()
    calls = qf._STOCHASTIC_CALLS[0]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        mt.quantize(check_pointers=False)                    # recorded, not run: nothing on the host is consulted
    assert qf._STOCHASTIC_CALLS[0] == calls and mt.entry_point.endswith('_levels_f32')
    replays = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replays.append([o.clone() for o in mt.outputs])
    for r, got in enumerate(replays):
        for i, (o, x, s) in enumerate(zip(got, xs, s_list)):
            assert same_bits(o, _uniform_at(x, s, bucket, k + r * n + i)), 'replay %d, tensor %d, s = %d' % (r, i, s)
    assert not any(same_bits(a, b) for a, b in zip(replays[0], replays[1]) if a.numel() >= 255 and not bool(torch.isnan(a).all()))
    assert int(mt.seed_cell.item()) & M64 == (k + 2 * n) & M64


# ---------------------------------------------------------------- the C ABI: the memory contract of the three entry points
ABI_SIZES = [257, 0, 1, 1031, 0, 4100, 3, 70001, 256]
ABI_LEVELS = [16, 256, 2, 17, 4, 3, 1000, 255, 16]


def _levels_at(phase):
    return A.Placed(A.inp(np.array(ABI_LEVELS, np.int32), phase, guard=('index', 2)), torch.device(DEV))


@pytest.mark.parametrize('stoch,clamp', [(0, 0), (1, 1)])
@pytest.mark.parametrize('bucket', [256, None])
def test_abi_memory_contract_of_the_quantizer_entry_points(bucket, stoch, clamp):
    lib, dev = _lib.load(), torch.device(DEV)
    nt, me, seed = len(ABI_SIZES), 0.5, 0xFFFFFFFFFFFFFFFE          # tensor 2 and the ones behind it wrap past 2^64
    tag = ('levels', bucket, stoch, clamp)
    xs = [A.data(n, bucket or 0, 600 + i) for i, n in enumerate(ABI_SIZES)]
    fx = A.Flat(ABI_SIZES, A.F32, dev, 'in', xs)
    wants = []
    for i, x in enumerate(xs):
        xd = torch.from_numpy(x).to(dev)
        q, nb = torch.empty_like(xd), max(1, lib.qd_num_buckets(x.size, bucket or 0))
        ab = torch.empty(2 * nb, device=dev)
        if x.size:
            ws = _lib.workspace(dev)
            _lib.check(lib.qd_uniform_f32(xd.data_ptr(), q.data_ptr(), x.size, bucket or 0, ABI_LEVELS[i], ab.data_ptr(),
                                          ab.data_ptr() + 4 * nb, None, None, clamp, me, stoch, (seed + i) & M64, ws.data_ptr(),
                                          ws.numel(), _lib.stream_ptr(dev)))
            torch.cuda.synchronize()
        wants.append((q.cpu().numpy(), float(ab[0]), float(ab[nb])) if x.size else None)
    results = []
    for phase in (0, 4, 8, 12):                              # the level array at each 4-byte phase of a 16-byte granule
        fq = A.Flat(ABI_SIZES, A.F32, dev, 'out', phases=[(0, 4, 8, 12)[(i + 3 + phase // 4) % 4] for i in range(nt)])
        mt = MultiTensorQuantizer(fx.views(), 16, bucket, outputs=fq.views())      # the plan and the table; the launches below are ours
        lv = _levels_at(phase)
        st = _lib.stream_ptr(dev)
        if bucket is None:
            nbytes = mt._tiles * 2 * 4                       # the documented size, exactly
            ws = A.Placed(A.Arr('out', A.U8, None, nbytes, 0, 'sentinel', None), dev)
            ws.fill(A._ws_bytes(A.FILLS[phase // 4 % 3], nbytes, lib, dev))
            ab = A.Placed(A.out(A.F32, 2 * nt, 4), dev)

            def call(levels, nb_):
                return lib.qd_multi_uniform_global_levels_f32(mt._table.data_ptr(), levels, nt, mt._tiles, clamp, me, stoch, seed, None,
                                                              ab.ptr, ws.ptr, nb_, st)
        else:
            nbytes = 0

            def call(levels, nb_):
                return lib.qd_multi_uniform_levels_f32(mt._table.data_ptr(), levels, nt, mt._tiles, bucket, clamp, me, stoch, seed, None, st)
        refused = [call(None, nbytes), call(lv.ptr + 1, nbytes), call(lv.ptr + 2, nbytes)]
        if bucket is None:
            refused.append(call(lv.ptr, nbytes - 1))
        torch.cuda.synchronize()
        assert refused == [A.ERR_INVALID] * 3 + ([A.ERR_WS] if bucket is None else []), (tag, refused)
        assert all(np.array_equal(o.view(np.uint32), np.full(o.size, A.F_SENT, np.uint32)) for o in [v.cpu().numpy() for v in fq.views()]), \
            (tag, 'a refused call wrote an output')
        if bucket is None:
            assert ab.untouched(ab.read(tag, 'alpha_beta'))
        rc = call(lv.ptr, nbytes)
        torch.cuda.synchronize()
        assert rc == 0, (tag, rc)
        got = fq.read(tag, 'q')                              # nothing between the tensors, every element written
        fx.read(tag, 'x')
        lv.read(tag, 'levels')                               # an input: not written
        for i, (g, w) in enumerate(zip(got, wants)):
            if w is not None:
                assert A._same(g, w[0]), (tag, phase, 'tensor %d of %d elements differs from qd_uniform_f32 at levels[%d], seed + %d'
                                          % (i, ABI_SIZES[i], i, i))
        if bucket is None:
            ws.read(tag, 'workspace')
            abv = ab.read(tag, 'alpha_beta')
            ab.assert_no_sentinel(abv, tag, 'alpha_beta')
            want_ab = np.array([[w[1], w[2]] if w is not None else [1.0, np.inf] for w in wants], np.float32).reshape(-1)
            assert A._same(abv, want_ab), (tag, phase, 'alpha_beta')
        results.append(got)
    for r in results[1:]:
        assert all(A._same(a, b) for a, b in zip(r, results[0])), (tag, 'differs between phases / workspace fills')


@pytest.mark.parametrize('bucket', [256, 100])
def test_abi_memory_contract_of_the_ste_entry_point(bucket):
    lib, dev = _lib.load(), torch.device(DEV)
    nt = len(ABI_SIZES)
    tag = ('ste levels', bucket)
    xs = [A.data(n, bucket, 700 + i) for i, n in enumerate(ABI_SIZES)]
    gs = [np.random.RandomState(800 + i).randn(n).astype(np.float32) for i, n in enumerate(ABI_SIZES)]
    fx = A.Flat(ABI_SIZES, A.F32, dev, 'in', xs)
    fg = A.Flat(ABI_SIZES, A.F32, dev, 'in', gs, guard='grad', phases=[(0, 4, 8, 12)[(i + 2) % 4] for i in range(nt)])
    wants = [ste.ste_bucket_backward(torch.from_numpy(x).to(dev), torch.from_numpy(g).to(dev), bucket, s).cpu().numpy() if x.size else None
             for x, g, s in zip(xs, gs, ABI_LEVELS)]
    for phase in (0, 4, 8, 12):
        fo = A.Flat(ABI_SIZES, A.F32, dev, 'out', phases=[(0, 4, 8, 12)[(i + 3 + phase // 4) % 4] for i in range(nt)])
        mt = MultiTensorSTE(fx.views(), fg.views(), 16, bucket, outs=fo.views())      # the plan and the table
        lv = _levels_at(phase)
        st = _lib.stream_ptr(dev)
        refused = [lib.qd_multi_ste_backward_levels_f32(mt._table.data_ptr(), p, nt, mt._tiles, bucket, 0, st) for p in (None, lv.ptr + 1, lv.ptr + 2)]
        torch.cuda.synchronize()
        assert refused == [A.ERR_INVALID] * 3, (tag, refused)
        assert all(np.array_equal(o.view(np.uint32), np.full(o.size, A.F_SENT, np.uint32)) for o in [v.cpu().numpy() for v in fo.views()])
        rc = lib.qd_multi_ste_backward_levels_f32(mt._table.data_ptr(), lv.ptr, nt, mt._tiles, bucket, 0, st)
        torch.cuda.synchronize()
        assert rc == 0, (tag, rc)
        got = fo.read(tag, 'out')
        fx.read(tag, 'x'); fg.read(tag, 'g'); lv.read(tag, 'levels')
        for i, (g, w) in enumerate(zip(got, wants)):
            if w is not None:
                assert A._same(g, w), (tag, phase, 'tensor %d of %d elements differs from qd_ste_bucket_backward_f32 at levels[%d]' % (i, ABI_SIZES[i], i))


# ---------------------------------------------------------------- the trainer
def _widths(n):
    return [8 if i in (0, n - 1) else (4, 2)[i % 2] for i in range(n)]


@pytest.mark.parametrize('style', ['none', 'complicated'])
def test_trainer_with_a_width_per_parameter_multi_equals_per_tensor(style):
    """8 bits for the first and the last parameter, 4 / 2 alternating in between: two steps of mode='multi' against
    mode='per_tensor', at the learning rate (the default) and under the comparison of
    tests/test_hip_distill.py::test_multi_equals_per_tensor_loop; what does not go through the convolutions -- the quantized
    weights and the STE gradient from the same masters / gradient -- bit for bit."""
    from harness import models
    from harness.distill import DistillTrainer, synthetic_batch
    dev = torch.device(DEV)
    torch.backends.cudnn.deterministic = True

    def trainer(mode):
        torch.manual_seed(0)
        st = models.student()
        return DistillTrainer(st, models.teacher(), dev, num_bits=_widths(len(list(st.parameters()))), bucket_size=256, mode=mode,
                              backprop_quantization_style=style)
    a, b = trainer('multi'), trainer('per_tensor')
    n = len(a.params)
    assert a.s_of == [2 ** w for w in _widths(n)] and a.mt.s == tuple(a.s_of) and a.mt._levels is not None
    losses = []
    for step in range(2):
        x, y = synthetic_batch(16, dev, seed=step)
        la, lb = a.step(x, y), b.step(x, y)
        losses.append((float(la), float(lb)))
    assert a.mt.entry_point == 'qd_multi_uniform_levels_f32'
    if style == 'complicated':
        assert a.mt_ste.entry_point == 'qd_multi_ste_backward_levels_f32'
    print('masters after two steps, %s: %d of %d elements differ in their bits, max |difference| %.3g'
          % (style, int((a.flat_master.view(torch.int32) != b.flat_master.view(torch.int32)).sum()), a.flat_master.numel(),
             float((a.flat_master - b.flat_master).abs().max())))
    assert all(abs(p - q) <= 1e-5 * max(1.0, abs(p)) for p, q in losses), losses
    assert torch.allclose(a.flat_master, b.flat_master, rtol=1e-4, atol=1e-6)
    assert same_bits(a.flat_master, b.flat_master), 'deterministic convolutions: the two modes end on the same bits'
    assert not torch.equal(a.flat_master, torch.zeros_like(a.flat_master))
    # from the same masters: the parameters the next forward runs on, bit for bit, each at its own width
    b.flat_master.copy_(a.flat_master)
    a.quantize(); b.quantize()
    for i, (pa, pb, m) in enumerate(zip(a.params, b.params, a.masters)):
        assert same_bits(pa.data.reshape(-1), pb.data.reshape(-1)), (style, i)
        assert same_bits(pa.data, quantization.uniformQuantization(m, a.s_of[i], bucket_size=256)[0]), (style, i)
    if style == 'complicated':                              # ... and the STE gradient from the same gradient
        grad = torch.randn_like(a.flat_grad)
        for t in (a, b):
            t.flat_grad.copy_(grad)
            t._quantized_step = True
            t.backward_quant()
        assert same_bits(a.flat_grad, b.flat_grad) and not same_bits(a.flat_grad, grad)
    b.restore()


# ---------------------------------------------------------------- compressed checkpoints
@pytest.mark.parametrize('bucket', [256, None])
def test_compressed_file_with_a_level_count_per_tensor_device_equals_host(tmp_path, bucket):
    s_list, sizes = [256, 4, 16, 3, 256, 2, 255], [0, 5, 256 * 3 + 7, 2048, 1000, 70001, 4096]
    gen = torch.Generator(device=DEV).manual_seed(8)
    dev_t = {'t%d' % i: torch.randn(n, device=DEV, generator=gen) for i, n in enumerate(sizes)}
    cpu_t = {k: v.cpu() for k, v in dev_t.items()}
    pd, pc = str(tmp_path / 'dev.qdz'), str(tmp_path / 'cpu.qdz')
    compressed.save_compressed(pd, dev_t, s=s_list, bucket_size=bucket)
    compressed.save_compressed(pc, cpu_t, s=s_list, bucket_size=bucket)
    assert open(pd, 'rb').read() == open(pc, 'rb').read()
    back = compressed.load_compressed(pd, device=torch.device(DEV))
    for (name, t), s in zip(dev_t.items(), s_list):
        want = quantization.uniformQuantization(t, s, bucket_size=bucket)[0] if t.numel() else t
        assert back[name].is_cuda and same_bits(back[name], want), (name, s)
