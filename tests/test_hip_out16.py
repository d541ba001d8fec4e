"""fp16 / bf16 outputs of the one-launch quantizer (MultiTensorQuantizer(out_dtype=...) over qd_multi_uniform_out16_f32 and
qd_multi_uniform_global_out16_f32).

The yardstick everywhere is the EXISTING fp32 launch on the same inputs and seeds -- which the rest of the suite holds to the
oracle -- copied to the CPU and converted there with .to(dtype): IEEE round to nearest even.  It is never the 16-bit launch
itself.  The comparison is on the 16-bit patterns where the expectation is no NaN, NaN for NaN elsewhere
(out16_cases.assert_same16).  Every case is a few thousand elements."""
import ctypes

import numpy as np
import pytest
import torch

import level_cases as L
import out16_cases as C
from quantized_distillation_amd import _lib
from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer
from test_hip_grid_trips import tensor_list

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = [torch.float16, torch.bfloat16]
DT_IDS = ['fp16', 'bf16']
BUCKETS = [256, 128, 64, 100, None]
SEED0 = 0x1234ABCD5678
GRID_CAP_DEFAULT = 1 << 20
GUARD = 64                      # sentinel elements before every carved tensor and after the last one
SENT16 = 0x5A5A                 # as a 16-bit pattern (the outputs are compared as patterns)
SENT32 = 777.0
PER_TENSOR_S = (2, 4, 16, 256, 5)
FORMS = {
    'scalar': lambda n: dict(s=16),
    'clamp': lambda n: dict(s=16, max_element=0.5),
    'stochastic': lambda n: dict(s=16, stochastic_rounding=True),
    'levels+clamp+stochastic': lambda n: dict(s=[PER_TENSOR_S[i % 5] for i in range(n)], max_element=0.5, stochastic_rounding=True),
}
_CACHE = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(mt):
    outs = mt.quantize(seed=SEED0) if mt.stochastic_rounding and not mt.seed_on_device else mt.quantize()
    torch.cuda.synchronize()
    return outs


def to16(outs32, dtype):
    """The expectation: the fp32 launch's outputs, converted on the CPU."""
    return [o.detach().cpu().to(dtype) for o in outs32]


def check(outs16, want16, tag):
    assert len(outs16) == len(want16)
    for i, (o, w) in enumerate(zip(outs16, want16)):
        C.assert_same16(o.reshape(-1), w.reshape(-1), tag + ('tensor %d of %d elements' % (i, w.numel()),))


def entry_of(bucket):
    return 'qd_multi_uniform_global_out16_f32' if bucket is None else 'qd_multi_uniform_out16_f32'


# ---------------------------------------------------------------- parity
def parity_list(bucket):
    if ('xs', bucket) not in _CACHE:
        _CACHE['xs', bucket] = [dev(x) for x in tensor_list(bucket)]
    return _CACHE['xs', bucket]


def parity_fp32(bucket, form):
    """The fp32 launch's outputs on the CPU: computed once per (bucket, form), never written."""
    if ('q32', bucket, form) not in _CACHE:
        xs = parity_list(bucket)
        mt = MultiTensorQuantizer(xs, bucket_size=bucket, **FORMS[form](len(xs)))
        assert mt.out_dtype is None and mt.entry_point is None
        _CACHE['q32', bucket, form] = [o.cpu() for o in run(mt)]
        assert 'out16' not in mt.entry_point
    return _CACHE['q32', bucket, form]


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('bucket', BUCKETS)
def test_equals_the_fp32_launch_converted(bucket, dtype, form):
    xs = parity_list(bucket)
    before = [x.clone() for x in xs]
    want = to16(parity_fp32(bucket, form), dtype)
    kw = FORMS[form](len(xs))
    mt = MultiTensorQuantizer(xs, bucket_size=bucket, out_dtype=dtype, **kw)
    assert mt.out_dtype == dtype and all(o.dtype == dtype and o.numel() == x.numel() for o, x in zip(mt.outputs, xs))
    assert mt._levels is not None and mt._levels.dtype == torch.int32, 'the 16-bit object always owns a levels array'
    assert mt._levels.tolist() == (kw['s'] if isinstance(kw['s'], list) else [16] * len(xs))
    outs = run(mt)
    assert mt.entry_point == entry_of(bucket)
    check(outs, want, (bucket, dtype, form))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(xs, before)), 'the inputs are inputs only'
    if bucket is None:                         # the alpha_beta rows have the bits of the fp32 launch's
        m32 = MultiTensorQuantizer(xs, bucket_size=None, **kw)
        run(m32)
        live = torch.tensor([x.numel() > 0 for x in xs], device=DEV)
        assert torch.equal(mt.alpha_beta.view(torch.int32)[live], m32.alpha_beta.view(torch.int32)[live])
    if kw.get('stochastic_rounding'):          # the draws are in use: another seed, other values
        again = mt.quantize(seed=SEED0 + 1000)
        torch.cuda.synchronize()
        assert mt.last_seed == SEED0 + 1000
        big = max(range(len(xs)), key=lambda i: xs[i].numel())
        assert not torch.equal(again[big].cpu().view(torch.int16), want[big].view(torch.int16))


def test_out_dtype_none_launches_what_it_always_launched():
    xs = parity_list(256)
    for kw, name in ((dict(s=16), 'qd_multi_uniform_f32'), (dict(s=16, max_element=0.5), 'qd_multi_uniform_opt_f32'),
                     (dict(s=[PER_TENSOR_S[i % 5] for i in range(len(xs))]), 'qd_multi_uniform_levels_f32')):
        for extra in (dict(), dict(out_dtype=None), dict(out_dtype=torch.float32)):
            mt = MultiTensorQuantizer(xs, bucket_size=256, **kw, **extra)
            outs = run(mt)
            assert mt.entry_point == name and mt.out_dtype is None and all(o.dtype == torch.float32 for o in outs)
            assert (mt._levels is None) == (not isinstance(kw['s'], list))


# ---------------------------------------------------------------- alignment and bounds
class Carved16(object):
    """Outputs carved out of one flat 16-bit buffer: tensor i starts `phases[i]` ELEMENTS (2 bytes each) past a 16-byte boundary,
    at least GUARD elements after the end of the one before; everything outside the tensors holds the pattern SENT16."""

    def __init__(self, sizes, phases, dtype):
        self.sizes, self.offsets, off = list(sizes), [], 0
        for n, ph in zip(sizes, phases):
            off = -(-(off + GUARD) // 8) * 8 + ph
            self.offsets.append(off)
            off += n
        self.total = off + GUARD
        self.dtype = dtype
        self.inside = torch.zeros(self.total, dtype=torch.bool, device=DEV)
        for o, n in zip(self.offsets, self.sizes):
            self.inside[o:o + n] = True

    def flat(self):
        f = torch.full((self.total,), SENT16, dtype=torch.int16, device=DEV).view(self.dtype)
        assert f.data_ptr() % 16 == 0
        return f

    def views(self, flat):
        vs = [flat[o:o + n] for o, n in zip(self.offsets, self.sizes)]
        for v, o in zip(vs, self.offsets):
            assert v.data_ptr() == flat.data_ptr() + 2 * o
        return vs

    def untouched_outside(self, flat):
        return bool((flat.view(torch.int16)[~self.inside] == SENT16).all())


def carve32(xs, phases):
    """Copies of the fp32 tensors xs, tensor i starting phases[i] floats past a 16-byte boundary of one flat buffer."""
    offsets, off = [], 0
    for x, ph in zip(xs, phases):
        off = -(-(off + GUARD) // 4) * 4 + ph
        offsets.append(off)
        off += x.numel()
    flat = torch.full((off + GUARD,), SENT32, device=DEV)
    assert flat.data_ptr() % 16 == 0
    views = []
    for x, o in zip(xs, offsets):
        flat[o:o + x.numel()].copy_(x)
        views.append(flat[o:o + x.numel()])
    return flat, views


def alignment_sizes(bucket):
    """16 tensors: whole tiles of full ROW buckets (the register path when the pointers allow it), ragged ones, short ones."""
    unit = bucket if bucket else 1024
    return [4 * unit, 2 * unit + 7, unit, 5 * unit + 1] * 4


OUT_PHASES = [i % 8 for i in range(16)]                # every 2-byte phase of 16 bytes: 0, 1, 2, 3, 4, 5, 6, 7
IN_PHASES = [(i // 8) % 2 for i in range(16)]          # 4-byte phases 0 and 1 of 16 bytes


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('bucket', BUCKETS)
def test_any_2_byte_alignment_gives_the_same_bits_and_writes_nothing_outside(bucket, dtype):
    sizes = alignment_sizes(bucket)
    gen = torch.Generator(device=DEV).manual_seed(17)
    xs = [torch.randn(n, device=DEV, generator=gen) for n in sizes]
    s_list = [PER_TENSOR_S[i % 5] for i in range(16)]
    for kw in (dict(), dict(stochastic_rounding=True, max_element=0.5)):
        want = to16(run(MultiTensorQuantizer(xs, s_list, bucket, **kw)), dtype)
        # the aligned run: every pointer on a 16-byte boundary -- full buckets / tiles on the register path
        ca = Carved16(sizes, [0] * 16, dtype)
        fa = ca.flat()
        fxa, xa = carve32(xs, [0] * 16)
        aligned = run(MultiTensorQuantizer(xa, s_list, bucket, outputs=ca.views(fa), **kw))
        assert ca.untouched_outside(fa)
        check(aligned, want, (bucket, dtype, 'aligned', tuple(kw)))
        # the same data at every phase: outputs 0 and 4 elements in still qualify for the register path (8-byte stores) while
        # their inputs are aligned, everything else takes the row path
        c = Carved16(sizes, OUT_PHASES, dtype)
        f = c.flat()
        fx, xv = carve32(xs, IN_PHASES)
        fx0 = fx.clone()
        outs = run(MultiTensorQuantizer(xv, s_list, bucket, outputs=c.views(f), **kw))
        assert c.untouched_outside(f), 'the launch wrote outside its outputs'
        assert torch.equal(fx.view(torch.int32), fx0.view(torch.int32))
        check(outs, want, (bucket, dtype, 'every phase', tuple(kw)))
        for i, (a, b) in enumerate(zip(outs, aligned)):
            C.assert_same16(a, b.cpu(), (bucket, dtype, 'phase %d / %d against the aligned run' % (OUT_PHASES[i], IN_PHASES[i])))


# ---------------------------------------------------------------- rounding
@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('bucket', list(C.BUCKETS))
def test_rounding_cases(bucket, dtype):
    """The table of tests/out16_cases.py (proven on the CPU by tests/test_out16_cases_host.py): ties, the top of each format, the
    first value that becomes inf, fp16 subnormals, negative values and a negative zero, a NaN and an inf."""
    if 'cases' not in _CACHE:
        _CACHE['cases'] = [dev(x) for _, x in C.all_tensors()]
    xs = _CACHE['cases']
    fmt = str(dtype).replace('torch.', '')
    s_list = [C.LEVELS[i % len(C.LEVELS)] for i in range(len(xs))]
    for kw in (dict(), dict(stochastic_rounding=True)):
        want = to16(run(MultiTensorQuantizer(xs, s_list, bucket, **kw)), dtype)
        outs = run(MultiTensorQuantizer(xs, s_list, bucket, out_dtype=dtype, **kw))
        check(outs, want, (bucket, dtype, 'rounding cases', tuple(kw)))
        for (name, v, intended), o in zip(C.EXACT, outs):
            p16 = C.patterns(o)
            assert (p16[0::2] == 0).all(), (name, fmt, bucket, 'the zeros')
            if intended[fmt] is not None:
                assert (p16[1::2] == intended[fmt]).all(), (name, fmt, bucket, '0x%04X, intended 0x%04X' % (p16[1], intended[fmt]))
        for (name, _), o, w in zip(C.nonfinite(), outs[len(C.EXACT):], want[len(C.EXACT):]):
            assert bool(torch.isnan(w).any()) and bool(torch.equal(torch.isnan(o).cpu(), torch.isnan(w))), (name, bucket)


# ---------------------------------------------------------------- later trips of the grid-stride loops
@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('bucket', BUCKETS)
def test_later_loop_trips_under_grid_caps_1_2_3(bucket, dtype):
    lib = _lib.load()
    xs = parity_list(bucket)
    for form in ('scalar', 'levels+clamp+stochastic'):
        want = to16(parity_fp32(bucket, form), dtype)
        mt = MultiTensorQuantizer(xs, bucket_size=bucket, out_dtype=dtype, **FORMS[form](len(xs)))
        assert mt._tiles >= 3 * 3 * 4, 'every wave of three blocks makes at least three trips'
        for cap in (1, 2, 3):
            prev = lib.qd_set_grid_cap(cap)
            try:
                assert prev == GRID_CAP_DEFAULT
                outs = run(mt)
            finally:
                lib.qd_set_grid_cap(prev)
            check(outs, want, (bucket, dtype, form, 'cap %d' % cap))
    assert lib.qd_set_grid_cap(-1) == GRID_CAP_DEFAULT, 'the cap reads back as the default'


# ---------------------------------------------------------------- the level ladder
@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('bucket', [256, None])
def test_level_ladder(bucket, dtype):
    """The 40 level counts of tests/level_cases.py, one per tensor, deterministic and stochastic."""
    if 'ladder' not in _CACHE:
        _CACHE['ladder'] = [dev(L.inputs(1283, 4000 + i)) for i in range(len(L.LADDER))]
    xs = _CACHE['ladder']
    s_list = list(L.LADDER)
    assert len(s_list) == 40
    for kw in (dict(), dict(stochastic_rounding=True)):
        want = to16(run(MultiTensorQuantizer(xs, s_list, bucket, **kw)), dtype)
        mt = MultiTensorQuantizer(xs, s_list, bucket, out_dtype=dtype, **kw)
        assert mt._levels.tolist() == s_list
        check(run(mt), want, (bucket, dtype, 'ladder', tuple(kw)))


# ---------------------------------------------------------------- seeds, capture, re-planning
SEED_SIZES = [700, 0, 4096, 257, 1024 + 5]


def seed_list():
    if 'seeds' not in _CACHE:
        gen = torch.Generator(device=DEV).manual_seed(23)
        _CACHE['seeds'] = [torch.randn(n, device=DEV, generator=gen) for n in SEED_SIZES]
    return _CACHE['seeds']


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('bucket', [256, None])
def test_tensor_i_draws_with_seed0_plus_i(bucket, dtype):
    xs = seed_list()
    mt = MultiTensorQuantizer(xs, 16, bucket, stochastic_rounding=True, out_dtype=dtype)
    outs = mt.quantize(seed=SEED0)
    torch.cuda.synchronize()
    assert mt.last_seed == SEED0
    for i, x in enumerate(xs):
        if x.numel():                                        # the fp32 launch of tensor i alone: position 0 draws with its seed0
            one = MultiTensorQuantizer([x], 16, bucket, stochastic_rounding=True).quantize(seed=SEED0 + i)
            torch.cuda.synchronize()
            C.assert_same16(outs[i], one[0].cpu().to(dtype), (bucket, dtype, 'tensor %d draws with seed0 + %d' % (i, i)))
    with pytest.raises(ValueError):
        MultiTensorQuantizer(xs, 16, bucket, out_dtype=dtype).quantize(seed=1)


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('bucket', [256, None])
def test_a_captured_launch_draws_anew_at_every_replay(bucket, dtype):
    """seed_on_device: replay r equals the by-value launch at seed0 + r * n_tensors (tensor i: + i).  The captured region is
    one chain on one stream -- the kernels of the launch, then the add_ on the seed word -- without parallel branches."""
    xs = seed_list()
    n = len(xs)
    mt = MultiTensorQuantizer(xs, 16, bucket, stochastic_rounding=True, seed_on_device=True, out_dtype=dtype)
    by_value16 = MultiTensorQuantizer(xs, 16, bucket, stochastic_rounding=True, out_dtype=dtype)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # warm-up outside the capture
        mt.quantize(check_pointers=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert mt.reseed(SEED0) == SEED0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        mt.quantize(check_pointers=False)                    # recorded, not run
        with pytest.raises(RuntimeError, match='during stream capture'):       # a by-value seed would be replayed: refused,
            by_value16.quantize(check_pointers=False)                           # before anything is launched
        with pytest.raises(RuntimeError, match='during stream capture'):
            by_value16.quantize(check_pointers=False, seed=SEED0)
    torch.cuda.synchronize()
    assert int(mt.seed_cell.item()) == SEED0, 'nothing ran during the capture'
    replays = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replays.append([o.clone() for o in mt.outputs])
    assert int(mt.seed_cell.item()) == SEED0 + 2 * n
    by_value = MultiTensorQuantizer(xs, 16, bucket, stochastic_rounding=True)
    for r, got in enumerate(replays):
        want = by_value.quantize(seed=SEED0 + r * n)
        torch.cuda.synchronize()
        check(got, to16(want, dtype), (bucket, dtype, 'replay %d' % r))
    assert not torch.equal(replays[0][2].view(torch.int16), replays[1][2].view(torch.int16))


@pytest.mark.parametrize('bucket', [256, None])
def test_the_table_is_planned_again_when_an_output_moved(bucket):
    xs = [x.clone() for x in seed_list()]
    dtype = torch.bfloat16
    mt = MultiTensorQuantizer(xs, [16, 4, 256, 5, 2], bucket, max_element=0.5, out_dtype=dtype)
    want = to16(run(MultiTensorQuantizer(xs, [16, 4, 256, 5, 2], bucket, max_element=0.5)), dtype)
    check(run(mt), want, (bucket, 'before'))
    levels_ptr = mt._levels.data_ptr()
    mt.outputs[2].set_(torch.full((4096 + 1,), 3.0, dtype=dtype, device=DEV)[1:])          # another storage, 2 bytes off 16
    outs = run(mt)
    assert mt._ptrs == mt._held() and mt._levels.data_ptr() == levels_ptr
    check(outs, want, (bucket, 'after an output moved'))


# ---------------------------------------------------------------- errors
def test_python_refusals():
    xs = seed_list()
    h = [torch.empty(x.numel(), dtype=torch.float16, device=DEV) for x in xs]
    b = [torch.empty(x.numel(), dtype=torch.bfloat16, device=DEV) for x in xs]
    with pytest.raises(TypeError):
        MultiTensorQuantizer(xs, 16, 256, outputs=h[:2] + b[2:])                        # mixed
    with pytest.raises(TypeError):
        MultiTensorQuantizer(xs, 16, 256, outputs=[torch.empty(x.numel(), dtype=torch.float64, device=DEV) for x in xs])
    with pytest.raises(TypeError):
        MultiTensorQuantizer(xs, 16, 256, outputs=[torch.empty_like(x) for x in xs], out_dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        MultiTensorQuantizer(xs, 16, 256, outputs=h, out_dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        MultiTensorQuantizer(xs, 16, 256, out_dtype=torch.float64)
    with pytest.raises(TypeError):                                                     # inputs stay fp32
        MultiTensorQuantizer([x.half() for x in xs], 16, 256, out_dtype=torch.float16)
    with pytest.raises(ValueError):
        MultiTensorQuantizer(xs, 16, 256, outputs=[t[:-1] if t.numel() else t for t in h])
    with pytest.raises(ValueError):
        MultiTensorQuantizer(xs, 16, 256, outputs=[torch.empty(2 * x.numel(), dtype=torch.float16, device=DEV)[::2] for x in xs])
    assert MultiTensorQuantizer(xs, 16, 256, outputs=h).out_dtype == torch.float16      # the outputs' own dtype is enough
    assert MultiTensorQuantizer(xs, 16, 256, outputs=b, out_dtype=torch.bfloat16).out_dtype == torch.bfloat16


def test_c_abi_refusals():
    lib = _lib.load()
    INVALID, TOO_SMALL = -1, -2
    xs = seed_list()
    st = _lib.stream_ptr(torch.device(DEV))
    cell = torch.zeros(2, dtype=torch.int64, device=DEV)
    for bucket in (256, None):
        mt = MultiTensorQuantizer(xs, 16, bucket, out_dtype=torch.float16)
        for o in mt.outputs:
            o.view(torch.int16).fill_(SENT16)
        tab, lev, n, tiles = mt._table.data_ptr(), mt._levels.data_ptr(), mt.n_tensors, mt._tiles

        def call(kind=1, levels=lev, seed_cell=None, stochastic=0, ws_bytes=None, total=tiles):
            if bucket is None:
                return lib.qd_multi_uniform_global_out16_f32(
                    tab, levels, n, total, kind, 0, 0.0, stochastic, 5, seed_cell, mt.alpha_beta.data_ptr(), mt._scratch.data_ptr(),
                    mt._scratch.numel() * 4 if ws_bytes is None else ws_bytes, st)
            return lib.qd_multi_uniform_out16_f32(tab, levels, n, total, bucket, kind, 0, 0.0, stochastic, 5, seed_cell, st)

        assert call(kind=0) == INVALID and call(kind=3) == INVALID and call(kind=-1) == INVALID
        assert call(levels=None) == INVALID and call(levels=lev + 2) == INVALID
        assert call(seed_cell=cell.data_ptr() + 4, stochastic=1) == INVALID
        assert call(total=-1) == INVALID
        assert call(total=0) == 0                            # nothing to do: no launch
        if bucket is None:
            assert call(ws_bytes=tiles * 8 - 1) == TOO_SMALL
        else:
            assert lib.qd_multi_uniform_out16_f32(tab, lev, n, tiles, 0, 1, 0, 0.0, 0, 5, None, st) == INVALID       # bucket 0
        assert lib.qd_multi_uniform_out16_f32(tab, lev, n, tiles, 256, 1, 1, -1.0, 0, 5, None, st) == INVALID          # the clamp limit
        torch.cuda.synchronize()
        assert all(bool((o.view(torch.int16) == SENT16).all()) for o in mt.outputs), 'a refused call wrote its outputs'
        assert call() == 0 and call(kind=1, seed_cell=cell.data_ptr() + 8, stochastic=1) == 0
        torch.cuda.synchronize()
        assert not any(bool((o.view(torch.int16) == SENT16).all()) for o in mt.outputs if o.numel())
    assert ctypes.sizeof(_lib.QdTensorDesc) == 32


def test_all_tensors_empty_launches_nothing():
    xs = [torch.empty(0, device=DEV), torch.empty(0, device=DEV)]
    for bucket in (256, None):
        mt = MultiTensorQuantizer(xs, 16, bucket, out_dtype=torch.float16)
        assert mt._tiles == 0 and [o.numel() for o in mt.quantize()] == [0, 0] and mt.entry_point is None


# ---------------------------------------------------------------- the recipe of INTEGRATION.md
def test_a_bf16_student_bound_to_fp32_masters():
    torch.manual_seed(0)
    student = torch.nn.Sequential(torch.nn.Linear(64, 96), torch.nn.ReLU(), torch.nn.Linear(96, 10)).to(DEV)
    masters = [p.detach().clone() for p in student.parameters()]                   # fp32, owned by the trainer
    student.to(torch.bfloat16)
    params = list(student.parameters())
    assert all(p.dtype == torch.bfloat16 for p in params)
    mt = MultiTensorQuantizer(masters, [256, 16, 256, 16], 256, outputs=[p.data for p in params])
    assert mt.out_dtype == torch.bfloat16 and mt.entry_point is None
    mt.quantize()
    torch.cuda.synchronize()
    assert mt.entry_point == 'qd_multi_uniform_out16_f32'
    want = to16(run(MultiTensorQuantizer(masters, [256, 16, 256, 16], 256)), torch.bfloat16)
    check([p.data for p in params], want, ('the parameters are the quantized masters',))
    x = torch.randn(32, 64, device=DEV).to(torch.bfloat16)
    loss = student(x).float().pow(2).mean()
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    assert all(p.grad is not None and p.grad.dtype == torch.bfloat16 and p.grad.shape == p.shape for p in params)
    # the update belongs to the caller: upcast the gradient, step the master, quantize again
    with torch.no_grad():
        for m, p in zip(masters, params):
            m.add_(p.grad.float(), alpha=-0.1)
    mt.quantize()
    torch.cuda.synchronize()
    want = to16(run(MultiTensorQuantizer(masters, [256, 16, 256, 16], 256)), torch.bfloat16)
    check([p.data for p in params], want, ('after a step',))
