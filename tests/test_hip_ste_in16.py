"""The one-launch STE backward reading fp16 / bf16 gradients (MultiTensorSTE with 16-bit grads over qd_multi_ste_in16_plan and
qd_multi_ste_backward_in16_f32).

The yardstick is the EXISTING fp32 launch on the widened gradients -- which the rest of the suite holds to the oracle and to
the exact sums -- or tests/exact_sum_cases.py itself; never the 16-bit launch.  Widening is exact, so every comparison is bit for
bit on the fp32 patterns (NaN for NaN where a NaN is expected: ste_in16_cases.assert_same32) and no tolerance appears.  Every
case is a few ten thousand elements."""
import ctypes

import numpy as np
import pytest
import torch

import exact_sum_cases as E
import grid_trip_cases as G
import level_cases as L
import ste_in16_cases as C
from quantized_distillation_amd import _lib
from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer, MultiTensorSTE
from test_hip_grid_trips import assert_trips, lib_cap_is_default

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
TIES = ('reference', 'true_arg')
SENT32 = 0x7FC0BEEF              # a quiet NaN no kernel produces
GUARD = 128                      # bytes of guard band before every carved tensor and after the last one
ENTRY = 'qd_multi_ste_backward_in16_f32'
_CACHE = {}


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev16(patterns, fmt):
    return dev(np.ascontiguousarray(patterns, np.uint16).view(np.int16)).view(C.torch_dtype(fmt))


def levels_for(form, n):
    return 16 if form == 'scalar' else [C.PER_TENSOR_S[i % 5] for i in range(n)]


def fp32_launch(xs, g32, s, bucket, tie):
    """The yardstick: the fp32 one launch on fp32 gradients into fresh outs; -> numpy per tensor."""
    outs = [torch.full_like(g, float('nan')) for g in g32]
    mt = MultiTensorSTE(xs, g32, s, bucket, outs=outs, tie_mode=tie)
    assert mt.grad_dtype is None
    res = mt.backward()
    torch.cuda.synchronize()
    assert mt.entry_point in (None, 'qd_multi_ste_backward_f32', 'qd_multi_ste_backward_levels_f32')
    return [o.cpu().numpy() for o in res]


def in16_launch(xs, g16, s, bucket, tie, outs=None):
    mt = MultiTensorSTE(xs, g16, s, bucket, outs=outs, tie_mode=tie)
    assert mt.grad_dtype == g16[0].dtype and mt._levels is not None and mt._levels.dtype == torch.int32
    res = mt.backward()
    torch.cuda.synchronize()
    assert mt.entry_point == (ENTRY if mt._tiles else None)
    assert all(o.dtype == torch.float32 for o in res)
    return mt, [o.cpu().numpy() for o in res]


def check(got, want, tag):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        C.assert_same32(a, b, tag + ('tensor %d of %d elements' % (i, b.size),))


def parity(bucket, fmt):
    """The parity list on the device, once per (bucket, format): x, g (16 bits), g widened by numpy on the CPU."""
    if (bucket, fmt) not in _CACHE:
        ts = C.parity_tensors(bucket, fmt)
        _CACHE[bucket, fmt] = ([dev(x) for x, _ in ts], [dev16(g, fmt) for _, g in ts], [dev(C.widen(g, fmt)) for _, g in ts])
    return _CACHE[bucket, fmt]


# ---------------------------------------------------------------- 1. parity with the fp32 launch
@pytest.mark.parametrize('fmt', C.FORMATS)
@pytest.mark.parametrize('bucket', C.BUCKETS)
def test_equals_the_fp32_launch_on_widened_gradients(bucket, fmt):
    xs, g16, g32 = parity(bucket, fmt)
    for g, w in zip(g16, g32):
        assert torch.equal(g.float().view(torch.int32), w.view(torch.int32))           # the device's .float() is numpy's widening
    for form in ('scalar', 'per tensor'):
        s = levels_for(form, len(xs))
        for tie in TIES:
            want = fp32_launch(xs, [g.float() for g in g16], s, bucket, tie)
            mt, got = in16_launch(xs, g16, s, bucket, tie)
            assert mt._tiles == C.total_tiles(bucket)
            check(got, want, (bucket, fmt, form, tie))


# ---------------------------------------------------------------- 2. fp32 gradients launch what they always launched
def test_fp32_gradients_launch_what_they_always_launched():
    xs, _, g32 = parity(256, 'bfloat16')
    for s, entry in ((16, 'qd_multi_ste_backward_f32'), ([16] * len(xs), 'qd_multi_ste_backward_f32'),
                     (levels_for('per tensor', len(xs)), 'qd_multi_ste_backward_levels_f32')):
        gs = [g.clone() for g in g32]
        mt = MultiTensorSTE(xs, gs, s, 256)
        assert mt.grad_dtype is None and mt.entry_point is None and mt.outs is mt.grads           # in place, as ever
        assert (mt._levels is None) == (entry == 'qd_multi_ste_backward_f32')
        mt.backward()
        torch.cuda.synchronize()
        assert mt.entry_point == entry


# ---------------------------------------------------------------- 3. every phase of g, x and out
class Carved(object):
    """The tensors of a list carved out of three byte buffers: g at `g_phase`, x at `x_phase`, out at `o_phase` bytes into a
    16-byte granule, each between guard bands.  The bands around g hold the format's NaN (a band that is read poisons a sum),
    out is sentinel-filled throughout."""

    def __init__(self, tensors, fmt, g_phase=0, x_phase=0, o_phase=0):
        self.fmt, self.ns = fmt, [x.size for x, _ in tensors]
        self.g_raw, self.g_off = self._buffer(2, g_phase, np.array([C.NAN16[fmt]], np.uint16))
        self.x_raw, self.x_off = self._buffer(4, x_phase, np.array([SENT32], np.uint32))
        self.o_raw, self.o_off = self._buffer(4, o_phase, np.array([SENT32], np.uint32))
        self.o_fill = self.o_raw.copy()
        for (x, g), go, xo in zip(tensors, self.g_off, self.x_off):
            self.g_raw[go:go + 2 * g.size] = np.ascontiguousarray(g, np.uint16).view(np.uint8)
            self.x_raw[xo:xo + 4 * x.size] = np.ascontiguousarray(x, F32).view(np.uint8)
        self.g_dev, self.x_dev, self.o_dev = dev(self.g_raw), dev(self.x_raw), dev(self.o_raw)
        assert all(t.data_ptr() % 16 == 0 for t in (self.g_dev, self.x_dev, self.o_dev))
        dt = C.torch_dtype(fmt)
        self.gs = [self.g_dev[o:o + 2 * n].view(dt) for o, n in zip(self.g_off, self.ns)]
        self.xs = [self.x_dev[o:o + 4 * n].view(torch.float32) for o, n in zip(self.x_off, self.ns)]
        self.outs = [self.o_dev[o:o + 4 * n].view(torch.float32) for o, n in zip(self.o_off, self.ns)]
        for ts, phase in ((self.gs, g_phase), (self.xs, x_phase), (self.outs, o_phase)):
            assert all(t.data_ptr() % 16 == phase for t in ts if t.numel())

    def _buffer(self, size, phase, fill):
        offs, cur = [], 0
        for n in self.ns:
            cur = (cur + GUARD + 15) // 16 * 16 + phase
            offs.append(cur)
            cur += n * size
        total = (cur + GUARD + 15) // 16 * 16
        return np.frombuffer(fill.tobytes() * (total // fill.itemsize), np.uint8).copy(), offs

    def results(self):
        """The outputs as numpy, after checking the guards: x and g bitwise unchanged, out written on [0, n) of every tensor
        and nowhere else."""
        assert np.array_equal(self.g_dev.cpu().numpy(), self.g_raw), 'g was written'
        assert np.array_equal(self.x_dev.cpu().numpy(), self.x_raw), 'x was written'
        h = self.o_dev.cpu().numpy()
        inside = np.zeros(h.size, bool)
        res = []
        for o, n in zip(self.o_off, self.ns):
            inside[o:o + 4 * n] = True
            v = h[o:o + 4 * n].copy().view(np.uint32)
            assert not np.any(v == SENT32), ('elements nothing wrote', np.flatnonzero(v == SENT32)[:8])
            res.append(v.view(F32))
        assert np.array_equal(h[~inside], self.o_fill[~inside]), 'written outside an output'
        return res


@pytest.mark.parametrize('fmt', C.FORMATS)
@pytest.mark.parametrize('bucket', C.BUCKETS)
def test_every_phase_gives_the_bits_of_the_aligned_run(bucket, fmt):
    ts = C.parity_tensors(bucket, fmt)
    s = levels_for('per tensor', len(ts))
    want = fp32_launch([dev(x) for x, _ in ts], [dev(C.widen(g, fmt)) for _, g in ts], s, bucket, 'reference')
    c0 = Carved(ts, fmt)
    in16_launch(c0.xs, c0.gs, s, bucket, 'reference', outs=c0.outs)
    aligned = c0.results()
    check(aligned, want, (bucket, fmt, 'all aligned'))
    for g_phase in C.G_PHASES:
        for k, x_phase in enumerate(C.F_PHASES):
            o_phase = C.F_PHASES[(k + g_phase // 2) % 4]
            c = Carved(ts, fmt, g_phase, x_phase, o_phase)
            mt, _ = in16_launch(c.xs, c.gs, s, bucket, 'reference', outs=c.outs)
            assert mt._tiles == C.total_tiles(bucket)                        # the cut does not look at g
            check(c.results(), aligned, (bucket, fmt, 'phases g / x / out', g_phase, x_phase, o_phase))


# ---------------------------------------------------------------- 4. the widening table
@pytest.mark.parametrize('fmt', C.FORMATS)
@pytest.mark.parametrize('bucket', C.BUCKETS)
def test_the_widening_table(bucket, fmt):
    x, g, want = C.widening_case(fmt, bucket)
    for g_phase in (0, 2):                                                   # the 8-byte loads and the element-wise ones
        for tie in TIES:
            c = Carved([(x, g)], fmt, g_phase)
            in16_launch(c.xs, c.gs, 16, bucket, tie, outs=c.outs)
            got = c.results()[0].view(np.uint32)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (bucket, fmt, g_phase, tie, int(bad[0]), hex(int(g[bad[0]])), hex(int(got[bad[0]])), hex(int(want[bad[0]])))


# ---------------------------------------------------------------- 5. exact sums
def run_exact(cases, fmt, bucket, tie):
    xs = [dev(c.x) for c in cases]
    for c in cases:                                                          # g is a 16-bit number: the expectation holds as it stands
        assert np.array_equal(C.bits(C.widen(C.to_patterns(c.g, fmt), fmt)), C.bits(c.g)), (c.id, fmt)
    gs = [dev16(C.to_patterns(c.g, fmt), fmt) for c in cases]
    _, got = in16_launch(xs, gs, [c.s for c in cases], bucket, tie)
    return got


@pytest.mark.parametrize('shape', E.ste_shapes(), ids=lambda s: '%d-%d-%d-%s' % s)
def test_single_tensor_exact_sums(shape):
    """Each case of exact_sum_cases as a list of one: S has one possible fp32 value, and g (+-1 .. +-4, 0) is a 16-bit number.
    All three level rows at scale 0; the scales 2^-70 and 2^-104 (the IEEE division) on one register row and one wave row."""
    bucket, nfull, tail, what = shape
    scales = E.STE_SCALES if (bucket, what) in ((256, 'vec'), (100, 'wave')) else (0,)
    for s, den in E.STE_LEVELS:
        for scale in scales:
            case = E.ste_case(s, den, bucket, nfull, tail, scale)
            for tie in TIES:
                want, _ = E.ste_expected(case, tie)                          # (asserts the order-free condition bucket by bucket)
                for fmt in C.FORMATS:
                    got = run_exact([case], fmt, bucket, tie)
                    assert E.same_bits(got[0], want), (case.id, tie, fmt) + E.first_difference(got[0], want)


@pytest.mark.parametrize('tie', TIES)
@pytest.mark.parametrize('bucket', [256, 100])
def test_multi_tensor_exact_sums(bucket, tie):
    cases = [E.ste_case(E.STE_LEVELS[r][0], E.STE_LEVELS[r][1], bucket, nfull, t) for r, nfull, t in E.MSTE_TENSORS]
    wants = [E.ste_expected(c, tie)[0] if c.n else np.zeros(0, F32) for c in cases]
    for fmt in C.FORMATS:
        got = run_exact(cases, fmt, bucket, tie)
        for i, c in enumerate(cases):
            assert E.same_bits(got[i], wants[i]), (bucket, tie, fmt, 'tensor', i, c.id) + E.first_difference(got[i], wants[i])


# ---------------------------------------------------------------- 6. the later trips of the grid-stride loop
@pytest.mark.parametrize('fmt', C.FORMATS)
@pytest.mark.parametrize('bucket', C.BUCKETS)
def test_later_loop_trips_under_grid_caps_1_2_3(lib, bucket, fmt):
    xs, g16, g32 = parity(bucket, fmt)
    s = levels_for('per tensor', len(xs))
    outs = [torch.empty(g.shape, dtype=torch.float32, device=DEV) for g in g16]
    mt = MultiTensorSTE(xs, g16, s, bucket, outs=outs)
    assert_trips('k_multi_ste_in16', mt._tiles, mt._tiles, 4, 4)            # every wave: >= 3 trips, the last one partial
    runs = {}
    for cap in (None,) + G.CAPS:
        for o in outs:
            o.fill_(float('nan'))
        with G.Capped(lib, cap):
            res = mt.backward()
        torch.cuda.synchronize()
        runs[cap] = [o.cpu().numpy().copy() for o in res]
    want = fp32_launch(xs, g32, s, bucket, 'reference')
    check(runs[None], want, (bucket, fmt, 'uncapped'))
    for cap in G.CAPS:
        for i, (a, b) in enumerate(zip(runs[cap], runs[None])):
            assert a.tobytes() == b.tobytes(), (bucket, fmt, 'cap', cap, 'tensor', i)
    assert lib_cap_is_default()


# ---------------------------------------------------------------- 7. the level ladder
@pytest.mark.parametrize('fmt', C.FORMATS)
def test_level_ladder(fmt):
    n, bucket = L.SHAPES['b256']
    ladder = list(L.LADDER)
    xs = [dev(L.inputs(n, 40 + i)) for i in range(len(ladder))]
    pats = [C.to_patterns(L.dense_gradient(n, 140 + i), fmt) for i in range(len(ladder))]
    g16 = [dev16(p, fmt) for p in pats]
    g32 = [dev(C.widen(p, fmt)) for p in pats]
    for tie in TIES:
        want = fp32_launch(xs, g32, ladder, bucket, tie)
        _, got = in16_launch(xs, g16, ladder, bucket, tie)
        check(got, want, ('ladder', fmt, tie))


# ---------------------------------------------------------------- 8. non-finite inputs
@pytest.mark.parametrize('fmt', C.FORMATS)
@pytest.mark.parametrize('bucket', [256, 1024, 100])
def test_non_finite_inputs(bucket, fmt):
    for name, x, g in C.nonfinite_cases(fmt, bucket):
        for tie in TIES:
            want = fp32_launch([dev(x)], [dev(C.widen(g, fmt))], 16, bucket, tie)
            if name.startswith('x'):
                assert np.isnan(want[0]).any(), (name, 'the bucket sum is NaN at the first NaN')
            else:
                assert (~np.isfinite(want[0])).sum() >= 7, name
            for g_phase in (0, 6):
                c = Carved([(x, g)], fmt, g_phase)
                in16_launch(c.xs, c.gs, 16, bucket, tie, outs=c.outs)
                check(c.results(), want, (bucket, fmt, name, tie, g_phase))


# ---------------------------------------------------------------- 9. re-plan, empty tensors
@pytest.mark.parametrize('fmt', C.FORMATS)
def test_the_table_is_planned_again_when_a_gradient_or_an_out_moved(fmt):
    ts = C.parity_tensors(256, fmt)
    xs, g16 = [dev(x) for x, _ in ts], [dev16(g, fmt) for _, g in ts]
    s = levels_for('per tensor', len(ts))
    want = fp32_launch(xs, [dev(C.widen(g, fmt)) for _, g in ts], s, 256, 'reference')
    mt, got = in16_launch(xs, g16, s, 256, 'reference')
    check(got, want, (fmt, 'before'))
    assert any(n == 0 for n in C.sizes(256)) and [o.numel() for o in mt.outs] == C.sizes(256)       # empty tensors in the list
    levels_ptr = mt._levels.data_ptr()
    i = max(range(len(ts)), key=lambda k: ts[k][0].size)
    n = ts[i][0].size
    moved = torch.zeros(n + 1, dtype=C.torch_dtype(fmt), device=DEV)[1:]    # another storage, 2 bytes off 16
    moved.copy_(g16[i])
    mt.grads[i].set_(moved)
    res = mt.backward()
    torch.cuda.synchronize()
    assert mt._ptrs == mt._held() and mt._levels.data_ptr() == levels_ptr and mt.grads[i].data_ptr() % 16 == 2
    check([o.cpu().numpy() for o in res], want, (fmt, 'after a gradient moved'))
    mt.outs[i].set_(torch.full((n + 1,), 3.0, device=DEV)[1:])              # another storage, 4 bytes off 16
    res = mt.backward()
    torch.cuda.synchronize()
    assert mt._ptrs == mt._held() and mt.outs[i].data_ptr() % 16 == 4
    check([o.cpu().numpy() for o in res], want, (fmt, 'after an out moved'))


def test_all_tensors_empty_launches_nothing():
    for dt in (torch.float16, torch.bfloat16):
        xs = [torch.empty(0, device=DEV), torch.empty(0, device=DEV)]
        mt = MultiTensorSTE(xs, [torch.empty(0, dtype=dt, device=DEV) for _ in xs], 16, 256)
        assert mt.grad_dtype == dt and mt._tiles == 0
        assert [o.numel() for o in mt.backward()] == [0, 0] and mt.entry_point is None
        assert all(o.dtype == torch.float32 for o in mt.outs)


# ---------------------------------------------------------------- 10. refusals
def test_python_refusals():
    xs, h, _ = parity(256, 'float16')
    _, b, g32 = parity(256, 'bfloat16')
    with pytest.raises(TypeError):
        MultiTensorSTE(xs, h[:3] + b[3:], 16, 256)                                      # mixed 16-bit types
    with pytest.raises(TypeError):
        MultiTensorSTE(xs, h[:3] + g32[3:], 16, 256)                                    # 16 and 32 bits
    with pytest.raises(TypeError):
        MultiTensorSTE(xs, h, 16, 256, outs=[torch.empty_like(g) for g in h])           # 16-bit outs
    with pytest.raises(TypeError):
        MultiTensorSTE(xs, b, 16, 256, outs=[torch.empty_like(g) for g in h])
    with pytest.raises(TypeError):
        MultiTensorSTE([x.half() for x in xs], h, 16, 256)                              # weights stay fp32
    with pytest.raises(TypeError):
        MultiTensorSTE([x.bfloat16() for x in xs], g32, 16, 256)
    with pytest.raises(TypeError):
        MultiTensorSTE(xs, [g.double() for g in g32], 16, 256)                          # any other dtype
    with pytest.raises(TypeError):
        MultiTensorSTE(xs, [g.to(torch.int16) for g in g32], 16, 256)
    with pytest.raises(ValueError):
        MultiTensorSTE(xs, [g[:-1] if g.numel() else g for g in h], 16, 256)
    with pytest.raises(ValueError):
        MultiTensorSTE(xs, [torch.empty(2 * g.numel(), dtype=g.dtype, device=DEV)[::2] for g in h], 16, 256)
    with pytest.raises(NotImplementedError):
        MultiTensorSTE(xs, h, 16, None)
    mt = MultiTensorSTE(xs, h, 16, 256)
    assert mt.grad_dtype == torch.float16 and mt.outs is not mt.grads
    assert all(o.dtype == torch.float32 and o.shape == g.shape for o, g in zip(mt.outs, mt.grads))
    from quantized_distillation_amd import ste
    with pytest.raises(TypeError):                                                      # the per-tensor call stays fp32-only
        ste.ste_bucket_backward(xs[3], h[3], 256, 16)


def test_c_abi_refusals(lib):
    INVALID = -1
    xs, h, _ = parity(256, 'float16')
    st = _lib.stream_ptr(torch.device(DEV))
    mt = MultiTensorSTE(xs, h, 16, 256)
    for o in mt.outs:
        o.view(torch.int32).fill_(0x5A5A5A5A)
    tab, lev, n, tiles = mt._table.data_ptr(), mt._levels.data_ptr(), mt.n_tensors, mt._tiles
    fn = lib.qd_multi_ste_backward_in16_f32
    for kind in (0, 3, -1):
        assert fn(tab, lev, n, tiles, 256, kind, 0, st) == INVALID
    assert fn(None, lev, n, tiles, 256, 1, 0, st) == INVALID
    assert fn(tab, None, n, tiles, 256, 1, 0, st) == INVALID and fn(tab, lev + 2, n, tiles, 256, 1, 0, st) == INVALID
    assert fn(tab, lev, 0, tiles, 256, 1, 0, st) == INVALID and fn(tab, lev, n, -1, 256, 1, 0, st) == INVALID
    assert fn(tab, lev, n, tiles, 0, 1, 0, st) == INVALID and fn(tab, lev, n, tiles, 256, 1, 2, st) == INVALID
    assert fn(tab, lev, n, 0, 256, 1, 0, st) == 0                            # nothing to do: no launch
    host = (_lib.QdSteDesc * 1)()
    host[0].x, host[0].g, host[0].out, host[0].n = xs[3].data_ptr(), h[3].data_ptr() + 1, mt.outs[3].data_ptr(), xs[3].numel()
    total = ctypes.c_int64(0)
    assert lib.qd_multi_ste_in16_plan(host, 1, 256, ctypes.byref(total)) == INVALID     # an odd g
    assert lib.qd_multi_ste_in16_plan(host, 1, 0, ctypes.byref(total)) == INVALID
    torch.cuda.synchronize()
    assert all(bool((o.view(torch.int32) == 0x5A5A5A5A).all()) for o in mt.outs), 'a refused call wrote its outputs'
    assert fn(tab, lev, n, tiles, 256, 1, 0, st) == 0
    torch.cuda.synchronize()
    assert not any(bool((o.view(torch.int32) == 0x5A5A5A5A).any()) for o in mt.outs)
    assert ctypes.sizeof(_lib.QdSteDesc) == 40


# ---------------------------------------------------------------- 11. the recipe of INTEGRATION.md
def test_a_bf16_student_steps_its_fp32_masters_through_the_one_launch_ste():
    torch.manual_seed(0)
    student = torch.nn.Sequential(torch.nn.Linear(64, 96), torch.nn.ReLU(), torch.nn.Linear(96, 10)).to(DEV)
    masters = [p.detach().clone() for p in student.parameters()]                   # fp32, owned by the trainer
    student.to(torch.bfloat16)
    params = list(student.parameters())
    s, bucket, lr = [256, 16, 256, 16], 256, 0.1
    # one flat 16-bit gradient buffer whose views are bound as p.grad: the table's pointers stay valid
    sizes = [p.numel() for p in params]
    flat16 = torch.zeros(sum(sizes), dtype=torch.bfloat16, device=DEV)
    flat32 = torch.zeros(sum(sizes), dtype=torch.float32, device=DEV)
    views16, views32, at = [], [], 0
    for p, n in zip(params, sizes):
        views16.append(flat16[at:at + n])
        views32.append(flat32[at:at + n])
        p.grad = views16[-1].view_as(p)
        at += n
    mt = MultiTensorQuantizer(masters, s, bucket, outputs=[p.data for p in params])
    mt_ste = MultiTensorSTE(masters, views16, s, bucket, outs=views32)
    assert mt_ste.grad_dtype == torch.bfloat16
    mt.quantize()
    x = torch.randn(32, 64, device=DEV).to(torch.bfloat16)
    student(x).float().pow(2).mean().backward()
    assert all(p.grad.data_ptr() == v.data_ptr() and p.grad.dtype == torch.bfloat16 for p, v in zip(params, views16))
    assert bool(flat16.float().abs().sum() > 0)
    tiles = mt_ste._tiles
    mt_ste.backward()
    torch.cuda.synchronize()
    assert mt_ste.entry_point == ENTRY and mt_ste._tiles == tiles
    # the same step the way the parent commit offers it: upcast, then the fp32 STE in place
    up = [p.grad.float().reshape(-1) for p in params]
    MultiTensorSTE(masters, up, s, bucket).backward()
    want = [m.clone().add_(u.view_as(m), alpha=-lr) for m, u in zip(masters, up)]
    with torch.no_grad():
        for m, v in zip(masters, views32):
            m.add_(v.view_as(m), alpha=-lr)
    torch.cuda.synchronize()
    for i, (m, w) in enumerate(zip(masters, want)):
        assert torch.equal(m.view(torch.int32), w.view(torch.int32)), ('master', i)
    mt.quantize()                                                                  # the next step's student
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p.float()).all()) for p in params)
