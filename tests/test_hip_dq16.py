"""The one-launch differentiable-quantization sweeps on a 16-bit student: MultiTensorDiffQuant with fp16 / bf16 outputs
(qd_multi_nearest_out16_f32) and fp16 / bf16 gradients (qd_multi_point_grad_in16_f32).

The yardstick is the EXISTING fp32 launch -- which the rest of the suite holds to the oracle and to the exact sums -- followed
by .cpu().to(dtype) (forward), or run on the widened gradients in freshly allocated buffers (backward), or the exact sums of
tests/exact_sum_cases.py; never the 16-bit launch.  The conversion of the store and the widening of the load are exact
operations, so every comparison is bit for bit (NaN for NaN where a NaN is expected) and no tolerance appears."""
import numpy as np
import pytest
import torch

import dq16_cases as C
import exact_sum_cases as E
import grid_trip_cases as G
from quantized_distillation_amd import _lib
from quantized_distillation_amd.multi_tensor import MultiTensorDiffQuant
from ste_in16_cases import assert_same32
from test_hip_grid_trips import assert_trips, lib_cap_is_default

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
GUARD = 128                      # bytes of guard band before every carved tensor and after the last one
SENT16 = 0x7FA5                  # a NaN pattern of both formats that no conversion produces
FWD, FWD16 = 'qd_multi_nearest_f32', 'qd_multi_nearest_out16_f32'
BWD, BWD16 = 'qd_multi_point_grad_f32', 'qd_multi_point_grad_in16_f32'
INVALID = -1
_CACHE = {}


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev16(patterns, fmt):
    return dev(np.ascontiguousarray(patterns, np.uint16).view(np.int16)).view(C.torch_dtype(fmt))


def empty_like(ts, dtype=torch.float32):
    return [torch.empty(t.numel(), dtype=dtype, device=DEV) for t in ts]


def sync():
    torch.cuda.synchronize()


def carve(ns, size, phase, fill):
    """A byte buffer of `fill` patterns and the byte offsets of tensors of ns[i] elements of `size` bytes, each `phase` bytes
    into a 16-byte granule between guard bands."""
    offs, cur = [], 0
    for n in ns:
        cur = (cur + GUARD + 15) // 16 * 16 + phase
        offs.append(cur)
        cur += n * size
    total = (cur + GUARD + 15) // 16 * 16
    return np.frombuffer(fill.tobytes() * (total // fill.itemsize), np.uint8).copy(), offs


# ================================================================ forward
def forward32(xs, pts, k, bucket):
    """The yardstick: the fp32 launch -> ([q fp32 on the CPU], [idx bytes])."""
    outs = [torch.full((x.numel(),), float('nan'), device=DEV) for x in xs]
    mt = MultiTensorDiffQuant(xs, outs, empty_like(xs), k, bucket)
    assert mt.out_dtype is None and mt.grad_dtype is None and mt.entry_point is None
    mt.forward(pts)
    sync()
    assert mt.entry_point == (FWD if mt._tiles else None)
    return [o.cpu() for o in outs], [i.cpu().numpy() for i in mt.indices]


def forward16(xs, pts, k, bucket, fmt, outs=None):
    dt = C.torch_dtype(fmt)
    if outs is None:
        outs = [dev16(np.full(x.numel(), SENT16, np.uint16), fmt) for x in xs]
    mt = MultiTensorDiffQuant(xs, outs, empty_like(xs), k, bucket)
    assert mt.out_dtype == dt and mt.grad_dtype is None
    res = mt.forward(pts)
    sync()
    assert mt.entry_point == (FWD16 if mt._tiles else None)
    assert all(o.dtype == dt for o in res)
    return mt, [o.cpu() for o in res], [i.cpu().numpy() for i in mt.indices]


def check_forward(got, idx, want32, want_idx, fmt, tag):
    dt = C.torch_dtype(fmt)
    for i, (g, w) in enumerate(zip(got, want32)):
        C.assert_same16(g, w.to(dt), tag + ('tensor %d of %d elements' % (i, w.numel()),))
        assert idx[i].tobytes() == want_idx[i].tobytes(), tag + ('idx of tensor', i)


@pytest.mark.parametrize('fmt', C.FORMATS)
@pytest.mark.parametrize('bucket', C.FWD_BUCKETS)
def test_the_rounding_table_and_the_non_finite_tensors(bucket, fmt):
    table = C.exact_tensors()
    xs = [dev(x) for _, x in table]
    for k in C.FWD_K:
        pts = dev(np.tile(C.points_row(k), (len(xs), 1)))
        want, want_idx = forward32(xs, pts, k, bucket)
        _, got, idx = forward16(xs, pts, k, bucket, fmt)
        check_forward(got, idx, want, want_idx, fmt, (bucket, k, fmt))
        for (name, v, pat), x, g32, g16 in zip(C.EXACT, xs, want, got):      # the fp32 result is {0, v}; the hand-written patterns
            assert torch.equal(g32.view(torch.int32), x.cpu().view(torch.int32)), (name, bucket, k)
            if pat[fmt] is not None:
                p = g16.view(torch.int16).numpy().view(np.uint16)
                assert (p[1::2] == pat[fmt]).all() and (p[0::2] == 0).all(), (name, bucket, k, fmt, hex(int(p[1])))
        for (name, x), g16, ix in zip(table[len(C.EXACT):], got[len(C.EXACT):], idx[len(C.EXACT):]):
            bad = ~torch.isfinite(g16.float()).numpy()                       # (the inf itself stays an inf, everything beside it is NaN)
            assert bad.all() if bucket is None else (bad[300] and not bad[0]), (name, bucket, k)
            if name == 'a NaN':
                assert ix[300] == k - 1, (name, 'a NaN master takes the last index', int(ix[300]))


@pytest.mark.parametrize('fmt', C.FORMATS)
@pytest.mark.parametrize('bucket', C.FWD_BUCKETS)
def test_a_random_list_with_ragged_buckets_and_small_tensors(bucket, fmt):
    for k in (4, 16, 256):
        ts, pts = C.random_list(bucket, k, fmt)
        xs, pd = [dev(x) for x, _ in ts], dev(pts)
        want, want_idx = forward32(xs, pd, k, bucket)
        mt, got, idx = forward16(xs, pd, k, bucket, fmt)
        assert mt._tiles == sum(C.forward_tiles(x.numel(), bucket) for x in xs)
        check_forward(got, idx, want, want_idx, fmt, (bucket, k, fmt))


@pytest.mark.parametrize('fmt', C.FORMATS)
@pytest.mark.parametrize('bucket', C.FWD_BUCKETS)
def test_every_phase_of_q_between_guard_bands(bucket, fmt):
    k = 16
    ts, pts = C.random_list(bucket, k, fmt)
    xs, pd = [dev(x) for x, _ in ts], dev(pts)
    ns = [x.numel() for x in xs]
    want, want_idx = forward32(xs, pd, k, bucket)
    dt = C.torch_dtype(fmt)
    for phase in C.PHASES:
        raw, offs = carve(ns, 2, phase, np.array([SENT16], np.uint16))
        buf = dev(raw)
        outs = [buf[o:o + 2 * n].view(dt) for o, n in zip(offs, ns)]
        assert all(o.data_ptr() % 16 == phase for o in outs if o.numel())
        _, got, idx = forward16(xs, pd, k, bucket, fmt, outs=outs)
        check_forward(got, idx, want, want_idx, fmt, (bucket, fmt, 'phase', phase))
        h = buf.cpu().numpy()
        inside = np.zeros(h.size, bool)
        for o, n in zip(offs, ns):
            inside[o:o + 2 * n] = True
        assert np.array_equal(h[~inside], raw[~inside]), (bucket, fmt, phase, 'written outside an output')


@pytest.mark.parametrize('fmt', C.FORMATS)
@pytest.mark.parametrize('bucket', C.FWD_BUCKETS)
def test_later_trips_of_the_forward_loop_under_grid_caps_1_2_3(lib, bucket, fmt):
    k = 16
    ts, pts = C.random_list(bucket, k, fmt)
    xs, pd = [dev(x) for x, _ in ts], dev(pts)
    want, want_idx = forward32(xs, pd, k, bucket)
    outs = empty_like(xs, C.torch_dtype(fmt))
    mt = MultiTensorDiffQuant(xs, outs, empty_like(xs), k, bucket)
    assert mt._tiles >= C.MIN_TILES
    assert_trips('k_multi_nearest_o16', mt._tiles, mt._tiles, 4, 4)          # every wave: >= 3 trips, the last one partial
    runs = {}
    for cap in (None,) + G.CAPS:
        for o in outs:
            o.view(torch.int16).fill_(SENT16)
        for i in mt.indices:
            i.fill_(255)
        with G.Capped(lib, cap):
            mt.forward(pd)
        sync()
        runs[cap] = ([o.cpu().clone() for o in outs], [i.cpu().numpy().copy() for i in mt.indices])
    check_forward(runs[None][0], runs[None][1], want, want_idx, fmt, (bucket, fmt, 'uncapped'))
    for cap in G.CAPS:
        for i in range(len(xs)):
            assert torch.equal(runs[cap][0][i].view(torch.int16), runs[None][0][i].view(torch.int16)), (bucket, fmt, 'cap', cap, i)
            assert runs[cap][1][i].tobytes() == runs[None][1][i].tobytes(), (bucket, fmt, 'cap', cap, 'idx', i)
    assert lib_cap_is_default()


# ================================================================ backward
def prepared(bucket, k, fmt, widening=False):
    """A random list after one fp32 forward: (xs, points, gradient patterns per tensor, the fp32 object) -- the indices of the
    backward tests are what that forward assigned."""
    key = (bucket, k, fmt, widening)
    if key not in _CACHE:
        ts, pts = C.random_list(bucket, k, fmt)
        if widening:
            ts = C.with_widening_patterns(ts, fmt)
        _CACHE[key] = ([dev(x) for x, _ in ts], dev(pts), [g for _, g in ts])
    return _CACHE[key]


def backward32(xs, pd, g32, k, bucket, indices=None):
    """The yardstick: the fp32 launch on fp32 gradients in freshly allocated (16-byte-aligned) buffers."""
    assert all(g.dtype == torch.float32 and g.data_ptr() % 16 == 0 for g in g32)
    mt = MultiTensorDiffQuant(xs, empty_like(xs), g32, k, bucket)
    mt.forward(pd)
    if indices is not None:
        for a, b in zip(mt.indices, indices):
            a.copy_(b)
    out = mt.backward()
    sync()
    assert mt.entry_point == BWD and mt.grad_dtype is None
    return mt, out.cpu().numpy()


def backward16(xs, pd, g16, k, bucket, fmt):
    mt = MultiTensorDiffQuant(xs, empty_like(xs), g16, k, bucket)
    assert mt.grad_dtype == C.torch_dtype(fmt) and mt.out_dtype is None
    mt.forward(pd)
    assert mt.entry_point == FWD
    out = mt.backward()
    sync()
    assert mt.entry_point == BWD16 and out.dtype == torch.float32
    return mt, out.cpu().numpy()


@pytest.mark.parametrize('fmt', C.FORMATS)
@pytest.mark.parametrize('bucket', C.BWD_BUCKETS)
@pytest.mark.parametrize('k', C.BWD_K)
def test_equals_the_fp32_launch_on_widened_gradients(k, bucket, fmt):
    for widening in (False, True):
        xs, pd, pats = prepared(bucket, k, fmt, widening)
        g16 = [dev16(p, fmt) for p in pats]
        g32 = [g.float() for g in g16]                                       # freshly allocated
        for g, p in zip(g32, pats):
            assert np.array_equal(g.cpu().numpy().view(np.uint32), C.widen(p, fmt).view(np.uint32))
        _, want = backward32(xs, pd, g32, k, bucket)
        _, got = backward16(xs, pd, g16, k, bucket, fmt)
        if widening:
            assert np.isnan(want).any() and np.isfinite(want).sum() > k
        else:
            assert np.isfinite(want).all() and np.count_nonzero(want) > k
        assert_same32(got, want, (k, bucket, fmt, 'widening table' if widening else 'random'))


@pytest.mark.parametrize('fmt', C.FORMATS)
@pytest.mark.parametrize('k,bucket', [(4, 256), (16, 100), (64, None), (65, 256), (256, 100)])
def test_every_phase_of_g_between_nan_guard_bands(k, bucket, fmt):
    xs, pd, pats = prepared(bucket, k, fmt)
    ns = [p.size for p in pats]
    _, want = backward32(xs, pd, [dev(C.widen(p, fmt)) for p in pats], k, bucket)
    assert np.isfinite(want).all()
    dt = C.torch_dtype(fmt)
    for phase in C.PHASES:
        raw, offs = carve(ns, 2, phase, np.array([C.NAN16[fmt]], np.uint16))  # a guard read into any sum turns it NaN
        for p, o in zip(pats, offs):
            raw[o:o + 2 * p.size] = p.view(np.uint8)
        buf = dev(raw)
        g16 = [buf[o:o + 2 * n].view(dt) for o, n in zip(offs, ns)]
        assert all(g.data_ptr() % 16 == phase for g in g16 if g.numel())
        _, got = backward16(xs, pd, g16, k, bucket, fmt)
        assert_same32(got, want, (k, bucket, fmt, 'phase', phase))
        assert np.array_equal(buf.cpu().numpy(), raw), 'the gradients were written'


@pytest.mark.parametrize('fmt', C.FORMATS)
def test_a_misaligned_idx_takes_the_strided_walk_as_the_fp32_launch_does(fmt):
    k, bucket = 16, 256
    xs, pd, pats = prepared(bucket, k, fmt)
    g16 = [dev16(p, fmt) for p in pats]
    res = {}
    for name, grads in (('fp32', [g.float() for g in g16]), ('in16', g16)):
        mt = MultiTensorDiffQuant(xs, empty_like(xs), grads, k, bucket)
        mt.forward(pd)
        sync()
        moved = []
        for i in mt.indices:                                                 # every idx one byte off a 4-byte boundary
            b = torch.zeros(i.numel() + 5, dtype=torch.uint8, device=DEV)[1:1 + i.numel()]
            b.copy_(i)
            moved.append(b)
        mt.indices = moved
        mt._plan()
        assert all(i.data_ptr() % 4 == 1 for i in mt.indices if i.numel())
        res[name] = mt.backward().cpu().numpy()
        sync()
    assert_same32(res['in16'], res['fp32'], (fmt, 'misaligned idx'))


def build_exact(mc, fmt):
    """MultiTensorDiffQuant over the case's tensors with 16-bit gradients, its index and alpha columns overwritten in place."""
    xs = [torch.zeros(n, dtype=torch.float32, device=DEV) for n in mc.sizes]
    grads = [dev16(C.to_patterns(g, fmt), fmt) for g in mc.g]
    mt = MultiTensorDiffQuant(xs, empty_like(xs), grads, mc.k, mc.bucket)
    held = mt._held()
    for i, n in enumerate(mc.sizes):
        if n:
            a = mt.scalings[i].alpha
            assert a.numel() == mc.alpha[i].size and mt.indices[i].numel() == n
            a.view(-1).copy_(torch.from_numpy(mc.alpha[i]))
            mt.indices[i].copy_(torch.from_numpy(mc.idx[i].astype(np.uint8)))
    assert mt._held() == held
    return mt


@pytest.mark.parametrize('bucket', E.M_BUCKETS)
@pytest.mark.parametrize('k', E.M_K)
def test_the_exact_sums_hold_with_16_bit_gradients(k, bucket):
    """137 tensors, the empty ones and the 2049-tile tensor that wraps the 2048 waves: every sum has ONE possible value."""
    mc = C.m_case(k, bucket)                                                 # (asserts the order-free condition tensor by tensor)
    want = np.stack(mc.want)
    for fmt in C.FORMATS:
        mt = build_exact(mc, fmt)
        got = mt.backward()
        sync()
        assert mt.entry_point == BWD16
        got = got.cpu().numpy()
        for i in range(len(mc.sizes)):
            assert E.same_bits(got[i], want[i]), (k, bucket, fmt, 'tensor', i, mc.sizes[i]) + E.first_difference(got[i], want[i])


@pytest.mark.parametrize('fmt', C.FORMATS)
def test_tensors_of_a_remainder_only(fmt):
    for k, bucket in ((4, 256), (16, 100), (65, None)):
        ns = [1, 3, 1023, 255, 700, 0, 513]
        rng = np.random.RandomState(k)
        xs = [dev(rng.randn(n).astype(F32)) for n in ns]
        pats = [C.to_patterns(rng.randn(n).astype(F32), fmt) for n in ns]
        pd = dev(np.sort(rng.rand(len(ns), k).astype(F32), axis=1))
        g16 = [torch.zeros(n + 1, dtype=C.torch_dtype(fmt), device=DEV)[1:] for n in ns]      # 2 bytes off 16
        for g, p in zip(g16, pats):
            g.copy_(dev16(p, fmt))
        _, want = backward32(xs, pd, [dev(C.widen(p, fmt)) for p in pats], k, bucket)
        mt, got = backward16(xs, pd, g16, k, bucket, fmt)
        assert mt._blocks == len(ns)                                         # one row each: the extra wave's
        assert_same32(got, want, (k, bucket, fmt))
        assert not got[5].any()                                              # the empty tensor: +0


# ================================================================ the class
def test_fp32_on_both_sides_launches_what_it_always_launched():
    xs, pd, pats = prepared(256, 16, 'bfloat16')
    g32 = [dev(C.widen(p, 'bfloat16')) for p in pats]
    mt = MultiTensorDiffQuant(xs, empty_like(xs), g32, 16, 256)
    assert mt.out_dtype is None and mt.grad_dtype is None and mt.entry_point is None
    mt.forward(pd)
    assert mt.entry_point == FWD
    mt.backward()
    sync()
    assert mt.entry_point == BWD


@pytest.mark.parametrize('fmt', C.FORMATS)
def test_16_bit_on_one_side_only_rebind_and_replan(fmt):
    k, bucket = 16, 256
    dt = C.torch_dtype(fmt)
    xs, pd, pats = prepared(bucket, k, fmt)
    g16 = [dev16(p, fmt) for p in pats]
    want_q, want_idx = forward32(xs, pd, k, bucket)
    _, want_g = backward32(xs, pd, [g.float() for g in g16], k, bucket)
    # 16-bit outputs with fp32 grads, and the reverse
    a = MultiTensorDiffQuant(xs, empty_like(xs, dt), [g.float() for g in g16], k, bucket)
    b = MultiTensorDiffQuant(xs, empty_like(xs), g16, k, bucket)
    assert (a.out_dtype, a.grad_dtype, b.out_dtype, b.grad_dtype) == (dt, None, None, dt)
    a.forward(pd), b.forward(pd)
    assert (a.entry_point, b.entry_point) == (FWD16, FWD)
    ga, gb = a.backward(), b.backward()
    sync()
    assert (a.entry_point, b.entry_point) == (BWD, BWD16)
    check_forward([o.cpu() for o in a.outputs], [i.cpu().numpy() for i in a.indices], want_q, want_idx, fmt, ('outputs only', fmt))
    for o, w in zip(b.outputs, want_q):
        assert torch.equal(o.cpu().view(torch.int32), w.view(torch.int32))
    assert_same32(ga.cpu().numpy(), want_g, ('fp32 grads', fmt))
    assert_same32(gb.cpu().numpy(), want_g, ('16-bit grads', fmt))
    # both sides 16-bit; rebind to new 16-bit buffers, 2 bytes off 16
    c = MultiTensorDiffQuant(xs, empty_like(xs, dt), g16, k, bucket)
    new_out = [torch.zeros(x.numel() + 1, dtype=dt, device=DEV)[1:] for x in xs]
    new_g = [torch.zeros(x.numel() + 1, dtype=dt, device=DEV)[1:] for x in xs]
    for n, g in zip(new_g, g16):
        n.copy_(g)
    c.rebind(outputs=new_out, grads=new_g)
    assert c.outputs[3].data_ptr() == new_out[3].data_ptr() and c.grads[3].data_ptr() % 16 == 2
    c.forward(pd)
    gc = c.backward()
    sync()
    check_forward([o.cpu() for o in new_out], [i.cpu().numpy() for i in c.indices], want_q, want_idx, fmt, ('rebound', fmt))
    assert_same32(gc.cpu().numpy(), want_g, ('rebound', fmt))
    other = torch.float16 if dt == torch.bfloat16 else torch.bfloat16
    for bad in (torch.float32, other):
        with pytest.raises(TypeError):
            c.rebind(outputs=empty_like(xs, bad))
        with pytest.raises(TypeError):
            c.rebind(grads=empty_like(xs, bad))
    with pytest.raises(TypeError):
        a.rebind(grads=g16)                                                  # fp32 at construction stays fp32
    assert c.outputs[3].data_ptr() == new_out[3].data_ptr()                  # a refused rebind changes nothing
    # a swapped p.data triggers the re-plan
    i = max(range(len(xs)), key=lambda j: xs[j].numel())
    fresh = torch.zeros(xs[i].numel() + 4, dtype=dt, device=DEV)[4:]
    c.outputs[i].set_(fresh)
    c.forward(pd)
    sync()
    assert c._ptrs == c._held() and c.outputs[i].data_ptr() == fresh.data_ptr()
    C.assert_same16(fresh.cpu(), want_q[i].to(dt), ('after p.data moved', fmt))


def test_the_type_errors():
    xs, pd, pats = prepared(256, 16, 'float16')
    h = [dev16(p, 'float16') for p in pats]
    b = [g.float().to(torch.bfloat16) for g in h]
    f = [g.float() for g in h]
    for mixed in (h[:3] + b[3:], h[:3] + f[3:], f[:3] + b[3:]):
        with pytest.raises(TypeError):
            MultiTensorDiffQuant(xs, mixed, f, 16, 256)
        with pytest.raises(TypeError):
            MultiTensorDiffQuant(xs, f, mixed, 16, 256)
    for other in (torch.float64, torch.int16):
        with pytest.raises(TypeError):
            MultiTensorDiffQuant(xs, [g.to(other) for g in f], f, 16, 256)
        with pytest.raises(TypeError):
            MultiTensorDiffQuant(xs, f, [g.to(other) for g in f], 16, 256)
    with pytest.raises(TypeError):
        MultiTensorDiffQuant([x.half() for x in xs], h, h, 16, 256)          # the masters stay fp32
    mt = MultiTensorDiffQuant(xs, h, b, 16, 256)                             # the two sides are independent
    assert mt.out_dtype == torch.float16 and mt.grad_dtype == torch.bfloat16
    with pytest.raises(ValueError):
        mt.forward(pd.to(torch.float64)[:, :8].float())                      # points: [ntensors, k] fp32, as ever


@pytest.mark.parametrize('fmt', C.FORMATS)
def test_one_graph_of_forward_and_backward_replays_to_the_eager_bits(fmt):
    k, bucket = 16, 256
    dt = C.torch_dtype(fmt)
    xs, pd, pats = prepared(bucket, k, fmt)
    g16 = [dev16(p, fmt) for p in pats]
    mt = MultiTensorDiffQuant(xs, empty_like(xs, dt), g16, k, bucket)
    gp = torch.empty(mt.n_tensors, k, device=DEV)
    mt.forward(pd)
    mt.backward(out=gp)
    sync()
    eager_q = [o.cpu().clone() for o in mt.outputs]
    eager_g = gp.cpu().numpy().copy()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                            # one stream, one branch
        mt.forward(pd)
        mt.backward(out=gp)
    for o in mt.outputs:
        o.view(torch.int16).fill_(SENT16)
    gp.fill_(float('nan'))
    graph.replay()
    sync()
    for i, (o, w) in enumerate(zip(mt.outputs, eager_q)):
        assert torch.equal(o.cpu().view(torch.int16), w.view(torch.int16)), (fmt, 'replayed output', i)
    assert gp.cpu().numpy().tobytes() == eager_g.tobytes()


# ================================================================ the C ABI
def test_c_abi_refusals_write_nothing(lib):
    k, bucket = 16, 256
    xs, pd, pats = prepared(bucket, k, 'float16')
    g16 = [dev16(p, 'float16') for p in pats]
    mt = MultiTensorDiffQuant(xs, empty_like(xs, torch.float16), g16, k, bucket)
    st = _lib.stream_ptr(torch.device(DEV))
    for o in mt.outputs:
        o.view(torch.int16).fill_(0x5A5A)
    for i in mt.indices:
        i.fill_(0xA5)
    gp = torch.full((mt.n_tensors, k), 7.0, device=DEV)
    mt._scratch.fill_(9.0)
    tab, n, tiles, rows = mt._table.data_ptr(), mt.n_tensors, mt._tiles, mt._blocks
    ws, wsb = mt._scratch.data_ptr(), mt._scratch.numel() * 4
    fwd, bwd = lib.qd_multi_nearest_out16_f32, lib.qd_multi_point_grad_in16_f32
    for kind in (0, 3, -1):                                                  # an unknown kind
        assert fwd(tab, n, tiles, bucket, pd.data_ptr(), k, kind, st) == INVALID
        assert bwd(tab, n, rows, bucket, k, kind, gp.data_ptr(), ws, wsb, st) == INVALID
    short = bwd(tab, n, rows, bucket, k, 1, gp.data_ptr(), ws, rows * k * 4 - 1, st)          # one byte short
    assert short == lib.qd_multi_point_grad_f32(tab, n, rows, bucket, k, gp.data_ptr(), ws, rows * k * 4 - 1, st) and short not in (0, INVALID)
    # an odd 16-bit pointer: the plan is where the host sees the pointers
    import ctypes
    host = (_lib.QdDiffQuantDesc * 1)()
    j = 3
    for field, t in (('u', mt.scaled[j]), ('q', mt.outputs[j]), ('idx', mt.indices[j]), ('alpha', mt.scalings[j].alpha),
                     ('beta', mt.scalings[j].beta), ('grad', mt.grads[j])):
        setattr(host[0], field, t.data_ptr())
    host[0].n = xs[j].numel()
    total = ctypes.c_int64(0)
    assert lib.qd_multi_dq_plan(host, 1, bucket, ctypes.byref(total)) > 0
    for field in ('q', 'grad'):
        keep = getattr(host[0], field)
        setattr(host[0], field, keep + 1)
        assert lib.qd_multi_dq_plan(host, 1, bucket, ctypes.byref(total)) == INVALID, field
        setattr(host[0], field, keep)
    sync()
    assert all(bool((o.view(torch.int16) == 0x5A5A).all()) for o in mt.outputs), 'a refused call wrote its outputs'
    assert all(bool((i == 0xA5).all()) for i in mt.indices) and bool((gp == 7.0).all()) and bool((mt._scratch == 9.0).all())
    assert fwd(tab, n, tiles, bucket, pd.data_ptr(), k, 1, st) == 0 and bwd(tab, n, rows, bucket, k, 1, gp.data_ptr(), ws, wsb, st) == 0
    sync()
    assert not any(bool((o.view(torch.int16) == 0x5A5A).all()) for o in mt.outputs if o.numel()) and not bool((gp == 7.0).all())


# ================================================================ the recipe of INTEGRATION.md
def test_a_bf16_student_learns_its_points_without_fp32_shadows():
    torch.manual_seed(0)
    student = torch.nn.Sequential(torch.nn.Linear(64, 96), torch.nn.ReLU(), torch.nn.Linear(96, 10)).to(DEV)
    masters = [p.detach().clone() for p in student.parameters()]           # fp32, owned by the trainer
    student.to(torch.bfloat16)
    params = list(student.parameters())
    k, bucket = 4, 256
    flat = torch.zeros(sum(p.numel() for p in params), dtype=torch.bfloat16, device=DEV)
    views, at = [], 0
    for p in params:                                                        # one flat gradient buffer whose views are p.grad
        views.append(flat[at:at + p.numel()])
        p.grad = views[-1].view_as(p)
        at += p.numel()
    mt = MultiTensorDiffQuant(masters, [p.data.view(-1) for p in params], views, k, bucket)
    assert mt.out_dtype == torch.bfloat16 and mt.grad_dtype == torch.bfloat16
    points = torch.linspace(0, 1, k, device=DEV).repeat(len(params), 1).contiguous()
    mt.forward(points)                                                      # the student's weights, straight from the masters
    x = torch.randn(32, 64, device=DEV).to(torch.bfloat16)
    student(x).float().pow(2).mean().backward()
    assert all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(params, views)) and bool(flat.float().abs().sum() > 0)
    got = mt.backward()
    sync()
    assert (mt.entry_point, got.shape) == (BWD16, (len(params), k))
    # the same step the way the parent commit offers it: fp32 shadows of the weights and of the gradients, copies around the sweeps
    shadow_q = [torch.empty(p.numel(), device=DEV) for p in params]
    shadow_g = [v.float() for v in views]
    ref = MultiTensorDiffQuant(masters, shadow_q, shadow_g, k, bucket)
    ref.forward(points)
    want = ref.backward()
    sync()
    for p, q in zip(params, shadow_q):
        assert torch.equal(p.data.view(-1).view(torch.int16), q.to(torch.bfloat16).view(torch.int16))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
