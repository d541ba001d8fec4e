"""The symbols of a whole model in one launch (qd_multi_uniform_symbols_u8; MultiTensorSymbols) on the cases of
tests/symbol_cases.py.  Every tensor's symbols, alpha and beta are compared bit for bit with the yardstick the header names --
the per-tensor device call qd_uniform_f32(x_i, <scratch>, n_i, bucket_i, s_i, alpha, beta, sym, ...) -- AND with the expectation
tests/test_symbol_cases_host.py proves on the CPU (libqd_host.so held to the reference's operations in numpy and to
uniformQuantization).  The symbols of all tensors are carved from one 0xA5-filled byte buffer, each tensor at its own byte phase,
alpha / beta sit inside sentinel-filled buffers at a 4-byte phase: every byte outside the contract's ranges is looked at.  No
test hands the kernel a buckets or levels array that disagrees with its plan."""
import numpy as np
import pytest
import torch

import bucket_cases as B
import symbol_cases as S
from quantized_distillation_amd import _lib
from quantized_distillation_amd.multi_tensor import MultiTensorSymbols
from test_hip_multi_stochastic import Carved, same_bits

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FILL, SENT, GUARD = 0xA5, 777.0, 64            # the symbol buffer's filling; alpha / beta's; bytes / floats between and around
ENTRY = 'qd_multi_uniform_symbols_u8'
_CACHE = {}


def np_of(t):
    return t.detach().cpu().numpy()


class SymCarved(object):
    """Symbol tensors of the given sizes carved out of one byte buffer filled with FILL, at least GUARD bytes apart, tensor i
    starting phases[i] bytes past a 16-byte boundary."""

    def __init__(self, sizes, phases):
        self.sizes, self.offsets, off = list(sizes), [], 0
        for n, ph in zip(sizes, phases):
            off = -(-(off + GUARD) // 16) * 16 + ph
            self.offsets.append(off)
            off += n
        self.total = off + GUARD
        self.inside = torch.zeros(self.total, dtype=torch.bool, device=DEV)
        for o, n in zip(self.offsets, self.sizes):
            self.inside[o:o + n] = True

    def flat(self):
        f = torch.full((self.total,), FILL, dtype=torch.uint8, device=DEV)
        assert f.data_ptr() % 16 == 0
        return f

    def views(self, flat):
        return [flat[o:o + n] for o, n in zip(self.offsets, self.sizes)]

    def untouched_outside(self, flat):
        return bool((flat[~self.inside] == FILL).all())


class AbCarved(object):
    """alpha and beta: `nb` floats each inside a SENT-filled buffer, 4 bytes past a 16-byte boundary."""

    def __init__(self, nb):
        self.nb = nb
        self.buf = [torch.full((nb + 2 * GUARD + 1,), SENT, device=DEV) for _ in range(2)]
        assert all(b.data_ptr() % 16 == 0 for b in self.buf)

    def views(self):
        return tuple(b[GUARD + 1:GUARD + 1 + self.nb] for b in self.buf)

    def untouched_outside(self):
        return all(bool((b[:GUARD + 1] == SENT).all()) and bool((b[GUARD + 1 + self.nb:] == SENT).all()) for b in self.buf)


def x_list(variant):
    """(Carved, the pristine flat input) of the cases, each tensor at its 4-byte phase: built once, never written."""
    if ('x', variant) not in _CACHE:
        c = Carved([k.n for k in S.CASES], [k.phase for k in S.CASES],
                   [torch.from_numpy(np.array(S.data(i, variant))).to(DEV) for i in range(len(S.CASES))])
        _CACHE['x', variant] = (c, c.flat())
    return _CACHE['x', variant]


def per_tensor(xs, levels, buckets):
    """[(sym, alpha, beta)] of the per-tensor device call the contract names, as numpy arrays."""
    lib, dev = _lib.load(), torch.device(DEV)
    ws = _lib.workspace(dev)
    out = []
    for x, s, b in zip(xs, levels, buckets):
        n = x.numel()
        nb = B.q_rule(n, b)['nb']
        sym = torch.full((n,), FILL, dtype=torch.uint8, device=DEV)
        alpha, beta = torch.full((max(nb, 1),), SENT, device=DEV), torch.full((max(nb, 1),), SENT, device=DEV)
        if n:
            scratch = torch.empty(n, device=DEV)
            _lib.check(lib.qd_uniform_f32(x.data_ptr(), scratch.data_ptr(), n, b, s, alpha.data_ptr(), beta.data_ptr(), sym.data_ptr(),
                                          None, 0, 0.0, 0, 0, ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))
        out.append((sym, alpha[:nb], beta[:nb]))
    torch.cuda.synchronize()
    return [tuple(np_of(t) for t in o) for o in out]


def loop_of(variant, assign):
    if ('loop', variant, assign) not in _CACHE:
        c, pristine = x_list(variant)
        _CACHE['loop', variant, assign] = per_tensor(c.views(pristine), S.LEVELS[assign], S.BUCKETS)
    return _CACHE['loop', variant, assign]


def launch(variant, assign, **kw):
    """One launch on the cases: (object, SymCarved, its flat buffer, AbCarved, the flat input it read)."""
    c, pristine = x_list(variant)
    fx = pristine.clone()
    sc = SymCarved([k.n for k in S.CASES], [S.sym_phase(i, assign) for i in range(len(S.CASES))])
    fs = sc.flat()
    ab = AbCarved(S.plan_rule()[3])
    mt = MultiTensorSymbols(c.views(fx), S.LEVELS[assign], S.BUCKETS, symbols=sc.views(fs), alpha_beta=ab.views(), **kw)
    return mt, sc, fs, ab, fx


def check(mt, variant, assign, what):
    loop = loop_of(variant, assign)
    for i, k in enumerate(S.CASES):
        got = np_of(mt.symbols[i]), np_of(mt.alpha[i]), np_of(mt.beta[i])
        for ref, name in ((loop[i], 'the per-tensor device call'), (S.expected(i, variant, assign), 'the CPU-proven expectation')):
            assert got[0].dtype == np.uint8 and np.array_equal(got[0], ref[0]), '%s: symbols of %s differ from %s' % (what, k.id, name)
            assert B.same(got[1], ref[1]) and B.same(got[2], ref[2]), '%s: alpha / beta of %s differ from %s' % (what, k.id, name)


# ---------------------------------------------------------------- bits and memory
@pytest.mark.parametrize('assign', list(S.LEVELS))
@pytest.mark.parametrize('variant', S.VARIANTS)
def test_one_launch_equals_the_per_tensor_call_and_writes_nothing_else(variant, assign):
    S.check_paths()
    mt, sc, fs, ab, fx = launch(variant, assign)
    assert mt.entry_point is None
    out = mt.encode()
    torch.cuda.synchronize()
    assert mt.entry_point == ENTRY and out is mt.symbols
    ft, fb, tiles, nb = S.plan_rule()
    assert mt._tiles == tiles and mt.buckets_total == nb and mt.bucket_size == tuple(S.BUCKETS) and mt.s == tuple(S.LEVELS[assign])
    assert mt._buckets.dtype == torch.int64 and mt._buckets.tolist() == S.BUCKETS and mt._levels.tolist() == S.LEVELS[assign]
    assert [a.numel() for a in mt.alpha] == [B.q_rule(k.n, k.bucket)['nb'] for k in S.CASES]
    assert [a.data_ptr() for a in mt.alpha if a.numel()] == [ab.views()[0].data_ptr() + 4 * f for f, a in zip(fb, mt.alpha) if a.numel()]   # table order, one flat tensor
    assert all(s.data_ptr() % 16 == S.sym_phase(i, assign) for i, s in enumerate(mt.symbols) if s.numel())
    assert ab.views()[0].data_ptr() % 16 == 4
    assert sc.untouched_outside(fs), 'a symbol was written outside [sym_i, sym_i + n_i)'
    assert ab.untouched_outside(), 'alpha / beta were written outside their buckets'
    assert same_bits(fx, x_list(variant)[1]), 'the inputs are inputs only'
    check(mt, variant, assign, (variant, assign))
    if variant == 'nonfinite':                 # a NaN bucket, an infinite one: symbol 0, the per-tensor call's alpha / beta
        assert bool(torch.isnan(mt.alpha[2][0])) and bool(torch.isinf(mt.alpha[2][1])) and not bool(mt.symbols[2][:512].any())


# ---------------------------------------------------------------- the later trips of the wave-stride loop
@pytest.mark.parametrize('cap', [1, 2])
def test_under_a_capped_grid_waves_take_later_trips_and_cross_tensors(cap):
    lib = _lib.load()
    mt, sc, fs, ab, _ = launch('finite', 'ladder')
    assert mt._tiles > 4 * 2 * 3, 'four waves per block: every wave makes three trips or more'
    prev = lib.qd_set_grid_cap(cap)
    try:
        mt.encode()
        torch.cuda.synchronize()
    finally:
        assert lib.qd_set_grid_cap(prev) == cap
    assert sc.untouched_outside(fs) and ab.untouched_outside()
    check(mt, 'finite', 'ladder', ('cap', cap))


# ---------------------------------------------------------------- other launches
@pytest.mark.parametrize('bucket', [256, 100])
def test_equal_entries_and_the_broadcast_int_equal_the_per_tensor_call(bucket):
    sizes, phases = [4 * 256, 0, 5 * 256 + 7, 100, 1, 9 * 256, 1000], [0, 0, 0, 0, 0, 1, 0]
    levels = [16, 4, 256, 2, 17, 16, 255]
    gen = torch.Generator(device=DEV).manual_seed(12)
    c = Carved(sizes, phases, [torch.randn(n, device=DEV, generator=gen) for n in sizes])
    xs = c.views(c.flat())
    want = per_tensor(xs, levels, [bucket] * len(sizes))
    a = MultiTensorSymbols(xs, levels, [bucket] * len(sizes))
    b = MultiTensorSymbols(xs, levels, bucket)
    a.encode(); b.encode()
    torch.cuda.synchronize()
    assert a.entry_point == b.entry_point == ENTRY and a.bucket_size == b.bucket_size == (bucket,) * len(sizes)
    for i in range(len(sizes)):
        for m in (a, b):
            assert np.array_equal(np_of(m.symbols[i]), want[i][0]), (bucket, i)
            assert B.same(np_of(m.alpha[i]), want[i][1]) and B.same(np_of(m.beta[i]), want[i][2]), (bucket, i)


def test_an_all_empty_list_makes_no_launch():
    xs = [torch.empty(0, device=DEV) for _ in range(3)]
    mt = MultiTensorSymbols(xs, [16, 4, 2], [256, 5, 1])
    out = mt.encode()
    torch.cuda.synchronize()
    assert mt._tiles == 0 and mt.buckets_total == 0 and mt.entry_point is None
    assert [t.numel() for t in out] == [0, 0, 0] and [a.numel() for a in mt.alpha] == [0, 0, 0]


def test_the_table_is_planned_again_after_a_tensor_was_replaced():
    mt, sc, fs, ab, fx = launch('finite', 'ladder')
    mt.encode()
    check(mt, 'finite', 'ladder', 'before')
    fresh = torch.full((S.CASES[2].n + 3,), FILL, dtype=torch.uint8, device=DEV)
    mt.symbols[2].set_(fresh[1:1 + S.CASES[2].n])            # another storage, one byte off: the packed stores become byte stores
    moved = torch.full((S.CASES[8].n + 1,), SENT, device=DEV)
    moved[1:].copy_(mt.inputs[8])
    mt.inputs[8].set_(moved[1:])                             # ... and a register-row tensor 4 bytes off: element by element
    alpha0 = mt.alpha[0].data_ptr()
    out = mt.encode()
    torch.cuda.synchronize()
    assert mt._ptrs == mt._held() and out[2].data_ptr() == fresh.data_ptr() + 1 and mt.alpha[0].data_ptr() == alpha0
    assert int(fresh[0]) == FILL and bool((fresh[1 + S.CASES[2].n:] == FILL).all()) and float(moved[0]) == SENT
    assert sc.untouched_outside(fs) and ab.untouched_outside()
    check(mt, 'finite', 'ladder', 'after the re-plan')


def test_encode_on_a_non_default_stream():
    mt, sc, fs, ab, _ = launch('nonfinite', 'rotated')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mt.encode()
    side.synchronize()
    assert sc.untouched_outside(fs) and ab.untouched_outside()
    check(mt, 'nonfinite', 'rotated', 'side stream')


def test_one_captured_encode_replays_on_the_inputs_of_the_moment():
    """Captured on the finite inputs, replayed after they were overwritten with the non-finite ones: the replay gives the new
    inputs' symbols -- nothing of the launch is frozen but the pointers."""
    mt, sc, fs, ab, fx = launch('finite', 'ladder')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # warm-up outside the capture
        mt.encode(check_pointers=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    check(mt, 'finite', 'ladder', 'eager')
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        mt.encode(check_pointers=False)                      # recorded, not run
    fx.copy_(x_list('nonfinite')[1])
    fs.fill_(FILL)
    for b in ab.buf:
        b.fill_(SENT)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert sc.untouched_outside(fs) and ab.untouched_outside()
    check(mt, 'nonfinite', 'ladder', 'replay')
