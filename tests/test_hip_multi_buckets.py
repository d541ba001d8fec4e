"""A bucket size per tensor in the one-launch quantizer and STE backward (qd_multi_uniform_buckets_f32,
qd_multi_ste_backward_buckets_f32; MultiTensorQuantizer / MultiTensorSTE with a sequence bucket_size) on the cases of
tests/bucket_cases.py.  Every result is compared bit for bit (int32 views, NaN positions equal) with the yardstick the header
names -- the per-tensor device call at (bucket_i, s_i): qd_uniform_f32 with seed0 + i, qd_ste_bucket_backward_f32 -- AND with the
expectation tests/test_bucket_cases_host.py proves on the CPU (libqd_host.so held to the numpy oracle; for the STE backward the
exact sums of order-free inputs).  No test hands the kernels a buckets array that disagrees with the plan."""
import numpy as np
import pytest
import torch

import bucket_cases as B
import quantization
from quantized_distillation_amd import _lib, ste
from quantized_distillation_amd.multi_tensor import (MultiTensorDiffQuant, MultiTensorQuantizer, MultiTensorSTE,
                                                     per_channel_bucket_sizes)
from test_hip_multi_stochastic import Carved, same_bits

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
Q_S = [c.s for c in B.Q_CASES]
Q_BUCKETS = [c.bucket for c in B.Q_CASES]
STE_S = [c.s for c in B.STE_CASES]
STE_BUCKETS = [c.bucket for c in B.STE_CASES]
LAUNCH = {'det': dict(), 'clamp': dict(max_element=B.MAX_ELEMENT), 'stoch': dict(stochastic_rounding=True),
          'stoch_cell': dict(stochastic_rounding=True, seed_on_device=True)}
_CACHE = {}


def np_of(t):
    return t.detach().cpu().numpy()


def q_list(variant):
    """(Carved, the pristine flat input) of the quantizer's cases, each at its phase: built once, never written."""
    if ('q', variant) not in _CACHE:
        c = Carved([k.n for k in B.Q_CASES], [k.phase for k in B.Q_CASES],
                   [torch.from_numpy(np.array(B.q_data(i, variant))).to(DEV) for i in range(len(B.Q_CASES))])
        _CACHE['q', variant] = (c, c.flat())
    return _CACHE['q', variant]


def per_tensor_q(variant, opt):
    """qd_uniform_f32 of libqd_hip.so on every tensor at (bucket_i, s_i) with seed SEED0 + i: once per (variant, options)."""
    opt = 'stoch' if opt == 'stoch_cell' else opt
    if ('loop', variant, opt) not in _CACHE:
        c, pristine = q_list(variant)
        lib, dev = _lib.load(), torch.device(DEV)
        ws = _lib.workspace(dev)
        me = B.OPTIONS[opt].get('max_element', False)
        outs = []
        for i, (x, k) in enumerate(zip(c.views(pristine), B.Q_CASES)):
            q = torch.empty_like(x)
            if k.n:
                _lib.check(lib.qd_uniform_f32(x.data_ptr(), q.data_ptr(), k.n, k.bucket, k.s, None, None, None, None,
                                              0 if me is False else 1, float(me), int(opt == 'stoch'), (B.SEED0 + i) & B.M64,
                                              ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))
            outs.append(q)
        torch.cuda.synchronize()
        _CACHE['loop', variant, opt] = [np_of(q) for q in outs]
    return _CACHE['loop', variant, opt]


def run_quantizer(xs, outputs, opt, **extra):
    mt = MultiTensorQuantizer(xs, Q_S, Q_BUCKETS, outputs=outputs, **LAUNCH[opt], **extra)
    if opt == 'stoch_cell':
        assert mt.reseed(B.SEED0) == B.SEED0
    outs = mt.quantize(seed=B.SEED0) if opt == 'stoch' else mt.quantize()
    torch.cuda.synchronize()
    return mt, outs


def check_q(outs, variant, opt, what):
    loop = per_tensor_q(variant, opt)
    host_opt = 'stoch' if opt == 'stoch_cell' else opt
    for i, (o, k) in enumerate(zip(outs, B.Q_CASES)):
        got = np_of(o)
        assert B.same(got, loop[i]), '%s: case %s differs from the per-tensor device call' % (what, k.id)
        assert B.same(got, B.expected_q(i, variant, host_opt)), '%s: case %s differs from the CPU-proven expectation' % (what, k.id)


# ---------------------------------------------------------------- the quantizer
@pytest.mark.parametrize('opt', list(LAUNCH))
@pytest.mark.parametrize('variant', ['finite', 'nonfinite'])
def test_quantizer_equals_the_per_tensor_call_at_each_bucket_size(variant, opt):
    B.check_paths()
    c, pristine = q_list(variant)
    fx, fq = pristine.clone(), c.flat(filled=False)
    mt, outs = run_quantizer(c.views(fx), c.views(fq), opt)
    assert mt.entry_point == 'qd_multi_uniform_buckets_f32' and mt.bucket_size == tuple(Q_BUCKETS) and mt.s == tuple(Q_S)
    assert mt._buckets.dtype == torch.int64 and mt._buckets.tolist() == Q_BUCKETS and mt._levels.tolist() == Q_S
    assert mt._tiles == sum(B.q_rule(k.n, k.bucket)['tiles'] for k in B.Q_CASES)
    assert c.untouched_outside(fq), 'the launch wrote outside its outputs'
    assert same_bits(fx, pristine), 'out of place: the inputs are inputs only'
    check_q(outs, variant, opt, (variant, opt))
    if opt in ('stoch', 'stoch_cell'):                      # the draws are in use
        assert not B.same(np_of(outs[8]), per_tensor_q(variant, 'det')[8])
    if opt == 'stoch_cell':
        assert int(mt.seed_cell.item()) & B.M64 == (B.SEED0 + len(B.Q_CASES)) & B.M64
    # in place (the outputs are the inputs): the same bits
    mt, outs = run_quantizer(c.views(fx), c.views(fx), opt)
    assert c.untouched_outside(fx)
    check_q(outs, variant, opt, (variant, opt, 'in place'))


@pytest.mark.parametrize('opt', ['det', 'stoch'])
def test_a_list_of_equal_entries_equals_the_scalar_launch_bit_for_bit(opt):
    sizes, phases = [4 * 256, 0, 5 * 256 + 7, 100, 1, 9 * 256], [0, 0, 0, 0, 0, 1]
    gen = torch.Generator(device=DEV).manual_seed(12)
    c = Carved(sizes, phases, [torch.randn(n, device=DEV, generator=gen) for n in sizes])
    x = c.flat()
    k = len(sizes)
    fa, fb = c.flat(filled=False), c.flat(filled=False)
    a = MultiTensorQuantizer(c.views(x), [16, 4, 256, 2, 17, 16], 256, outputs=c.views(fa), **LAUNCH[opt])
    b = MultiTensorQuantizer(c.views(x), [16, 4, 256, 2, 17, 16], [256] * k, outputs=c.views(fb), **LAUNCH[opt])
    seed = {'seed': 99} if opt == 'stoch' else {}
    a.quantize(**seed); b.quantize(**seed)
    torch.cuda.synchronize()
    assert a.entry_point == 'qd_multi_uniform_levels_f32' and b.entry_point == 'qd_multi_uniform_buckets_f32'
    assert a.bucket_size == 256 and b.bucket_size == (256,) * k and a._buckets is None
    assert a._tiles == b._tiles and c.untouched_outside(fa) and c.untouched_outside(fb)
    assert same_bits(fa, fb)


def test_the_table_is_planned_again_after_an_output_tensor_was_replaced():
    c, pristine = q_list('finite')
    xs = [v.clone() for v in c.views(pristine)]
    mt = MultiTensorQuantizer(xs, Q_S, Q_BUCKETS, stochastic_rounding=True)
    check_q(mt.quantize(seed=B.SEED0), 'finite', 'stoch', 'before')
    table_ptr, buckets = mt._table.data_ptr(), mt._buckets
    fresh = torch.full((xs[2].numel() + 1,), 777.0, device=DEV)
    mt.outputs[2].set_(fresh[1:])                           # another storage, 4 bytes off: the register rows become scalar rows
    mt.outputs[9].set_(torch.empty(xs[9].numel(), device=DEV))
    outs = mt.quantize(seed=B.SEED0)
    torch.cuda.synchronize()
    assert mt._ptrs == mt._held() and outs[2].data_ptr() == fresh.data_ptr() + 4 and table_ptr != 0
    assert mt._buckets is not buckets and mt._buckets.tolist() == Q_BUCKETS, 'the bucket array is rebuilt with the table'
    assert float(fresh[0]) == 777.0
    check_q(outs, 'finite', 'stoch', 'after the re-plan')


# ---------------------------------------------------------------- the STE backward
def ste_list():
    """The exact cases carved into x and g buffers, each at its phase."""
    if 'ste' not in _CACHE:
        n = len(B.STE_CASES)
        c = Carved([k.n for k in B.STE_CASES], [k.phase for k in B.STE_CASES],
                   [torch.from_numpy(np.array(B.ste_data(i)[0])).to(DEV) for i in range(n)])
        x = c.flat()
        c.data = [torch.from_numpy(np.array(B.ste_data(i)[1])).to(DEV) for i in range(n)]
        _CACHE['ste'] = (c, x, c.flat())
    return _CACHE['ste']


def check_ste(outs, xs, gs, tie_mode, what):
    for i, (o, x, g, k) in enumerate(zip(outs, xs, gs, B.STE_CASES)):
        if k.n:
            want = ste.ste_bucket_backward(x, g, k.bucket, k.s, tie_mode=tie_mode)
            assert B.same(np_of(o), np_of(want)), '%s: case %s differs from the per-tensor device call' % (what, k.id)
        assert B.same(np_of(o), B.expected_ste(i, tie_mode)), '%s: case %s differs from the exact sums' % (what, k.id)


@pytest.mark.parametrize('tie_mode', ['reference', 'true_arg'])
def test_ste_equals_the_per_tensor_call_and_the_exact_sums(tie_mode):
    c, x, g = ste_list()
    x0, g0 = x.clone(), g.clone()
    out = c.flat(filled=False)
    mt = MultiTensorSTE(c.views(x), c.views(g), STE_S, STE_BUCKETS, outs=c.views(out), tie_mode=tie_mode)
    outs = mt.backward()
    torch.cuda.synchronize()
    assert mt.entry_point == 'qd_multi_ste_backward_buckets_f32' and mt.bucket_size == tuple(STE_BUCKETS)
    assert mt._buckets.tolist() == STE_BUCKETS and mt._levels.tolist() == STE_S
    assert mt._tiles == sum(B.ste_rule(k.n, k.bucket)['tiles'] for k in B.STE_CASES)
    assert c.untouched_outside(out) and same_bits(x, x0) and same_bits(g, g0)
    check_ste(outs, c.views(x), c.views(g), tie_mode, (tie_mode, 'out of place'))
    gi = g.clone()                                          # in place on the gradient
    outs = MultiTensorSTE(c.views(x), c.views(gi), STE_S, STE_BUCKETS, tie_mode=tie_mode).backward()
    torch.cuda.synchronize()
    assert c.untouched_outside(gi) and outs[0].data_ptr() == c.views(gi)[0].data_ptr()
    check_ste(outs, c.views(x), c.views(g), tie_mode, (tie_mode, 'in place'))


@pytest.mark.parametrize('tie_mode', ['reference', 'true_arg'])
def test_ste_on_random_data_at_mixed_level_counts_equals_the_per_tensor_call(tie_mode):
    """Normal values (one NaN, one +inf), the level counts 2, 4, 16, 17, 256 per tensor: every bucket summed by the body and in
    the order the per-tensor call uses, so the bits agree although the sums depend on their order."""
    c, _, _ = ste_list()
    gen = torch.Generator(device=DEV).manual_seed(77)
    x = torch.randn(c.total, device=DEV, generator=gen)
    g = torch.randn(c.total, device=DEV, generator=gen)
    xs, gs = c.views(x), c.views(g)
    xs[0][70] = float('nan')
    xs[4][300] = float('inf')
    s_list = [B.LEVELS[i % 5] for i in range(len(xs))]
    out = c.flat(filled=False)
    outs = MultiTensorSTE(xs, gs, s_list, STE_BUCKETS, outs=c.views(out), tie_mode=tie_mode).backward()
    torch.cuda.synchronize()
    assert c.untouched_outside(out)
    for i, (o, xi, gi, k) in enumerate(zip(outs, xs, gs, B.STE_CASES)):
        if k.n:
            want = ste.ste_bucket_backward(xi, gi, k.bucket, s_list[i], tie_mode=tie_mode)
            assert B.same(np_of(o), np_of(want)), (tie_mode, k.id, s_list[i])
    assert bool(torch.isnan(outs[0]).any()) and bool(torch.isnan(outs[4]).any())


# ---------------------------------------------------------------- the later trips of the grid-stride loops
@pytest.mark.parametrize('cap', [1, 2])
def test_both_classes_under_a_capped_grid(cap):
    lib = _lib.load()
    c, pristine = q_list('finite')
    sc, sx, sg = ste_list()
    fq, so = c.flat(filled=False), sc.flat(filled=False)
    mt = MultiTensorQuantizer(c.views(pristine), Q_S, Q_BUCKETS, outputs=c.views(fq), stochastic_rounding=True, max_element=False)
    st = MultiTensorSTE(sc.views(sx), sc.views(sg), STE_S, STE_BUCKETS, outs=sc.views(so))
    assert mt._tiles > 4 * 2 * 3 and st._tiles > 4 * 2 * 2, 'four waves per block: every wave makes three trips or more'
    prev = lib.qd_set_grid_cap(cap)
    try:
        outs = mt.quantize(seed=B.SEED0)
        gouts = st.backward()
        torch.cuda.synchronize()
    finally:
        assert lib.qd_set_grid_cap(prev) == cap
    assert c.untouched_outside(fq) and sc.untouched_outside(so)
    check_q(outs, 'finite', 'stoch', ('cap', cap))
    check_ste(gouts, sc.views(sx), sc.views(sg), 'reference', ('cap', cap))


# ---------------------------------------------------------------- capture
def test_one_captured_step_of_quantize_and_ste_replays_as_two_eager_steps():
    c, pristine = q_list('finite')
    sc, sx, sg = ste_list()
    n = len(B.Q_CASES)
    k = 0x7FFFFFFFFFFFFFF0                                   # the int64 cell wraps to negative on the way
    g = sg.clone()
    mt = MultiTensorQuantizer(c.views(pristine), Q_S, Q_BUCKETS, stochastic_rounding=True, seed_on_device=True)
    st = MultiTensorSTE(sc.views(sx), sc.views(g), STE_S, STE_BUCKETS)          # in place: step two runs on step one's gradient

    def step():
        mt.quantize(check_pointers=False)
        st.backward(check_pointers=False)

    def snapshot():
        torch.cuda.synchronize()
        return [o.clone() for o in mt.outputs], g.clone()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # warm-up outside the capture
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g.copy_(sg)
    mt.reseed(k)
    eager = []
    for _ in range(2):
        step()
        eager.append(snapshot())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()                                               # recorded, not run
    assert mt.entry_point == 'qd_multi_uniform_buckets_f32' and st.entry_point == 'qd_multi_ste_backward_buckets_f32'
    g.copy_(sg)
    mt.reseed(k)
    torch.cuda.synchronize()
    for r in range(2):
        graph.replay()
        qs, grad = snapshot()
        assert all(same_bits(a, b) for a, b in zip(qs, eager[r][0])), 'replay %d: the quantizer' % r
        assert same_bits(grad, eager[r][1]), 'replay %d: the STE backward' % r
    assert not same_bits(eager[0][0][8], eager[1][0][8]) and not same_bits(eager[0][1], eager[1][1])
    assert int(mt.seed_cell.item()) & B.M64 == (k + 2 * n) & B.M64
    lib, dev = _lib.load(), torch.device(DEV)               # the first step against the header's per-tensor call
    x8 = c.views(pristine)[8]
    q = torch.empty_like(x8)
    _lib.check(lib.qd_uniform_f32(x8.data_ptr(), q.data_ptr(), x8.numel(), Q_BUCKETS[8], Q_S[8], None, None, None, None, 0, 0.0, 1,
                                  (k + 8) & B.M64, None, 0, _lib.stream_ptr(dev)))
    torch.cuda.synchronize()
    assert same_bits(eager[0][0][8], q)


# ---------------------------------------------------------------- the trainer
@pytest.mark.parametrize('style', ['none', 'complicated'])
def test_trainer_per_channel_multi_equals_per_tensor(style):
    from harness import models
    from harness.distill import DistillTrainer, synthetic_batch
    dev = torch.device(DEV)
    torch.backends.cudnn.deterministic = True

    def trainer(mode):
        torch.manual_seed(0)
        return DistillTrainer(models.student(), models.teacher(), dev, num_bits=4, bucket_size='per_channel', mode=mode,
                              backprop_quantization_style=style)
    a, b = trainer('multi'), trainer('per_tensor')
    want = per_channel_bucket_sizes(a.params)
    assert a.bucket_of == b.bucket_of == want and a.mt.bucket_size == tuple(want) and len(set(want)) > 2
    for step in range(3):
        x, y = synthetic_batch(16, dev, seed=step)
        a.step(x, y); b.step(x, y)
    assert a.mt.entry_point == 'qd_multi_uniform_buckets_f32'
    if style == 'complicated':
        assert a.mt_ste.entry_point == 'qd_multi_ste_backward_buckets_f32'
    assert same_bits(a.flat_master, b.flat_master), 'the two modes end on the same bits'
    assert not torch.equal(a.flat_master, torch.zeros_like(a.flat_master))
    a.quantize()                                            # the parameters the next forward runs on: one scale pair per channel
    torch.cuda.synchronize()
    for i, (p, m) in enumerate(zip(a.params, a.masters)):
        assert same_bits(p.data, quantization.uniformQuantization(m, 16, bucket_size=want[i])[0]), (style, i)
    b.restore()


# ---------------------------------------------------------------- what is deliberately not built
def test_the_combinations_that_are_not_built_say_so_on_device_tensors():
    xs = [torch.zeros(300, device=DEV), torch.zeros(5, device=DEV)]
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(NotImplementedError, match='fp16 / bf16 outputs'):
            MultiTensorQuantizer(xs, 16, [256, 5], out_dtype=dt)
        with pytest.raises(NotImplementedError, match='fp16 / bf16 outputs'):
            MultiTensorQuantizer(xs, 16, [256, 5], outputs=[t.to(dt) for t in xs])
        with pytest.raises(NotImplementedError, match='fp16 / bf16 grads'):
            MultiTensorSTE(xs, [t.to(dt) for t in xs], 16, [256, 5])
    with pytest.raises(NotImplementedError, match='MultiTensorDiffQuant'):
        MultiTensorDiffQuant(xs, [torch.empty_like(t) for t in xs], [torch.empty_like(t) for t in xs], 4, [256, 5])
