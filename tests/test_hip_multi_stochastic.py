"""The one-launch quantizer with options (MultiTensorQuantizer's stochastic_rounding / max_element / seed_on_device over
qd_multi_uniform_opt_f32 and qd_multi_uniform_global_opt_f32) against its yardstick: the per-tensor call
quantization.uniformQuantization with the same options at the same seed -- which tests/stochastic_cases.py and the goldens
pin to the reference.  Everything is compared as int32 bit patterns (NaN payloads count), no tolerance.  Both sides start from
the same value of the process's stochastic call counter, so tensor i of the launch draws what the i-th call of the loop does."""
import numpy as np
import pytest
import torch

import quantization
from quantization import quant_functions as qf
from quantized_distillation_amd import _lib
from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64                      # sentinel floats before every tensor and after the last one
SENT = 777.0
OPTIONS = [(stoch, me) for stoch in (False, True) for me in (False, 0.05)]
OPT_IDS = ['%s-%s' % ('stoch' if st else 'det', 'clamp' if me else 'noclamp') for st, me in OPTIONS]


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Carved(object):
    """Tensors of the given sizes carved out of one flat buffer, at least GUARD floats apart, each starting `phase[i]` floats
    past a 16-byte boundary; everything outside the tensors holds SENT."""

    def __init__(self, sizes, phases, data=None):
        self.sizes, self.offsets, off = list(sizes), [], 0
        for n, ph in zip(sizes, phases):
            off = -(-(off + GUARD) // 4) * 4 + ph
            self.offsets.append(off)
            off += n
        self.total = off + GUARD
        self.inside = torch.zeros(self.total, dtype=torch.bool, device=DEV)
        for o, n in zip(self.offsets, self.sizes):
            self.inside[o:o + n] = True
        self.data = data

    def flat(self, filled=True):
        f = torch.full((self.total,), SENT, device=DEV)
        assert f.data_ptr() % 16 == 0
        if filled:
            for o, x in zip(self.offsets, self.data):
                f[o:o + x.numel()].copy_(x)
        return f

    def views(self, flat):
        return [flat[o:o + n] for o, n in zip(self.offsets, self.sizes)]

    def untouched_outside(self, flat):
        return bool((flat[~self.inside] == SENT).all())


def _values(sizes, seed, special=None):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    xs = [0.1 * torch.randn(n, device=DEV, generator=gen) for n in sizes]       # the 0.05 clamp bites
    if special is not None:
        x = xs[special]                         # 4096 elements: a NaN, a bucket with +inf and a constant bucket (at bucket 256)
        x[100] = float('nan')
        x[300] = float('inf')
        x[512:768] = 0.03
    return xs


# 1 / 255: below one bucket; 256: exactly one; 1024 + 3 * 256: whole tiles plus a part of one; 5 * 256 + 7: a ragged last bucket;
# 0 in the middle: owns no tile but a seed; 1024 one float off 16-byte alignment; 4096 with the non-finite buckets
BUCKETED_SIZES = [1, 255, 256, 1024 + 3 * 256, 5 * 256 + 7, 0, 1024, 4096]
BUCKETED_PHASES = [0, 0, 0, 0, 0, 0, 1, 0]
GLOBAL_SIZES = [1023, 1024, 1025, 5000, 0, 2048]
GLOBAL_PHASES = [0, 0, 0, 0, 0, 1]
_LISTS = {}


def the_list(kind):
    """(Carved, pristine flat input) of the bucketed / no-bucket list: built once, never written."""
    if kind not in _LISTS:
        if kind == 'bucketed':
            c = Carved(BUCKETED_SIZES, BUCKETED_PHASES, _values(BUCKETED_SIZES, 5, special=7))
        else:
            c = Carved(GLOBAL_SIZES, GLOBAL_PHASES, _values(GLOBAL_SIZES, 6))
        _LISTS[kind] = (c, c.flat())
    return _LISTS[kind]


class counter_at(object):
    """Run a block from a given value of the process's stochastic call counter and put the old value back."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.saved = qf._STOCHASTIC_CALLS[0]
        qf._STOCHASTIC_CALLS[0] = self.value

    def __exit__(self, *exc):
        qf._STOCHASTIC_CALLS[0] = self.saved


def loop(xs, s, bucket, stoch, me, passes=1):
    """The per-tensor loop, `passes` times over the list: -> per pass the list of (q, ScalingFunction)."""
    return [[quantization.uniformQuantization(x, s, stochastic_rounding=stoch, max_element=me, bucket_size=bucket) for x in xs]
            for _ in range(passes)]


def run_both(kind, s, bucket, stoch, me, in_place, start=1000):
    """-> (the quantizer after ONE launch, its outputs, the loop's (q, sf) list): same inputs, same pointer alignment, same
    counter state.  Checks the guard bands and, out of place, that the inputs were not written."""
    c, pristine = the_list(kind)
    with counter_at(start):
        want = loop(c.views(pristine), s, bucket, stoch, me)[0]
        calls_loop = qf._STOCHASTIC_CALLS[0]
    fx = pristine.clone()
    fq = fx if in_place else c.flat(filled=False)
    with counter_at(start):
        mt = MultiTensorQuantizer(c.views(fx), s, bucket, outputs=c.views(fq), stochastic_rounding=stoch, max_element=me)
        outs = mt.quantize()
        assert qf._STOCHASTIC_CALLS[0] == calls_loop == start + (len(c.sizes) if stoch else 0)
    torch.cuda.synchronize()
    assert [o.data_ptr() for o in outs] == [v.data_ptr() for v in c.views(fq)]
    assert c.untouched_outside(fq), 'the launch wrote outside its outputs'
    if not in_place:
        assert same_bits(fx, pristine), 'out of place: the inputs are inputs only'
    return mt, outs, want


def check_equal(outs, want, what):
    for i, (o, (q, _sf)) in enumerate(zip(outs, want)):
        assert same_bits(o, q.reshape(-1)), '%s: tensor %d of %d elements differs from the per-tensor call' % (what, i, o.numel())


@pytest.mark.parametrize('in_place', [False, True], ids=['out_of_place', 'in_place'])
@pytest.mark.parametrize('stoch,me', OPTIONS, ids=OPT_IDS)
@pytest.mark.parametrize('bucket,s', [(256, 2), (256, 16), (256, 17), (256, 256), (64, 16), (128, 16), (100, 16), (512, 16)])
def test_bucketed_equals_the_per_tensor_loop(bucket, s, stoch, me, in_place):
    mt, outs, want = run_both('bucketed', s, bucket, stoch, me, in_place)
    check_equal(outs, want, (bucket, s, stoch, me, in_place))
    if stoch:
        assert mt.last_seed == _seed_at(1000)
        # the draws are in use: the deterministic result differs somewhere (2 levels aside, every element has a coin to toss)
        det = loop(the_list('bucketed')[0].views(the_list('bucketed')[1]), s, bucket, False, me)[0]
        assert not same_bits(outs[3], det[3][0])
    if me:
        assert float(torch.nan_to_num(torch.cat([o for o in outs[:7]]), nan=0.0).abs().max()) <= 0.05 * (1 + 2.0 / (s - 1)) + 1e-6


def _seed_at(counter):
    with counter_at(counter):
        return qf.next_stochastic_seed(peek=True)


@pytest.mark.parametrize('in_place', [False, True], ids=['out_of_place', 'in_place'])
@pytest.mark.parametrize('stoch,me', OPTIONS, ids=OPT_IDS)
@pytest.mark.parametrize('s', [16, 256])
def test_no_buckets_equals_the_per_tensor_loop(s, stoch, me, in_place):
    mt, outs, want = run_both('global', s, None, stoch, me, in_place)
    check_equal(outs, want, (None, s, stoch, me, in_place))
    for i, (q, sf) in enumerate(want):
        if q.numel():
            ab = torch.stack([sf.alpha.reshape(-1)[0], sf.beta.reshape(-1)[0]])
            assert same_bits(mt.alpha_beta[i], ab), (i, mt.alpha_beta[i], ab)


def test_successive_launches_follow_the_loops_passes_and_a_given_seed_reproduces():
    c, pristine = the_list('bucketed')
    xs = c.views(pristine)
    n = len(xs)
    with counter_at(50):
        passes = loop(xs, 16, 256, True, False, passes=3)
    with counter_at(50 + n):                               # where the loop's second pass starts
        mt = MultiTensorQuantizer(xs, 16, 256, stochastic_rounding=True)
        second = [o.clone() for o in mt.quantize()]
        seed_second = mt.last_seed
        third = [o.clone() for o in mt.quantize()]
        assert mt.last_seed == (seed_second + n) & 0xFFFFFFFFFFFFFFFF and qf._STOCHASTIC_CALLS[0] == 50 + 3 * n
    check_equal(second, passes[1], 'pass two')
    check_equal(third, passes[2], 'pass three')
    assert not any(same_bits(a, b) for a, b in zip(second, third) if a.numel() >= 255)
    # a seed given by value: reproducible, the counter is left alone
    with counter_at(7):
        again = [o.clone() for o in mt.quantize(seed=seed_second)]
        assert qf._STOCHASTIC_CALLS[0] == 7 and mt.last_seed == seed_second
    check_equal(again, passes[1], 'quantize(seed=)')
    # ... and modulo 2^64: the list position is added with wrap-around
    top = 0xFFFFFFFFFFFFFFFD
    wrapped = [o.clone() for o in mt.quantize(seed=top)]
    for i in (2, 3, 4, 7):                                 # seeds 2^64 - 1, 0, 1 and 4
        q = torch.empty_like(xs[i])
        _lib.check(_lib.load().qd_uniform_f32(xs[i].data_ptr(), q.data_ptr(), xs[i].numel(), 256, 16, None, None, None, None, 0, 0.0,
                                              1, (top + i) & 0xFFFFFFFFFFFFFFFF, None, 0, _lib.stream_ptr(torch.device(DEV))))
        assert same_bits(wrapped[i], q), i
    with pytest.raises(ValueError, match='seed='):
        MultiTensorQuantizer(xs, 16, 256).quantize(seed=3)


def test_the_position_in_the_list_selects_the_seed_not_the_rank_among_non_empty_tensors():
    c, pristine = the_list('bucketed')
    xs = c.views(pristine)
    empty = BUCKETED_SIZES.index(0)
    full = [o.clone() for o in MultiTensorQuantizer(xs, 16, 256, stochastic_rounding=True).quantize(seed=99)]
    fewer = [o.clone() for o in MultiTensorQuantizer(xs[:empty] + xs[empty + 1:], 16, 256, stochastic_rounding=True).quantize(seed=99)]
    for i in range(empty):
        assert same_bits(full[i], fewer[i]), i
    for i in range(empty + 1, len(xs)):                    # the tensors behind the empty one moved up one seed
        assert not same_bits(full[i], fewer[i - 1]), i
    shifted = [o.clone() for o in MultiTensorQuantizer(xs[empty + 1:], 16, 256, stochastic_rounding=True).quantize(seed=99 + empty + 1)]
    for a, b in zip(full[empty + 1:], shifted):
        assert same_bits(a, b)


def _per_tensor_at(xs, s, bucket, me, seed0):
    """qd_uniform_f32 of every tensor with seed0 + i: what the header promises tensor i equals."""
    lib, outs = _lib.load(), []
    ws = torch.empty(lib.qd_workspace_bytes(), dtype=torch.uint8, device=DEV)
    for i, x in enumerate(xs):
        q = torch.empty_like(x)
        if x.numel():
            _lib.check(lib.qd_uniform_f32(x.data_ptr(), q.data_ptr(), x.numel(), bucket or 0, s, None, None, None, None,
                                          0 if me is False else 1, float(me), 1, (seed0 + i) & 0xFFFFFFFFFFFFFFFF,
                                          ws.data_ptr(), ws.numel(), _lib.stream_ptr(torch.device(DEV))))
        outs.append(q)
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize('kind,bucket', [('bucketed', 256), ('global', None)])
def test_device_seed_is_advanced_on_the_stream_and_a_captured_launch_draws_anew_at_every_replay(kind, bucket):
    c, pristine = the_list(kind)
    xs = c.views(pristine)
    n = len(xs)
    k = 0x7FFFFFFFFFFFFFF0                                   # the int64 cell wraps to negative on the way: the same 64 bits
    with counter_at(300):
        mt = MultiTensorQuantizer(xs, 16, bucket, stochastic_rounding=True, max_element=0.05, seed_on_device=True)
        assert qf._STOCHASTIC_CALLS[0] == 300 + n            # construction reseeds from the process counter
        assert mt.seed_cell.dtype == torch.int64 and mt.seed_cell.numel() == 1
        assert int(mt.seed_cell.item()) & 0xFFFFFFFFFFFFFFFF == _seed_at(300)
        assert mt.reseed(k) == k and qf._STOCHASTIC_CALLS[0] == 300 + n
        with pytest.raises(ValueError, match='seed='):
            mt.quantize(seed=5)
        launches = 0
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                        # warm-up outside the capture
            eager = [o.clone() for o in mt.quantize(check_pointers=False)]
        launches += 1
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            mt.quantize(check_pointers=False)                # recorded, not run: nothing on the host is consulted
        assert qf._STOCHASTIC_CALLS[0] == 300 + n
        replays = []
        for _ in range(3):
            graph.replay()
            torch.cuda.synchronize()
            replays.append([o.clone() for o in mt.outputs])
    for r, got in enumerate([eager] + replays):
        want = _per_tensor_at(xs, 16, bucket, 0.05, k + r * n)
        for i, (a, b) in enumerate(zip(got, want)):
            assert same_bits(a, b), 'launch %d, tensor %d' % (r, i)
    assert not any(same_bits(a, b) for a, b in zip(replays[0], replays[1]) if a.numel() >= 255)
    launches += 3
    assert int(mt.seed_cell.item()) & 0xFFFFFFFFFFFFFFFF == (k + launches * n) & 0xFFFFFFFFFFFFFFFF
    assert int(mt.seed_cell.item()) < 0


def test_by_value_seed_is_refused_during_capture():
    c, pristine = the_list('bucketed')
    mt = MultiTensorQuantizer(c.views(pristine), 16, 256, stochastic_rounding=True)
    mt.quantize()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    before = qf._STOCHASTIC_CALLS[0]
    with torch.cuda.graph(graph, stream=side):
        with pytest.raises(RuntimeError, match='during stream capture'):
            mt.quantize(check_pointers=False)
        with pytest.raises(RuntimeError, match='during stream capture'):
            mt.quantize(check_pointers=False, seed=4)
        torch.zeros(4, device=DEV).add_(1)                   # (something to record: an empty capture is no graph)
    assert qf._STOCHASTIC_CALLS[0] == before


def test_defaults_take_the_existing_entry_points():
    """All options off: the object is today's -- same results as the plain launches through the C ABI, and the option entry
    points with stochastic == 0 && clamp == 0 give the same again."""
    lib = _lib.load()
    for kind, bucket in (('bucketed', 256), ('bucketed', 100), ('global', None)):
        c, pristine = the_list(kind)
        xs = c.views(pristine)
        mt = MultiTensorQuantizer(xs, 16, bucket, stochastic_rounding=False, max_element=False, subtract_mean=False,
                                  seed_on_device=False)
        assert mt.seed_cell is None and mt.last_seed is None
        with counter_at(11):
            got = [o.clone() for o in mt.quantize()]
            assert qf._STOCHASTIC_CALLS[0] == 11
        check_equal(got, loop(xs, 16, bucket, False, False)[0], kind)
        for o in mt.outputs:
            o.fill_(SENT)
        st = _lib.stream_ptr(torch.device(DEV))
        if bucket is None:
            ab = mt.alpha_beta.clone()
            mt.alpha_beta.fill_(SENT)
            _lib.check(lib.qd_multi_uniform_global_opt_f32(mt._table.data_ptr(), mt.n_tensors, mt._tiles, 16, 0, 0.0, 0, 123, None,
                                                           mt.alpha_beta.data_ptr(), mt._scratch.data_ptr(), mt._scratch.numel() * 4, st))
            rows = [i for i, n in enumerate(c.sizes) if n]
            assert same_bits(mt.alpha_beta[rows], ab[rows])
        else:
            _lib.check(lib.qd_multi_uniform_opt_f32(mt._table.data_ptr(), mt.n_tensors, mt._tiles, bucket, 16, 0, 0.0, 0, 123, None, st))
        torch.cuda.synchronize()
        check_equal(mt.outputs, [(g, None) for g in got], 'the option entry point with every option off')


def test_distill_trainer_multi_equals_the_per_tensor_loop_with_stochastic_rounding():
    """DistillTrainer(stochastic_rounding=True, max_element=...): after one quantize() the shadows of mode='multi' hold what
    the parameters of mode='per_tensor' hold, from the same counter state.  (Nothing behind the convolutions is compared.)"""
    from harness import models
    from harness.distill import DistillTrainer

    def trainer(mode, me):
        torch.manual_seed(0)
        return DistillTrainer(models.student(), models.teacher(), torch.device(DEV), num_bits=4, bucket_size=256, mode=mode,
                              stochastic_rounding=True, max_element=me)

    for me in (False, 0.05):
        with counter_at(4000):
            a = trainer('multi', me)                         # the device seed is reserved here ...
            assert a.mt.seed_on_device and a.mt.stochastic_rounding and a.mt.max_element is me
            nq = a.mt.n_tensors
            assert qf._STOCHASTIC_CALLS[0] == 4000 + nq
            a.quantize()
            a.quantize()                                     # ... and advanced on the device: the host counter stays
            assert qf._STOCHASTIC_CALLS[0] == 4000 + nq
        with counter_at(4000):
            b = trainer('per_tensor', me)
            b.flat_master.copy_(a.flat_master)
            b.quantize()
            first = [p.data.clone() for p in b.params]
            b.quantize()
            assert qf._STOCHASTIC_CALLS[0] == 4000 + 2 * nq
        torch.cuda.synchronize()
        assert len(a.params) == len(b.params) == nq
        for i, (pa, pb) in enumerate(zip(a.params, b.params)):
            assert same_bits(pa.data.reshape(-1), pb.data.reshape(-1)), (me, i)
        assert not all(same_bits(f.reshape(-1), pb.data.reshape(-1)) for f, pb in zip(first, b.params))
    plain = DistillTrainer(models.student(), models.teacher(), torch.device(DEV), num_bits=4, bucket_size=256)
    assert not plain.mt.stochastic_rounding and plain.mt.max_element is False and plain.mt.seed_cell is None


def test_distill_trainer_captures_a_stochastic_step_that_draws_anew_at_every_replay():
    """DistillTrainer.capture() unchanged with stochastic_rounding=True: the quantize launch inside graph A reads the device seed
    word and the captured add_ advances it, so two replays on the same batch and masters' layout round differently and the
    host counter is never consulted."""
    from harness import models
    from harness.distill import DistillTrainer, synthetic_batch
    torch.manual_seed(0)
    tr = DistillTrainer(models.student(), models.teacher(), torch.device(DEV), num_bits=4, bucket_size=256, mode='multi',
                        stochastic_rounding=True, lr=0.0, weight_decay=0.0)        # lr 0: the masters stay, only the draws move
    x, y = synthetic_batch(16, torch.device(DEV), seed=3)
    tr.step(x, y)
    tr.capture(x, y, warmup=3)
    assert tr._graph_fb is not None
    nq, calls = tr.mt.n_tensors, qf._STOCHASTIC_CALLS[0]
    master0 = tr.flat_master.clone()
    shadows, cells = [], []
    for _ in range(3):
        cells.append(int(tr.mt.seed_cell.item()))
        loss = tr.step(x, y)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss))
        shadows.append(tr.flat_shadow.clone())
    cells.append(int(tr.mt.seed_cell.item()))
    assert torch.equal(tr.flat_master, master0)
    assert [b - a for a, b in zip(cells, cells[1:])] == [nq] * 3
    assert qf._STOCHASTIC_CALLS[0] == calls
    assert not same_bits(shadows[0], shadows[1]) and not same_bits(shadows[1], shadows[2])
    # replay r is the per-tensor call at the seed the cell held when it ran
    qi = [i for i in range(len(tr.params)) if tr.quantized[i]]
    want = _per_tensor_at([tr.masters[i].reshape(-1) for i in qi], tr.s, 256, False, cells[2] & 0xFFFFFFFFFFFFFFFF)
    for i, w in zip(qi, want):
        assert same_bits(tr.params[i].data.reshape(-1), w), i
