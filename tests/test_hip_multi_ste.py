"""Multi-tensor K7 on the GPU: MultiTensorSTE.backward() (qd_multi_ste_backward_f32, one launch for a whole model) gives, tensor by
tensor and bit for bit, what ste.ste_bucket_backward (qd_ste_bucket_backward_f32) gives on the same pointers, writes nothing
outside its outputs, agrees with the oracle to K7's own bound, and can sit in a captured step.

Comparisons are on the raw bits (int32 views): torch.equal on floats calls two identical NaNs different."""
import numpy as np
import pytest
import torch

from harness import kernel_bench, models
from oracle import oracle_c as oc
from quantized_distillation_amd import ste
from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer, MultiTensorSTE

import errlog
from test_hip_property import make

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 4                       # 777-filled elements before every tensor and after the last one
BUCKETS = [64, 128, 256, 512, 1024, 100, 7]
LEVELS = [2, 4, 16, 256]


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Carved(object):
    """Tensors of the given sizes carved out of flat buffers, GUARD (+ gap) elements apart: x, g, and two out buffers of the
    same layout (one for the multi-tensor launch, one for the per-tensor calls), everything outside the tensors = 777."""

    def __init__(self, xs, gs, gap):
        self.offsets, off = [], 0
        for x in xs:
            off += GUARD + gap
            self.offsets.append(off)
            off += x.size
        self.total = off + GUARD
        self.sizes = [x.size for x in xs]
        self.x, self.g = self.flat(xs), self.flat(gs)
        self.inside = torch.zeros(self.total, dtype=torch.bool, device=DEV)
        for o, n in zip(self.offsets, self.sizes):
            self.inside[o:o + n] = True

    def flat(self, arrays=None):
        f = torch.full((self.total,), 777.0, device=DEV)
        if arrays is not None:
            for o, a in zip(self.offsets, arrays):
                f[o:o + a.size].copy_(torch.from_numpy(a))
        return f

    def views(self, flat):
        return [flat[o:o + n] for o, n in zip(self.offsets, self.sizes)]

    def untouched_outside(self, flat):
        return bool((flat[~self.inside] == 777.0).all())


def run_both(c, bucket, s, tie_mode, in_place):
    """-> (outs of ONE multi-tensor launch, outs of the per-tensor calls), on the same x and on buffers of the same layout (so
    every pointer has the same alignment in both).  Checks the guards and that x was not written."""
    x_before = c.x.clone()
    xs = c.views(c.x)
    if in_place:
        g_multi, g_loop = c.g.clone(), c.g.clone()
        mt = MultiTensorSTE(xs, c.views(g_multi), s, bucket, tie_mode=tie_mode)
        outs = mt.backward()
        assert all(o.data_ptr() == g.data_ptr() for o, g in zip(outs, c.views(g_multi)))
        want = [ste.ste_bucket_backward(x, g, bucket, s, out=g, tie_mode=tie_mode) for x, g in zip(xs, c.views(g_loop))]
        flat_multi, flat_loop = g_multi, g_loop
    else:
        flat_multi, flat_loop = c.flat(), c.flat()
        g_before = c.g.clone()
        mt = MultiTensorSTE(xs, c.views(c.g), s, bucket, outs=c.views(flat_multi), tie_mode=tie_mode)
        outs = mt.backward()
        want = [ste.ste_bucket_backward(x, g, bucket, s, out=o, tie_mode=tie_mode)
                for x, g, o in zip(xs, c.views(c.g), c.views(flat_loop))]
        assert same_bits(c.g, g_before), 'out of place: the gradients are inputs only'
    assert same_bits(c.x, x_before), 'the weights are inputs only'
    assert c.untouched_outside(flat_multi), 'the multi-tensor launch wrote outside its outputs'
    assert c.untouched_outside(flat_loop)
    return outs, want


def random_list(seed, kind, big=None):
    rng = np.random.RandomState(seed)
    count = 1 + seed % 12                                   # 1 .. 12 tensors
    sizes = [int(rng.randint(1, 301)) if rng.rand() < 0.5 else int(rng.randint(300, 70001)) for _ in range(count)]
    if big is not None:
        sizes[len(sizes) // 2] = big
    xs = [make(n, seed + 13 * i, (kind + i) % 6) for i, n in enumerate(sizes)]
    gs = [np.random.RandomState((seed + 13 * i) ^ 77).randn(n).astype(np.float32) for i, n in enumerate(sizes)]
    return xs, gs


@pytest.mark.parametrize('s', LEVELS)
@pytest.mark.parametrize('bucket', BUCKETS)
def test_bit_identical_to_the_per_tensor_call(bucket, s):
    """Lists of 1-12 tensors of 1 .. 70 000 elements, the six input kinds rotating through each list, with and without a
    3-element gap between the tensors, both tie modes, in place and out of place: EVERY element of EVERY tensor equals the
    per-tensor call's, bit for bit."""
    case = 0
    for tie_mode in ('reference', 'true_arg'):
        for in_place in (True, False):
            for gap in (0, 3):
                seed = 1000 * bucket + 10 * s + case          # list lengths 1 .. 12 all occur over the parametrisation
                xs, gs = random_list(seed, kind=case % 6)
                outs, want = run_both(Carved(xs, gs, gap), bucket, s, tie_mode, in_place)
                assert len(outs) == len(want) == len(xs)
                for i, (o, w) in enumerate(zip(outs, want)):
                    assert same_bits(o, w), (bucket, s, tie_mode, in_place, gap, i, xs[i].size,
                                             int((o.view(torch.int32) != w.view(torch.int32)).sum()))
                case += 1


@pytest.mark.parametrize('bucket', BUCKETS)
def test_bit_identical_with_a_tensor_of_several_million_elements(bucket):
    """One tensor of 5.2 M elements (not a multiple of any bucket size) between small ones: more tiles than the grid has waves,
    so the grid-stride loop crosses tensor boundaries."""
    for k, (tie_mode, in_place, gap) in enumerate((('reference', True, 3), ('true_arg', False, 0))):
        xs, gs = random_list(7 + 12 * bucket + k, kind=k, big=5 * (1 << 20) + 77)
        outs, want = run_both(Carved(xs, gs, gap), bucket, 16, tie_mode, in_place)
        for i, (o, w) in enumerate(zip(outs, want)):
            assert same_bits(o, w), (bucket, tie_mode, in_place, i, xs[i].size)


@pytest.mark.parametrize('bucket,s', [(256, 16), (64, 4), (128, 256), (512, 2), (1024, 16), (100, 16), (7, 4)])
def test_matches_the_oracle(bucket, s):
    """Each tensor of a multi-tensor launch against oracle_c.ste_complicated_backward, to the project's bound for K7 (errlog.TOL =
    1e-6 of the sum of the magnitudes of a bucket's terms) -- on the input kinds 0 .. 3, the ones K7's own oracle test
    (tests/test_hip_property.py::test_ste_backward_matches_oracle) holds that bound on."""
    rng = np.random.RandomState(bucket + s)
    sizes = [int(v) for v in rng.randint(1, 70001, size=7)] + [bucket, 3 * bucket + 1, 5]
    xs = [make(n, 31 * bucket + i, i % 4) for i, n in enumerate(sizes)]
    gs = [np.random.RandomState(i ^ 77).randn(n).astype(np.float32) for i, n in enumerate(sizes)]
    c = Carved(xs, gs, 3)
    outs = MultiTensorSTE(c.views(c.x), c.views(c.g), s, bucket).backward()
    assert c.untouched_outside(c.g)
    for i, (x, g, o) in enumerate(zip(xs, gs, outs)):
        out = o.cpu().numpy()
        ref = oc.ste_complicated_backward(x, g, s, bucket)
        errlog.check_ste('multi-tensor K7 vs float64 oracle', out, x, g, s, bucket, (bucket, s, i, x.size))
        errlog.check_ste('multi-tensor K7 vs oracle_c (fp32 output)', out, x, g, s, bucket, (bucket, s, i, x.size), ref_out=ref)


@pytest.mark.parametrize('tie_mode', ['reference', 'true_arg'])
def test_buckets_that_hold_a_nan_or_an_infinity(tie_mode):
    """The cases of tests/test_hip_host_agreement.py::test_ste_backward_on_buckets_that_hold_a_nan_or_an_infinity inside a
    multi-tensor list (twice: once behind an odd-sized tensor), equal to the per-tensor result."""
    n, bucket = 64 * 256 + 77, 256
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, generator=g)
    gr = torch.randn(n, generator=g)
    for b in range(0, 64, 3):
        pos = sorted(int(v) for v in torch.randint(0, bucket, (2,), generator=g))
        x[b * bucket + pos[0]] = x[b * bucket + pos[1]] = float('nan')
    for b in range(1, 64, 6):
        x[b * bucket + 7] = float('inf') if b % 2 else float('-inf')
    x[64 * bucket + 5] = float('nan')                                            # the short last bucket too
    small = torch.randn(1001, generator=g)
    small[17] = float('nan')
    xs = [make(1000, 1, 0), x.numpy(), small.numpy(), make(301, 2, 0), x.numpy(), make(5, 3, 0)]
    gs = [np.random.RandomState(i).randn(a.size).astype(np.float32) for i, a in enumerate(xs)]
    gs[1] = gs[4] = gr.numpy()
    for in_place in (True, False):
        outs, want = run_both(Carved(xs, gs, 3), bucket, 16, tie_mode, in_place)
        for i, (o, w) in enumerate(zip(outs, want)):
            assert same_bits(o, w), (tie_mode, in_place, i)
        nans = int(torch.isnan(outs[1]).sum())
        assert nans >= 22 + 1 and int(torch.isnan(outs[2]).sum()) >= 1, 'the NaN buckets must show in the result'
        assert int(torch.isnan(outs[0]).sum()) == 0 and int(torch.isnan(outs[3]).sum()) == 0


def _shape_list(name):
    if name in ('student', 'wrn'):
        return [int(np.prod(sh)) for sh in kernel_bench.model_shapes(name)]
    with torch.device('meta'):
        m = models.ResNetK((2, 2, 2, 2), 1.5) if name == 'resnet18_k1.5' else models.Seq2SeqLSTM()
    return [p.numel() for p in m.parameters()]


@pytest.mark.parametrize('name', ['student', 'wrn', 'resnet18_k1.5', 'lstm_seq2seq'])
def test_baseline_shape_lists_in_one_launch(name):
    """The parameter lists of the BASELINE configurations (harness/models.py) as the trainer lays them out: views of one flat
    master and one flat gradient, in place, bucket 256, 16 levels."""
    from harness.flat import FlatLayout
    sizes = _shape_list(name)
    layout = FlatLayout([(n,) for n in sizes])
    gen = torch.Generator(device=DEV).manual_seed(len(sizes))
    flat_x = torch.randn(layout.total, device=DEV, generator=gen) * 0.05
    flat_g = torch.randn(layout.total, device=DEV, generator=gen)
    g_multi, g_loop = flat_g.clone(), flat_g.clone()
    xs = layout.views(flat_x)
    outs = MultiTensorSTE(xs, layout.views(g_multi), 16, 256).backward()
    assert len(outs) == len(sizes)
    for x, g in zip(xs, layout.views(g_loop)):
        ste.ste_bucket_backward(x, g, 256, 16, out=g)
    assert same_bits(g_multi, g_loop)                        # the whole flat buffer: every tensor and the layout's padding
    assert not same_bits(g_multi, flat_g)


def test_argument_errors_on_device_tensors():
    w = [torch.zeros(300, device=DEV), torch.zeros(10, device=DEV)]
    with pytest.raises(ValueError):
        MultiTensorSTE(w, [torch.zeros(300, device=DEV), torch.zeros(11, device=DEV)], 16, 256)
    with pytest.raises(ValueError):
        MultiTensorSTE(w, [torch.zeros(300, device=DEV), torch.zeros(10, device=DEV)], 16, 256,
                       outs=[torch.zeros(300, device=DEV), torch.zeros(9, device=DEV)])
    with pytest.raises(ValueError):
        MultiTensorSTE(w, [torch.zeros(600, device=DEV)[::2], torch.zeros(10, device=DEV)], 16, 256)
    with pytest.raises(TypeError):
        MultiTensorSTE(w, [torch.zeros(300, device=DEV, dtype=torch.float64), torch.zeros(10, device=DEV)], 16, 256)
    with pytest.raises(RuntimeError, match='HIP device'):
        MultiTensorSTE(w, [torch.zeros(300), torch.zeros(10)], 16, 256)


def test_replans_when_a_tensor_has_moved_and_bumps_the_version_counters():
    gen = torch.Generator().manual_seed(3)
    x = [torch.randn(5000, generator=gen).to(DEV), torch.randn(700, generator=gen).to(DEV)]
    g = [torch.randn(5000, generator=gen).to(DEV), torch.randn(700, generator=gen).to(DEV)]
    want = [ste.ste_bucket_backward(a, b, 256, 16) for a, b in zip(x, g)]
    mt = MultiTensorSTE(x, g, 16, 256)
    v0 = [t._version for t in g]
    outs = mt.backward()
    assert all(same_bits(o, w) for o, w in zip(outs, want))
    assert all(t._version > v for t, v in zip(g, v0))
    # the storage of a held gradient is swapped: the table is rebuilt from the tensors the object holds
    fresh = torch.randn(5000, generator=gen).to(DEV)
    want0 = ste.ste_bucket_backward(x[0], fresh, 256, 16)
    g[0].set_(fresh.clone())
    outs = mt.backward()
    assert same_bits(outs[0], want0) and outs[0].data_ptr() == g[0].data_ptr()
    # empty tensors own no tile; a list of only empty tensors launches nothing
    e = torch.zeros(0, device=DEV)
    assert MultiTensorSTE([e, x[1], e], [e, g[1].clone(), e], 16, 256).backward()[1].numel() == 700
    assert MultiTensorSTE([e], [e], 16, 256).backward()[0].numel() == 0


def test_distill_trainer_multi_equals_per_tensor_loop():
    """DistillTrainer(style='complicated'): mode='multi' runs ONE MultiTensorSTE launch in backward_quant(), mode='per_tensor'
    the reference-shaped loop; same masters, same flat gradient in -> the same flat gradient out, bit for bit."""
    from harness.distill import DistillTrainer, synthetic_batch

    def trainer(mode, first_last):
        torch.manual_seed(0)
        return DistillTrainer(models.student(), models.teacher(), torch.device(DEV), num_bits=4, bucket_size=256, mode=mode,
                              quantize_first_and_last_layer=first_last, backprop_quantization_style='complicated')

    for first_last in (True, False):
        a, b = trainer('multi', first_last), trainer('per_tensor', first_last)
        assert isinstance(a.mt_ste, MultiTensorSTE) and not hasattr(b, 'mt_ste')
        x, y = synthetic_batch(16, torch.device(DEV), seed=3)
        a.quantize()
        a.forward_backward(x, y)                          # one real step's gradient
        grad = a.flat_grad.clone()
        b.flat_master.copy_(a.flat_master)
        for t in (a, b):
            t.flat_grad.copy_(grad)
            t._quantized_step = True
            t.backward_quant()
        assert same_bits(a.flat_grad, b.flat_grad), first_last
        assert not same_bits(a.flat_grad, grad)
        if not first_last:                                # the excluded first and last tensors keep their gradient
            n = len(a.params)
            for i in (0, n - 1):
                lo, hi = a.layout.offsets[i], a.layout.end(i)
                assert same_bits(a.flat_grad[lo:hi], grad[lo:hi])


def test_captures_and_replays_in_a_single_stream_graph():
    """quantize (multi-tensor K1) -> bucket-aware STE backward (multi-tensor K7) -> SGD update captured in ONE single-stream
    graph and replayed once on new gradients == the same three calls eagerly."""
    sizes = [int(np.prod(sh)) for sh in kernel_bench.model_shapes('student')]
    gen = torch.Generator(device=DEV).manual_seed(11)
    masters = [torch.randn(n, device=DEV, generator=gen) * 0.1 for n in sizes]
    shadows = [torch.empty_like(m) for m in masters]
    grads = [torch.randn(n, device=DEV, generator=gen) for n in sizes]
    new_grads = [torch.randn(n, device=DEV, generator=gen) for n in sizes]
    start = [m.clone() for m in masters]
    q = MultiTensorQuantizer(masters, 16, 256, outputs=shadows)
    mt = MultiTensorSTE(masters, grads, 16, 256)

    def step():
        q.quantize(check_pointers=False)
        mt.backward(check_pointers=False)
        torch._foreach_add_(masters, grads, alpha=-0.01)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                          # warm-up outside the capture
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for m, s0, g, ng in zip(masters, start, grads, new_grads):
        m.copy_(s0); g.copy_(ng)
    graph.replay()
    torch.cuda.synchronize()
    got_m, got_g, got_q = [m.clone() for m in masters], [g.clone() for g in grads], [s.clone() for s in shadows]
    for m, s0, g, ng in zip(masters, start, grads, new_grads):
        m.copy_(s0); g.copy_(ng)
    step()                                                 # eagerly, on the same buffers
    torch.cuda.synchronize()
    for i in range(len(sizes)):
        assert same_bits(got_q[i], shadows[i]) and same_bits(got_g[i], grads[i]) and same_bits(got_m[i], masters[i]), i
    assert not any(same_bits(g, ng) for g, ng in zip(got_g, new_grads) if g.numel() > 256)
