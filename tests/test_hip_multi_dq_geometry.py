"""MultiTensorDiffQuant (qd_multi_nearest_f32 / qd_multi_point_grad_f32, csrc/qd_multi_dq.hip) on every geometry the per-tensor
functions take: no buckets (bucket_size=None: the element-tiled forward kernel), buckets that are no power of two (alpha looked
up per element in the backward sweep) and up to 256 points per tensor (one wave per block above 64).

The oracles are code this path does not touch: the per-tensor calls nonUniformQuantization_variable.forward / .backward, the
C oracle (oracle/), and a float64 sum of the fp32 products on the device."""
import numpy as np
import pytest
import torch

import abi_contract as A
import errlog
from oracle import oracle_c as oc
from quantized_distillation_amd import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

BIG = 2049 * 1024 + 5            # 2049 full gradient tiles: wave 0 of the 2048 takes a second one (the wrap-around of the row layout)
# Carved misaligns the odd positions: the large tensor sits at an even one, so the vectorised bodies run over the wrap-around;
# 100003 (97 full tiles) and 4097 take the element-wise ones
SIZES = [1, 1024, BIG, 3, 255, 100003, 1023, 4097, 1025, 2500, 4097, 1, 2500, 1024]
BUCKETS = (None, 7, 100, 1000, 1025, 3000, 256)
KS = (1, 2, 4, 5, 64, 65, 128, 200, 256)
# every k with None; every other bucket with one k of each backward instantiation it can reach (k <= 4: registers, 5 ... 64:
# four waves per block, > 64: one wave per block)
SWEEP = [(None, k) for k in KS] + [(7, 4), (7, 64), (7, 256), (100, 2), (100, 5), (100, 65), (1000, 1), (1000, 128),
                                   (1025, 4), (1025, 200), (3000, 5), (3000, 256), (256, 1), (256, 64), (256, 65), (256, 200),
                                   (256, 256)]
assert {b for b, _ in SWEEP} == set(BUCKETS) and {k for b, k in SWEEP if b is None} == set(KS)


class Carved(object):
    """Tensors of the given sizes; every odd one is a view into ONE flat buffer, 4 or 12 bytes past a 16-byte boundary
    (uint8: 4 or 6 bytes, so that some are not 4-byte aligned either)."""

    def __init__(self, sizes, dtype, fill=None):
        isz = torch.empty(0, dtype=dtype).element_size()
        self.flat = torch.zeros(sum(n * isz + 48 for n in sizes), dtype=torch.uint8, device=DEV)
        assert self.flat.data_ptr() % 16 == 0
        self.tensors, off = [], 0
        for i, n in enumerate(sizes):
            if i % 2:
                off = -(-off // 16) * 16 + ((4, 12) if isz == 4 else (4, 6))[(i // 2) % 2]
                t = self.flat[off:off + n * isz].view(dtype)
                off += n * isz
            else:
                t = torch.zeros(n, dtype=dtype, device=DEV)
            if fill is not None:
                t.copy_(fill[i])
            self.tensors.append(t)


@pytest.fixture(scope='module')
def world():
    """The weights and gradients of SIZES (computed once, never changed), and per bucket size the per-tensor objects."""
    gen = torch.Generator().manual_seed(11)
    ws = [torch.randn(n, generator=gen).to(DEV) for n in SIZES]
    grads = Carved(SIZES, torch.float32, [torch.randn(n, generator=gen) for n in SIZES]).tensors
    return {'ws': ws, 'grads': grads, 'fns': {}, 'wnp': [w.cpu().numpy() for w in ws]}


def per_tensor(world, bucket):
    import quantization
    if bucket not in world['fns']:
        world['fns'][bucket] = [quantization.nonUniformQuantization_variable(bucket_size=bucket, pre_process_tensors=True, tensor=w)
                                for w in world['ws']]
    return world['fns'][bucket]


def alpha_per_element(alpha, n, bucket):
    alpha = alpha.reshape(-1)
    if bucket is None or n <= bucket:
        return alpha[0].expand(n)
    return alpha.repeat_interleave(bucket)[:n]


def build(world, bucket, k):
    """The one-launch object over carved outputs and gradients, with the odd tensors' resident u and indices carved too (the
    element-wise fall-back of the forward sweep, the scalar spans of the backward one)."""
    from quantized_distillation_amd.multi_tensor import MultiTensorDiffQuant
    outs = Carved(SIZES, torch.float32).tensors
    mt = MultiTensorDiffQuant(world['ws'], outs, world['grads'], k, bucket)
    mt.scaled = Carved(SIZES, torch.float32, mt.scaled).tensors
    mt.indices = Carved(SIZES, torch.uint8).tensors
    mt._plan()
    assert any(t.data_ptr() % 16 for t in mt.scaled) and any(t.data_ptr() % 4 for t in mt.indices)
    return mt, outs


def check(world, bucket, k, pts, counts, tag):
    """Forward bit-exact against the per-tensor call and the C oracle; backward within the reduction bound of the float64 sum
    of the fp32 products, per point, and bit-identical over 20 launches."""
    mt, outs = build(world, bucket, k)
    mt.forward(pts)
    got = mt.backward()
    assert all(torch.equal(mt.backward(), got) for _ in range(20)), (tag, 'not deterministic')
    pts_np = pts.cpu().numpy()
    for i, (fn, g, n, c) in enumerate(zip(per_tensor(world, bucket), world['grads'], SIZES, counts)):
        q = fn.forward(None, pts[i, :c].contiguous())
        idx = fn.savedForBackward.raw_indices().view(-1)
        assert torch.equal(q.view(-1), outs[i]) and torch.equal(idx, mt.indices[i]), (tag, 'forward vs the per-tensor call', i, n)
        want = oc.nonuniform_quantize(world['wnp'][i], pts_np[i, :c], bucket, 'midpoint')
        assert np.array_equal(outs[i].cpu().numpy(), want['q'].reshape(-1)), (tag, 'forward vs the oracle', i, n)
        assert np.array_equal(mt.indices[i].cpu().numpy(), want['idx'].reshape(-1).astype(np.uint8)), (tag, 'indices vs the oracle', i, n)
        gp = fn.backward(g)[1]
        prod = (g * alpha_per_element(fn.scaling_function.alpha, n, bucket)).double()       # the fp32 products, exactly
        ix = mt.indices[i].long()
        exact = torch.zeros(k, dtype=torch.float64, device=DEV).index_add_(0, ix, prod).cpu().numpy()
        absum = torch.zeros(k, dtype=torch.float64, device=DEV).index_add_(0, ix, prod.abs()).cpu().numpy()
        errlog.check_sum('K6m point gradient, any geometry', got[i].cpu().numpy(), exact, absum, tag + (i, n), n_terms=n)
        errlog.check_sum('K6 point gradient, any geometry', gp.cpu().numpy(), exact[:c], absum[:c], tag + (i, n), n_terms=n)
        assert bool((got[i, c:] == 0).all()), (tag, 'a padded point received a gradient', i)


def sorted_points(k, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.sort(torch.rand(len(SIZES), k, generator=gen), dim=1)[0].to(DEV)


@pytest.mark.parametrize('bucket,k', SWEEP)
def test_forward_and_backward_on_every_geometry(world, bucket, k):
    check(world, bucket, k, sorted_points(k, 1000 + k), [k] * len(SIZES), ('sweep', bucket, k))


@pytest.mark.parametrize('bucket', [None, 100])
@pytest.mark.parametrize('k', [65, 256])
def test_rows_padded_with_inf_from_a_shorter_count(world, bucket, k):
    """The trainer's layout: tensor i has counts[i] <= k points, the rest of its row is +inf and is never assigned."""
    rng = np.random.RandomState(k)
    counts = [int(c) for c in rng.choice([1, 4, 63, 64, 65, k - 1, k], len(SIZES))]
    counts[SIZES.index(BIG)] = k // 2
    pts = sorted_points(k, 2000 + k)
    for i, c in enumerate(counts):
        pts[i, c:] = float('inf')
    check(world, bucket, k, pts, counts, ('padded', bucket, k))


def same_nan_else_close(got, want, absum, tag):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (tag, 'NaN-ness', got, want)
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), (tag, 'infinities', got, want)
    fin = np.isfinite(want)
    assert np.all(np.abs(got[fin] - want[fin]) <= 2e-6 * absum[fin]), (tag, got, want)     # two fp32 sums, each within 1e-6 of exact


@pytest.mark.parametrize('k', [4, 5, 256])
def test_nan_and_inf_without_buckets(k):
    """bucket_size=None: the whole tensor is one bucket, so a NaN makes its alpha / beta NaN and every u with them -- all
    indices k - 1 (255 at k = 256: it fits the byte), q NaN; +inf makes alpha inf.  The point gradients are poisoned exactly
    as the per-tensor call's, and the other tensors of the launch are what they are without those two."""
    import quantization
    from quantized_distillation_amd.multi_tensor import MultiTensorDiffQuant
    sizes = [2500, 4097, 1025, 100003]
    gen = torch.Generator().manual_seed(5)
    ws = [torch.randn(n, generator=gen) for n in sizes]
    ws[0][1300] = float('nan')
    ws[1][7] = float('inf')
    ws = [w.to(DEV) for w in ws]
    grads = [torch.randn(n, generator=gen).to(DEV) for n in sizes]
    outs = [torch.empty(n, device=DEV) for n in sizes]
    pts = torch.sort(torch.rand(len(sizes), k, generator=gen), dim=1)[0].to(DEV)
    mt = MultiTensorDiffQuant(ws, outs, grads, k, None)
    mt.forward(pts)
    got = mt.backward().cpu().numpy()
    assert bool((mt.indices[0] == k - 1).all()) and bool(torch.isnan(outs[0]).all())
    for i, (w, g, n) in enumerate(zip(ws, grads, sizes)):
        fn = quantization.nonUniformQuantization_variable(bucket_size=None, pre_process_tensors=True, tensor=w)
        q = fn.forward(None, pts[i]).view(-1)
        assert torch.equal(fn.savedForBackward.raw_indices().view(-1), mt.indices[i]), i
        assert torch.equal(torch.isnan(q), torch.isnan(outs[i])) and torch.equal(q[~torch.isnan(q)], outs[i][~torch.isnan(q)]), i
        want = oc.nonuniform_quantize(w.cpu().numpy(), pts[i].cpu().numpy(), None, 'midpoint')
        assert np.array_equal(mt.indices[i].cpu().numpy(), want['idx'].reshape(-1).astype(np.uint8)), i
        assert np.array_equal(outs[i].cpu().numpy(), want['q'].reshape(-1), equal_nan=True), i
        gp = fn.backward(g)[1].cpu().numpy()
        prod = (g * fn.scaling_function.alpha.reshape(-1)[0]).double().abs()
        absum = torch.zeros(k, dtype=torch.float64, device=DEV).index_add_(0, mt.indices[i].long(), prod).cpu().numpy()
        same_nan_else_close(got[i], gp, absum, (k, i))
        if i >= 2:
            assert np.isfinite(got[i]).all() and bool(torch.isfinite(outs[i]).all()), i
    assert np.isnan(got[0, k - 1]) and not np.isnan(got[0, :k - 1]).any()          # only the point that holds the elements


# ---------------------------------------------------------------- the memory contract at the C ABI
def run_multi_dq(nt, bucket, k, lib):
    """abi_contract.run_multi_dq for bucket_size=None too (`bucket == 0` at the C ABI): every column of the plan -- u, q, idx,
    grad -- is a carved view between guards, `points` and grad_points sit between guards, the scratch holds exactly
    total_blocks * k floats whose prior contents do not matter, and one byte less is refused with nothing written."""
    from quantized_distillation_amd.multi_tensor import MultiTensorDiffQuant
    sizes = A.MULTI_LISTS[nt]
    cb = bucket or 0
    tag = ('K5m/K6m', nt, bucket, k)
    xs = [A.data(n, cb, 700 + i) for i, n in enumerate(sizes)]
    gs = [np.random.RandomState(800 + i).randn(n).astype(np.float32) for i, n in enumerate(sizes)]
    pts = np.stack([A.points(k, seed=900 + i) for i in range(nt)])
    fq = A.Flat(sizes, A.F32, DEV, 'out')
    fg = A.Flat(sizes, A.F32, DEV, 'in', gs, guard='grad', phases=[(0, 4, 8, 12)[(i + 2) % 4] for i in range(nt)])
    mt = MultiTensorDiffQuant([torch.from_numpy(x).to(DEV) for x in xs], fq.views(), fg.views(), k, bucket)
    sds = [oc.scale_down(x, bucket) for x in xs]
    fu = A.Flat(sizes, A.F32, DEV, 'in', [sd['u'] for sd in sds], phases=[(0, 4, 8, 12)[(i + 3) % 4] for i in range(nt)])
    fi = A.Flat(sizes, A.U8, DEV, 'out', phases=[(0, 4, 8, 12)[i % 4] for i in range(nt)], valid_max=k - 1)
    for got, sd in zip(mt.scaled, sds):
        assert A._same(got.cpu().numpy(), sd['u'].reshape(-1)[:got.numel()]), (tag, 'scale_down differs from the oracle')
    mt.scaled, mt.indices = fu.views(), fi.views()
    mt._plan()
    pp = A.Placed(A.inp(pts.reshape(-1), 4), DEV)
    wants = [oc.nonuniform_quantize(x, p, bucket, 'midpoint') for x, p in zip(xs, pts)]
    mt.forward(pp.buf[pp.off:pp.off + pp.nbytes].view(torch.float32).view(nt, k))
    torch.cuda.synchronize(DEV)
    pp.read(tag, 'points')
    fu.read(tag, 'u')
    for i, (q, ix, w) in enumerate(zip(fq.read(tag, 'q'), fi.read(tag, 'idx'), wants)):
        assert A._same(q, w['q'].reshape(-1)) and A._same(ix, w['idx'].reshape(-1).astype(np.uint8)), (tag, 'forward: tensor %d (%d elements)' % (i, sizes[i]))
    fi.arr = fi.arr._replace(role='in')                       # the backward sweep only reads them
    fi.image = fi.buf.cpu().numpy()
    assert mt._blocks == sum(min(n // 1024, 2048) + 1 for n in sizes)
    nbytes = mt._blocks * k * 4
    results = []
    for fill in A.FILLS:
        ws = A.Placed(A.Arr('out', A.U8, None, nbytes, 0, 'sentinel', None), DEV)
        ws.fill(A._ws_bytes(fill, nbytes, lib, DEV))
        gp = A.Placed(A.out(A.F32, nt * k, 8), DEV)
        gp_view = gp.buf[gp.off:gp.off + gp.nbytes].view(torch.float32).view(nt, k)
        rc = lib.qd_multi_point_grad_f32(mt._table.data_ptr(), nt, mt._blocks, cb, k, gp.ptr, ws.ptr, nbytes - 1, _lib.stream_ptr(DEV))
        torch.cuda.synchronize(DEV)
        assert rc == A.ERR_WS and gp.untouched(gp.read(tag, 'grad_points')), (tag, rc)
        assert ws.untouched(ws.read(tag, 'workspace')), (tag, 'the refused call wrote into the workspace')
        mt._scratch = A._ws_view(ws)
        mt.backward(out=gp_view)
        torch.cuda.synchronize(DEV)
        ws.read(tag, 'workspace')
        fg.read(tag, 'grad')
        fi.read(tag, 'idx')
        got = gp.read(tag, 'grad_points')
        gp.assert_no_sentinel(got, tag, 'grad_points')
        for i, (g, w, sd) in enumerate(zip(gs, wants, sds)):
            want, absum = oc.point_grad(g, w['idx'], sd['alpha'], bucket, k)
            errlog.check_sum('K6m point gradient at the C ABI, any geometry', got[i * k:(i + 1) * k], want, absum, tag + (i,))
        results.append(got)
    for r in results[1:]:
        assert A._same(r, results[0]), (tag, 'differs between workspace fills')


@pytest.mark.parametrize('bucket,k', [(None, 5), (100, 65), (None, 256)])
def test_memory_contract(bucket, k):
    run_multi_dq(7, bucket, k, _lib.load())


# ---------------------------------------------------------------- the trainer
def test_trainer_without_buckets_equals_the_per_tensor_loop():
    """DiffQuantTrainer(mode='multi', bucket_size=None) against mode='per_tensor' from the same state: identical quantized
    weights, each one's point gradients within the reduction bound of the float64 sum of its own fp32 products, and the same
    trajectory over 3 steps (the tolerance of test_multi_tensor_diffquant_equals_per_tensor).

    lr = 3e-4, not that test's 1e-2: without buckets a point moves a quarter of a whole tensor at once and the loop is
    unstable at larger rates.  Measured with two copies of the PER-TENSOR trainer, same seed, same batches (the gradients of
    the convolutions are not bit-reproducible run to run): at 1e-2 they differ by 1.7e-3 in the loss of the third step, at
    1e-3 by 3.2e-3 (points 1.7e-2 apart), so nothing can be held to 1e-4 of either; at 3e-4 and 1e-4 they agree to 3e-10 in
    the points.  At 3e-4 the points travel up to 4.4e-3 in the three steps, 4 x the largest difference allclose lets through
    (atol + rtol |p| = 1.1e-3) -- no rate was found that is stable and travels 10 x that.  So on top of the issue's tolerance
    the two trajectories must agree to 1 % of the distance travelled: point gradients within 1e-6 sum|terms| of exact are,
    at a cancellation of 1e3 in the sum, within 0.1 % of the gradient that moves the points, while a one-launch gradient wrong
    by a factor in the later steps parts them by a good share of that distance."""
    from harness import models
    from harness.diffquant import DiffQuantTrainer
    from harness.distill import synthetic_batch
    torch.manual_seed(0)
    a = DiffQuantTrainer(models.student(), DEV, num_points=4, bucket_size=None, lr=3e-4, mode='per_tensor')
    torch.manual_seed(0)
    b = DiffQuantTrainer(models.student(), DEV, num_points=4, bucket_size=None, lr=3e-4, mode='multi')
    assert torch.equal(a.points, b.points)
    start = a.points.clone()
    x, y = synthetic_batch(16, DEV, seed=5)
    a.quantize(); b.quantize()
    for pa, pb in zip(a.params, b.params):
        assert torch.equal(pa.data, pb.data)
    for row in range(len(a.slots)):
        assert torch.equal(a.fns[row].savedForBackward.raw_indices().view(-1), b.mt.indices[row])
    a.forward_backward(x, y); b.forward_backward(x, y)
    a.point_gradients(); b.point_gradients()
    for row, i in enumerate(a.slots):
        ix = b.mt.indices[row].long()
        for tr, alpha, kind in ((a, a.fns[row].scaling_function.alpha, 'K6'), (b, b.mt.scalings[row].alpha, 'K6m')):
            prod = (tr.params[i].grad.reshape(-1) * alpha.reshape(-1)[0]).double()
            exact = torch.zeros(4, dtype=torch.float64, device=DEV).index_add_(0, ix, prod).cpu().numpy()
            absum = torch.zeros(4, dtype=torch.float64, device=DEV).index_add_(0, ix, prod.abs()).cpu().numpy()
            errlog.check_sum(kind + ' point gradient inside DiffQuantTrainer, no buckets', tr.points_grad[row].cpu().numpy(), exact,
                             absum, i, n_terms=ix.numel())
    for step in range(3):
        xs, ys = synthetic_batch(16, DEV, seed=20 + step)
        la, lb = a.step(xs, ys), b.step(xs, ys)
        assert abs(float(la) - float(lb)) <= 1e-4 * max(1.0, abs(float(la)))
    assert torch.allclose(a.points, b.points, rtol=1e-3, atol=1e-4)      # same trajectory up to fp32 summation order
    moved = float((a.points - start).abs().max())
    apart = float((a.points - b.points).abs().max())
    print('points moved by up to %.3g, the two trajectories are %.3g apart' % (moved, apart))
    assert moved >= 10 * 1e-4                                            # they did move: ten times allclose's atol at the least
    assert apart <= 0.01 * moved


def test_trainer_takes_up_to_256_points_per_tensor():
    """Counts as the automatic assignment hands them out when the gradient norms are skewed: the largest tensor gets 200 of
    them and mode='multi' constructs and steps; at 257 it raises ValueError (the index is a byte)."""
    from harness import models
    from harness.diffquant import DiffQuantTrainer
    from harness.distill import synthetic_batch

    class HandSet(DiffQuantTrainer):
        top = 200

        def _assign_counts(self, batches, counts):
            sizes = [self.params[i].numel() for i in self.slots]
            return [self.top if n == max(sizes) else c for n, c in zip(sizes, counts)]

    torch.manual_seed(0)
    tr = HandSet(models.student(), DEV, num_points=4, lr=1e-2, mode='multi', assign_bits_automatically=True)
    assert tr.k == 200 and max(tr.counts) == 200 and min(tr.counts) == 4
    pad = torch.isinf(tr.points)
    x, y = synthetic_batch(16, DEV, seed=5)
    assert bool(torch.isfinite(tr.step(x, y)))
    assert bool((tr.points_grad[pad] == 0).all()) and torch.equal(torch.isinf(tr.points), pad)
    assert all(bool(torch.isfinite(tr.params[i].data).all()) for i in tr.slots)
    big = tr.counts.index(200)
    assert int(tr.mt.indices[big].max()) > 64                           # the points beyond 64 are in use
    HandSet.top = 257
    with pytest.raises(ValueError, match='256'):
        HandSet(models.student(), DEV, num_points=4, lr=1e-2, mode='multi', assign_bits_automatically=True)
