"""qdl_kd_loss_f32 (libqd_loss.so): value and logit gradient against the harness formulas in float64 (bound: 4 x fp32 torch on the CPU over the same
cases, profiles/kd_loss_error.txt), the exact zeros, a row's bit-for-bit independence, loud rows, the autograd modules, one trainer step, one graph."""
import itertools

import pytest
import torch

from harness import models
from harness.distill import DistillTrainer, fused_cnn_kd_loss_fn, synthetic_batch
from quantized_distillation_amd import _lib, _loss, kd_loss

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
COLS = (1, 2, 10, 63, 64, 65, 'W', 'W+1', 1001, 'L', 'L+1')               # W, L: the last column count of the wave and of the LDS staging
ROWS, TS = (1, 3, 5), (1.0, 2.0, 4.5)
CASES = list(itertools.product(COLS, ROWS, TS))
BAND, FILL, W8 = 16, -7.25, 0.7
OUTS = ('grad', 'row_kl', 'row_nll', 'loss')


@pytest.fixture(scope='module')
def lib():
    return _loss.load()


def width(lib, cols):
    return cols if isinstance(cols, int) else {'W': lib.qdl_wave_cols(), 'L': lib.qdl_lds_cols()}[cols[0]] + (len(cols) > 1)


def data(lib, cols, rows, seed):
    g = torch.Generator().manual_seed(seed)
    c = width(lib, cols)
    return torch.randn(rows, c, generator=g) * 3.0, torch.randn(rows, c, generator=g) * 3.0, torch.randint(0, c, (rows,), generator=g)


def scales(rows, cols, T):
    return W8 * T * T / (rows * cols), (1.0 - W8) / rows                 # models.kd_loss: kl_scale, nll_scale


def call(lib, z, t, y, T, ks, ns, ignore=-100, cap=0):
    """The raw call on CPU tensors: inputs between bands of NaN, outputs between bands of FILL that must survive."""
    def banded(n, fill, src=None):
        buf = torch.full((n + 2 * BAND,), fill, device=DEV)
        if src is not None:
            buf[BAND:BAND + n] = src.flatten().to(DEV)
        return buf
    rows, cols = z.shape
    zi, ti = banded(rows * cols, float('nan'), z), banded(rows * cols, float('nan'), t)
    yd = y.to(DEV)
    out = {n: banded(k, FILL) for n, k in zip(OUTS, (rows * cols, rows, rows, 1))}
    ptr = lambda b: b.data_ptr() + 4 * BAND                                # noqa: E731
    lib.qdl_set_grid_cap(cap)
    rc = lib.qdl_kd_loss_f32(ptr(zi), ptr(ti), yd.data_ptr(), rows, cols, T, ks, ns, ignore, *[ptr(out[n]) for n in OUTS], _lib.stream_ptr(DEV))
    lib.qdl_set_grid_cap(0)
    torch.cuda.synchronize()
    assert rc == 0 and all(bool((b[:BAND] == FILL).all()) and bool((b[-BAND:] == FILL).all()) for b in out.values())
    res = {n: out[n][BAND:-BAND].cpu() for n in OUTS}
    res['grad'] = res['grad'].view(rows, cols)
    return res


def harness(z, t, y, T):
    """models.kd_loss in the dtype of z: loss, d loss / d z, and per row the KL and NLL it weighs (weight 1 and weight 0 on the row alone)."""
    z = z.clone().requires_grad_(True)
    loss = models.kd_loss(z, t, y, T, W8)
    (grad,) = torch.autograd.grad(loss, z)
    row = lambda i, w: models.kd_loss(z[i:i + 1], t[i:i + 1], y[i:i + 1], T, w).detach()   # noqa: E731
    return {'grad': grad, 'loss': loss.detach().reshape(1), 'row_kl': torch.stack([row(i, 1.0) for i in range(len(z))]) * z.shape[1] / T ** 2,
            'row_nll': torch.stack([row(i, 0.0) for i in range(len(z))])}


def units(got, ref, ks, ns, T):
    """The worst error per output: grad in 2^-24 (|kl_scale| / T + |nll_scale|), the values in 2^-24 (|value| + 1)."""
    return {n: float(((got[n].double() - ref[n]).abs() / (2.0 ** -24 * ((abs(ks) / T + abs(ns)) if n == 'grad' else ref[n].abs() + 1.0))).max()) for n in OUTS}


@pytest.fixture(scope='module')
def refs(lib):
    """Per case the float64 reference and fp32 torch's distance from it; 'worst': fp32 torch's worst over all cases, per output."""
    out = {'worst': dict.fromkeys(OUTS, 0.0)}
    for i, (cols, rows, T) in enumerate(CASES):
        z, t, y = data(lib, cols, rows, i)
        ref = harness(z.double(), t.double(), y, T)
        base = units(harness(z, t, y, T), ref, *scales(rows, z.shape[1], T), T)
        out[cols, rows, T] = (ref, base)
        out['worst'] = {n: max(out['worst'][n], base[n]) for n in OUTS}
    assert all(v > 0 for v in out['worst'].values()), out['worst']
    return out


@pytest.mark.parametrize('cols,rows,T', CASES)
def test_against_float64_within_four_times_fp32_torch(lib, refs, cols, rows, T):
    z, t, y = data(lib, cols, rows, CASES.index((cols, rows, T)))
    ref, base = refs[cols, rows, T]
    ks, ns = scales(rows, z.shape[1], T)
    ours = units(call(lib, z, t, y, T, ks, ns), ref, ks, ns, T)
    print('kd_loss cols %s rows %d T %s:' % (cols, rows, T), ' '.join('%s %.3f (fp32 torch %.3f, bound %.3f)' % (n, ours[n], base[n], 4 * refs['worst'][n]) for n in OUTS))
    assert all(ours[n] <= 4 * refs['worst'][n] for n in OUTS), (ours, refs['worst'])


@pytest.mark.parametrize('cols,T', itertools.product(COLS, TS))
def test_exact_zeros_and_ignored_rows(lib, cols, T):
    z, _, y = data(lib, cols, 3, 7)
    same = call(lib, z, z.clone(), y, T, 0.3, 0.0)                        # teacher == student, no NLL: pt and ps are the same operations
    assert not same['row_kl'].any() and not same['grad'].any()
    z[1], y[1] = float('nan'), -3                                         # an ignored row is not read
    got, alone = call(lib, z, z.flip(1), y, T, 0.3, 0.6, ignore=-3), call(lib, z[2:], z.flip(1)[2:], y[2:], T, 0.3, 0.6, ignore=-3)
    assert not got['grad'][1].any() and got['row_kl'][1] == 0 and got['row_nll'][1] == 0 and bool(torch.isfinite(got['loss']))
    assert torch.equal(got['grad'][2:], alone['grad']) and bool(got['grad'][0].any()) == (z.shape[1] > 1)


@pytest.mark.parametrize('cols,T', itertools.product(COLS, TS))
def test_a_row_depends_on_nothing_but_itself(lib, cols, T):
    z, t, y = data(lib, cols, 5, 11)
    ks, ns = scales(5, z.shape[1], T)
    base, capped = call(lib, z, t, y, T, ks, ns), call(lib, z, t, y, T, ks, ns, cap=1)
    assert all(torch.equal(base[n], capped[n]) for n in OUTS) and all(bool(torch.isfinite(base[n]).all()) for n in OUTS)
    zbad, ybad = z.clone(), y.clone()
    zbad[1, -1], ybad[3] = float('inf'), z.shape[1]                       # a non-finite row and an out-of-range target: loud, and alone
    loud = call(lib, zbad, t, ybad, T, ks, ns, cap=2)
    assert all(bool(torch.isnan(loud[n][r]).all()) for n in ('grad', 'row_nll') for r in (1, 3)) and bool(torch.isnan(loud['row_kl'][1])) and not bool(torch.isfinite(loud['loss']))
    for r in (0, 2, 4):
        alone = call(lib, z[r:r + 1], t[r:r + 1], y[r:r + 1], T, ks, ns)
        assert all(torch.equal(alone[n][0], base[n][r]) and torch.equal(loud[n][r], base[n][r]) for n in OUTS[:3]), (r, cols, T)


def test_the_modules_through_backward(lib, refs):
    bound = {n: 4 * refs['worst'][n] for n in OUTS}
    z, t, y = data(lib, 1001, 5, 21)
    y[1] = y[4] = 1                                                       # two padded positions
    for fused, plain, kw, ks, ns, T in ((kd_loss.fused_kd_loss, models.kd_loss, dict(temperature=4.5), *scales(5, 1001, 4.5), 4.5),
                                        (kd_loss.fused_word_kd_loss, models.word_kd_loss, dict(batch=2), W8 / 2, (1 - W8) / 2, 1.0)):
        for up in (1.0, 0.5):
            zd, z64 = z.to(DEV).requires_grad_(True), z.double().requires_grad_(True)
            loss, ref = fused(zd, t.to(DEV), y.to(DEV), **kw), plain(z64, t.double(), y, **kw)
            (loss * up).backward()
            (ref * up).backward()
            assert loss.dim() == 0 and abs(loss.item() - ref.item()) <= bound['loss'] * 2.0 ** -24 * (abs(ref.item()) + 1)
            assert float((zd.grad.double().cpu() - z64.grad).abs().max()) <= bound['grad'] * 2.0 ** -24 * (ks / T + ns) * up


def test_one_trainer_step_with_the_fused_loss(lib, refs):
    """The step computes the logits of the default step, bit for bit, and hands the float64 formula's gradient of them to the student."""
    seen = {}
    x, y = synthetic_batch(8, DEV, seed=1)
    for name, kw in (('fused', dict(loss_fn=fused_cnn_kd_loss_fn)), ('default', {})):
        def hook(module, inputs, out, name=name):
            seen[name] = out.detach().cpu()
            out.register_hook(lambda g: seen.__setitem__(name + ' grad', g.cpu()))
        torch.manual_seed(0)
        tr = DistillTrainer(models.student(), models.teacher(), DEV, num_bits=4, bucket_size=256, mode='multi', **kw)
        tr.student.register_forward_hook(hook)
        tr.step(x, y)
    with torch.no_grad():
        teacher = tr.teacher(x).cpu()
    assert torch.equal(seen['fused'], seen['default'])
    ref = harness(seen['fused'].double(), teacher.double(), y.cpu(), 2.0)['grad']
    ks, ns = scales(8, seen['fused'].shape[1], 2.0)
    assert float((seen['fused grad'].double() - ref).abs().max()) <= 4 * refs['worst']['grad'] * 2.0 ** -24 * (ks / 2.0 + ns)


@pytest.mark.parametrize('cols', (10, 1001, 'L+1'))
def test_one_graph_replayed_on_other_data(lib, cols):
    sets = [tuple(v.to(DEV) for v in data(lib, cols, 5, 30 + i)) for i in range(3)]
    eager = [kd_loss.kd_loss_rows(z, t, y, 2.0, 0.4, 0.3, 1) for z, t, y in sets]
    bufs = [v.clone() for v in sets[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        outs = kd_loss.kd_loss_rows(*bufs, 2.0, 0.4, 0.3, 1)
    torch.cuda.synchronize()
    for r in (1, 2, 0, 1):
        [b.copy_(v) for b, v in zip(bufs, sets[r])]
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(o, e) for o, e in zip(outs, eager[r])), r
