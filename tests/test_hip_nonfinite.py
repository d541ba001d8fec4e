"""NaN and +-inf on every path beyond uniformQuantization: nearest-point forward (K4 / K5), point gradient (K6), scale_down ->
inv_scale_down (K2 / K3), the clamp / truncated-STE epilogues (K8), the multi-tensor launches, the packed codec and the
Huffman-coded checkpoints.

The expected values are the reference's own results on CPU tensors (tests/golden/nonfinite_paths.npz, produced by
tests/golden/gen_golden.py at 1 and at 8 torch threads: only what agreed is stored) and the oracle, which
tests/test_oracle_golden.py pins to the same file.  Everything is compared bit for bit, a NaN matching a NaN at the same
position and an infinity an infinity of the same sign; the finite bins of a point gradient go through errlog.check_sum.

The tests that need no device-only entry point take the device from `DEV`: tests/test_nonfinite_host.py runs them again on
CPU tensors (libqd_host.so)."""
import numpy as np
import pytest
import torch

import quantization
from nonfinite_cases import G, PATTERNS, nonfinite_model, plant, same
from oracle import oracle_c as oc
from oracle import oracle_np as onp
from quantized_distillation_amd import _lib, ste

import errlog

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SIZES = (1, 255, 256, 257, 1023, 1024, 1025, 3000)          # what the neighbour-isolation lists are drawn from


@pytest.fixture(scope='module', autouse=True)
def _built():
    if DEV != 'cpu':
        assert torch.cuda.is_available(), 'these tests need the MI355X'
        _lib.load()
    _lib.host()
    oc.build()


def forms(a):
    """The tensor forms every case runs in: freshly allocated, and a view that starts 4 bytes into an allocation."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.full((t.numel() + 5,), 777.0, dtype=t.dtype)
    buf[1:1 + t.numel()] = t
    buf = buf.to(DEV)
    yield 'own', t.clone().to(DEV)
    yield 'offset', buf[1:1 + t.numel()]


def check_point_grad(got, golden, g, idx, alpha, bucket, k, tag):
    """Non-finite bins by position and sign against the golden; the finite ones against the float64 sums."""
    got = got.detach().cpu().numpy()
    want, absum = onp.point_grad(g, idx, alpha, bucket, k)
    fin = np.isfinite(golden)
    assert np.array_equal(np.isnan(got), np.isnan(golden)), (tag, got, golden)
    assert np.array_equal(got[np.isinf(golden)], golden[np.isinf(golden)]) and np.array_equal(np.isinf(got), np.isinf(golden)), (tag, got, golden)
    assert np.array_equal(np.isfinite(want), fin), (tag, 'the oracle poisons other points than the reference', want, golden)
    errlog.check_sum('K6 point gradient, non-finite inputs', got[fin], want[fin], absum[fin], tag, n_terms=g.size)
    errlog.check_sum('K6 point gradient, non-finite inputs (reference fp32 sum)', golden[fin], want[fin], absum[fin], tag, n_terms=g.size)


@pytest.mark.parametrize('bucket', [256, 100, None])
@pytest.mark.parametrize('k', [2, 4, 16])
def test_nearest_point_and_point_gradient_goldens(k, bucket):
    """K4 (nonUniformQuantization), K5 (the pre-processed variable form) and K6 (its backward) on the seven non-finite inputs.
    Every element of a bucket whose alpha or beta is NaN has index k - 1: a NaN orders after every point (np.searchsorted in
    the reference, quant_functions.py:267-268 and :572).  The reference's pre-processed path gave the plain path's indices
    and values on every one of these cases, and its plain backward the pre-processed one's sums (checked by the generator)."""
    z = G()
    g = z.g
    seen = 0
    for i, m in enumerate(z.meta['cases']):
        if m['k'] != k or m['bucket'] != bucket:
            continue
        seen += 1
        c = z.nearest(i)
        x, pts, want_q, want_idx, alpha = c['x'], c['pts'], c['q'], c['idx'], c['alpha']
        assert (~np.isfinite(want_q)).any() and np.all(want_idx[np.isnan(x)] == k - 1)
        pd = torch.from_numpy(pts).to(DEV)
        for form, xd in forms(x):
            tag = (i, m, form)
            q, idx, sf = quantization.nonUniformQuantization(xd, pd, bucket_size=bucket)
            assert same(idx, want_idx), (tag, np.flatnonzero(idx.cpu().numpy() != want_idx)[:8])
            assert same(q, want_q) and same(sf.alpha, alpha) and same(sf.beta, c['beta']), tag
            assert same(xd, x), (tag, 'the input was modified')
            q8, idx8, _ = quantization.nonUniformQuantization(xd, pd, bucket_size=bucket, index_dtype=torch.uint8)
            assert same(idx8.long(), want_idx) and same(q8, want_q), tag
            fn = quantization.nonUniformQuantization_variable(bucket_size=bucket, pre_process_tensors=True, tensor=xd)
            assert same(fn.forward(None, pd), want_q), tag
            assert same(fn.savedForBackward['indices'], want_idx), tag
            for gform, gd in forms(g):
                _, gp = fn.backward(gd)
                check_point_grad(gp, c['gp'], g, want_idx, alpha, bucket, k, tag + (gform,))
            fnp = quantization.nonUniformQuantization_variable(bucket_size=bucket)
            assert same(fnp.forward(xd, pd), want_q), tag
            _, gp = fnp.backward(torch.from_numpy(g).to(DEV))
            check_point_grad(gp, c['gp'], g, want_idx, alpha, bucket, k, tag + ('plain',))
            # in place: the result IS the input tensor, which now holds the quantized values
            qi, idxi, _ = quantization.nonUniformQuantization(xd, pd, bucket_size=bucket, modify_in_place=True)
            assert same(qi, want_q) and same(idxi, want_idx), tag
            assert qi.data_ptr() == xd.data_ptr() and same(xd, want_q), (tag, 'modify_in_place did not write the input')
    assert seen == len(PATTERNS)


def test_point_gradient_of_a_finite_tensor_under_a_nonfinite_gradient():
    """K6 poisons exactly the points whose index set holds the non-finite gradient element: one NaN, one +inf (the bin is
    +inf), a +inf and a -inf on the same point (inf - inf: NaN)."""
    z = G()
    pts = z.pts(4)
    kinds = set()
    for i in range(len(z.meta['grads'])):
        c = z.grad(i)
        gg, idx, alpha, golden = c['g'], c['idx'], c['alpha'], c['gp']
        hit = sorted(set(int(idx[pos]) for pos, _ in c['plant']))
        assert list(np.flatnonzero(~np.isfinite(golden))) == hit, (c['kind'], golden)
        kinds.add((c['kind'], 'nan' if np.isnan(golden[hit[0]]) else 'inf'))
        fn = quantization.nonUniformQuantization_variable(bucket_size=c['bucket'], pre_process_tensors=True,
                                                          tensor=torch.from_numpy(z.base).to(DEV))
        fn.forward(None, torch.from_numpy(pts).to(DEV))
        assert same(fn.savedForBackward['indices'], idx)
        for form, gd in forms(gg):
            _, gp = fn.backward(gd)
            check_point_grad(gp, golden, gg, idx, alpha, c['bucket'], 4, (i, c['kind'], c['bucket'], form))
    assert kinds == {('nan', 'nan'), ('pinf', 'inf'), ('pair', 'nan')}


def test_point_gradient_with_a_nan_bucket_alpha_through_the_c_abi():
    """qd_point_grad_f32 with uint8 and int64 indices: a NaN alpha of ONE bucket poisons the points that bucket's elements sit
    on and no other; an inf alpha gives +-inf or (both signs on one point) NaN."""
    lib = _lib.host() if DEV == 'cpu' else _lib.load()
    rng = np.random.RandomState(5)
    n, bucket, k = 3000, 256, 4
    g = rng.randn(n).astype(np.float32)
    idx = rng.randint(0, 3, size=n).astype(np.int64)               # point 3 is used by the poisoned bucket only
    idx[256 * 5:256 * 6] = 3
    idx[256 * 7 + 9] = 2
    alpha = (rng.rand(12) + 0.5).astype(np.float32)
    alpha[5], alpha[7] = np.nan, np.inf
    g[256 * 7:256 * 8] = np.abs(g[256 * 7:256 * 8])                  # one sign: bins 0 .. 2 become +inf, none NaN
    want, absum = onp.point_grad(g, idx, alpha, bucket, k)
    assert np.isnan(want[3]) and np.all(np.isposinf(want[:3]))
    alpha2 = alpha.copy()
    alpha2[7] = 1.25                                                # only the NaN bucket left: points 0 .. 2 are finite
    want2, absum2 = onp.point_grad(g, idx, alpha2, bucket, k)
    assert np.isnan(want2[3]) and np.all(np.isfinite(want2[:3]))
    ws = _lib.workspace(torch.device(DEV)) if DEV != 'cpu' else None
    wsp, wsn = (ws.data_ptr(), ws.numel()) if ws is not None else (None, 0)
    st = _lib.stream_ptr() if DEV != 'cpu' else None
    for ib, it in ((8, idx), (1, idx.astype(np.uint8))):
        for a, w, ab in ((alpha, want, absum), (alpha2, want2, absum2)):
            out = torch.full((k,), 777.0, device=DEV)
            gd, idd, ad = (torch.from_numpy(v).to(DEV) for v in (g, it, a))
            _lib.check(lib.qd_point_grad_f32(gd.data_ptr(), idd.data_ptr(), ib, ad.data_ptr(), n, bucket, k, out.data_ptr(), wsp, wsn, st))
            got = out.cpu().numpy()
            fin = np.isfinite(w)
            assert np.array_equal(np.isnan(got), np.isnan(w)) and np.array_equal(got[np.isinf(w)], w[np.isinf(w)]), (ib, got, w)
            errlog.check_sum('K6 point gradient, NaN / inf bucket alpha', got[fin], w[fin], ab[fin], (ib,), n_terms=n)


@pytest.mark.parametrize('bucket', [256, 100, None])
def test_scale_down_and_inverse_goldens(bucket):
    """K2 then K3 on the seven inputs: u in the padded bucket layout, alpha / beta, and inv_scale_down(u), against the
    reference and the C oracle."""
    z = G()
    seen = 0
    for i, m in enumerate(z.meta['scale']):
        if m['bucket'] != bucket:
            continue
        seen += 1
        c = z.scale(i)
        x = c['x']
        for form, xd in forms(x):
            sf = quantization.ScalingFunction('linear', False, False, bucket)
            u = sf.scale_down(xd)
            assert same(u, c['u']) and same(sf.alpha, c['alpha']) and same(sf.beta, c['beta']), (m, form)
            assert same(sf.inv_scale_down(u), c['back']), (m, form)
            r = oc.scale_down(x, bucket)
            assert same(u.reshape(-1)[:x.size], r['u']) and same(sf.alpha.reshape(-1), r['alpha']), (m, form)
    assert seen == len(PATTERNS)


def test_inverse_scaling_propagates_nonfinite_alpha_beta_and_u():
    """K3 through the C ABI: y = u alpha + beta with NaN / +-inf in alpha, in beta and in u, out of place, in place and on a
    view at a 4-byte offset; 0 x inf is NaN, inf + -inf is NaN, a finite bucket next to them is untouched."""
    lib = _lib.host() if DEV == 'cpu' else _lib.load()
    st = _lib.stream_ptr() if DEV != 'cpu' else None
    rng = np.random.RandomState(9)
    for n, bucket in ((3000, 256), (3000, 100), (3000, 0), (255, 256)):
        nb = lib.qd_num_buckets(n, bucket)
        padded = lib.qd_padded_length(n, bucket)
        row = padded // nb
        u = rng.rand(padded).astype(np.float32)
        u[::53] = 0.0
        u[7], u[n // 2], u[n - 1] = np.nan, np.inf, -np.inf
        alpha, beta = (rng.rand(nb) + 0.5).astype(np.float32), rng.randn(nb).astype(np.float32)
        for j, (a, b) in enumerate(((np.nan, 0.5), (np.inf, 0.5), (1.5, np.nan), (1.5, np.inf), (np.inf, -np.inf), (-np.inf, 1.0))):
            if 1 + 2 * j < nb:
                alpha[1 + 2 * j], beta[1 + 2 * j] = a, b
        if nb == 1:
            alpha[0] = np.inf
        with np.errstate(invalid='ignore'):
            want = ((u * np.repeat(alpha, row)).astype(np.float32) + np.repeat(beta, row)).astype(np.float32)
            want = (want + np.float32(0.0)).astype(np.float32)[:n]
        assert np.isnan(want).any() and (nb == 1 or np.isfinite(want).any())
        ad, bd = torch.from_numpy(alpha).to(DEV), torch.from_numpy(beta).to(DEV)
        for form, ud in forms(u):
            y = torch.full((n + 2,), 777.0, device=DEV)
            _lib.check(lib.qd_inv_scale_f32(ud.data_ptr(), y[1:].data_ptr(), n, bucket, ad.data_ptr(), bd.data_ptr(), None, st))
            assert same(y[1:1 + n], want) and float(y[0]) == 777.0 and float(y[n + 1]) == 777.0, (n, bucket, form)
            _lib.check(lib.qd_inv_scale_f32(ud.data_ptr(), ud.data_ptr(), n, bucket, ad.data_ptr(), bd.data_ptr(), None, st))
            assert same(ud[:n], want), (n, bucket, form, 'in place')


def test_training_loop_epilogues_golden():
    """K8: clamp(-1, 1) leaves a NaN as it is and maps +-inf to +-1; grad[w.abs() > 1] = 0 keeps the gradient where w is NaN
    (the comparison is false) and zeroes it where w is +-inf; +-1 exactly is inside."""
    z = G().z
    w, g = z['e_w'], z['e_g']
    assert np.isnan(w).sum() >= 2 and np.isinf(w).sum() >= 3 and np.all(g != 0)
    assert np.array_equal(np.isnan(z['e_clamped']), np.isnan(w)) and np.all(z['e_truncated'][np.isnan(w)] == g[np.isnan(w)])
    assert np.all(z['e_truncated'][np.isinf(w)] == 0) and np.all(z['e_truncated'][np.abs(w) == 1] == g[np.abs(w) == 1])
    for form, wd in forms(w):
        for gform, gd in forms(g):
            out = ste.truncated_ste_(gd, wd, 1.0)
            assert same(out, z['e_truncated']) and same(gd, z['e_truncated']) and same(wd, w), (form, gform)
        out = ste.clamp_(wd, 1.0)
        assert same(out, z['e_clamped']) and same(wd, z['e_clamped']), form
    assert same(onp.truncated_ste_mask(w, g), z['e_truncated'])


# ---------------------------------------------------------------------------------------------------------------------------
# neighbour isolation: lists of tensors carved from one flat buffer

def carve(arrays, fill=777.0, gap=3):
    """Views of one flat buffer on DEV holding `arrays` with `gap` elements of `fill` before each (so that the bases are not
    16-byte aligned) and after the last; returns (flat, views, mask of the gap elements)."""
    total = sum(a.size + gap for a in arrays) + gap
    flat = torch.full((total,), fill, dtype=torch.float32)
    keep = torch.ones(total, dtype=torch.bool)
    spans, off = [], 0
    for a in arrays:
        off += gap
        flat[off:off + a.size] = torch.from_numpy(a)
        keep[off:off + a.size] = False
        spans.append((off, off + a.size))
        off += a.size
    flat = flat.to(DEV)
    return flat, [flat[lo:hi] for lo, hi in spans], keep


def isolation_lists():
    """(name, sizes, index of the poisoned tensor, position of the non-finite element in it).  The four placements of the issue:
    the last bucket of tensor i with tensor i + 1 starting right behind it, the first bucket of tensor i + 1, a tensor
    shorter than a bucket that shares a wave tile (four buckets) with its neighbours, a tensor alone in its tile."""
    return [
        ('last bucket of tensor i', (257, 3000, 1025, 256, 1, 255, 1024, 1023), 1, 2999),
        ('last full bucket of tensor i', (1023, 1024, 255, 257, 3000, 1, 1025), 1, 1023),
        ('first bucket of tensor i + 1', (1024, 1025, 3000, 257, 255, 1, 256), 2, 0),
        ('short tensor sharing a tile', (255, 1, 255, 257, 1, 256, 1023), 1, 0),
        ('short tensor between short tensors', (1, 255, 1, 255, 1, 3000), 3, 100),
        ('tensor alone in its tile', (3000, 1024, 1025, 256, 1023, 257), 1, 600),
    ]


def isolation_inputs(sizes, seed):
    rng = np.random.RandomState(seed)
    return [(rng.randn(n) * (0.05 + 0.3 * i)).astype(np.float32) for i, n in enumerate(sizes)]


@pytest.mark.parametrize('value', [np.nan, np.inf, -np.inf], ids=['nan', 'pinf', 'ninf'])
@pytest.mark.parametrize('bucket', [256, 100, None])
def test_per_tensor_calls_on_neighbouring_views_are_isolated(bucket, value):
    """The per-tensor half of the isolation cases (it runs on CPU tensors too): uniformQuantization of every view of the flat
    buffer equals the oracle on that tensor alone -- the poison of one call reaches neither another call nor the gaps."""
    for name, sizes, ti, pos in isolation_lists():
        xs = isolation_inputs(sizes, 11)
        xs[ti][pos] = value
        flat, views, keep = carve(xs)
        outs_flat, outs, _ = carve([np.zeros_like(x) for x in xs])
        for j, (x, v, o) in enumerate(zip(xs, views, outs)):
            q, sf = quantization.uniformQuantization(v, 16, bucket_size=bucket)
            o.copy_(q)
            r = oc.uniform_quantize(x, 16, bucket, want_idx=False, want_lev=False)
            assert same(q, r['q']) and same(sf.alpha.reshape(-1), r['alpha']) and same(sf.beta.reshape(-1), r['beta']), (name, j)
            assert bool(np.isnan(r['q']).any()) == (j == ti), (name, j)
        assert bool((flat.cpu()[keep] == 777.0).all()) and bool((outs_flat.cpu()[keep] == 777.0).all()), name


@pytest.mark.parametrize('value', [np.nan, np.inf, -np.inf], ids=['nan', 'pinf', 'ninf'])
@pytest.mark.parametrize('bucket', [256, 100, None])
def test_multi_tensor_quantizer_isolates_a_poisoned_tensor(bucket, value):
    """One launch over 6-8 tensors, one of which holds a NaN / an infinity: every output equals the per-tensor call and the
    oracle, the finite tensors equal what they give when the poisoned tensor is finite (k_multi_uniform takes its division
    path per wave, k_mg_minmax / k_mg_fold poison per tile), the gaps keep their 777, alpha_beta row by row."""
    from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer
    assert DEV != 'cpu'
    for name, sizes, ti, pos in isolation_lists():
        clean = isolation_inputs(sizes, 11)
        xs = [x.copy() for x in clean]
        xs[ti][pos] = value
        results = {}
        for label, arrays in (('poisoned', xs), ('clean', clean)):
            _, ins, _ = carve(arrays)
            flat_out, outs, keep = carve([np.zeros_like(x) for x in arrays])
            mt = MultiTensorQuantizer(ins, 16, bucket, outputs=outs)
            mt.quantize()
            assert bool((flat_out.cpu()[keep] == 777.0).all()), (name, label)
            results[label] = [o.cpu().numpy() for o in outs]
            for j, (x, v, o) in enumerate(zip(arrays, ins, outs)):
                r = oc.uniform_quantize(x, 16, bucket, want_idx=False, want_lev=False)
                q, sf = quantization.uniformQuantization(v, 16, bucket_size=bucket)
                assert same(o, r['q']) and same(o, q.cpu().numpy()), (name, label, j, int(np.isnan(o.cpu().numpy()).sum()), int(np.isnan(r['q']).sum()))
                if bucket is None:
                    assert same(mt.alpha_beta[j], np.array([r['alpha'][0], r['beta'][0]], np.float32)), (name, label, j)
        for j in range(len(sizes)):
            if j != ti:
                assert np.array_equal(results['poisoned'][j], results['clean'][j]) and np.isfinite(results['poisoned'][j]).all(), (name, j)
        assert np.isnan(results['poisoned'][ti]).any()


@pytest.mark.parametrize('value', [np.nan, np.inf, -np.inf], ids=['nan', 'pinf', 'ninf'])
def test_multi_tensor_diff_quant_isolates_a_poisoned_tensor(value):
    """K5m / K6m over the same lists (bucket 256): quantized values, uint8 indices and the point gradients of every tensor
    equal the per-tensor pre-processed call and the oracle; the rows of the finite tensors equal the clean run's."""
    from quantized_distillation_amd.multi_tensor import MultiTensorDiffQuant
    assert DEV != 'cpu'
    k, bucket = 4, 256
    for name, sizes, ti, pos in isolation_lists():
        clean = isolation_inputs(sizes, 11)
        xs = [x.copy() for x in clean]
        xs[ti][pos] = value
        gs = isolation_inputs(sizes, 12)
        rng = np.random.RandomState(13)
        pts = np.sort(rng.rand(len(sizes), k), axis=1).astype(np.float32)
        pd = torch.from_numpy(pts).to(DEV)
        rows = {}
        for label, arrays in (('poisoned', xs), ('clean', clean)):
            _, ins, _ = carve(arrays)
            _, grads, _ = carve(gs)
            flat_out, outs, keep = carve([np.zeros_like(x) for x in arrays])
            dq = MultiTensorDiffQuant(ins, outs, grads, k, bucket)
            dq.forward(pd)
            gp = dq.backward().cpu().numpy()
            assert bool((flat_out.cpu()[keep] == 777.0).all()), (name, label)
            rows[label] = (gp, [o.cpu().numpy() for o in outs])
            for j, (x, v, o) in enumerate(zip(arrays, ins, outs)):
                r = oc.nonuniform_quantize(x, pts[j], bucket, 'midpoint')
                assert same(o, r['q']) and same(dq.indices[j].long(), r['idx']), (name, label, j)
                fn = quantization.nonUniformQuantization_variable(bucket_size=bucket, pre_process_tensors=True, tensor=v)
                assert same(fn.forward(None, pd[j]), r['q']) and same(fn.savedForBackward['indices'], r['idx']), (name, label, j)
                _, one = fn.backward(grads[j])
                want, absum = onp.point_grad(gs[j], r['idx'], r['alpha'], bucket, k)
                fin = np.isfinite(want)
                for got in (gp[j], one.cpu().numpy()):
                    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[np.isinf(want)], want[np.isinf(want)]), (name, label, j, got, want)
                    errlog.check_sum('K6m point gradient, poisoned neighbour', got[fin], want[fin], absum[fin], (name, label, j), n_terms=x.size)
                assert fin.all() == (label == 'clean' or j != ti), (name, label, j, want)
        for j in range(len(sizes)):
            if j != ti:
                assert np.array_equal(rows['poisoned'][0][j], rows['clean'][0][j]) and np.array_equal(rows['poisoned'][1][j], rows['clean'][1][j]), (name, j)


def check_ste_against_oracle(out, x, g, s, bucket, tag):
    """K7 / K7m against the oracle (onp.ste_complicated_backward, errlog.check_ste).  A bucket of x that holds a NaN or an
    infinity quantizes to NaN as a whole: the reference adds and subtracts S = NaN at the bucket's FIRST element (torch
    reports min and max of the all-NaN quantized bucket there), so out is NaN at that element and g at every other one.
    The remaining buckets -- finite x -- are checked as one tensor: every position but the two touched ones equals g bit
    for bit, the touched ones hold g +- S within the tolerance of the bucket sum."""
    n = x.size
    row = min(bucket, n)
    nb = -(-n // row)
    with np.errstate(invalid='ignore'):
        ref = onp.ste_complicated_backward(x, g, s, bucket)
    bad = np.array([not np.isfinite(x[b * row:(b + 1) * row]).all() for b in range(nb)])
    keep = np.ones(n, bool)
    for b in np.flatnonzero(bad):
        sl = slice(b * row, min((b + 1) * row, n))
        want = g[sl].copy()
        want[0] = np.nan
        assert np.array_equal(out[sl], want, equal_nan=True), (tag, b, 'a non-finite bucket: NaN at its first element, g elsewhere')
        assert np.array_equal(np.isnan(ref[sl]), np.isnan(want)), (tag, b, 'the oracle puts the NaN elsewhere')
        keep[sl] = False
    if keep.any():
        if not bad.any():
            errlog.check_ste('K7m bucket sum, isolation lists', out, x, g, s, bucket, tag)
        else:
            # the finite buckets one by one (each is a tensor of one bucket to the oracle; a ragged last one included)
            for b in np.flatnonzero(~bad):
                sl = slice(b * row, min((b + 1) * row, n))
                errlog.check_ste('K7m bucket sum, isolation lists', out[sl], x[sl], g[sl], s, bucket, tag + (int(b),))


@pytest.mark.parametrize('value', [np.nan, np.inf, -np.inf], ids=['nan', 'pinf', 'ninf'])
@pytest.mark.parametrize('bucket', [256, 100])
def test_multi_tensor_ste_isolates_a_poisoned_tensor(bucket, value):
    """K7m over the same lists: bit-identical to the per-tensor K7 on every tensor, the finite tensors bit-identical to the
    clean run, NaN only in the poisoned tensor's poisoned bucket."""
    from quantized_distillation_amd.multi_tensor import MultiTensorSTE
    assert DEV != 'cpu'
    for name, sizes, ti, pos in isolation_lists():
        clean = isolation_inputs(sizes, 11)
        xs = [x.copy() for x in clean]
        xs[ti][pos] = value
        gs = isolation_inputs(sizes, 12)
        res = {}
        for label, arrays in (('poisoned', xs), ('clean', clean)):
            _, ws, _ = carve(arrays)
            _, grads, _ = carve(gs)
            flat_out, outs, keep = carve([np.zeros_like(x) for x in arrays])
            MultiTensorSTE(ws, grads, 16, bucket, outs=outs).backward()
            assert bool((flat_out.cpu()[keep] == 777.0).all()), (name, label)
            res[label] = [o.cpu().numpy() for o in outs]
            for j, (w, g_, o) in enumerate(zip(ws, grads, outs)):
                assert same(o, ste.ste_bucket_backward(w, g_, bucket, 16).cpu().numpy()), (name, label, j)
                check_ste_against_oracle(o.cpu().numpy(), arrays[j], gs[j], 16, bucket, (name, label, j))
        for j in range(len(sizes)):
            if j != ti:
                assert np.array_equal(res['poisoned'][j], res['clean'][j]) and np.isfinite(res['poisoned'][j]).all(), (name, j)
        row = min(bucket, sizes[ti])
        bad = np.flatnonzero(np.isnan(res['poisoned'][ti]))
        assert bad.size >= 1 and np.all(bad // row == pos // row), (name, bad)
        ok = np.ones(sizes[ti], bool)
        ok[(pos // row) * row:(pos // row + 1) * row] = False
        assert np.array_equal(res['poisoned'][ti][ok], res['clean'][ti][ok]), name


# ---------------------------------------------------------------------------------------------------------------------------
# codec and compressed files

@pytest.mark.parametrize('s,bits', [(2, 1), (16, 4), (256, 8)])
@pytest.mark.parametrize('bucket', [256, 100, None])
def test_pack_unpack_and_level_bytes_on_nonfinite_buckets(bucket, s, bits):
    """codec.pack_uniform -> unpack equals the quantizer's output on the seven inputs; the uint8 level output of
    qd_uniform_f32 equals libqd_host.so's byte for byte (a NaN level is stored as 0 by both) and the oracle's."""
    from quantized_distillation_amd import codec
    assert DEV != 'cpu'
    base = G().base
    lib, hostlib = _lib.load(), _lib.host()
    ws = _lib.workspace(torch.device(DEV))
    for pat in PATTERNS:
        x = plant(base, pat, bucket)
        n = x.size
        r = oc.uniform_quantize(x, s, bucket, want_idx=False)
        assert np.isnan(r['q']).any()
        xd = torch.from_numpy(x).to(DEV)
        q, _ = quantization.uniformQuantization(xd, s, bucket_size=bucket)
        assert same(q, r['q']), pat
        pk = codec.pack_uniform(xd, s, bucket, bits=bits)
        assert same(pk.unpack(), r['q']) and same(pk.alpha.reshape(-1), r['alpha']) and same(pk.beta.reshape(-1), r['beta']), pat
        assert same(codec.level_histogram(xd, s, bucket), np.bincount(r['lev'], minlength=s)), pat
        nb = lib.qd_num_buckets(n, bucket or 0)
        xh = torch.from_numpy(x)
        qh, abh, lh = torch.empty(n), torch.empty(2, nb), torch.full((n,), 99, dtype=torch.uint8)
        qg, abg, lg = torch.empty(n, device=DEV), torch.empty(2, nb, device=DEV), torch.full((n,), 99, dtype=torch.uint8, device=DEV)
        _lib.check(hostlib.qd_uniform_f32(xh.data_ptr(), qh.data_ptr(), n, bucket or 0, s, abh[0].data_ptr(), abh[1].data_ptr(), lh.data_ptr(),
                                          None, 0, 0.0, 0, 0, None, 0, None))
        _lib.check(lib.qd_uniform_f32(xd.data_ptr(), qg.data_ptr(), n, bucket or 0, s, abg[0].data_ptr(), abg[1].data_ptr(), lg.data_ptr(),
                                      None, 0, 0.0, 0, 0, ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
        assert same(lg, lh.numpy()) and same(lg, r['lev'].astype(np.uint8)), (pat, np.flatnonzero(lg.cpu().numpy() != lh.numpy())[:8])
        assert same(qg, qh.numpy()) and same(abg, abh.numpy()), pat
        assert int(lh.numpy()[np.isnan(r['q'])].max()) == 0, pat


@pytest.mark.parametrize('mode', ['uniform', 'nonuniform'])
def test_compressed_checkpoint_of_a_model_with_nonfinite_buckets(tmp_path, mode):
    """save_compressed does not refuse such a model: the file written from device tensors and the one written from their CPU
    copies are byte-identical, and both decode -- on either side -- to exactly what the quantizer gives (NaN buckets NaN)."""
    from quantized_distillation_amd import compressed as C
    assert DEV != 'cpu'
    ts = nonfinite_model()
    pts = torch.tensor([0.0, 0.3, 0.6, 1.0])
    kw = dict(s=16) if mode == 'uniform' else dict(points=[pts] * 3)
    pc, pd = str(tmp_path / 'cpu.qd'), str(tmp_path / 'dev.qd')
    C.save_compressed(pc, ts, bucket_size=256, **kw)
    C.save_compressed(pd, {k_: t.to(DEV) for k_, t in ts.items()}, bucket_size=256, **kw)
    assert open(pc, 'rb').read() == open(pd, 'rb').read()
    for path in (pc, pd):
        for device in ('cpu', DEV):
            out = C.load_compressed(path, device=device)
            for name, t in ts.items():
                want = (quantization.uniformQuantization(t, 16, bucket_size=256)[0] if mode == 'uniform'
                        else quantization.nonUniformQuantization(t, pts, bucket_size=256)[0])
                wd = (quantization.uniformQuantization(t.to(DEV), 16, bucket_size=256)[0] if mode == 'uniform'
                      else quantization.nonUniformQuantization(t.to(DEV), pts, bucket_size=256)[0])
                assert torch.isnan(want).any() and not torch.isnan(want).all()
                assert same(out[name], want.numpy()) and same(wd, want.numpy()), (path, device, name)
