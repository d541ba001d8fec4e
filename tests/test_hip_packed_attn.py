"""A global-attention step on the device (libqd_infer_attn.so, include/qd_infer_attn.h) at the C ABI -- the context kernel against
float64 torch, the output projection against the float64 sums with the bit-exact weights of tests/packed_layer_cases.py -- and
PackedGlobalAttention on top.  Every fp32 tolerance is 4 x what fp32 torch reaches on the CPU on the same cases (profiles/packed_attn_error.txt)."""
import numpy as np
import pytest
import torch

import packed_layer_cases as P
from test_hip_packed_layers import DEV, FLOAT_GUARD, Placed, fmt, place_weight
from quantized_distillation_amd import _infer, _infer_attn, _lib, packed_layers

pytestmark = pytest.mark.gpu

DIMS = (1, 7, 64, 261, 1030)           # a ragged group alone | a lane's second trip (261 = 65 groups + 1) | a thread's second trip in the context pass
SOURCES = (1, 3, 9, 50)                # fewer positions than waves, later trips of a wave.  (1030, 50) does not fit into LDS: the global path under aliasing
U = 2.0 ** -24


@pytest.fixture(scope='module')
def lib():
    return _infer_attn.load()


def on_device(a, phase=0):
    src = torch.from_numpy(np.array(a).reshape(-1))                       # `phase` floats into a fresh allocation; a copy: the shared cases are read-only
    t = torch.empty(a.size + 3, dtype=src.dtype, device=DEV)[phase:phase + a.size]
    t.copy_(src)
    return t


def context(lib, q, keys, values=None, lengths=None, phase=0):
    """One qda_attn_context_f32; values None: the same pointer as keys.  (align, ctx) as numpy."""
    batch, S, dim = keys.shape
    dq, dk = on_device(q, phase), on_device(keys, (phase + 1) % 4)
    dv = dk if values is None else on_device(values, (phase + 2) % 4)
    dl = None if lengths is None else on_device(np.asarray(lengths, np.int64))
    align, ctx = (torch.full((n + 3,), 7.0, device=DEV)[(phase + k) % 4:][:n] for k, n in ((3, batch * S), (0, batch * dim)))
    rc = lib.qda_attn_context_f32(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), None if dl is None else dl.data_ptr(), batch, S, dim,
                                  align.data_ptr(), ctx.data_ptr(), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == 0, rc
    return align.cpu().numpy().reshape(batch, S), ctx.cpu().numpy().reshape(batch, dim)


def context_problem(dim, S, batch, mixed, seed):
    rng = np.random.RandomState(seed)
    q = (rng.randn(batch, dim) * 2.0 / np.sqrt(dim)).astype(np.float32)             # scores of sigma 2: a softmax that is neither flat nor one-hot
    keys, values = rng.randn(batch, S, dim).astype(np.float32), rng.randn(batch, S, dim).astype(np.float32)
    lengths = np.array([1, S, (S + 1) // 2, S, 1][:batch] if batch > 1 else [max(1, S - 1)], np.int64) if mixed else None
    return q, keys, values, lengths


def padded(a, lengths, fill):
    out = a.copy()                                                       # `fill` (cycled) at every position at or past the row's length
    for b, n in enumerate(lengths if lengths is not None else ()):
        out[b, max(int(n), 0):] = np.resize(np.asarray(fill, np.float32), out[b, max(int(n), 0):].shape)
    return out


def reference(q, keys, values, lengths, dtype):
    """The torch composition on the CPU in `dtype`, the padding zeroed; (align, ctx, sum_s align |v|)."""
    k, v = (torch.from_numpy(padded(a, lengths, 0.0)).to(dtype) for a in (keys, values))
    score = torch.bmm(k, torch.from_numpy(q).to(dtype).unsqueeze(2)).squeeze(2)
    if lengths is not None:
        score = score.masked_fill(torch.arange(keys.shape[1])[None, :] >= torch.from_numpy(lengths)[:, None], float('-inf'))
    align = torch.softmax(score, dim=1)
    return align.numpy(), torch.bmm(align.unsqueeze(1), v).squeeze(1).numpy(), torch.bmm(align.unsqueeze(1), v.abs()).squeeze(1).numpy()


def context_errors(got, q, keys, values, lengths):                       # (align, ctx) against float64: units 2^-24 and 2^-24 sum_s align_s |v_s|
    a64, c64, mag = reference(q, keys, values, lengths, torch.float64)
    return float(np.abs(got[0] - a64).max() / U), float((np.abs(got[1] - c64) / (U * mag)).max())


CONTEXT_CASES = [(dim, S, batch, mixed) for dim in DIMS for S in SOURCES for batch in (1, 5) for mixed in (False, True)]


@pytest.fixture(scope='module')
def context_baseline():
    """What fp32 torch reaches on the CPU over ALL the cases, once: the bound is 4 x this."""
    worst = np.zeros(2)
    for k, case in enumerate(CONTEXT_CASES):
        q, keys, values, lengths = context_problem(*case, seed=k)
        for v in (values, keys):                                          # keys: the aliased call's problem
            worst = np.maximum(worst, context_errors(reference(q, keys, v, lengths, torch.float32)[:2], q, keys, v, lengths))
    return worst


@pytest.mark.parametrize('dim', DIMS)
def test_context_bounds_padding_and_one_result_on_either_path(lib, context_baseline, dim):
    worst = np.zeros(2)
    for k, case in enumerate(CONTEXT_CASES):
        if case[0] != dim:
            continue
        q, keys, values, lengths = context_problem(*case, seed=k)
        got = context(lib, q, keys, values, lengths, phase=k % 4)
        worst = np.maximum(worst, context_errors(got, q, keys, values, lengths))
        alias = context(lib, q, keys, None, lengths, phase=(k + 1) % 4)                   # LDS-resident where it fits ...
        copy = context(lib, q, keys, keys.copy(), lengths, phase=(k + 2) % 4)             # ... and the same floats from memory
        assert all(a.tobytes() == c.tobytes() for a, c in zip(alias, copy)), (case, 'the resident and the global path differ')
        assert context_errors(alias, q, keys, keys, lengths)[1] <= 4 * context_baseline[1], case
        if lengths is not None:                                           # NaN and inf in every padded position: never read
            wild = [context(lib, q, padded(keys, lengths, [np.nan, np.inf]), v if v is None else padded(v, lengths, [-np.inf, np.nan]), lengths)
                    for v in (values, None)]
            zero = [context(lib, q, padded(keys, lengths, 0.0), v if v is None else padded(v, lengths, 0.0), lengths) for v in (values, None)]
            assert all(w.tobytes() == z.tobytes() for ws, zs in zip(wild, zero) for w, z in zip(ws, zs)), (case, 'padding was read')
            for b, n in enumerate(lengths):
                assert not wild[0][0][b, n:].view(np.uint32).any(), (case, 'align is not +0.0 in the padding')
    print('dim %d: align %.2f x 2^-24 (fp32 torch %.2f), ctx %.2f x 2^-24 sum align |v| (fp32 torch %.2f)'
          % (dim, worst[0], context_baseline[0], worst[1], context_baseline[1]))
    assert worst[0] <= 4 * context_baseline[0] and worst[1] <= 4 * context_baseline[1], (worst, context_baseline)


def test_context_edge_lengths(lib):
    q, keys, values, _ = context_problem(261, 9, 5, False, 77)
    lengths = np.array([1, 0, -3, 14, 9], np.int64)
    align, ctx = context(lib, q, padded(keys, np.maximum(lengths, 0), np.nan), padded(values, np.maximum(lengths, 0), np.nan), lengths)
    assert align[0, 0] == 1.0 and ctx[0].tobytes() == values[0, 0].tobytes(), 'one position: align 1, ctx the row itself'
    assert np.isnan(align[1:3]).all() and np.isnan(ctx[1:3]).all(), 'lengths <= 0: NaN rows'
    full = context(lib, q, keys, values, None)
    assert align[3:].tobytes() == full[0][3:].tobytes() and ctx[3:].tobytes() == full[1][3:].tobytes(), 'lengths > S is lengths = S'


@pytest.mark.parametrize('dim,S', ((261, 9), (500, 50), (1030, 50)))    # resident | resident beyond 64 KiB of LDS | too large: from memory
def test_a_context_row_does_not_depend_on_the_batch_or_the_grid(lib, dim, S):
    q, keys, values, _ = context_problem(dim, S, 5, False, 88)
    lengths = np.array([S, 0, 1, (S + 1) // 2, S], np.int64)             # a row masked everywhere between rows that are not
    for v in (values, None):
        full = context(lib, q, keys, v, lengths)
        assert lib.qda_set_grid_cap(1) == 0
        try:
            capped = context(lib, q, keys, v, lengths)
        finally:
            assert lib.qda_set_grid_cap(0) == 1
        assert all(P.same_floats(c, f) for c, f in zip(capped, full)), 'one block for all five rows'
        if v is None:
            assert all(P.same_floats(c, f) for c, f in zip(context(lib, q, keys, keys.copy(), lengths), full)), 'the resident and the global path differ'
        for i in range(5):
            one = context(lib, q[i:i + 1], keys[i:i + 1], None if v is None else v[i:i + 1], lengths[i:i + 1])
            assert all(P.same_floats(o, f[i:i + 1]) for o, f in zip(one, full)), 'row %d alone' % i


OUT_DIMS = (1, 5, 64, 70, 130)         # a part shorter than a group | ... | a part ending mid-slab: part 1 starts off a slab boundary | two slabs per part
OUT_BATCHES = (1, 17, 65)              # three idle waves | a wave with one row | a second chunk
OUT_BUCKETS = (None, 7, 256)           # 7: buckets straddle rows and the boundary between the parts


def out(lib, wt, ctx, x, bias, guarded=False):
    """One qda_attn_out_packed_f32 with pre asked for; (attn_h, pre) as numpy.  guarded: every array between guard bands, all read back."""
    batch, dim = x.shape
    ins = {k: v for k, v in dict(ctx=ctx, x=x, bias=bias).items() if v is not None}
    if guarded:
        dev = {k: Placed(np.float32, v.size, 4 * (i + 1), 64, FLOAT_GUARD, v) for i, (k, v) in enumerate(ins.items())}
        dev.update({k: Placed(np.float32, batch * dim, 4 + 8 * i, 64, FLOAT_GUARD) for i, k in enumerate(('attn_h', 'pre'))})
        wts = place_weight(wt, phase=4)
        ptr, wptr = {k: o.ptr for k, o in dev.items()}, [o.ptr for o in wts]
    else:
        dev = {k: on_device(v, i + 1) for i, (k, v) in enumerate(ins.items())}
        dev.update({k: torch.full((batch * dim,), float('nan'), device=DEV) for k in ('attn_h', 'pre')})
        wts = [torch.from_numpy(np.array(a)).to(DEV) for a in (wt.packed, wt.alpha, wt.beta)]
        ptr, wptr = {k: t.data_ptr() for k, t in dev.items()}, [t.data_ptr() for t in wts]
    f = fmt(wt, *wptr)
    rc = lib.qda_attn_out_packed_f32(*f[:3], *f[5:], dim, ptr['ctx'], ptr['x'], batch, ptr.get('bias'), ptr['attn_h'], ptr['pre'], _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == 0, rc
    if guarded:
        for o, name in zip(wts, ('packed', 'alpha', 'beta')):
            o.read('weight', name)
        got = {k: o.read('guarded', k) for k, o in dev.items()}           # inputs unchanged, outputs wholly written, nothing around any of them
        return got['attn_h'].reshape(batch, dim), got['pre'].reshape(batch, dim)
    return dev['attn_h'].cpu().numpy().reshape(batch, dim), dev['pre'].cpu().numpy().reshape(batch, dim)


def out_problem(dim, bucket, bits, batch, seed, exact=False, nonfinite=False):
    wt = P.exact_weight(dim, 2 * dim, bucket, bits) if exact else P.general_weight(dim, 2 * dim, bucket, 2 ** bits, bits, nonfinite)
    cx, bias = P.linear_inputs(2 * dim, dim, batch, seed, exact)
    return wt, np.ascontiguousarray(cx[:, :dim]), np.ascontiguousarray(cx[:, dim:]), bias, cx


def tanh_errors(attn_h, pre):
    fin = np.isfinite(pre)                                               # (the kernel's, fp32 torch's on the CPU) worst |tanh - float64 tanh| of the call's own pre, units of 2^-24
    want = np.tanh(pre[fin].astype(np.float64))
    return float(np.abs(attn_h[fin] - want).max() / U), float(np.abs(torch.tanh(torch.from_numpy(pre[fin])).numpy() - want).max() / U)


@pytest.mark.parametrize('bits', (2, 3, 4, 8))
def test_out_within_the_bounds(lib, bits):
    cases = [(dim, bucket, False) for dim in OUT_DIMS for bucket in OUT_BUCKETS] + [(70, 7, True), (130, 256, True)]
    worst = np.zeros(3)
    for k, (dim, bucket, nonfinite) in enumerate(cases):
        batch = OUT_BATCHES[(k + bits) % 3]
        wt, ctx, x, bias, cx = out_problem(dim, bucket, bits, batch, 300 + k + bits, nonfinite=nonfinite)
        bias = None if (k + bits) % 2 else bias
        y64, mag = P.linear_expected(wt.w, cx, bias)
        assert not nonfinite or (np.isnan(y64).any() and np.isfinite(y64).any())      # check_linear holds them in kind
        attn_h, pre = out(lib, wt, ctx, x, bias)
        ratio = P.check_linear(pre, y64, mag, (dim, bucket, bits, batch))
        assert np.array_equal(np.isnan(attn_h), np.isnan(pre)) and np.array_equal(attn_h[np.isinf(pre)], np.sign(pre[np.isinf(pre)]))
        worst = np.maximum(worst, (ratio,) + tanh_errors(attn_h, pre))
    print('bits %d: pre error / sum|terms| = %.3g; tanh %.2f x 2^-24 (fp32 torch %.2f)' % ((bits,) + tuple(worst)))
    assert worst[1] <= 4 * worst[2], worst


@pytest.mark.parametrize('bits', (2, 3, 4, 8))
def test_out_bit_for_bit_on_exact_sums(lib, bits):
    """Small-integer activations, power-of-two alpha: every partial sum is exact, so a wrong column offset or a part switch in the wrong
    place changes bits.  (5, 7) is left out: 50 elements leave a last bucket of one, which cannot hold its own minimum and maximum."""
    for k, (dim, bucket) in enumerate((d, b) for d in OUT_DIMS for b in OUT_BUCKETS if (d, b) != (5, 7)):
        batch = OUT_BATCHES[(k + bits + 1) % 3]
        wt, ctx, x, bias, cx = out_problem(dim, bucket, bits, batch, 400 + k + bits, exact=True)
        assert P.exact_condition(wt, cx, bias)
        y64, _ = P.linear_expected(wt.w, cx, bias)
        _, pre = out(lib, wt, ctx, x, bias)
        assert np.array_equal(pre.view(np.uint32), y64.astype(np.float32).view(np.uint32)), (dim, bucket, batch)


@pytest.mark.parametrize('bits', (2, 3, 4, 8))
def test_an_out_row_does_not_depend_on_the_batch_or_the_grid(lib, bits):
    dim, bucket = ((70, 7), (130, 256), (70, None), (130, 7))[bits % 4]
    wt, ctx, x, bias, _ = out_problem(dim, bucket, bits, 65, 500 + bits)
    full = out(lib, wt, ctx, x, bias)
    for i in (0, 63, 64):
        one = out(lib, wt, ctx[i:i + 1], x[i:i + 1], bias)
        assert all(o.tobytes() == f[i:i + 1].tobytes() for o, f in zip(one, full)), 'row %d alone' % i
    assert lib.qda_set_grid_cap(1) == 0
    try:
        capped = out(lib, wt, ctx, x, bias)
    finally:
        assert lib.qda_set_grid_cap(0) == 1
    assert all(c.tobytes() == f.tobytes() for c, f in zip(capped, full)), 'one block for every tile'
    assert all(g.tobytes() == f.tobytes() for g, f in zip(out(lib, wt, ctx, x, bias, guarded=True), full)), 'no alignment changes a bit of the result'


def module_problem(form, batch=5, S=9, dim=70):
    torch.manual_seed(6)
    nn = torch.nn
    att = packed_layers.PackedGlobalAttention.from_linears(nn.Linear(2 * dim, dim).to(DEV), nn.Linear(dim, dim, bias=False).to(DEV) if form == 'general' else None,
                                                           s=16, bucket_size=64)
    query, memory = torch.randn(batch, dim, device=DEV), torch.randn(batch, S, dim, device=DEV)
    keys = torch.randn(batch, S, dim, device=DEV) * 0.3 if form == 'keys' else None
    return att, query, memory, torch.tensor([S, 1, 4, S, 2], device=DEV), keys


@pytest.mark.parametrize('form', ('general', 'dot', 'keys'))
def test_the_module_is_the_hand_written_sequence_and_agrees_with_float64_torch(lib, form):
    """Against the float64 composition on unpack()'s weights on the CPU; the tolerance is 4 x the largest deviation of the same
    composition in fp32 on the CPU from it."""
    att, query, memory, lengths, keys = module_problem(form)
    with torch.no_grad():
        attn_h, align = att(query, memory, lengths, keys)
    st, o = _lib.stream_ptr(DEV), att.out
    q = query
    if form == 'general':
        q = torch.empty_like(query)
        assert _infer.load().qdi_linear_packed_f32(*att.linear_in._format_args(), query.data_ptr(), 5, None, q.data_ptr(), st) == 0
    ks = memory if keys is None else keys
    want_align, ctx, want_h = torch.empty_like(align), torch.empty_like(query), torch.empty_like(query)
    assert lib.qda_attn_context_f32(q.data_ptr(), ks.data_ptr(), memory.data_ptr(), lengths.data_ptr(), 5, 9, 70, want_align.data_ptr(), ctx.data_ptr(), st) == 0
    assert lib.qda_attn_out_packed_f32(o.packed.data_ptr(), o.alpha.data_ptr(), o.beta.data_ptr(), o.bucket_size, o.s, o.bits, 70, ctx.data_ptr(),
                                       query.data_ptr(), 5, o.bias.data_ptr(), want_h.data_ptr(), None, st) == 0
    torch.cuda.synchronize()
    assert attn_h.grad_fn is None and torch.equal(attn_h.view(torch.int32), want_h.view(torch.int32)) and torch.equal(align.view(torch.int32), want_align.view(torch.int32))

    lin_out, lin_in = (None if m is None else m.cpu() for m in att.unpack())

    def compose(dtype):
        x, mem = query.cpu().to(dtype), memory.cpu().to(dtype)
        k = mem if keys is None else keys.cpu().to(dtype)
        qq = x if lin_in is None else lin_in.to(dtype)(x)
        score = torch.bmm(k, qq.unsqueeze(2)).squeeze(2).masked_fill(torch.arange(9)[None, :] >= lengths.cpu()[:, None], float('-inf'))
        a = torch.softmax(score, dim=1)
        return torch.tanh(lin_out.to(dtype)(torch.cat([torch.bmm(a.unsqueeze(1), mem).squeeze(1), x], dim=1))), a

    with torch.no_grad():
        r32 = [t.double() for t in compose(torch.float32)]
        r64 = compose(torch.float64)
    for got, a, b, name in ((attn_h, r32[0], r64[0], 'attn_h'), (align, r32[1], r64[1], 'align')):
        err, tol = float((got.cpu().double() - b).abs().max()), 4 * float((a - b).abs().max())
        print('%s %s: |module - float64| = %.3g, tolerance %.3g' % (form, name, err, tol))
        assert got.shape == b.shape and err <= tol, (name, err, tol)


def test_a_captured_forward_replays_on_new_inputs():
    att, query, memory, lengths, _ = module_problem('general')
    ins = [(torch.randn_like(query), torch.randn_like(memory), torch.tensor(ls, device=DEV)) for ls in ([9, 1, 4, 9, 2], [3, 9, 9, 1, 5], [1, 2, 3, 4, 5])]
    with torch.no_grad():
        eager = [att(*t) for t in ins]
        bufs = [t.clone() for t in ins[0]]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        torch.cuda.synchronize()                                         # every library was loaded by the eager calls above
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            outs = att(*bufs)
    torch.cuda.synchronize()
    for r in (1, 2, 0, 1):
        for b, t in zip(bufs, ins[r]):
            b.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(o.view(torch.int32), e.view(torch.int32)) for o, e in zip(outs, eager[r])), r
