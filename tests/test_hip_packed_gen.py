"""The end of a decoder step on the device (libqd_infer_gen.so, include/qd_infer_gen.h) at the C ABI, and PackedGenerator on top.
The reference for everything is y = qdm_linear_packed_f32 on the same packed weight, bias and x -- which tests/test_hip_packed_mm.py
holds to float64 -- so only what is new is checked here: the logits are y's bits, lse against the float64 logsumexp of y (bound: 4 x
what fp32 torch.logsumexp reaches on the CPU over the same cases, profiles/packed_gen_error.txt), the top k against a lexsort of y."""
import functools

import numpy as np
import pytest
import torch

from quantized_distillation_amd import _infer_gen, _infer_mm, _lib, codec, packed_layers

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
U = 2.0 ** -24
PAD = 16                               # sentinel floats around every output
# a ragged tile | a ragged panel | several panels | dim no multiple of 4 or 64 | buckets straddling rows (37) and not (256)
SHAPES = ((1, 1), (15, 3), (16, 64), (17, 65), (63, 130), (64, 500), (65, 37), (130, 200), (200, 66))
# every shape twice: m, bits, bucket and bias rotate so that each shape meets two of each
CASES = [(V, dim, (1, 5, 65)[(n + r) % 3], (2, 3, 8)[(n + 2 * r) % 3], (37, 256)[(n + r) % 2], bool((n + r) % 2)) for r in (0, 1) for n, (V, dim) in enumerate(SHAPES)]


@pytest.fixture(scope='module')
def lib():
    return _infer_gen.load()


def fmt(pk):
    return (pk.packed.data_ptr(), pk.alpha.data_ptr(), pk.beta.data_ptr(), pk.shape[0], pk.shape[1], pk.bucket_size or 0, pk.s, pk.bits)


def linear(pk, x, bias):
    """y: the batched Linear of libqd_infer_mm.so, the reference of every test here."""
    y = torch.empty(x.shape[0], pk.shape[0], device=DEV)
    assert _infer_mm.load().qdm_linear_packed_f32(*fmt(pk), x.data_ptr(), x.shape[0], None if bias is None else bias.data_ptr(), y.data_ptr(),
                                                  _lib.stream_ptr(DEV)) == 0
    return y


def generate(lib, pk, x, bias, k=0, want_logp=True, kbuf=None):
    """One qdn_generator_packed_f32, every output between sentinel bands that must survive; (lse, logp or None, top_val, top_idx).
    kbuf: the size of the top buffers where it is not k (k == 0 with buffers that must stay untouched)."""
    m, V = x.shape[0], pk.shape[0]
    kb = k if kbuf is None else kbuf
    sizes = dict(lse=m, logp=m * V if want_logp else 0, top_val=m * kb, top_idx=m * kb, work=lib.qdn_generator_work_bytes(V, m, k) // 4)
    bufs = {n: torch.full((c + 2 * PAD,), 7.0 if n != 'top_idx' else 7, dtype=torch.int64 if n == 'top_idx' else torch.float32, device=DEV) for n, c in sizes.items()}
    ptr = {n: b[PAD:].data_ptr() if sizes[n] else None for n, b in bufs.items()}
    rc = lib.qdn_generator_packed_f32(*fmt(pk), x.data_ptr(), m, None if bias is None else bias.data_ptr(), ptr['lse'], ptr['logp'], k, ptr['top_val'],
                                      ptr['top_idx'], ptr['work'], _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == 0, rc
    for n, b in bufs.items():
        assert (b[:PAD] == 7).all() and (b[PAD + sizes[n]:] == 7).all(), (n, 'written outside the array')
    if kbuf:
        assert (bufs['top_val'] == 7).all() and (bufs['top_idx'] == 7).all(), 'k == 0 wrote to the top-k buffers'
    body = {n: b[PAD:PAD + sizes[n]] for n, b in bufs.items()}
    return body['lse'], body['logp'].view(m, V) if want_logp else None, body['top_val'].view(m, kb), body['top_idx'].view(m, kb)


@functools.lru_cache(maxsize=None)
def problem(V, dim, m, bits, bucket, biased, positive=False):
    """(pk, x, bias, y).  Logits of a standard deviation of about 30: the exponentials span many orders of magnitude."""
    g = torch.Generator().manual_seed(1000 * V + 10 * dim + m + bits)
    W, x = torch.randn(V, dim, generator=g), torch.randn(m, dim, generator=g) * 30.0 / dim ** 0.5
    if positive:                                                          # duplicated rows, one bucket per row: equal logits that are the largest
        W, x = W.abs(), x.abs() / 30.0
        for a, b in ((3, 7), (5, 21), (10, 130)):                         # inside one tile | across tiles of a panel | across panels
            W[a] = W[b] = W[a] * 3.0
    pk = codec.pack_uniform(W.to(DEV), 1 << bits, bucket, bits)
    bias = (torch.randn(V, generator=g) * 3.0).to(DEV) if biased else None
    x = x.to(DEV)
    return pk, x, bias, linear(pk, x, bias)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def lse_units(lse, y):
    """|lse - float64 logsumexp(y)| in units of 2^-24 (|lse| + 1), the worst row."""
    want = torch.logsumexp(y.double().cpu(), dim=1)
    return float(((lse.double().cpu() - want).abs() / (U * (want.abs() + 1.0))).max())


def expected_order(y_row):
    """The header's total order: NaN first, then descending, ties to the lower index."""
    nan = np.isnan(y_row)
    return np.lexsort((np.arange(y_row.size), np.where(nan, 0.0, -y_row), ~nan))


def check_topk(top_val, top_idx, y, lse, k):
    yc, idx, val, ls = y.cpu().numpy(), top_idx.cpu().numpy(), top_val.cpu(), lse.cpu()
    for i in range(yc.shape[0]):
        want = expected_order(yc[i])[:k]
        assert np.array_equal(idx[i, :len(want)], want), (i, idx[i], want)
        assert (idx[i, len(want):] == -1).all() and (val[i, len(want):] == float('-inf')).all(), 'V < k: -inf and -1'
        got, ref = val[i, :len(want)], torch.from_numpy(yc[i, want]) - ls[i]
        assert same_bits(got[~ref.isnan()], ref[~ref.isnan()]) and torch.equal(got.isnan(), ref.isnan()), (i, got, ref)


@pytest.mark.parametrize('case', CASES, ids=str)
def test_logits_are_the_batched_linears_bits(lib, case):
    pk, x, bias, y = problem(*case)
    lse, logp, _, _ = generate(lib, pk, x, bias)
    assert same_bits(logp, y - lse[:, None])


def test_lse_against_float64_within_four_times_fp32_torch(lib):
    """Both figures are measured here, over the same cases; the baseline must not be zero (it would make the bound empty)."""
    ours = base = 0.0
    for case in CASES:
        pk, x, bias, y = problem(*case)
        ours = max(ours, lse_units(generate(lib, pk, x, bias, want_logp=False)[0], y))
        base = max(base, lse_units(torch.logsumexp(y.cpu(), dim=1), y))
    print('lse: %.3f x 2^-24 (|lse| + 1); fp32 torch.logsumexp on the CPU %.3f; bound %.3f' % (ours, base, 4 * base))
    assert base > 0 and ours <= 4 * base, (ours, base)


@pytest.mark.parametrize('k', (1, 5, 16))
def test_topk_is_the_lexsort_of_y(lib, k):
    cases = [CASES[0], CASES[1], CASES[7], CASES[8], CASES[13], (200, 66, 5, 3, 66, False, True), (200, 66, 65, 8, 66, False, True)]
    for case in cases:                                                    # V < k among them (V = 1, 15); the last two: ties
        pk, x, bias, y = problem(*case)
        if len(case) == 7:
            yc = y.cpu()
            assert same_bits(yc[:, 3], yc[:, 7]) and same_bits(yc[:, 5], yc[:, 21]) and same_bits(yc[:, 10], yc[:, 130]), 'the duplicated rows tie'
            assert set(expected_order(yc[0].numpy())[:6].tolist()) == {3, 7, 5, 21, 10, 130}, 'and lead'
        lse, _, top_val, top_idx = generate(lib, pk, x, bias, k, want_logp=False)
        check_topk(top_val, top_idx, y, lse, k)


@pytest.mark.parametrize('what', ('nan bucket', 'nan bucket at word 0', 'nan in x', 'one nan word', 'inf bucket', 'bias -inf on a panel', 'bias -inf everywhere'))
def test_non_finite_in_kind_with_float64(lib, what):
    V, dim, m = 1 if what == 'one nan word' else 130, 200, 5
    g = torch.Generator().manual_seed(5)
    W, x = torch.randn(V, dim, generator=g), (torch.randn(m, dim, generator=g) * 2.0).to(DEV)
    bias = torch.randn(V, generator=g)
    if what == 'nan bucket':
        W[70, 3] = float('nan')
    if what in ('nan bucket at word 0', 'one nan word'):                  # NaN sorts first at the lowest index there is
        W[0, 3] = float('nan')
    if what == 'nan in x':                                                # every logit of row 2 is NaN: its top k are the words 0 .. k - 1
        x[2, 7] = float('nan')
    if what == 'inf bucket':
        W[129, 199] = float('inf')
    if what == 'bias -inf on a panel':
        bias[64:128] = float('-inf')
    if what == 'bias -inf everywhere':
        bias[:] = float('-inf')
    pk, bias = codec.pack_uniform(W.to(DEV), 16, 50, 4), bias.to(DEV)     # 50 divides 64 x 200: the first panel's rows are whole buckets
    y = linear(pk, x, bias)
    lse, logp, top_val, top_idx = generate(lib, pk, x, bias, 5)
    y64 = y.double().cpu()
    lse64 = torch.logsumexp(y64, dim=1)
    assert torch.equal(lse.cpu().isnan(), lse64.isnan()) and torch.equal(lse.cpu()[lse64.isinf()].double(), lse64[lse64.isinf()]), (lse, lse64)
    assert not what.startswith('bias') or not lse.isnan().any()
    lp64 = y64 - lse64[:, None]
    assert torch.equal(logp.cpu().isnan(), lp64.isnan()) and torch.equal(logp.cpu()[lp64.isinf()].double(), lp64[lp64.isinf()])
    want = y - lse[:, None]
    assert same_bits(logp[~want.isnan()], want[~want.isnan()]) and torch.equal(logp.isnan(), want.isnan())
    if what == 'nan in x':
        assert top_idx[2].tolist() == [0, 1, 2, 3, 4] and lse.isnan().tolist() == [False, False, True, False, False]
    if what == 'one nan word':
        assert lse.isnan().all() and (top_idx == torch.tensor([0, -1, -1, -1, -1], device=DEV)).all()
    check_topk(top_val, top_idx, y, lse, 5)
    if what == 'bias -inf on a panel':
        # on the host: the panel's words removed from the float64 sum; lse within 4 x what fp32 torch.logsumexp reaches on the rest
        rest = torch.cat([y[:, :64], y[:, 128:]], dim=1)
        base = lse_units(torch.logsumexp(rest.cpu(), dim=1), rest)
        assert base > 0 and lse_units(lse, rest) <= 4 * base, (lse_units(lse, rest), base)
        # and bit for bit -- both sides are calls of the library: -inf on every word past the first panel against the first panel alone
        head = codec.pack_uniform(W[:64].to(DEV), 16, 50, 4)
        assert same_bits(head.packed, pk.packed[:head.packed.numel()]) and same_bits(head.alpha, pk.alpha[:head.alpha.numel()])
        b2 = bias.clone()
        b2[128:] = float('-inf')                                          # now words 64 .. 129 are -inf: lse is the first panel's
        assert same_bits(generate(lib, pk, x, b2)[0], generate(lib, head, x, bias[:64].contiguous())[0])


def test_rows_do_not_depend_on_the_batch_the_grid_or_what_was_asked_for(lib):
    pk, x, bias, y = problem(200, 66, 65, 3, 37, True)
    full = generate(lib, pk, x, bias, 5)
    for i in (0, 63, 64):
        one = generate(lib, pk, x[i:i + 1].contiguous(), bias, 5)
        assert all(same_bits(o, f[i:i + 1]) for o, f in zip(one, full)), 'row %d alone' % i
    for cap in (1, 3):
        assert lib.qdn_set_grid_cap(cap) == 0
        try:
            capped = generate(lib, pk, x, bias, 5)
        finally:
            assert lib.qdn_set_grid_cap(0) == cap
        assert all(same_bits(c, f) for c, f in zip(capped, full)), 'grid cap %d' % cap
    bare = generate(lib, pk, x, bias, 0, want_logp=False, kbuf=5)         # nothing asked for: lse alone, the top buffers untouched
    assert same_bits(bare[0], full[0])
    assert same_bits(generate(lib, pk, x, bias, 16, want_logp=False)[3][:, :5], full[3])


def test_the_module_is_the_raw_call_replays_from_a_graph_and_refuses(lib):
    torch.manual_seed(3)
    lin = torch.nn.Linear(66, 200).to(DEV)
    gen = packed_layers.PackedGenerator.from_linear(lin, 16, bucket_size=37)
    xs = [torch.randn(2, 5, 66, device=DEV) * 4.0 for _ in range(3)]
    with torch.no_grad():
        eager = [gen(x, topk=5) for x in xs]
        raw = generate(lib, gen.as_packed_uniform(), xs[0].view(10, 66), gen.bias, 5)
        assert all(same_bits(a.reshape(b.shape), b) for a, b in zip((eager[0].lse, eager[0].log_probs, eager[0].top_values), raw))
        assert torch.equal(eager[0].top_indices.view(10, 5), raw[3]) and eager[0].log_probs.shape == (2, 5, 200) and eager[0].log_probs.grad_fn is None
        assert gen(xs[0], log_probs=False)[::2] == (None, None) and same_bits(gen(xs[0], log_probs=False).lse, eager[0].lse)
        assert same_bits(gen.unpack().weight, gen.as_packed_uniform().unpack())
        buf = xs[0].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            outs = gen(buf, topk=5)
    torch.cuda.synchronize()
    for r in (1, 2, 0, 1):
        buf.copy_(xs[r])
        graph.replay()
        torch.cuda.synchronize()
        assert all(same_bits(o, e) for o, e in zip(outs[:3], eager[r][:3])) and torch.equal(outs[3], eager[r][3]), r
    for x, kw, err in ((xs[0].cpu(), {}, NotImplementedError), (xs[0].double(), {}, TypeError), (xs[0], dict(topk=17), ValueError),
                       (xs[0].clone().requires_grad_(), {}, RuntimeError)):
        with pytest.raises(err):
            gen(x, **kw)
