"""A GRU step from packed weights on the device (libqd_infer_gru.so, include/qd_infer_gru.h) at the C ABI: gi and gh against the
float64 sums with the bit-exact weights of tests/packed_layer_cases.py, the epilogue against float64 on the call's own gates, and
PackedGRUCell / PackedGRU / pack_modules(rnn=True) on top."""
import numpy as np
import pytest
import torch

import packed_layer_cases as P
from test_hip_packed_layers import DEV, FLOAT_GUARD, Placed, fmt, place_weight
from quantized_distillation_amd import _infer_gru, _infer_mm, _lib, packed_layers

pytestmark = pytest.mark.gpu

# (input, hidden, bucket): two unit-tiles, the second with one unit, rows mid-word, both parts one ragged slab | a full and a ragged slab
# in each part, buckets straddling rows, 17 unit-tiles | several buckets inside a group of four | one unit, one bucket
SHAPES = ((37, 5, 256), (100, 67, 100), (5, 6, 3), (37, 1, None))
BATCHES = (1, 16, 17, 64, 65)


@pytest.fixture(scope='module')
def lib():
    return _infer_gru.load()


def wargs(wt, ptrs):
    f = fmt(wt, *ptrs)
    return f[:3] + f[5:]                                                  # packed, alpha, beta, bucket, levels, bits


def run(lib, wih, whh, h, x=None, pre=None, bias_ih=None, bias_hh=None, guarded=False):
    """One qdg_gru_cell_packed_f32 with the gates asked for; (h', gi, gh) as numpy.  guarded: every array between guard bands at a
    4-byte phase of its own, all of them read back."""
    batch, hidden = h.shape
    ins = {k: v for k, v in dict(x=x, pre=pre, h=h, bias_ih=bias_ih, bias_hh=bias_hh).items() if v is not None}
    sizes = dict(h_out=batch * hidden, gates=6 * batch * hidden)
    weights = [(k, w) for k, w in (('ih', wih), ('hh', whh)) if w is not None]
    if guarded:
        dev = {k: Placed(np.float32, v.size, 4 * (i % 4), 64, FLOAT_GUARD, v) for i, (k, v) in enumerate(ins.items())}
        dev.update({k: Placed(np.float32, n, 4 + 8 * i, 64, FLOAT_GUARD) for i, (k, n) in enumerate(sizes.items())})
        wts = {k: place_weight(w, phase=4 + 4 * i) for i, (k, w) in enumerate(weights)}
        ptr = {k: o.ptr for k, o in dev.items()}
        wptr = {k: [o.ptr for o in w3] for k, w3 in wts.items()}
    else:
        dev = {k: torch.from_numpy(np.array(v)).to(DEV) for k, v in ins.items()}
        dev.update({k: torch.full((n,), float('nan'), device=DEV) for k, n in sizes.items()})
        wts = {k: [torch.from_numpy(np.array(a)).to(DEV) for a in (w.packed, w.alpha, w.beta)] for k, w in weights}
        ptr = {k: t.data_ptr() for k, t in dev.items()}
        wptr = {k: [t.data_ptr() for t in w3] for k, w3 in wts.items()}
    with torch.cuda.device(DEV):
        rc = lib.qdg_gru_cell_packed_f32(*(wargs(wih, wptr['ih']) if wih is not None else (None, None, None, 0, 0, 0)), *wargs(whh, wptr['hh']),
                                         hidden, 0 if x is None else x.shape[1], ptr.get('x'), ptr.get('pre'), ptr['h'], batch,
                                         ptr.get('bias_ih'), ptr.get('bias_hh'), ptr['h_out'], ptr['gates'], _lib.stream_ptr(DEV))
        torch.cuda.synchronize()
    assert rc == 0, rc
    if guarded:
        for k, w3 in wts.items():
            for o, name in zip(w3, ('packed', 'alpha', 'beta')):
                o.read(k, name)
        got = {k: o.read('guarded', k) for k, o in dev.items()}         # inputs unchanged, outputs wholly written, nothing around any of them
    else:
        got = {k: dev[k].cpu().numpy() for k in sizes}
    gates = got['gates'].reshape(batch, 2, 3 * hidden)
    return got['h_out'].reshape(batch, hidden), gates[:, 0], gates[:, 1]


def problem(shape, bits, batch, seed, exact=False, nonfinite=False, scale=1.0):
    """(wih, whh, x, h, bias_ih, bias_hh) of one case."""
    inp, hid, bucket = shape
    if exact:
        wih, whh = P.exact_weight(3 * hid, inp, bucket, bits), P.exact_weight(3 * hid, hid, bucket, bits)
    else:
        wih, whh = P.general_weight(3 * hid, inp, bucket, 2 ** bits, bits), P.general_weight(3 * hid, hid, bucket, 2 ** bits, bits, nonfinite)
    (x, b_ih), (h, b_hh) = P.linear_inputs(inp, 3 * hid, batch, seed, exact), P.linear_inputs(hid, 3 * hid, batch, seed + 1, exact)
    return wih, whh, (x * scale).astype(np.float32), (h * scale).astype(np.float32), b_ih, b_hh


@pytest.mark.parametrize('bits', P.BITS)
def test_gates_within_the_bound(lib, bits):
    cases = [(sh, BATCHES[(k + bits) % 5], False) for k, sh in enumerate(SHAPES)] + [(SHAPES[1], 17, True)]
    for k, (shape, batch, nonfinite) in enumerate(cases):
        wih, whh, x, h, b_ih, b_hh = problem(shape, bits, batch, 700 + k + bits, nonfinite=nonfinite)
        b_ih, b_hh = (None if k % 3 == 1 else b_ih), (None if k % 3 == 2 else b_hh)
        gh64, gh_mag = P.linear_expected(whh.w, h, b_hh)                   # b_hn inside gh_n; bias_ih in gi, in cell mode only
        assert not nonfinite or (np.isnan(gh64).any() and np.isfinite(gh64).any())    # check_linear holds them in kind
        _, gi, gh = run(lib, wih, whh, h, x=x, bias_ih=b_ih, bias_hh=b_hh)
        ri = P.check_linear(gi, *P.linear_expected(wih.w, x, b_ih), (shape, batch, 'gi, cell mode'))
        rh = P.check_linear(gh, gh64, gh_mag, (shape, batch, 'gh, cell mode'))
        pre = (np.random.RandomState(bits + k).randn(batch, 3 * shape[1]) * 2).astype(np.float32)
        _, gi_pre, gh_pre = run(lib, None, whh, h, pre=pre, bias_hh=b_hh)
        assert gi_pre.tobytes() == pre.tobytes() and P.same_floats(gh_pre, gh), (shape, batch, 'pre mode: gi is pre, gh the same sum')
        print('%s batch %d bits %d: error / sum|terms| = %.3g (gi), %.3g (gh)' % (shape, batch, bits, ri, rh))


@pytest.mark.parametrize('bits', P.BITS)
def test_gates_bit_for_bit_on_exact_sums(lib, bits):
    for k, shape in enumerate(SHAPES):
        batch = BATCHES[(k + bits + 2) % 5]
        wih, whh, x, h, b_ih, b_hh = problem(shape, bits, batch, 800 + k + bits, exact=True)
        assert P.exact_condition(wih, x, b_ih) and P.exact_condition(whh, h, b_hh)
        _, gi, gh = run(lib, wih, whh, h, x=x, bias_ih=b_ih, bias_hh=b_hh)
        for got, (w, a, b) in ((gi, (wih, x, b_ih)), (gh, (whh, h, b_hh))):
            y64, _ = P.linear_expected(w.w, a, b)
            assert np.array_equal(got.view(np.uint32), y64.astype(np.float32).view(np.uint32)), (shape, batch)


@pytest.mark.parametrize('bits', P.BITS)
def test_the_epilogue_against_float64_on_its_own_gates(lib, bits):
    """Unit: 2^-24 (|h| + 1).  The fp32 reference formulas (numpy one operation at a time; torch.sigmoid / torch.tanh) both reach
    10.06 units against float64 on 2 10^6 Gaussian gates (sigma 3) and states (sigma 2) -- an error of r of half an ulp enters tanhf's
    argument times gh_n --; the bound is 4 x that: 40.2.  The kernel reaches 3.94 at the most over the eight widths."""
    wih, whh, x, h, b_ih, b_hh = problem(SHAPES[1], bits, 65, 900 + bits, scale=2.0)
    h_out, gi, gh = run(lib, wih, whh, h, x=x, bias_ih=b_ih, bias_hh=b_hh)
    a, b = gi.astype(np.float64).reshape(65, 3, -1), gh.astype(np.float64).reshape(65, 3, -1)
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))                               # noqa: E731
    z = sig(a[:, 1] + b[:, 1])
    h64 = (1.0 - z) * np.tanh(a[:, 2] + sig(a[:, 0] + b[:, 0]) * b[:, 2]) + z * h.astype(np.float64)
    hu = float((np.abs(h_out - h64) / (np.abs(h) + 1.0)).max() * 2.0 ** 24)
    print("bits %d: gates sigma %.2f, worst h' error %.2f x 2^-24 (|h| + 1)" % (bits, (a + b).std(), hu))
    assert (a + b).std() > 2.0 and hu <= 40.2, hu


@pytest.mark.parametrize('bits', P.BITS)
def test_a_batch_row_does_not_depend_on_the_batch_or_the_grid(lib, bits):
    wih, whh, x, h, b_ih, b_hh = problem(SHAPES[1], bits, 65, 1000 + bits)
    full = run(lib, wih, whh, h, x=x, bias_ih=b_ih, bias_hh=b_hh)
    for i in (0, 63, 64):
        one = run(lib, wih, whh, h[i:i + 1], x=x[i:i + 1], bias_ih=b_ih, bias_hh=b_hh)
        assert all(o.tobytes() == f[i:i + 1].tobytes() for o, f in zip(one, full)), 'row %d alone' % i
    assert lib.qdg_set_grid_cap(1) == 0
    try:
        capped = run(lib, wih, whh, h, x=x, bias_ih=b_ih, bias_hh=b_hh)
    finally:
        assert lib.qdg_set_grid_cap(0) == 1
    assert all(o.tobytes() == f.tobytes() for o, f in zip(capped, full)), 'one block for all 34 tiles'
    if bits in (3, 8):                                                     # between guard bands, both modes: 17 rows of (37, 5), 65 of (100, 67)
        wih, whh, x, h, b_ih, b_hh = problem(SHAPES[bits % 2], bits, 65 if bits % 2 else 17, 1100 + bits)
        plain = run(lib, wih, whh, h, x=x, bias_ih=b_ih, bias_hh=b_hh)
        guarded = run(lib, wih, whh, h, x=x, bias_ih=b_ih, bias_hh=b_hh, guarded=True)
        assert all(g.tobytes() == p.tobytes() for g, p in zip(guarded, plain)), 'no alignment changes a bit of the result'
        assert all(g.tobytes() == p.tobytes() for g, p in zip(run(lib, None, whh, h, pre=plain[1], guarded=True), run(lib, None, whh, h, pre=plain[1])))


def _steps(lib, pg, x, h0):
    """PackedGRU by hand at the C ABI: per layer and direction one qdm_linear_packed_f32 over all steps, then T pre-mode calls."""
    mm, st, dirs = _infer_mm.load(), _lib.stream_ptr(DEV), 2 if pg.bidirectional else 1
    T, batch, H = x.shape[0], x.shape[1], pg.hidden_size
    inp, h_n = x.contiguous(), torch.empty_like(h0)
    for layer in range(pg.num_layers):
        outs = []
        for d in range(dirs):
            cl = pg.cells[layer * dirs + d]
            pre, out = torch.empty(T, batch, 3 * H, device=DEV), torch.empty(T, batch, H, device=DEV)
            assert mm.qdm_linear_packed_f32(*cl.ih._format_args(), inp.data_ptr(), T * batch, cl.ih.bias.data_ptr(), pre.data_ptr(), st) == 0
            h = h0[layer * dirs + d]
            for t in (range(T - 1, -1, -1) if d else range(T)):
                assert lib.qdg_gru_cell_packed_f32(None, None, None, 0, 0, 0, cl.hh.packed.data_ptr(), cl.hh.alpha.data_ptr(), cl.hh.beta.data_ptr(),
                                                   cl.hh.bucket_size, cl.hh.s, cl.hh.bits, H, 0, None, pre[t].data_ptr(), h.data_ptr(), batch, None,
                                                   cl.hh.bias.data_ptr(), out[t].data_ptr(), None, st) == 0
                h = out[t]
            h_n[layer * dirs + d] = h
            outs.append(out)
        inp = torch.cat(outs, dim=2)
    return inp, h_n


@pytest.mark.parametrize('form', ('hx', 'no hx', 'batch_first', 'unbatched'))
def test_packed_gru_is_the_hand_written_sequence_and_agrees_with_float64_torch(lib, form):
    """Against torch's own float64 nn.GRU holding unpack()'s weights on the CPU (the gate order, where r multiplies); the tolerance is
    4 x the largest deviation of that module in fp32 on the CPU from the float64 one on the same inputs."""
    torch.manual_seed(3)
    gru = torch.nn.GRU(37, 5, num_layers=2, bidirectional=True, batch_first=form == 'batch_first').to(DEV)
    pg = packed_layers.PackedGRU.from_gru(gru, 16, bucket_size=64)
    x = torch.randn(3, 3, 37, device=DEV)
    h0 = torch.zeros(4, 3, 5, device=DEV) if form == 'no hx' else torch.randn(4, 3, 5, device=DEV)
    if form == 'unbatched':
        x, h0 = x[:, :1], h0[:, :1]
    xin = x.transpose(0, 1) if form == 'batch_first' else x[:, 0] if form == 'unbatched' else x
    hin = None if form == 'no hx' else h0[:, 0] if form == 'unbatched' else h0
    with torch.no_grad():
        out, h_n = pg(xin, hin)
        want = _steps(lib, pg, x, h0)
        got = (out.transpose(0, 1) if form == 'batch_first' else out.view(want[0].shape), h_n.view(want[1].shape))
        assert out.grad_fn is None and all(torch.equal(g.contiguous().view(torch.int32), w.view(torch.int32)) for g, w in zip(got, want))
        ref32 = pg.unpack().cpu()
        o32, hn32 = ref32(xin.cpu(), None if hin is None else hin.cpu())
        o64, hn64 = ref32.double()(xin.cpu().double(), None if hin is None else hin.cpu().double())
    tol = 4 * max(float((a.double() - b).abs().max()) for a, b in ((o32, o64), (hn32, hn64)))
    err = max(float((a.cpu().double() - b).abs().max()) for a, b in ((out, o64), (h_n, hn64)))
    print('%s: |PackedGRU - float64 nn.GRU| = %.3g, tolerance %.3g' % (form, err, tol))
    assert out.shape == o64.shape and h_n.shape == hn64.shape and err <= tol, (err, tol)


def test_packed_gru_cell_is_the_cell_mode_call(lib):
    wih, whh, x, h, b_ih, b_hh = problem(SHAPES[1], 3, 17, 1200)
    cell = torch.nn.GRUCell(100, 67).to(DEV)
    with torch.no_grad():
        for p, v in ((cell.weight_ih, wih.W), (cell.weight_hh, whh.W), (cell.bias_ih, b_ih), (cell.bias_hh, b_hh)):
            p.copy_(torch.from_numpy(np.array(v)))
    pc = packed_layers.PackedGRUCell.from_gru_cell(cell, 8, bucket_size=100, bits=3)
    xd, hd = (torch.from_numpy(np.array(v)).to(DEV) for v in (x, h))
    h1 = pc(xd, hd)
    assert h1.grad_fn is None and h1.cpu().numpy().tobytes() == run(lib, wih, whh, h, x=x, bias_ih=b_ih, bias_hh=b_hh)[0].tobytes()
    assert torch.equal(pc(xd), pc(xd, torch.zeros_like(hd))) and pc(xd[0], hd[0]).shape == (67,)      # no state: zeros; unbatched


def test_pack_modules_replaces_a_gru_and_a_gru_cell():
    nn = torch.nn
    torch.manual_seed(4)
    model = nn.ModuleDict(dict(enc=nn.GRU(12, 10, 2), cell=nn.GRUCell(12, 10), lin=nn.Linear(10, 7))).to(DEV)
    report = packed_layers.pack_modules(model, 16, rnn=True)
    assert isinstance(model['enc'], packed_layers.PackedGRU) and isinstance(model['cell'], packed_layers.PackedGRUCell)
    assert set(report) == {'enc', 'cell', 'lin'} and all(t.dim() < 2 for t in list(model.parameters()) + list(model.buffers()))
    assert report['cell'] == (4 * (30 * 12 + 30 * 10 + 60), model['cell'].nbytes) and report['enc'][1] == model['enc'].nbytes < report['enc'][0]
    x = torch.randn(5, 3, 12, device=DEV)
    with torch.no_grad():
        out, h_n = model['enc'](x)
        want, _ = model['enc'].unpack().double()(x.double())
    assert out.shape == want.shape and h_n.shape == (2, 3, 10) and float((out.double() - want).abs().max()) < 1e-5


def test_a_captured_cell_replays_on_new_inputs():
    torch.manual_seed(5)
    pc = packed_layers.PackedGRUCell.from_gru_cell(torch.nn.GRUCell(37, 5).to(DEV), 16, bucket_size=64)
    ins = [(torch.randn(17, 37, device=DEV), torch.randn(17, 5, device=DEV)) for _ in range(3)]
    eager = [pc(x, h) for x, h in ins]
    bufs = [t.clone() for t in ins[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                        # warm-up outside the capture
        pc(bufs[0], bufs[1])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        h1 = pc(bufs[0], bufs[1])
    torch.cuda.synchronize()
    for r in (1, 2, 0, 1):
        for b, t in zip(bufs, ins[r]):
            b.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(h1.view(torch.int32), eager[r].view(torch.int32)), r
