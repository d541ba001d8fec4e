"""An LSTM step from packed weights on the device (libqd_infer_rnn.so, include/qd_infer_rnn.h) at the C ABI: the pre-activations
against the float64 sums with the bit-exact weights of tests/packed_layer_cases.py, the epilogue against float64 on the call's own
gates, and PackedLSTMCell / PackedLSTM / pack_modules(rnn=True) on top."""
import numpy as np
import pytest
import torch

import packed_layer_cases as P
from test_hip_packed_layers import DEV, FLOAT_GUARD, Placed, fmt, place_weight
from quantized_distillation_amd import _infer_mm, _infer_rnn, _lib, packed_layers

pytestmark = pytest.mark.gpu

# (input, hidden, bucket): two unit-tiles, the second with one unit, rows mid-word, both parts one ragged slab | a full and a ragged slab
# in each part, buckets straddling rows, 17 tiles | several buckets inside a group of four | one unit, one bucket
SHAPES = ((37, 5, 256), (100, 67, 100), (5, 6, 3), (37, 1, None))
BATCHES = (1, 16, 17, 64, 65)


@pytest.fixture(scope='module')
def lib():
    return _infer_rnn.load()


def wargs(wt, ptrs):
    f = fmt(wt, *ptrs)
    return f[:3] + f[5:]                                                  # packed, alpha, beta, bucket, levels, bits


def run(lib, wih, whh, h, c, x=None, pre=None, bias_ih=None, bias_hh=None, guarded=False):
    """One qdr_lstm_cell_packed_f32 with c_out = c and the gates asked for; (h', c', gates) as numpy.  guarded: every array between
    guard bands at a 4-byte phase of its own, all of them read back."""
    batch, hidden = h.shape
    ins = {k: v for k, v in dict(x=x, pre=pre, h=h, c=c, bias_ih=bias_ih, bias_hh=bias_hh).items() if v is not None}
    sizes = dict(h_out=batch * hidden, gates=4 * batch * hidden)
    if guarded:
        dev = {k: Placed(np.float32, v.size, 4 * (i % 4), 64, FLOAT_GUARD, v) for i, (k, v) in enumerate(ins.items())}
        dev.update({k: Placed(np.float32, n, 4 + 8 * i, 64, FLOAT_GUARD) for i, (k, n) in enumerate(sizes.items())})
        dev['c'].is_input = False                                         # c_out: written in place
        wts = {k: place_weight(w, phase=ph) for k, w, ph in (('ih', wih, 4), ('hh', whh, 8)) if w is not None}
        ptr = {k: o.ptr for k, o in dev.items()}
        wptr = {k: [o.ptr for o in w3] for k, w3 in wts.items()}
    else:
        dev = {k: torch.from_numpy(np.array(v)).to(DEV) for k, v in ins.items()}
        dev.update({k: torch.full((n,), float('nan'), device=DEV) for k, n in sizes.items()})
        wts = {k: [torch.from_numpy(np.array(a)).to(DEV) for a in (w.packed, w.alpha, w.beta)] for k, w in (('ih', wih), ('hh', whh)) if w is not None}
        ptr = {k: t.data_ptr() for k, t in dev.items()}
        wptr = {k: [t.data_ptr() for t in w3] for k, w3 in wts.items()}
    with torch.cuda.device(DEV):
        rc = lib.qdr_lstm_cell_packed_f32(*(wargs(wih, wptr['ih']) if wih is not None else (None, None, None, 0, 0, 0)), *wargs(whh, wptr['hh']),
                                          hidden, 0 if x is None else x.shape[1], ptr.get('x'), ptr.get('pre'), ptr['h'], ptr['c'], batch,
                                          ptr.get('bias_ih'), ptr.get('bias_hh'), ptr['h_out'], ptr['c'], ptr['gates'], _lib.stream_ptr(DEV))
        torch.cuda.synchronize()
    assert rc == 0, rc
    if guarded:
        for k, w3 in wts.items():
            for o, name in zip(w3, ('packed', 'alpha', 'beta')):
                o.read(k, name)
        got = {k: o.read('guarded', k) for k, o in dev.items()}         # inputs unchanged, outputs wholly written, nothing around any of them
    else:
        got = {k: dev[k].cpu().numpy() for k in ('h_out', 'c', 'gates')}
    return got['h_out'].reshape(batch, hidden), got['c'].reshape(batch, hidden), got['gates'].reshape(batch, 4 * hidden)


def problem(shape, bits, batch, seed, exact=False, nonfinite=False, scale=1.0):
    """(wih, whh, x, h, c, bias_ih, bias_hh) of one case."""
    inp, hid, bucket = shape
    if exact:
        wih, whh = P.exact_weight(4 * hid, inp, bucket, bits), P.exact_weight(4 * hid, hid, bucket, bits)
    else:
        wih, whh = P.general_weight(4 * hid, inp, bucket, 2 ** bits, bits), P.general_weight(4 * hid, hid, bucket, 2 ** bits, bits, nonfinite)
    (x, b_ih), (h, b_hh) = P.linear_inputs(inp, 4 * hid, batch, seed, exact), P.linear_inputs(hid, 4 * hid, batch, seed + 1, exact)
    c = (np.random.RandomState(seed).randn(batch, hid) * 2).astype(np.float32)     # sigma 2: tanhf(c') leaves its linear range
    return wih, whh, (x * scale).astype(np.float32), (h * scale).astype(np.float32), c, b_ih, b_hh


def expected_gates(wih, whh, x, h, b_ih, b_hh, pre=None):
    y, mag = P.linear_expected(whh.w, h, b_hh)
    y2, mag2 = (pre.astype(np.float64), np.abs(pre.astype(np.float64))) if pre is not None else P.linear_expected(wih.w, x, b_ih)
    with np.errstate(invalid='ignore'):
        return y + y2, mag + mag2


@pytest.mark.parametrize('bits', P.BITS)
def test_gates_within_the_bound(lib, bits):
    cases = [(sh, BATCHES[(k + bits) % 5], False) for k, sh in enumerate(SHAPES)] + [(SHAPES[1], 17, True)]
    for k, (shape, batch, nonfinite) in enumerate(cases):
        wih, whh, x, h, c, b_ih, b_hh = problem(shape, bits, batch, 700 + k + bits, nonfinite=nonfinite)
        b_ih, b_hh = (None if k % 3 == 1 else b_ih), (None if k % 3 == 2 else b_hh)
        y64, mag = expected_gates(wih, whh, x, h, b_ih, b_hh)
        assert not nonfinite or (np.isnan(y64).any() and np.isfinite(y64).any())      # check_linear holds them in kind
        _, _, gates = run(lib, wih, whh, h, c, x=x, bias_ih=b_ih, bias_hh=b_hh)
        ratio = P.check_linear(gates, y64, mag, (shape, batch, 'cell mode'))
        pre = (np.random.RandomState(bits + k).randn(batch, 4 * shape[1]) * 2).astype(np.float32)
        _, _, gates = run(lib, None, whh, h, c, pre=pre, bias_hh=b_hh)
        ratio_pre = P.check_linear(gates, *expected_gates(None, whh, None, h, None, b_hh, pre), (shape, batch, 'pre mode'))
        print('%s batch %d bits %d: error / sum|terms| = %.3g (cell mode), %.3g (pre mode)' % (shape, batch, bits, ratio, ratio_pre))


@pytest.mark.parametrize('bits', P.BITS)
def test_gates_bit_for_bit_on_exact_sums(lib, bits):
    for k, shape in enumerate(SHAPES):
        batch = BATCHES[(k + bits + 2) % 5]
        wih, whh, x, h, c, b_ih, b_hh = problem(shape, bits, batch, 800 + k + bits, exact=True)
        both = wih._replace(w=np.concatenate([wih.w, whh.w], axis=1), tag=wih.tag + ' | ' + whh.tag)
        assert P.exact_condition(both, np.concatenate([x, h], axis=1), np.abs(b_ih) + np.abs(b_hh))
        y64, _ = expected_gates(wih, whh, x, h, b_ih, b_hh)
        _, _, gates = run(lib, wih, whh, h, c, x=x, bias_ih=b_ih, bias_hh=b_hh)
        assert np.array_equal(gates.view(np.uint32), y64.astype(np.float32).view(np.uint32)), (shape, batch)


@pytest.mark.parametrize('bits', P.BITS)
def test_the_epilogue_against_float64_on_its_own_gates(lib, bits):
    """Units: 2^-24 (|c| + 1) for c', 2^-24 for h'.  The fp32 reference formulas (numpy, torch.sigmoid / torch.tanh) reach 2.88 and
    4.10 of them against float64 on 2 10^6 Gaussian gates (sigma 3) and cells (sigma 2); the bound is 4 x that: 11.5 and 16.4."""
    wih, whh, x, h, c, b_ih, b_hh = problem(SHAPES[1], bits, 65, 900 + bits, scale=2.0)
    h_out, c_out, gates = run(lib, wih, whh, h, c, x=x, bias_ih=b_ih, bias_hh=b_hh)
    a = gates.astype(np.float64).reshape(65, 4, -1)
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))                               # noqa: E731
    c64 = sig(a[:, 1]) * c.astype(np.float64) + sig(a[:, 0]) * np.tanh(a[:, 2])
    h64 = sig(a[:, 3]) * np.tanh(c64)
    cu = float((np.abs(c_out - c64) / (np.abs(c) + 1.0)).max() * 2.0 ** 24)
    hu = float(np.abs(h_out - h64).max() * 2.0 ** 24)
    print('bits %d: gates sigma %.2f, worst c\' error %.2f x 2^-24 (|c| + 1), worst h\' error %.2f x 2^-24' % (bits, a.std(), cu, hu))
    assert a.std() > 2.0 and cu <= 11.5 and hu <= 16.4, (cu, hu)


@pytest.mark.parametrize('bits', P.BITS)
def test_a_batch_row_does_not_depend_on_the_batch_or_the_grid(lib, bits):
    wih, whh, x, h, c, b_ih, b_hh = problem(SHAPES[1], bits, 65, 1000 + bits)
    full = run(lib, wih, whh, h, c, x=x, bias_ih=b_ih, bias_hh=b_hh)
    for i in (0, 63, 64):
        one = run(lib, wih, whh, h[i:i + 1], c[i:i + 1], x=x[i:i + 1], bias_ih=b_ih, bias_hh=b_hh)
        assert all(o.tobytes() == f[i:i + 1].tobytes() for o, f in zip(one, full)), 'row %d alone' % i
    assert lib.qdr_set_grid_cap(1) == 0
    try:
        capped = run(lib, wih, whh, h, c, x=x, bias_ih=b_ih, bias_hh=b_hh)
    finally:
        assert lib.qdr_set_grid_cap(0) == 1
    assert all(o.tobytes() == f.tobytes() for o, f in zip(capped, full)), 'one block for all 34 tiles'


@pytest.mark.parametrize('bits', P.BITS)
def test_reads_and_writes_stay_inside_their_arrays(lib, bits):
    wih, whh, x, h, c, b_ih, b_hh = problem(SHAPES[bits % 2], bits, 65 if bits % 2 else 17, 1100 + bits)
    plain = run(lib, wih, whh, h, c, x=x, bias_ih=b_ih, bias_hh=b_hh)
    guarded = run(lib, wih, whh, h, c, x=x, bias_ih=b_ih, bias_hh=b_hh, guarded=True)
    assert all(g.tobytes() == p.tobytes() for g, p in zip(guarded, plain)), 'no alignment changes a bit of the result'
    pre = plain[2]                                                         # pre mode between guard bands too
    assert all(g.tobytes() == p.tobytes() for g, p in zip(run(lib, None, whh, h, c, pre=pre, guarded=True), run(lib, None, whh, h, c, pre=pre)))


def _steps(lib, pl, x, h0, c0):
    """PackedLSTM by hand at the C ABI: per layer and direction one qdm_linear_packed_f32 over all steps, then T pre-mode calls."""
    mm, st, dirs = _infer_mm.load(), _lib.stream_ptr(DEV), 2 if pl.bidirectional else 1
    T, batch, H = x.shape[0], x.shape[1], pl.hidden_size
    inp, h_n, c_n = x.contiguous(), torch.empty_like(h0), c0.clone()
    for layer in range(pl.num_layers):
        outs = []
        for d in range(dirs):
            cl = pl.cells[layer * dirs + d]
            pre, out = torch.empty(T, batch, 4 * H, device=DEV), torch.empty(T, batch, H, device=DEV)
            assert mm.qdm_linear_packed_f32(*cl.ih._format_args(), inp.data_ptr(), T * batch, cl.ih.bias.data_ptr(), pre.data_ptr(), st) == 0
            h, c = h0[layer * dirs + d], c_n[layer * dirs + d]
            for t in (range(T - 1, -1, -1) if d else range(T)):
                assert lib.qdr_lstm_cell_packed_f32(None, None, None, 0, 0, 0, cl.hh.packed.data_ptr(), cl.hh.alpha.data_ptr(), cl.hh.beta.data_ptr(),
                                                    cl.hh.bucket_size, cl.hh.s, cl.hh.bits, H, 0, None, pre[t].data_ptr(), h.data_ptr(), c.data_ptr(),
                                                    batch, None, cl.hh.bias.data_ptr(), out[t].data_ptr(), c.data_ptr(), None, st) == 0
                h = out[t]
            h_n[layer * dirs + d] = h
            outs.append(out)
        inp = torch.cat(outs, dim=2)
    return inp, h_n, c_n


@pytest.mark.parametrize('bidirectional, batch_first', ((True, False), (False, True)))
def test_packed_lstm_is_the_hand_written_sequence_and_agrees_with_float64(lib, bidirectional, batch_first):
    torch.manual_seed(3)
    lstm = torch.nn.LSTM(11, 6, num_layers=2, bidirectional=bidirectional, batch_first=batch_first).to(DEV)
    pl = packed_layers.PackedLSTM.from_lstm(lstm, 16, bucket_size=64)
    x, dirs = torch.randn(3, 17, 11, device=DEV), 2 if bidirectional else 1
    h0, c0 = torch.randn(2 * dirs, 17, 6, device=DEV), torch.randn(2 * dirs, 17, 6, device=DEV) * 2
    with torch.no_grad():
        out, (h_n, c_n) = pl(x.transpose(0, 1) if batch_first else x, (h0, c0))
        want = _steps(lib, pl, x, h0, c0)
        got = (out.transpose(0, 1) if batch_first else out, h_n, c_n)
        assert out.grad_fn is None and all(torch.equal(g.contiguous().view(torch.int32), w.view(torch.int32)) for g, w in zip(got, want))
        ref32 = pl.unpack().cpu()
        xin = (x.transpose(0, 1) if batch_first else x).cpu()
        o32, (hn32, cn32) = ref32(xin, (h0.cpu(), c0.cpu()))
        o64, (hn64, cn64) = ref32.double()(xin.double(), (h0.cpu().double(), c0.cpu().double()))
    assert max(float((a.double() - b).abs().max()) for a, b in ((o32, o64), (hn32, hn64), (cn32, cn64))) < 1e-6      # torch's own fp32 at this shape
    assert out.shape == o64.shape and max(float((a.cpu().double() - b).abs().max()) for a, b in ((out, o64), (h_n, hn64), (c_n, cn64))) < 1e-5


def test_packed_lstm_cell_is_the_cell_mode_call(lib):
    wih, whh, x, h, c, b_ih, b_hh = problem(SHAPES[1], 3, 17, 1200)
    cell = torch.nn.LSTMCell(100, 67).to(DEV)
    with torch.no_grad():
        for p, v in ((cell.weight_ih, wih.W), (cell.weight_hh, whh.W), (cell.bias_ih, b_ih), (cell.bias_hh, b_hh)):
            p.copy_(torch.from_numpy(np.array(v)))
    pc = packed_layers.PackedLSTMCell.from_lstm_cell(cell, 8, bucket_size=100, bits=3)
    xd, hd, cd = (torch.from_numpy(np.array(v)).to(DEV) for v in (x, h, c))
    h1, c1 = pc(xd, (hd, cd))
    want_h, want_c, _ = run(lib, wih, whh, h, c, x=x, bias_ih=b_ih, bias_hh=b_hh)
    assert h1.grad_fn is None and h1.cpu().numpy().tobytes() == want_h.tobytes() and c1.cpu().numpy().tobytes() == want_c.tobytes()
    with torch.no_grad():
        h64, c64 = pc.unpack().cpu().double()(xd.cpu().double(), (hd.cpu().double(), cd.cpu().double()))
    assert float((h1.cpu().double() - h64).abs().max()) < 1e-5 and float((c1.cpu().double() - c64).abs().max()) < 1e-5
    z = pc(xd)                                                            # no state: zeros
    assert torch.equal(z[0], pc(xd, (torch.zeros_like(hd), torch.zeros_like(cd)))[0])


def test_a_seq2seq_model_runs_with_no_fp32_weight_matrix_left():
    from harness.models import Seq2SeqLSTM
    nn = torch.nn
    torch.manual_seed(4)
    model = Seq2SeqLSTM(v_src=50, v_tgt=40, emb=12, hidden=10).to(DEV).eval()
    report = packed_layers.pack_modules(model, 16, rnn=True)
    assert not any(isinstance(m, (nn.LSTM, nn.LSTMCell, nn.Linear, nn.Embedding)) for m in model.modules())
    assert {'encoder', 'dec_cells.0', 'dec_cells.1'} <= set(report) and all(t.dim() < 2 for t in list(model.parameters()) + list(model.buffers()))
    ref = Seq2SeqLSTM(v_src=50, v_tgt=40, emb=12, hidden=10)
    for name in ('src_emb', 'tgt_emb', 'encoder', 'attn_in', 'attn_out', 'generator'):
        setattr(ref, name, getattr(model, name).unpack())
    ref.dec_cells = nn.ModuleList([cl.unpack() for cl in model.dec_cells])
    src, tgt = torch.randint(0, 50, (7, 17), device=DEV), torch.randint(0, 40, (5, 17), device=DEV)
    with torch.no_grad():
        logits, want = model(src, tgt), ref.to(DEV).double()(src, tgt)
    assert logits.shape == (5 * 17, 40) and float((logits.double() - want).abs().max()) < 1e-5


def test_a_captured_cell_replays_on_new_inputs():
    torch.manual_seed(5)
    pc = packed_layers.PackedLSTMCell.from_lstm_cell(torch.nn.LSTMCell(37, 5).to(DEV), 16, bucket_size=64)
    ins = [(torch.randn(17, 37, device=DEV), torch.randn(17, 5, device=DEV), torch.randn(17, 5, device=DEV) * 2) for _ in range(3)]
    eager = [pc(x, (h, c)) for x, h, c in ins]
    bufs = [t.clone() for t in ins[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                        # warm-up outside the capture
        pc(bufs[0], (bufs[1], bufs[2]))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        h1, c1 = pc(bufs[0], (bufs[1], bufs[2]))
    torch.cuda.synchronize()
    for r in (1, 2, 0, 1):
        for b, t in zip(bufs, ins[r]):
            b.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(h1.view(torch.int32), eager[r][0].view(torch.int32)) and torch.equal(c1.view(torch.int32), eager[r][1].view(torch.int32)), r
