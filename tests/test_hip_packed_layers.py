"""Linear and Embedding from packed weights on the device (libqd_infer.so, include/qd_infer.h;
quantized_distillation_amd/packed_layers.py) against tests/packed_layer_cases.py.

At the C ABI every case runs between guard bands with sentinel-filled outputs: `packed` sits between bands of 0xFF bytes more
than one row wide (a kernel that reads another row's worth past the stream still reads its own allocation, and shows it in
the result), x, y and out at every 4-byte phase of a 16-byte granule.  The packed stream is built twice -- by the numpy
reference and by codec.pack_uniform on the device -- and must be the same bytes.  Embedding: bit for bit.  Linear: bit for bit
on the exact cases, within 1e-6 of sum |terms| on the general ones (tests/errlog.py records the achieved ratio)."""
import numpy as np
import pytest
import torch

import errlog
import packed_layer_cases as P
from quantized_distillation_amd import _infer, _lib, codec, packed_layers

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
F_SENT = 0x7FC5A5A5                  # abi_contract.F_SENT: a quiet NaN with a payload no arithmetic produces
FLOAT_GUARD = np.array([np.nan, 3e38, np.nan, -3e38], np.float32)


@pytest.fixture(scope='module')
def lib():
    return _infer.load()


class Placed(object):
    """One array in a flat device buffer of its own: `guard` bytes (at least) in front of and behind it, tiled with
    `pattern`; the payload `phase` bytes into a 16-byte granule.  data None: an output, pre-filled with the sentinel."""

    def __init__(self, dtype, n, phase, guard, pattern, data=None):
        self.dtype = np.dtype(dtype)
        isz = self.dtype.itemsize
        self.nbytes = n * isz
        total = guard + 32 + self.nbytes + guard + 16
        self.buf = torch.empty(total, dtype=torch.uint8, device=DEV)
        base = self.buf.data_ptr()
        self.off = guard + (-(base + guard)) % 16 + phase
        assert (base + self.off - phase) % 16 == 0 and self.off >= guard and total - self.off - self.nbytes >= guard
        pat = np.asarray(pattern, self.dtype)
        img = np.full(total, 0xEE, np.uint8)
        s = self.off % isz
        cnt = (total - s) // isz
        img[s:s + cnt * isz] = pat[(np.arange(cnt) - (self.off - s) // isz) % len(pat)].view(np.uint8)
        if data is not None:
            img[self.off:self.off + self.nbytes] = np.ascontiguousarray(data, self.dtype).reshape(-1).view(np.uint8)
        elif self.dtype == np.float32:
            img[self.off:self.off + self.nbytes] = np.full(n, F_SENT, np.uint32).view(np.uint8)
        self.is_input = data is not None
        self.image = img
        self.buf.copy_(torch.from_numpy(img.copy()))
        self.ptr = base + self.off

    def read(self, tag, name):
        got = self.buf.cpu().numpy()
        lo, hi = self.off, self.off + self.nbytes
        assert np.array_equal(got[:lo], self.image[:lo]), (tag, name, 'written in front of the array')
        assert np.array_equal(got[hi:], self.image[hi:]), (tag, name, 'written behind the array')
        payload = got[lo:hi].copy().view(self.dtype)
        if self.is_input:
            assert np.array_equal(got[lo:hi], self.image[lo:hi]), (tag, name, 'an input was written over')
        else:
            left = payload.view(np.uint32) == F_SENT
            assert not left.any(), (tag, name, '%d elements never written, first at %d' % (left.sum(), np.nonzero(left)[0][0] if left.any() else -1))
        return payload


def place_weight(wt, phase=0):
    """packed between bands more than one row wide (0xFF: level indices no case holds everywhere), alpha and beta between
    NaN / +-3e38."""
    row_bytes = (wt.cols * wt.bits + 7) // 8
    return (Placed(np.uint8, wt.packed.size, phase, 64 + 16 * ((row_bytes + 15) // 16), [0xFF], wt.packed),
            Placed(np.float32, wt.alpha.size, 8, 64, FLOAT_GUARD, wt.alpha), Placed(np.float32, wt.beta.size, 4, 64, FLOAT_GUARD, wt.beta))


def fmt(wt, packed, alpha, beta):
    return (packed, alpha, beta, wt.rows, wt.cols, 0 if wt.bucket is None else wt.bucket, wt.s, wt.bits)


def run_embedding(lib, c, weight_ptrs, tag):
    wt = c.weight
    _, _, idx = P.inputs_of(c)
    pidx = Placed(np.int64, idx.size, 8 if c.phase in (4, 12) else 0, 64, [0], idx)           # the guard: a valid index
    pout = Placed(np.float32, idx.size * wt.cols, c.phase, 64, FLOAT_GUARD)
    with torch.cuda.device(DEV):
        rc = lib.qdi_embedding_packed_f32(*fmt(wt, *weight_ptrs), pidx.ptr, idx.size, pout.ptr, _lib.stream_ptr(DEV))
        torch.cuda.synchronize()
    assert rc == 0, (tag, rc)
    pidx.read(tag, 'idx')
    return pout.read(tag, 'out')


def run_linear(lib, c, weight_ptrs, tag):
    wt = c.weight
    x, bias, _ = P.inputs_of(c)
    px = Placed(np.float32, x.size, c.phase, 64, FLOAT_GUARD, x)
    pb = None if bias is None else Placed(np.float32, bias.size, 12, 64, FLOAT_GUARD, bias)
    py = Placed(np.float32, c.m * wt.rows, (c.phase + 4) % 16, 64, FLOAT_GUARD)
    with torch.cuda.device(DEV):
        rc = lib.qdi_linear_packed_f32(*fmt(wt, *weight_ptrs), px.ptr, c.m, None if pb is None else pb.ptr, py.ptr, _lib.stream_ptr(DEV))
        torch.cuda.synchronize()
    assert rc == 0, (tag, rc)
    px.read(tag, 'x')
    if pb is not None:
        pb.read(tag, 'bias')
    return py.read(tag, 'y').reshape(c.m, wt.rows)


def check_outputs(c, out, y, tag, record=True):
    wt = c.weight
    x, bias, idx = P.inputs_of(c)
    assert P.same_floats(out, P.embedding_expected(wt.w, idx)), (tag, 'embedding')
    y64, mag = P.linear_expected(wt.w, x, bias)
    if c.exact:
        assert np.array_equal(y.view(np.uint32), y64.astype(np.float32).view(np.uint32)), (tag, 'linear, exact case')
        return 0.0
    return P.check_linear(y, y64, mag, tag, errlog.check_sum if record else None)


def device_pack(wt):
    """codec.pack_uniform of the case's weight on the device: the same bytes as the numpy reference of the stream."""
    pk = codec.pack_uniform(torch.from_numpy(np.array(wt.W)).to(DEV), wt.s, wt.bucket, wt.bits)
    assert np.array_equal(pk.packed.cpu().numpy(), wt.packed), (wt.tag, 'the device packs other bytes than the reference')
    assert P.same_floats(pk.alpha.cpu().numpy(), wt.alpha) and P.same_floats(pk.beta.cpu().numpy(), wt.beta), wt.tag
    return pk


# ---------------------------------------------------------------- 1. every case at the C ABI
@pytest.mark.parametrize('bits', P.BITS)
def test_every_case_at_the_c_abi(lib, bits):
    worst = 0.0
    for i, c in enumerate(P.all_cases(bits)):
        wt = c.weight
        tag = (wt.tag, 'm %d count %d phase %d' % (c.m, c.count, c.phase))
        placed = place_weight(wt, phase=(0, 4, 8, 12)[i % 4])
        ptrs = tuple(p.ptr for p in placed)
        out, y = run_embedding(lib, c, ptrs, tag), run_linear(lib, c, ptrs, tag)
        for p, name in zip(placed, ('packed', 'alpha', 'beta')):
            p.read(tag, name)
        worst = max(worst, check_outputs(c, out, y, tag))
        # the stream the device packs is the same bytes, and the layers give the same bits from it
        pk = device_pack(wt)
        dptrs = (pk.packed.data_ptr(), pk.alpha.data_ptr(), pk.beta.data_ptr())
        assert run_embedding(lib, c, dptrs, tag).tobytes() == out.tobytes(), tag
        assert run_linear(lib, c, dptrs, tag).tobytes() == y.tobytes(), (tag, 'the same call gives other bits')
    assert worst < P.TOL


@pytest.mark.parametrize('bits', (1, 3, 4, 8))
def test_under_a_grid_cap(lib, bits):
    """1, 2 and 3 blocks: the later trips of the row loop and of the embedding's group loop.  Embedding gives the uncapped bits;
    Linear stays within the bound, gives the exact cases' bits -- and, its order being free of the grid, the uncapped bits."""
    picks = [c for c in P.all_cases(bits) if (c.weight.rows, c.weight.cols) in ((67, 37), (67, 100), (3, 2085))]
    assert any(c.exact for c in picks) and any(not c.exact for c in picks)
    for c in picks:
        tag = (c.weight.tag, 'grid cap')
        placed = place_weight(c.weight)                          # (kept alive: the pointers below are into its buffers)
        ptrs = tuple(p.ptr for p in placed)
        base_out, base_y = run_embedding(lib, c, ptrs, tag), run_linear(lib, c, ptrs, tag)
        for cap in (1, 2, 3):
            assert lib.qdi_set_grid_cap(cap) == 0
            try:
                out, y = run_embedding(lib, c, ptrs, tag + (cap,)), run_linear(lib, c, ptrs, tag + (cap,))
            finally:
                assert lib.qdi_set_grid_cap(0) == cap
            check_outputs(c, out, y, tag + (cap,), record=False)
            assert out.tobytes() == base_out.tobytes() and y.tobytes() == base_y.tobytes(), tag + (cap,)


def test_refusals_write_nothing(lib):
    c = P.general_cases(4)[0]
    wt = c.weight
    packed, alpha, beta = place_weight(wt)
    x, bias, idx = P.inputs_of(c)
    px, pidx = Placed(np.float32, x.size, 0, 64, FLOAT_GUARD, x), Placed(np.int64, idx.size, 0, 64, [0], idx)
    py, pout = Placed(np.float32, c.m * wt.rows, 0, 64, FLOAT_GUARD), Placed(np.float32, idx.size * wt.cols, 0, 64, FLOAT_GUARD)
    st = _lib.stream_ptr(DEV)
    good = fmt(wt, packed.ptr, alpha.ptr, beta.ptr)
    for bad in ((packed.ptr + 2,) + good[1:], good[:5] + (-1,) + good[6:], good[:6] + (257, 8), good[:6] + (17, 4), good[:6] + (16, 9),
                (None,) + good[1:]):
        assert lib.qdi_embedding_packed_f32(*bad, pidx.ptr, idx.size, pout.ptr, st) == -1
        assert lib.qdi_linear_packed_f32(*bad, px.ptr, c.m, None, py.ptr, st) == -1
    assert lib.qdi_linear_packed_f32(*good, px.ptr + 2, c.m, None, py.ptr, st) == -1
    assert lib.qdi_embedding_packed_f32(*good, pidx.ptr + 4, idx.size, pout.ptr, st) == -1
    assert lib.qdi_embedding_packed_f32(*good, pidx.ptr, 0, pout.ptr, st) == 0 and lib.qdi_linear_packed_f32(*good, px.ptr, 0, None, py.ptr, st) == 0
    torch.cuda.synchronize()
    for p in (py, pout):
        got = p.buf.cpu().numpy()
        assert np.array_equal(got, p.image), 'a refused or an empty call wrote'


# ---------------------------------------------------------------- 2. the modules
def _bound_check(y, x, w, bias, tag):
    """PackedLinear's output against x.double() @ unpack().double().T within the bound."""
    x2 = x.reshape(-1, x.shape[-1]).double()
    y64 = x2 @ w.double().T
    mag = x2.abs() @ w.double().abs().T
    if bias is not None:
        y64, mag = y64 + bias.double(), mag + bias.double().abs()
    return P.check_linear(y.reshape(y64.shape).cpu().numpy(), y64.cpu().numpy(), mag.cpu().numpy(), tag, errlog.check_sum)


@pytest.mark.parametrize('s,bits,bucket', ((16, None, 256), (5, None, 100), (2, None, None), (200, 8, 64), (8, 4, 3)))
def test_modules_against_unpack(s, bits, bucket):
    g = torch.Generator().manual_seed(s)
    lin = torch.nn.Linear(100, 67).to(DEV)
    emb = torch.nn.Embedding(67, 37).to(DEV)
    pl = packed_layers.PackedLinear.from_linear(lin, s, bucket, bits)
    pe = packed_layers.PackedEmbedding.from_embedding(emb, s, bucket, bits)
    want_bits = codec.min_bits_for_levels(s) if bits is None else bits
    assert pl.bits == pe.bits == want_bits and pl.packed.numel() == (67 * 100 * want_bits + 7) // 8
    nb = 1 if bucket is None else -(-6700 // bucket)
    assert pl.nbytes == pl.packed.numel() + 8 * nb + 4 * 67 and pl.fp32_nbytes == 4 * 6700 + 4 * 67
    pk = codec.pack_uniform(emb.weight.detach(), s, bucket, want_bits)
    w_emb, w_lin = pk.unpack(), pl.as_packed_uniform().unpack()
    idx = torch.randint(0, 67, (3, 5, 7), generator=g).to(DEV)
    out = pe(idx)
    assert out.shape == (3, 5, 7, 37) and out.grad_fn is None and torch.equal(out.view(torch.int32), w_emb[idx].view(torch.int32))
    assert torch.equal(pe(idx).view(torch.int32), out.view(torch.int32))
    un = pe.unpack()
    assert isinstance(un, torch.nn.Embedding) and torch.equal(un.weight.detach().view(torch.int32), w_emb.view(torch.int32))
    for shape in ((100,), (1, 100), (9, 100), (2, 3, 100)):
        x = torch.randn(*shape, generator=g).to(DEV)
        y = pl(x)
        assert y.shape == shape[:-1] + (67,) and y.grad_fn is None and not y.requires_grad
        _bound_check(y, x, w_lin, lin.bias.detach(), (s, bits, bucket, shape))
        assert torch.equal(pl(x).view(torch.int32), y.view(torch.int32)), 'the same call gives the same bits'
    xt = torch.randn(100, 4, generator=g).to(DEV).t()                                   # not contiguous: made so
    assert not xt.is_contiguous() and torch.equal(pl(xt).view(torch.int32), pl(xt.contiguous()).view(torch.int32))
    ul = pl.unpack()
    assert isinstance(ul, torch.nn.Linear) and torch.equal(ul.weight.detach().view(torch.int32), w_lin.view(torch.int32))
    assert torch.equal(ul.bias.detach(), lin.bias.detach())
    assert pe(torch.empty(0, dtype=torch.int64, device=DEV)).shape == (0, 37) and pl(torch.empty(0, 100, device=DEV)).shape == (0, 67)


def test_inference_only_and_buffers_move():
    lin = torch.nn.Linear(37, 5, bias=False).to(DEV)
    pl = packed_layers.PackedLinear.from_linear(lin, 16)
    x = torch.randn(4, 37, device=DEV)
    with pytest.raises(RuntimeError, match=r'unpack\(\)'):
        pl(x.clone().requires_grad_())
    with torch.no_grad():
        y = pl(x.clone().requires_grad_())
    assert y.grad_fn is None and not y.requires_grad and pl.bias is None and pl.nbytes == pl.as_packed_uniform().nbytes
    moved = pl.cpu()
    assert not moved.packed.is_cuda
    with pytest.raises(NotImplementedError, match='HIP device only'):
        moved(x.cpu())
    back = moved.to(DEV)
    assert torch.equal(back(x).view(torch.int32), y.view(torch.int32))
    with pytest.raises(NotImplementedError, match='HIP device only'):
        back(x.cpu())
    # an index out of range gives a row of NaN; nothing else changes
    pe = packed_layers.PackedEmbedding.from_embedding(torch.nn.Embedding(5, 6).to(DEV), 4)
    out = pe(torch.tensor([0, -1, 5, 4], device=DEV))
    assert torch.isnan(out[1:3]).all() and torch.isfinite(out[0]).all() and torch.isfinite(out[3]).all()


def test_one_capture_of_both_modules_replayed_on_new_inputs():
    g = torch.Generator().manual_seed(3)
    pl = packed_layers.PackedLinear.from_linear(torch.nn.Linear(100, 67).to(DEV), 8, 256, 3)
    pe = packed_layers.PackedEmbedding.from_embedding(torch.nn.Embedding(67, 37).to(DEV), 32, 100, 5)
    xs = [torch.randn(9, 100, generator=g).to(DEV) for _ in range(3)]
    idxs = [torch.randint(0, 67, (300,), generator=g).to(DEV) for _ in range(3)]
    eager = [(pl(x).clone(), pe(i).clone()) for x, i in zip(xs, idxs)]
    x_buf, i_buf = xs[0].clone(), idxs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # warm-up outside the capture
        pl(x_buf), pe(i_buf)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                   # one chain on one stream: Linear, then Embedding
        y, out = pl(x_buf), pe(i_buf)
    torch.cuda.synchronize()
    for r in (1, 2, 0):
        x_buf.copy_(xs[r]), i_buf.copy_(idxs[r])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int32), eager[r][0].view(torch.int32)), 'replay %d, linear' % r
        assert torch.equal(out.view(torch.int32), eager[r][1].view(torch.int32)), 'replay %d, embedding' % r


def test_pack_modules_on_the_seq2seq_student():
    from harness.models import Seq2SeqLSTM
    torch.manual_seed(0)
    model = Seq2SeqLSTM(v_src=50, v_tgt=50, emb=16, hidden=32).to(DEV).eval()
    before = {n: m for n, m in model.named_modules() if isinstance(m, (torch.nn.Linear, torch.nn.Embedding))}
    assert sorted(before) == ['attn_in', 'attn_out', 'generator', 'src_emb', 'tgt_emb']
    weights = {n: m.weight.detach().clone() for n, m in before.items()}
    src, tgt = torch.randint(0, 50, (7, 3), device=DEV), torch.randint(0, 50, (5, 3), device=DEV)
    with torch.no_grad():
        ref_shape = model(src, tgt).shape
    s = {'src_emb': 16, 'tgt_emb': 5, 'generator': 4, 'attn_in': 256, 'attn_out': 2}
    report = packed_layers.pack_modules(model, s, bucket_size=64)
    assert sorted(report) == sorted(before)
    for name, old in before.items():
        new = getattr(model, name)
        assert isinstance(new, packed_layers.PackedEmbedding if isinstance(old, torch.nn.Embedding) else packed_layers.PackedLinear)
        bits = codec.min_bits_for_levels(s[name])
        n = old.weight.numel()
        nbias = 0 if getattr(old, 'bias', None) is None else 4 * old.bias.numel()
        assert report[name] == (4 * n + nbias, (n * bits + 7) // 8 + 8 * (-(-n // 64)) + nbias) == (new.fp32_nbytes, new.nbytes), name
        w = codec.pack_uniform(weights[name], s[name], 64, bits).unpack()
        if isinstance(old, torch.nn.Embedding):
            idx = torch.randint(0, 50, (4, 3), device=DEV)
            assert torch.equal(new(idx).view(torch.int32), w[idx].view(torch.int32)), name
        else:
            x = torch.randn(6, old.in_features, device=DEV)
            _bound_check(new(x), x, w, None if old.bias is None else old.bias.detach(), name)
    assert not [m for m in model.modules() if type(m) in (torch.nn.Linear, torch.nn.Embedding)]
    assert sum(isinstance(m, (torch.nn.LSTM, torch.nn.LSTMCell)) for m in model.modules()) == 3           # left as they are
    with torch.no_grad():
        logits = model(src, tgt)
    assert logits.shape == ref_shape == (15, 50) and torch.isfinite(logits).all()
    kept = Seq2SeqLSTM(v_src=50, v_tgt=50, emb=16, hidden=32).to(DEV)
    assert sorted(packed_layers.pack_modules(kept, 16, skip=('generator', 'src_emb'))) == ['attn_in', 'attn_out', 'tgt_emb']
    assert isinstance(kept.generator, torch.nn.Linear) and isinstance(kept.src_emb, torch.nn.Embedding)
