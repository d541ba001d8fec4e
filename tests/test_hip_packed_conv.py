"""nn.Conv2d from packed weights on the device (libqd_infer_conv.so, include/qd_infer_conv.h) at the C ABI, against a plain numpy
im2col (explicit loops over the window, zeros outside the image) multiplied in float64 with the bit-exact weights of
tests/packed_layer_cases.py, and PackedConv2d / pack_modules(conv=True) on top."""
import copy

import numpy as np
import pytest
import torch

import packed_layer_cases as P
from test_hip_packed_layers import DEV, FLOAT_GUARD, Placed, place_weight
from quantized_distillation_amd import _infer_conv, _lib, packed_layers

pytestmark = pytest.mark.gpu

# (cout, cin, kh, kw, stride, pad, batch, h, w, bucket, bucket of the exact case: every bucket holds two elements)
GEOS = (
    (19, 3, 3, 3, (1, 1), (1, 1), 2, 9, 7, 256, 100),    # a ragged N tile; K = 27: one ragged slab, rows mid-word; 126 pixels, an image boundary inside a wave; rows of 7
    (16, 8, 3, 3, (2, 2), (1, 1), 11, 10, 9, 100, 100),  # K = 72: a prefetched slab + a ragged one; stride 2; 275 pixels: a second, ragged chunk; buckets straddle rows
    (3, 70, 1, 1, (2, 2), (0, 0), 2, 8, 8, None, None),  # the shortcut: 1 x 1, no padding, fewer channels than a tile
    (16, 3, 7, 7, (2, 2), (3, 3), 1, 12, 11, 256, 256),  # the stem: K = 147, three slabs; padding wider than a wave's row
    (5, 4, 1, 3, (2, 1), (0, 2), 3, 6, 5, 3, 3),         # every h / w asymmetry at once; padding at the kernel's extent; several buckets per group of four
)


@pytest.fixture(scope='module')
def lib():
    return _infer_conv.load()


def im2col(x, kh, kw, stride, pad):
    """[n oh ow, cin kh kw] of x [n, cin, h, w]: column (ci kh + a) kw + b, 0.0 outside the image."""
    n, c, h, w = x.shape
    oh, ow = (h + 2 * pad[0] - kh) // stride[0] + 1, (w + 2 * pad[1] - kw) // stride[1] + 1
    xp = np.zeros((n, c, h + 2 * pad[0], w + 2 * pad[1]), x.dtype)
    xp[:, :, pad[0]:pad[0] + h, pad[1]:pad[1] + w] = x
    cols = np.empty((n, oh, ow, c, kh, kw), x.dtype)
    for a in range(kh):
        for b in range(kw):
            cols[:, :, :, :, a, b] = xp[:, :, a:a + stride[0] * oh:stride[0], b:b + stride[1] * ow:stride[1]].transpose(0, 2, 3, 1)
    return cols.reshape(n * oh * ow, c * kh * kw), oh, ow


def inputs(g, seed, exact=False, nan=False):
    cout, cin, _, _, _, _, batch, h, w = g[:9]
    x, bias = P.linear_inputs(cin * h * w, cout, batch, seed, exact, nan)
    return x.reshape(batch, cin, h, w), bias


def args(wt, g, packed, alpha, beta, x, bias, y):
    cout, cin, kh, kw, stride, pad, batch, h, w = g[:9]
    return (packed, alpha, beta, cout, cin, kh, kw, 0 if wt.bucket is None else wt.bucket, wt.s, wt.bits, x, batch, h, w,
            stride[0], stride[1], pad[0], pad[1], bias, y, _lib.stream_ptr(DEV))


def call(lib, wt, g, x, bias):
    """One qdc_conv2d_packed_f32 on plain device tensors; y [n, cout, oh, ow] as numpy."""
    g = g[:6] + (x.shape[0],) + g[7:]
    keep = [torch.from_numpy(np.array(a)).to(DEV) for a in (wt.packed, wt.alpha, wt.beta, x)]
    bd = None if bias is None else torch.from_numpy(np.array(bias)).to(DEV)
    _, oh, ow = im2col(x[:1, :1], g[2], g[3], g[4], g[5])
    y = torch.full((x.shape[0], g[0], oh, ow), float('nan'), device=DEV)
    with torch.cuda.device(DEV):
        rc = lib.qdc_conv2d_packed_f32(*args(wt, g, *(t.data_ptr() for t in keep), None if bd is None else bd.data_ptr(), y.data_ptr()))
        torch.cuda.synchronize()
    assert rc == 0, (wt.tag, rc)
    return y.cpu().numpy()


def as_rows(y):
    """[n, cout, oh, ow] as the [pixels, cout] matrix of the GEMM."""
    return y.transpose(0, 2, 3, 1).reshape(-1, y.shape[1])


@pytest.mark.parametrize('bits', P.BITS)
def test_general_cases_within_the_bound(lib, bits):
    cases = [(GEOS[(bits + i) % 5], False) for i in range(4)] + [(GEOS[1 + 2 * (bits % 2)], True)]      # both leave channels finite
    for k, (g, nonfinite) in enumerate(cases):
        wt = P.general_weight(g[0], g[1] * g[2] * g[3], g[9], 2 ** bits, bits, nonfinite)
        x, bias = inputs(g, 700 + k + bits, nan=nonfinite)
        bias = None if k % 2 else bias
        y64, mag = P.linear_expected(wt.w, im2col(x, *g[2:6])[0], bias)
        assert not nonfinite or (np.isnan(y64).any() and np.isfinite(y64).any())   # check_linear holds the non-finite outputs in kind
        ratio = P.check_linear(as_rows(call(lib, wt, g, x, bias)), y64, mag, (wt.tag, g))
        print('%s %s: error / sum|terms| = %.3g' % (wt.tag, g, ratio))


@pytest.mark.parametrize('bits', P.BITS)
def test_exact_cases_bit_for_bit(lib, bits):
    for k in range(3):
        g = GEOS[(bits + 2 * k) % 5]
        wt = P.exact_weight(g[0], g[1] * g[2] * g[3], g[10], bits)
        x, bias = inputs(g, 800 + k + bits, exact=True)
        cols = im2col(x, *g[2:6])[0]
        assert P.exact_condition(wt, cols, bias)
        y64, _ = P.linear_expected(wt.w, cols, bias)
        assert np.array_equal(as_rows(call(lib, wt, g, x, bias)).view(np.uint32), y64.astype(np.float32).view(np.uint32)), (wt.tag, g)


@pytest.mark.parametrize('bits', P.BITS)
def test_an_image_does_not_depend_on_its_batch_or_the_grid(lib, bits):
    g = GEOS[1]
    wt = P.general_weight(16, 72, 100, 2 ** bits, bits)
    x, bias = inputs(g, 900 + bits)
    y = call(lib, wt, g, x, bias)
    for n in (0, 5, 10):                                           # image 10 straddles the two pixel chunks
        assert call(lib, wt, g, x[n:n + 1], bias).tobytes() == y[n:n + 1].tobytes(), (wt.tag, 'image %d alone' % n)
    assert lib.qdc_set_grid_cap(1) == 0
    try:
        capped = call(lib, wt, g, x, bias)
    finally:
        assert lib.qdc_set_grid_cap(0) == 1
    assert capped.tobytes() == y.tobytes(), (wt.tag, 'one block for both tiles')


@pytest.mark.parametrize('bits', P.BITS)
def test_reads_and_writes_stay_inside_their_arrays(lib, bits):
    g = GEOS[1]
    wt = P.general_weight(16, 72, 100, 2 ** bits, bits)
    x, bias = inputs(g, 1000 + bits)
    placed = place_weight(wt, phase=(0, 4, 8, 12)[bits % 4])
    px, pb = Placed(np.float32, x.size, 4, 64, FLOAT_GUARD, x), Placed(np.float32, bias.size, 8, 64, FLOAT_GUARD, bias)
    py = Placed(np.float32, 11 * 16 * 5 * 5, 12, 64, FLOAT_GUARD)
    with torch.cuda.device(DEV):
        rc = lib.qdc_conv2d_packed_f32(*args(wt, g, *(p.ptr for p in placed), px.ptr, pb.ptr, py.ptr))
        torch.cuda.synchronize()
    assert rc == 0
    for p, name in zip(placed + (px, pb), ('packed', 'alpha', 'beta', 'x', 'bias')):
        p.read(wt.tag, name)
    y = py.read(wt.tag, 'y').reshape(11, 16, 5, 5)                  # nothing around y written, every element of it written
    P.check_linear(as_rows(y), *P.linear_expected(wt.w, im2col(x, *g[2:6])[0], bias), (wt.tag, 'between guard bands'))
    assert y.tobytes() == call(lib, wt, g, x, bias).tobytes(), 'no alignment changes a bit of the result'


def _module(bits=3):
    g = GEOS[1]
    wt = P.general_weight(16, 72, 100, 2 ** bits, bits)
    conv = torch.nn.Conv2d(8, 16, 3, stride=2, padding=1).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(np.array(wt.W)).view(16, 8, 3, 3))
    return packed_layers.PackedConv2d.from_conv2d(conv, wt.s, wt.bucket, bits), wt, g, conv.bias.detach().cpu().numpy()


def test_the_module_is_the_c_abi_call(lib):
    pc, wt, g, bias = _module()
    assert np.array_equal(pc.packed.cpu().numpy(), wt.packed) and (pc.in_channels, pc.out_channels) == (8, 16)
    x, _ = inputs(g, 1100)
    xd = torch.from_numpy(np.array(x)).to(DEV)
    y = pc(xd)
    assert y.shape == (11, 16, 5, 5) and y.is_contiguous() and y.grad_fn is None
    assert y.cpu().numpy().tobytes() == call(lib, wt, g, x, bias).tobytes()
    assert torch.equal(pc(xd.contiguous(memory_format=torch.channels_last)).view(torch.int32), y.view(torch.int32))
    back = pc.unpack()
    assert (back.stride, back.padding) == ((2, 2), (1, 1)) and torch.equal(back.bias, pc.bias)
    assert torch.equal(back.weight.detach().view(torch.int32), pc.as_packed_uniform().unpack().view(16, 8, 3, 3).view(torch.int32))
    with pytest.raises(RuntimeError, match='inference only'):
        pc(xd.clone().requires_grad_())


def test_a_captured_call_replays_on_new_inputs():
    pc, _, _, _ = _module()
    gen = torch.Generator().manual_seed(5)
    xs = [torch.randn(11, 8, 10, 9, generator=gen).to(DEV) for _ in range(3)]
    eager = [pc(x).clone() for x in xs]
    x_buf = xs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # warm-up outside the capture
        pc(x_buf)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        y = pc(x_buf)
    torch.cuda.synchronize()
    for r in (1, 2, 0, 1):
        x_buf.copy_(xs[r])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int32), eager[r].view(torch.int32)), 'replay on input %d' % r


def test_pack_modules_replaces_convolutions():
    nn = torch.nn
    torch.manual_seed(7)
    model = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.Conv2d(8, 6, 3, stride=2), nn.Flatten(), nn.Linear(96, 5)).to(DEV)
    fp32 = copy.deepcopy(model)
    report = packed_layers.pack_modules(model, 16, conv=True)
    assert [type(m).__name__ for m in model] == ['PackedConv2d', 'ReLU', 'PackedConv2d', 'Flatten', 'PackedLinear']
    assert report == {k: (model[int(k)].fp32_nbytes, model[int(k)].nbytes) for k in ('0', '2', '4')}
    assert report['0'][0] == 4 * (8 * 27 + 8) and all(packed < fp32_bytes for fp32_bytes, packed in report.values())
    x = torch.randn(2, 3, 9, 9, device=DEV)
    one_by_one = packed_layers.PackedLinear.from_linear(fp32[4], 16)(torch.flatten(packed_layers.PackedConv2d.from_conv2d(fp32[2], 16)(
        torch.relu(packed_layers.PackedConv2d.from_conv2d(fp32[0], 16)(x))), 1))
    assert torch.equal(model(x).view(torch.int32), one_by_one.view(torch.int32))
