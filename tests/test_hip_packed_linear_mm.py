"""The batched Linear layer from packed weights on the device (libqd_infer_mm.so, include/qd_infer_mm.h) at the C ABI, against
the float64 product with the bit-exact weights of tests/packed_layer_cases.py, and PackedLinear(batched_from=...) on top."""
import numpy as np
import pytest
import torch

import packed_layer_cases as P
from test_hip_packed_layers import DEV, FLOAT_GUARD, Placed, fmt, place_weight
from quantized_distillation_amd import _infer_mm, _lib, packed_layers

pytestmark = pytest.mark.gpu

# (rows, cols, bucket): four full N tiles + 3 rows, rows mid-word, a ragged slab | one slab + a ragged one, buckets straddling rows |
# 33 slabs, fewer rows than an MFMA tile | several buckets inside a group of four | one row, no buckets
SHAPES = ((67, 37, 256), (67, 100, 100), (3, 2085, 256), (67, 5, 3), (1, 37, None))
MS = (1, 16, 17, 64, 65, 130)            # five of the six per width, so every width meets a ragged m-chunk and a second chunk


@pytest.fixture(scope='module')
def lib():
    return _infer_mm.load()


def call(lib, wt, x, bias, ptrs=None):
    """One qdm_linear_packed_f32 on plain device tensors (ptrs: the weight placed elsewhere); y [m, rows] as numpy."""
    keep = [torch.from_numpy(np.array(a)).to(DEV) for a in (wt.packed, wt.alpha, wt.beta)]
    xd = torch.from_numpy(np.array(x)).to(DEV)
    bd = None if bias is None else torch.from_numpy(np.array(bias)).to(DEV)
    m = x.shape[0]
    y = torch.full((m, wt.rows), float('nan'), device=DEV)
    with torch.cuda.device(DEV):
        rc = lib.qdm_linear_packed_f32(*fmt(wt, *(ptrs or [t.data_ptr() for t in keep])), xd.data_ptr(), m,
                                       None if bd is None else bd.data_ptr(), y.data_ptr(), _lib.stream_ptr(DEV))
        torch.cuda.synchronize()
    assert rc == 0, (wt.tag, rc)
    return y.cpu().numpy()


@pytest.mark.parametrize('bits', P.BITS)
def test_general_cases_within_the_bound(lib, bits):
    cases = [(P.general_weight(r, c, b, 2 ** bits, bits), MS[(hi + bits) % 6], False) for hi, (r, c, b) in enumerate(SHAPES)]
    cases.append((P.general_weight(67, 37, 256, 2 ** bits, bits, True), 17, True))
    for k, (wt, m, nan_row) in enumerate(cases):
        x, bias = P.linear_inputs(wt.cols, wt.rows, m, 300 + k + bits, False, nan_row)
        bias = None if k % 2 else bias
        y64, mag = P.linear_expected(wt.w, x, bias)
        assert not nan_row or (np.isnan(y64).any() and np.isfinite(y64).any())   # check_linear holds the non-finite outputs in kind
        ratio = P.check_linear(call(lib, wt, x, bias), y64, mag, (wt.tag, 'm %d' % m))
        print('%s m %d: error / sum|terms| = %.3g' % (wt.tag, m, ratio))


@pytest.mark.parametrize('bits', P.BITS)
def test_exact_cases_bit_for_bit(lib, bits):
    shapes = [s for s in SHAPES if s in P.EXACT_SHAPES]
    assert len(shapes) == 4
    for hi, (r, c, b) in enumerate(shapes):
        wt, m = P.exact_weight(r, c, b, bits), MS[(hi + bits + 3) % 6]
        x, bias = P.linear_inputs(wt.cols, wt.rows, m, 400 + hi + bits, True)
        assert P.exact_condition(wt, x, bias)
        y64, _ = P.linear_expected(wt.w, x, bias)
        assert np.array_equal(call(lib, wt, x, bias).view(np.uint32), y64.astype(np.float32).view(np.uint32)), (wt.tag, m)


@pytest.mark.parametrize('bits', P.BITS)
def test_a_row_does_not_depend_on_the_batch_or_the_grid(lib, bits):
    wt = P.general_weight(67, 100, 100, 2 ** bits, bits)
    x, bias = P.linear_inputs(wt.cols, wt.rows, 65, 500 + bits)
    y = call(lib, wt, x, bias)
    for i in (0, 63, 64):
        assert call(lib, wt, x[i:i + 1], bias).tobytes() == y[i:i + 1].tobytes(), (wt.tag, 'row %d alone' % i)
    assert lib.qdm_set_grid_cap(1) == 0
    try:
        capped = call(lib, wt, x, bias)
    finally:
        assert lib.qdm_set_grid_cap(0) == 1
    assert capped.tobytes() == y.tobytes(), (wt.tag, 'one block for all ten tiles')


@pytest.mark.parametrize('bits', P.BITS)
def test_reads_and_writes_stay_inside_their_arrays(lib, bits):
    wt, m = P.general_weight(67, 100, 100, 2 ** bits, bits), 65      # two slabs: the prefetched one and a ragged last one
    x, bias = P.linear_inputs(wt.cols, wt.rows, m, 600 + bits)
    placed = place_weight(wt, phase=(0, 4, 8, 12)[bits % 4])
    px, pb = Placed(np.float32, x.size, 4, 64, FLOAT_GUARD, x), Placed(np.float32, bias.size, 8, 64, FLOAT_GUARD, bias)
    py = Placed(np.float32, m * wt.rows, 12, 64, FLOAT_GUARD)
    with torch.cuda.device(DEV):
        rc = lib.qdm_linear_packed_f32(*fmt(wt, *(p.ptr for p in placed)), px.ptr, m, pb.ptr, py.ptr, _lib.stream_ptr(DEV))
        torch.cuda.synchronize()
    assert rc == 0
    for p, name in zip(placed + (px, pb), ('packed', 'alpha', 'beta', 'x', 'bias')):
        p.read(wt.tag, name)
    y = py.read(wt.tag, 'y').reshape(m, wt.rows)                    # nothing around y written, every element of it written
    P.check_linear(y, *P.linear_expected(wt.w, x, bias), (wt.tag, 'between guard bands'))
    assert y.tobytes() == call(lib, wt, x, bias).tobytes(), 'no alignment changes a bit of the result'


def _module(batched_from, bits=3):
    wt = P.general_weight(67, 100, 100, 2 ** bits, bits)
    lin = torch.nn.Linear(100, 67).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(np.array(wt.W)))
    return packed_layers.PackedLinear.from_linear(lin, wt.s, wt.bucket, bits, batched_from=batched_from), wt, lin.bias.detach().cpu().numpy()


def test_a_captured_call_replays_on_new_inputs():
    pl, _, _ = _module(16)
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(65, 100, generator=g).to(DEV) for _ in range(3)]
    eager = [pl(x).clone() for x in xs]
    x_buf = xs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # warm-up outside the capture
        pl(x_buf)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        y = pl(x_buf)
    torch.cuda.synchronize()
    for r in (1, 2, 0, 1):
        x_buf.copy_(xs[r])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int32), eager[r].view(torch.int32)), 'replay on input %d' % r


def test_the_module_switches_at_batched_from():
    pl, wt, bias = _module(16)
    plain = packed_layers.PackedLinear(pl.as_packed_uniform(), pl.bias)      # the same weight and bias, batched_from=None
    assert plain.batched_from is None and np.array_equal(pl.packed.cpu().numpy(), wt.packed)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 9, 100, generator=g)                      # 18 rows: the batched kernel
    y = pl(x.to(DEV))
    assert y.shape == (2, 9, 67) and y.grad_fn is None
    x2 = x.reshape(18, 100).numpy()
    P.check_linear(y.reshape(18, 67).cpu().numpy(), *P.linear_expected(wt.w, x2, bias), 'PackedLinear(batched_from=16), 18 rows')
    assert y.reshape(18, 67).cpu().numpy().tobytes() == call(_infer_mm.load(), wt, x2, bias).tobytes()
    x = torch.randn(2, 7, 100, generator=g).to(DEV)              # 14 rows: the decode-time kernel, as without batched_from
    assert torch.equal(pl(x).view(torch.int32), plain(x).view(torch.int32))
