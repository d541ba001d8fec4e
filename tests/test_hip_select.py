"""Device order statistics (qd_order_stats_f32, csrc/qd_select.hip) behind initialize_quantization_points
(ref: quantization/help_functions.py:140-154): bit-exact against a host sort; below that, the bit-pattern cases of
tests/select_cases.py (non-finite values, span edges, block counts, shared key prefixes, the wrapper's three paths) and
initialize_quantization_points on tensors that hold a NaN or an infinity."""
import numpy as np
import pytest
import torch

import select_cases as S

pytestmark = pytest.mark.gpu


def _host(values, ranks):
    return np.sort(values.cpu().numpy().reshape(-1), kind='stable')[ranks]


def _same_bits(a, b):
    """Bit equality, except that +0 and -0 are the same value: among EQUAL elements a sort's order is arbitrary (numpy's
    partition and torch.sort are not specified either), and the select orders -0 before +0."""
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)
    zero = (a == 0) & (b == 0)
    return np.array_equal(np.where(zero, np.float32(0), a).view(np.uint32), np.where(zero, np.float32(0), b).view(np.uint32))


def _cases():
    g = torch.Generator().manual_seed(11)
    yield 'gauss', torch.randn(300007, generator=g)
    yield 'unit', torch.rand(70001, generator=g)
    yield 'one', torch.tensor([3.5])
    yield 'five', torch.tensor([2.0, -1.0, 0.0, 7.0, -1.0])
    yield 'constant', torch.full((40000,), 0.25)
    yield 'two-valued', (torch.rand(50000, generator=g) > 0.3).float()
    yield 'few-levels', torch.randint(0, 7, (123457,), generator=g).float() / 6
    yield 'tiny', torch.randn(65536, generator=g) * 1e-41              # denormals
    yield 'huge', torch.randn(65536, generator=g) * 1e37
    yield 'signed-zero', torch.cat([torch.zeros(100), -torch.zeros(100), torch.randn(1000, generator=g)])
    yield 'near-ties', 0.5 + torch.randint(-3, 4, (200000,), generator=g).float() * 2.0 ** -24
    yield 'large', torch.randn(5308416 + 3, generator=g) * 0.05


@pytest.mark.parametrize('name,values', list(_cases()), ids=[c[0] for c in _cases()])
def test_order_statistics_match_a_host_sort(name, values):
    import quantization.help_functions as qhf
    dev = values.cuda()
    n = dev.numel()
    rng = np.random.default_rng(3)
    for m in (1, 2, 8, 31, 32, 33, 64):
        ranks = rng.integers(0, n, size=m)
        ranks[0] = 0
        ranks[-1] = n - 1
        got = qhf.order_statistics(dev, ranks)
        assert _same_bits(got, _host(values, ranks)), (name, m)
    # sort fallback (more than 2 x 32 distinct ranks) gives the same values
    if n > 200:
        ranks = rng.permutation(n)[:150]
        assert _same_bits(qhf.order_statistics(dev, ranks), _host(values, ranks))


def test_unaligned_start_and_repeated_ranks():
    import quantization.help_functions as qhf
    g = torch.Generator().manual_seed(5)
    base = torch.randn(100003, generator=g).cuda()
    for off in (1, 2, 3):
        view = base[off:off + 99991]
        ranks = np.array([5, 5, 0, 99990, 777, 5, 50000])
        assert _same_bits(qhf.order_statistics(view, ranks), _host(view, ranks))


def test_nan_orders_last():
    import quantization.help_functions as qhf
    v = torch.randn(10000)
    v[17] = float('nan')
    got = qhf.order_statistics(v.cuda(), np.array([0, 9998, 9999]))
    want = np.sort(v.numpy())[[0, 9998, 9999]]
    assert _same_bits(got[:2], want[:2]) and np.isnan(got[2])


def test_argument_errors():
    import quantization.help_functions as qhf
    from quantized_distillation_amd import _lib
    v = torch.randn(1000).cuda()
    with pytest.raises(IndexError):
        qhf.order_statistics(v, np.array([1000]))
    with pytest.raises(TypeError):
        qhf.order_statistics(v.double(), np.array([1]))
    lib = _lib.load()
    out = torch.empty(4, device='cuda')
    ws = torch.empty(lib.qd_order_stats_workspace_bytes(2), dtype=torch.uint8, device='cuda')
    bad = np.array([5, 3], dtype=np.int64)                               # decreasing
    assert lib.qd_order_stats_f32(v.data_ptr(), 1000, bad.ctypes.data, 2, out.data_ptr(), ws.data_ptr(), ws.numel(), 0) == -1
    ok = np.array([3, 5], dtype=np.int64)
    assert lib.qd_order_stats_f32(v.data_ptr(), 1000, ok.ctypes.data, 2, out.data_ptr(), ws.data_ptr(), 16, 0) == -2
    many = np.arange(33, dtype=np.int64)
    assert lib.qd_order_stats_f32(v.data_ptr(), 1000, many.ctypes.data, 33, out.data_ptr(), ws.data_ptr(), ws.numel(), 0) == -3


def test_initialize_quantization_points_equals_numpy_percentile():
    """The reference's own formula on the host (help_functions.py:150) against the device path, model-sized."""
    import quantization
    import quantization.help_functions as qhf
    g = torch.Generator().manual_seed(2)
    for n, k in ((800000, 4), (123457, 16), (300000, 32), (50000, 256)):
        x = (torch.randn(n, generator=g) * 0.05).cuda()
        sf = quantization.ScalingFunction('linear', False, False, 256, False)
        got = qhf.initialize_quantization_points(x, sf, k).cpu().numpy()
        scaled = sf.scale_down(x).view(-1)[0:n].cpu().numpy()
        want = np.percentile(scaled, np.linspace(0, 100, num=k)).astype(np.float32)
        assert _same_bits(got, want), (n, k)


# ------------------------------------------------------------------------------------------------ tests/select_cases.py
# The shared cases (proved on the host by tests/test_select_host.py): inputs built from bit patterns, the expected answer
# an integer sort with every NaN on the one largest key.  Each case runs through the radix select AND through the sort
# fallback on the device, and on the CPU copy; all three must return the expected values.

def _check_all_paths(cid):
    c = S.case(cid)
    want = c.expected()
    for path in ('select', 'sort', 'host'):
        S.same(S.run(c, path), want, (cid, path))


@pytest.mark.parametrize('cid', S.NONFINITE_IDS)
def test_select_nonfinite_case(cid):
    """A NaN orders last whatever its sign bit and payload (0xFFC00000 is what 0/0 gives on the host): rank 0 is -inf, the
    ranks past the last number are NaN."""
    _check_all_paths(cid)


@pytest.mark.parametrize('group', ['span_v%d' % v for v in S.SPAN_NVEC] + ['span_tiny'])
def test_select_span_edges(group):
    for cid in S.GROUPS[group]:
        c = S.case(cid)
        t = c.tensor('cuda')
        assert S.head_of(c.offset, c.n) == min(((16 - t.data_ptr() % 16) % 16) // 4, c.n), cid      # the head the kernel will see
        _check_all_paths(cid)


@pytest.mark.parametrize('cid', S.BLOCKS_IDS)
def test_select_block_counts(cid):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus >= S.MIN_CUS, 'the launcher caps the blocks at %d CUs: the list of block counts does not mean what it says' % cus
    _check_all_paths(cid)


@pytest.mark.parametrize('cid', S.PREFIX_IDS)
def test_select_shared_prefixes(cid):
    _check_all_paths(cid)


@pytest.mark.parametrize('cid', S.WRAPPER_IDS)
def test_order_statistics_wrapper_case(cid, monkeypatch):
    """Besides the three forced paths: the wrapper's own choice.  Up to 64 distinct ranks it selects (two passes above 32),
    from 65 it sorts."""
    import quantization.help_functions as qhf
    _check_all_paths(cid)
    c = S.case(cid)
    sorts = []
    real_sort = torch.sort
    monkeypatch.setattr(torch, 'sort', lambda *a, **k: (sorts.append(1), real_sort(*a, **k))[1])
    got = qhf.order_statistics(c.tensor('cuda'), c.ranks)
    monkeypatch.undo()
    assert got.dtype == np.float32 and got.shape == c.ranks.shape
    S.same(got, c.expected(), (cid, 'device'))
    assert len(sorts) == (1 if np.unique(c.ranks).size > 64 else 0), cid


def test_select_abi_repeated_ranks_and_sign_set_nan():
    """qd_order_stats_f32 itself with EQUAL neighbouring ranks (non-decreasing is the contract; the wrapper never sends
    them): the rows of equal targets are shared in both sub-passes."""
    from quantized_distillation_amd import _lib
    lib = _lib.load()
    c = S.case('nf-several')
    n, nnan = c.n, len(S.SEVERAL_NANS)
    ranks = np.array([0, 0, 1, 5, 5, 5, n - nnan - 1, n - nnan - 1, n - nnan, n - nnan, n - 1, n - 1], dtype=np.int64)
    x = c.tensor('cuda')
    out = torch.full((ranks.size + 2,), 777.0, device='cuda')
    ws = torch.empty(lib.qd_order_stats_workspace_bytes(ranks.size), dtype=torch.uint8, device='cuda')
    assert lib.qd_order_stats_f32(x.data_ptr(), n, ranks.ctypes.data, ranks.size, out.data_ptr() + 4, ws.data_ptr(), ws.numel(), 0) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[0] == 777.0 and got[-1] == 777.0
    S.same(got[1:-1], S.Case('abi', c.bits, ranks).expected(), 'abi')


@pytest.mark.parametrize('shape', S.PCT_SHAPES, ids=S.PCT_SHAPE_IDS)
def test_percentile_points_of_nonfinite_tensors(shape):
    """The reference's literal line (help_functions.py:150) on the device's scaled tensor copied to the host, and the same
    call on the CPU copy of the tensor: one NaN in the scaled tensor -- from a NaN, or from a +-inf through its bucket's
    alpha and beta -- makes every point NaN; the clean tensor of each shape keeps its points."""
    import quantization
    import quantization.help_functions as qhf
    for cid, x, bucket, k in S.percentile_cases(shape):
        xd = torch.from_numpy(x).cuda()
        assert np.array_equal(xd.cpu().numpy().view(np.uint32), x.view(np.uint32))         # the planted bits arrived
        sf = quantization.ScalingFunction('linear', False, False, bucket)
        got = qhf.initialize_quantization_points(xd, sf, k)
        assert got.is_cuda and got.dtype == torch.float32
        scaled = quantization.ScalingFunction('linear', False, False, bucket).scale_down(xd).view(-1)[0:x.size].cpu().numpy()
        with np.errstate(invalid='ignore'):
            want = np.percentile(scaled, np.linspace(0, 100, num=k)).astype(np.float32)
        S.same_points(got.cpu().numpy(), want, cid)
        assert bool(np.isnan(want).all()) == ('clean' not in cid) and np.isnan(want).any() == np.isnan(want).all(), cid
        host = qhf.initialize_quantization_points(torch.from_numpy(x), quantization.ScalingFunction('linear', False, False, bucket), k)
        S.same_points(got.cpu().numpy(), host.numpy(), (cid, 'device against CPU tensor'))
