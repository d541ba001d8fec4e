"""Both nearest-point rules on ties and crowded points, on the device: every kernel the launcher of qd_nearest_point_f32 can
reach (tests/nearest_cases.py ROWS, each row held to its kernel by tests/test_nearest_cases_host.py on the CPU), the
multi-tensor launches with their own table and search (csrc/qd_multi_dq.hip), and the Python entry points.

Everything is compared bit for bit with the numpy reference of tests/nearest_cases.py: indices, q, alpha, beta.  The cases put
at least half of their elements exactly on a point, a midpoint, a boundary of the 256- or the 2048-cell table or an fp32
neighbour of one, so `<` for `<=` in a search, `<=` for the strict `<` of the distance rule, or a midpoint rounded as
(p + q) / 2 fails here."""
import numpy as np
import pytest
import torch

import nearest_cases as C
from quantized_distillation_amd import _lib

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
GUARD = 64                                   # bytes of sentinel on either side of every carved tensor
Q_FILL = 777.0                               # no q, alpha or beta of any case comes near it
DTYPES = {8: torch.int64, 1: torch.uint8}
IDX_FILL = {8: -1, 1: 255}


@pytest.fixture(scope='module', autouse=True)
def _built():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    _lib.load()


def carve(n, dtype, off_bytes, fill):
    """(buffer, view): n elements that start off_bytes past a 16-byte boundary, GUARD bytes of `fill` on either side."""
    isz = torch.empty(0, dtype=dtype).element_size()
    assert off_bytes % isz == 0
    lead = (GUARD + off_bytes) // isz
    buf = torch.full((lead + n + GUARD // isz,), fill, dtype=dtype, device=DEV)
    view = buf[lead:lead + n]
    assert view.data_ptr() % 16 == off_bytes % 16
    return buf, view


def guards_intact(buf, view, fill):
    lead = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((buf[:lead] == fill).all()) and bool((buf[lead + view.numel():] == fill).all())


def dev(a, off_bytes=0):
    t = torch.from_numpy(np.array(a))        # (a copy: the cases are read-only)
    _, view = carve(t.numel(), t.dtype, off_bytes, 0)
    view.copy_(t)
    return view


def host(t):
    return t.detach().cpu().numpy()


def stream():
    return torch.cuda.current_stream().cuda_stream


def run(lib, ws, xd, prescaled, pd, rule, n, bucket, ad, bd, width, idx_off=0, q_off=0, want_q=True):
    """One qd_nearest_point_f32 call into sentinel-filled, guarded outputs; returns (q, idx) as numpy (None where not asked for)."""
    qbuf, q = carve(n, torch.float32, q_off, Q_FILL)
    ibuf, idx = carve(n, DTYPES[width], idx_off, IDX_FILL[width]) if width else (None, None)
    _lib.check(lib.qd_nearest_point_f32(xd.data_ptr(), prescaled, pd.data_ptr(), pd.numel(), rule, q.data_ptr() if want_q else None,
                                        idx.data_ptr() if width else None, width or 8, n, bucket, ad.data_ptr(), bd.data_ptr(), None, 0, 0.0,
                                        ws.data_ptr(), ws.numel(), stream()))
    assert guards_intact(qbuf, q, Q_FILL) and (not width or guards_intact(ibuf, idx, IDX_FILL[width])), 'a write outside the outputs'
    if not want_q:
        assert bool((q == Q_FILL).all()), 'indices only wrote q'
    return (host(q) if want_q else None), (host(idx).astype(np.int64) if width else None)


@pytest.mark.parametrize('k', C.K)
def test_single_tensor_call_on_every_kernel(k):
    """qd_nearest_point_f32 through the C ABI: every row of the geometry table x four of the seven point sets x both rules x the row's index
    forms (int64, uint8 up to 256 points, none), raw and pre-scaled; the indices-only form where the library serves it."""
    lib = _lib.load()
    ws = torch.empty(lib.qd_workspace_bytes(), dtype=torch.uint8, device=DEV)
    for ri, row, name, pts, case in C.cases_of(k):
        n, bucket = row.n, row.bucket
        nb = case['alpha'].size
        pd, xd = dev(pts), dev(case['x'], row.x_off)
        x_bits = host(xd).view(np.int32).copy()
        previous = lib.qd_set_single_fused_mode(row.fused_mode) if row.fused_mode is not None else None
        try:
            for rule in C.RULES:
                want_idx, want_q = C.expect(case, pts, rule)
                seen = []
                for width, off, _ in row.forms:
                    if width == 1 and k > 256:
                        continue
                    tag = (k, ri, name, rule, width, off)
                    if row.prescaled:
                        ad, bd = dev(case['alpha']), dev(case['beta'])
                    else:
                        ad, bd = torch.full((nb,), Q_FILL, device=DEV), torch.full((nb,), Q_FILL, device=DEV)
                    q, idx = run(lib, ws, xd, row.prescaled, pd, rule, n, bucket, ad, bd, width, off, q_off=row.x_off)
                    if idx is not None:
                        bad = np.flatnonzero(idx != want_idx)
                        assert bad.size == 0, (tag, bad.size, bad[:5], case['u'][bad[:5]], idx[bad[:5]], want_idx[bad[:5]])
                        seen.append(idx)
                    bad = np.flatnonzero(~((q == want_q) | (np.isnan(q) & np.isnan(want_q))))
                    assert bad.size == 0, (tag, bad.size, bad[:5], q[bad[:5]], want_q[bad[:5]])
                    assert np.array_equal(host(ad), case['alpha'], equal_nan=True) and np.array_equal(host(bd), case['beta'], equal_nan=True), tag
                    if C.indices_only_served(row, width, off):
                        _, idx2 = run(lib, ws, xd, 1, pd, rule, n, bucket, ad, bd, width, off, want_q=False)
                        assert np.array_equal(idx2, idx), (tag, 'indices only')
                assert all(np.array_equal(s, seen[0]) for s in seen[1:]), (k, ri, name, rule, 'the index widths disagree')
        finally:
            if previous is not None:
                lib.qd_set_single_fused_mode(previous)
        assert np.array_equal(host(xd).view(np.int32), x_bits), (k, ri, name, 'the input was modified')


# ----------------------------------------------------------------------------------------------------- multi-tensor launch
def multi_object(k, bucket, out_dtype):
    """MultiTensorDiffQuant over the seven tensors of C.multi_case, its resident u / alpha / beta replaced by the case's
    pre-scaled values; the odd tensors' u, q and idx sit off the alignment the register path needs."""
    from quantized_distillation_amd.multi_tensor import MultiTensorDiffQuant
    cases = C.multi_case(k, bucket)
    isz = torch.empty(0, dtype=out_dtype).element_size()
    sizes = [c['u'].size for _, c in cases]
    keep, outs = [], []
    for i, n in enumerate(sizes):
        buf, view = carve(n, out_dtype, isz if i % 2 else 0, 0)
        keep.append(buf)
        outs.append(view)
    weights = [torch.zeros(n, device=DEV) for n in sizes]
    mt = MultiTensorDiffQuant(weights, outs, [torch.zeros(n, device=DEV) for n in sizes], k, bucket or None)
    mt.scaled = [dev(c['u'], 4 if i % 2 else 0) for i, (_, c) in enumerate(cases)]
    mt.indices = []
    for i, n in enumerate(sizes):
        buf, view = carve(n, torch.uint8, 2 if i % 2 else 0, 255)
        keep.append(buf)
        mt.indices.append(view)
    for sf, (_, c) in zip(mt.scalings, cases):
        sf.alpha, sf.beta = dev(c['alpha']), dev(c['beta'])
    mt._plan()
    return mt, outs, keep


@pytest.mark.parametrize('bucket', C.MULTI_BUCKETS)
@pytest.mark.parametrize('k', C.MULTI_K)
def test_multi_tensor_launches(k, bucket):
    """qd_multi_nearest_f32 and qd_multi_nearest_out16_f32 (fp16, bf16): seven tensors with seven different point sets in one
    table.  Indices against the numpy midpoint reference; q against its fp32 bits (16-bit outputs: their IEEE conversion);
    and both against the per-tensor call the header says they equal."""
    lib = _lib.load()
    ws = torch.empty(lib.qd_workspace_bytes(), dtype=torch.uint8, device=DEV)
    cases = C.multi_case(k, bucket)
    pts = torch.from_numpy(np.stack([p for p, _ in cases])).to(DEV)              # [tensors, k]
    want = [C.expect(c, p, C.MIDPOINT) for p, c in cases]
    single = []
    for i, (p, c) in enumerate(cases):
        single.append(run(lib, ws, dev(c['u'], 4 if i % 2 else 0), 1, dev(p), C.MIDPOINT, c['u'].size, bucket, dev(c['alpha']), dev(c['beta']), 1))
    for out_dtype, entry in ((torch.float32, 'qd_multi_nearest_f32'), (torch.float16, 'qd_multi_nearest_out16_f32'),
                             (torch.bfloat16, 'qd_multi_nearest_out16_f32')):
        mt, outs, keep = multi_object(k, bucket, out_dtype)
        mt.forward(pts)
        assert mt.entry_point == entry
        for i, (p, c) in enumerate(cases):
            tag = (k, bucket, str(out_dtype), i, C.SETS[i])
            idx = host(mt.indices[i]).astype(np.int64)
            bad = np.flatnonzero(idx != want[i][0])
            assert bad.size == 0, (tag, bad.size, bad[:5], c['u'][bad[:5]], idx[bad[:5]], want[i][0][bad[:5]])
            assert np.array_equal(idx, single[i][1]), (tag, 'indices vs the per-tensor call')
            assert not np.isnan(want[i][1]).any()
            for ref in (want[i][1], single[i][0]):
                ref_t = torch.from_numpy(ref).to(out_dtype)                      # IEEE round to nearest even (fp32: the bits themselves)
                bits = torch.int32 if out_dtype == torch.float32 else torch.int16
                assert torch.equal(outs[i].cpu().view(bits), ref_t.view(bits)), (tag, 'q')
        for i in range(len(cases)):                                              # nothing written around q (0) and idx (255)
            assert guards_intact(keep[i], outs[i], 0) and guards_intact(keep[len(cases) + i], mt.indices[i], 255), (k, bucket, i)


# ------------------------------------------------------------------------------------------------------------ Python API
API_CASES = [(100, 100 * 70 + 43, 65, 'bell'), (256, 256 * 40 + 131, 16, 'dups'), (1000, 1000 * 10 + 333, 256, 'cell bounds'),
             (33, 33 * 300 + 17, 5, 'outside'), (64, 64 * 150 + 37, 200, 'full precision')]


@pytest.mark.parametrize('bucket,n,k,name', API_CASES)
def test_python_entry_points(bucket, n, k, name):
    """nonUniformQuantization (distance rule; int64 and uint8 indices), nonUniformQuantization_variable with
    pre_process_tensors=True and SearchSorted(u).query (midpoint rule) on multi-bucket tie cases."""
    import quantization
    from quantization.quant_functions import SearchSorted
    pts = C.points(name, k, 41)
    case = C.raw_case(pts, n, bucket, 42, unscaled=name == 'full precision')
    xd, pd = dev(case['x']), dev(pts)
    want_idx, want_q = C.expect(case, pts, C.DISTANCE)
    for dt in (None, torch.uint8):
        q, idx, sf = quantization.nonUniformQuantization(xd, pd, bucket_size=bucket, **({} if dt is None else {'index_dtype': dt}))
        assert idx.dtype == (dt or torch.int64)
        assert np.array_equal(host(idx).astype(np.int64).reshape(-1), want_idx), (bucket, k, name, dt)
        assert np.array_equal(host(q).reshape(-1), want_q, equal_nan=True)
        assert np.array_equal(host(sf.alpha).reshape(-1), case['alpha'], equal_nan=True)
        assert np.array_equal(host(sf.beta).reshape(-1), case['beta'], equal_nan=True)
    want_idx, want_q = C.expect(case, pts, C.MIDPOINT)
    fn = quantization.nonUniformQuantization_variable(bucket_size=bucket, pre_process_tensors=True, tensor=xd)
    q = fn.forward(None, pd)
    assert np.array_equal(host(q).reshape(-1), want_q, equal_nan=True), (bucket, k, name, 'pre-processed q')
    assert np.array_equal(host(fn.savedForBackward['indices']).astype(np.int64).reshape(-1), want_idx), (bucket, k, name, 'pre-processed idx')
    idx = SearchSorted(dev(case['u'])).query(pd)
    assert idx.dtype == torch.int64 and np.array_equal(host(idx).reshape(-1), want_idx), (bucket, k, name, 'SearchSorted.query')
