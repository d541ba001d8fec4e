"""Every floating-point reduction of libqd_hip.so bit for bit, on inputs whose sums do not depend on their order.

tests/errlog.py holds K6 / K6m (the point gradient), the bucket sums of K7 (the STE backward) and qd_mean_f32 to
1e-6 x sum|terms|, which one dropped, doubled or misplaced element passes.  The cases of tests/exact_sum_cases.py (proved on the
CPU by tests/test_exact_sum_cases_host.py, and again here for every case that runs) have ONE possible fp32 result per sum, so
the comparison is by bit pattern and no tolerance appears: a term in the wrong bin, under the wrong bucket's alpha, lost at a
loop boundary or added twice is off by at least a whole unit.  The shapes reach every kernel of qd_point_grad_f32's
dispatcher with at least two trips of its unrolled loop, the per-lane tail, the n % 4 leftovers and a ragged last bucket in one
launch (under qd_set_grid_cap 1, 2, 3 and uncapped), K6m's tile -> wave -> row bookkeeping with a tensor that wraps the 2048
waves, both bodies of K7 and the two stages of the mean."""
import numpy as np
import pytest
import torch

from quantized_distillation_amd import _lib

import exact_sum_cases as E
import grid_trip_cases as C
from test_hip_grid_trips import Out, assert_trips, dev, inp, lib_cap_is_default, stream_tail

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
ALL_CAPS = (None,) + E.CAPS


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def assert_bits(got, want, tag):
    assert E.same_bits(np.asarray(got, F32), np.asarray(want, F32)), (tag,) + E.first_difference(np.asarray(got, F32), np.asarray(want, F32))


# ------------------------------------------------------------------------------------------------ K6
class PgDevice(object):
    """A case's g, idx and alpha on the device, g and idx at the given byte phases of a 16-byte granule."""

    def __init__(self, case, idx_bytes, g_phase=0, idx_phase=0, g=None):
        assert 0 <= case.idx.min() and case.idx.max() < case.k               # (an index past k would leave the kernel's table)
        self.case, self.idx_bytes, self.g_phase = case, idx_bytes, g_phase
        self.kg, self.gp = inp(case.g if g is None else g, g_phase)
        self.ki, self.ip = inp(case.idx.astype(np.int64 if idx_bytes == 8 else np.uint8), idx_phase)
        self.ka, self.ap = inp(case.alpha, 8)

    def g_view(self):
        return self.kg[self.g_phase:self.g_phase + 4 * self.case.n].view(torch.float32)

    def run(self, lib):
        c = self.case
        out = Out(F32, c.k, 0)
        rc = lib.qd_point_grad_f32(self.gp, self.ip, self.idx_bytes, self.ap, c.n, c.bucket or 0, c.k, out.ptr, *stream_tail())
        assert rc == 0, (c.id, rc)
        torch.cuda.synchronize()
        return out.get()


def assert_pg_trips(path, case):
    """Under each cap: two trips of the unrolled loop and a per-lane tail behind them (k_point_grad_fast), three rounds
    (k_point_grad_turns / _any) -- and what test_hip_grid_trips.py asserts of the same launch."""
    n, k = case.n, case.k
    assert_trips('k_point_grad_*', n // 4 // 8, n, 256 * 4 * 2, 256, own_cap=512)
    for cap in E.CAPS:
        geo = E.pg_geometry(path, n, k, cap)
        if 'unrolled' in geo:
            assert geo['unrolled'] >= 2 and geo['tail_first'] < n // 4, (case.id, cap, geo)
        else:
            assert geo['rounds'] >= 3, (case.id, cap, geo)
    assert n % 4 != 0 and (case.bucket is None or n % case.bucket != 0)


def run_pg_case(lib, case, idx_bytes, caps=ALL_CAPS, g_phase=0, idx_phase=0, kernel=None, trips=True):
    want, _ = E.pg_expected(case)                                            # (asserts the order-free condition)
    path = E.pg_path(case.k, idx_bytes, case.n, case.bucket, g_phase, idx_phase)
    assert kernel is None or path['kernel'] == kernel, (case.id, path)
    if trips:
        assert_pg_trips(path, case)
    d = PgDevice(case, idx_bytes, g_phase, idx_phase)
    for cap in caps:
        with C.Capped(lib, cap):
            got = d.run(lib)
        assert_bits(got, want, (case.id, path['kernel'], 'idx bytes', idx_bytes, 'phases', g_phase, idx_phase, 'cap', cap))


@pytest.mark.parametrize('k', E.PG_K)
def test_point_gradient_bit_for_bit_on_every_path(lib, k):
    kernel = E.PG_KERNEL_OF_K[k]
    for idx_bytes in (8, 1) if k <= 256 else (8,):
        for bucket in E.PG_BUCKETS:
            for n in E.PG_LENGTHS:
                run_pg_case(lib, E.pg_case(n, k, bucket), idx_bytes, kernel=kernel)
        run_pg_case(lib, E.pg_case(E.PG_N, k, 100, scaled=True), idx_bytes, kernel=kernel)
        for g_phase, bucket in zip(E.PG_G_PHASES, (7, 256)):                 # 16-byte loads of g at a dword-aligned address
            run_pg_case(lib, E.pg_case(E.PG_N, k, bucket), idx_bytes, g_phase=g_phase, kernel=kernel)
        run_pg_case(lib, E.pg_case(E.PG_N, k, 256, kind='one'), idx_bytes, kernel=kernel)
    assert lib_cap_is_default()


@pytest.mark.parametrize('route', E.pg_any_routes(), ids=lambda r: 'k%d-idx%d-g+%d-idx+%d-bucket%s' % r)
def test_point_gradient_scalar_kernel_by_every_route(lib, route):
    k, idx_bytes, g_phase, idx_phase, bucket = route
    run_pg_case(lib, E.pg_case(E.PG_N, k, bucket), idx_bytes, g_phase=g_phase, idx_phase=idx_phase, kernel='any')
    assert lib_cap_is_default()


def test_point_gradient_at_the_full_grid(lib):
    """n = 2^21 + 3, g in {+-1}, alpha in {1, 2}: 2 n <= 2^24.  512 blocks, every one of them in the unrolled loop, and the
    512-row fold."""
    case = E.pg_case(E.PG_BIG_N, 64, 100, small=True)
    path = E.pg_path(64, 1, case.n, 100)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    geo = E.pg_geometry(path, case.n, 64, 1 << 20)
    assert geo['blocks'] == 512 <= 2 * cus and geo['unrolled'] >= 1, (geo, cus)      # (64 KiB tables: two resident blocks per compute unit)
    run_pg_case(lib, case, 1, caps=(None,), kernel='merged', trips=False)


@pytest.mark.parametrize('k', [4, 16, 64, 128, 256, 1024])
def test_point_gradient_one_hot_markers(lib, k):
    """g = 0 but g[e] = 1: alpha[bucket(e)] in bin idx[e], +0.0 everywhere else -- at the elements where a loop hands over to
    the next, under cap 2 (the unrolled loop, then the tail) and uncapped."""
    n = E.PG_LENGTHS[-1]
    for idx_bytes in (8, 1) if k <= 256 else (8,):
        for bucket in E.PG_BUCKETS:
            case = E.pg_case(n, k, bucket)
            path = E.pg_path(k, idx_bytes, n, bucket)
            assert path['kernel'] == E.PG_KERNEL_OF_K[k]
            d = PgDevice(case, idx_bytes, g=np.zeros(n, F32))
            gv = d.g_view()
            for cap in (2, None):
                for e in E.pg_marker_positions(path, n, k, bucket, cap if cap else 1 << 20):
                    gv[e] = 1.0
                    with C.Capped(lib, cap):
                        got = d.run(lib)
                    gv[e] = 0.0
                    assert_bits(got, E.pg_marker_expected(case, e), (case.id, path['kernel'], idx_bytes, 'cap', cap, 'element', e))
    assert lib_cap_is_default()


# ------------------------------------------------------------------------------------------------ K6m
def build_multi(mc):
    """MultiTensorDiffQuant over the case's tensors, its index and alpha columns overwritten in place with the case's."""
    from quantized_distillation_amd.multi_tensor import MultiTensorDiffQuant
    xs = [torch.zeros(n, dtype=torch.float32, device=DEV) for n in mc.sizes]
    outs = [torch.empty_like(x) for x in xs]
    grads = [dev(g) for g in mc.g]
    mt = MultiTensorDiffQuant(xs, outs, grads, mc.k, mc.bucket)
    held = mt._held()
    for i, n in enumerate(mc.sizes):
        if n:
            a = mt.scalings[i].alpha
            assert a.numel() == mc.alpha[i].size and mt.indices[i].numel() == n
            a.view(-1).copy_(torch.from_numpy(mc.alpha[i]))
            mt.indices[i].copy_(torch.from_numpy(mc.idx[i].astype(np.uint8)))
    assert mt._held() == held
    return mt, grads


@pytest.mark.parametrize('bucket', E.M_BUCKETS)
@pytest.mark.parametrize('k', E.M_K)
def test_multi_tensor_point_gradient_bit_for_bit(lib, k, bucket):
    mc = E.m_case(k, bucket)                                                 # (asserts the order-free condition tensor by tensor)
    nt = len(mc.sizes)
    mt, grads = build_multi(mc)
    want = np.stack(mc.want)
    for cap in (None, 1):                                                    # (a fixed grid: the cap must not change it)
        with C.Capped(lib, cap):
            got = mt.backward()
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        for i in range(nt):
            assert_bits(got[i], want[i], ('K6m', k, bucket, 'cap', cap, 'tensor', i, mc.sizes[i]))
    # the per-tensor call on the same device buffers
    for i, n in enumerate(mc.sizes):
        if n:
            out = Out(F32, k, 0)
            rc = lib.qd_point_grad_f32(grads[i].data_ptr(), mt.indices[i].data_ptr(), 1, mt.scalings[i].alpha.data_ptr(), n, bucket or 0, k,
                                       out.ptr, *stream_tail())
            assert rc == 0
            torch.cuda.synchronize()
            assert_bits(out.get(), want[i], ('K6 per tensor', k, bucket, 'tensor', i, n))
    # one-hot markers across tensor and tile boundaries: the whole [tensors, k] result
    for g in grads:
        g.zero_()
    for i, e in E.m_marker_positions(mc.sizes):
        grads[i][e] = 1.0
        got = mt.backward()
        torch.cuda.synchronize()
        grads[i][e] = 0.0
        exp = np.zeros((nt, k), F32)
        _, row = E.geometry(mc.sizes[i], bucket)
        exp[i, mc.idx[i][e]] = mc.alpha[i][e // row]
        assert_bits(got.cpu().numpy(), exp, ('K6m marker', k, bucket, 'tensor', i, 'element', e))
    assert lib_cap_is_default()


# ------------------------------------------------------------------------------------------------ K7
def ste_call(lib, case, tie, phase):
    kx, xp = inp(case.x, phase)
    kg, gp = inp(case.g, phase)
    out = Out(F32, case.n, phase)
    rc = lib.qd_ste_bucket_backward_f32(xp, gp, out.ptr, case.n, case.bucket, case.s, 0 if tie == 'reference' else 1, _lib.stream_ptr())
    assert rc == 0, (case.id, rc)
    torch.cuda.synchronize()
    return out.get()


@pytest.mark.parametrize('shape', E.ste_shapes(), ids=lambda s: '%d-%d-%d-%s' % s)
def test_ste_bucket_sums_bit_for_bit(lib, shape):
    """The WHOLE output: g everywhere, g + S and g - S at the two touched places of every bucket, S with one possible value.
    The register tiles (rows 64 .. 1024) with the ragged last bucket behind them in ste_wave_bucket, ste_wave_bucket for every
    other row; phase 4: the same kernels with x, g and out 4 bytes into a 16-byte granule (fp32 data needs four-byte alignment
    only, csrc/qd_common.h: kDataAlign).  x times 2^-104 takes the IEEE division (exact_sum_cases.STE_SCALES)."""
    bucket, nfull, tail, what = shape
    if what == 'vec':
        bpw = 4 if bucket <= 256 else 1
        assert_trips('k_ste_backward_vec', -(-nfull // bpw), -(-nfull // bpw), 4, 4)
    elif what == 'wave':
        assert_trips('k_ste_backward', nfull + 1, nfull + 1, 4, 4)
    for s, den in E.STE_LEVELS:
        for scale in E.STE_SCALES:
            case = E.ste_case(s, den, bucket, nfull, tail, scale)
            for tie in E.STE_TIES:
                want, _ = E.ste_expected(case, tie)                          # (asserts the order-free condition bucket by bucket)
                for phase in (0, 4):
                    for cap in ALL_CAPS:
                        with C.Capped(lib, cap):
                            got = ste_call(lib, case, tie, phase)
                        assert_bits(got, want, (case.id, tie, 'phase', phase, 'cap', cap))
    assert lib_cap_is_default()


@pytest.mark.parametrize('tie', E.STE_TIES)
@pytest.mark.parametrize('bucket', [256, 100])
def test_multi_tensor_ste_bit_for_bit(lib, bucket, tie):
    from quantized_distillation_amd import ste
    from quantized_distillation_amd.multi_tensor import MultiTensorSTE
    cases = [E.ste_case(E.STE_LEVELS[r][0], E.STE_LEVELS[r][1], bucket, nfull, t) for r, nfull, t in E.MSTE_TENSORS * 2]     # (twice: three trips under cap 3)
    wants = [E.ste_expected(c, tie)[0] if c.n else np.zeros(0, F32) for c in cases]
    xd, gd = [dev(c.x) for c in cases], [dev(c.g) for c in cases]
    outs = [torch.empty_like(g) for g in gd]
    mt = MultiTensorSTE(xd, gd, [c.s for c in cases], bucket, outs=outs, tie_mode=tie)
    assert_trips('k_multi_ste_lv', mt._tiles, mt._tiles, 4, 4)
    for cap in ALL_CAPS:
        for o in outs:
            o.fill_(float('nan'))
        with C.Capped(lib, cap):
            res = mt.backward()
        torch.cuda.synchronize()
        assert mt.entry_point == 'qd_multi_ste_backward_levels_f32'
        for i, c in enumerate(cases):
            assert_bits(res[i].cpu().numpy(), wants[i], ('K7m', bucket, tie, 'cap', cap, 'tensor', i, c.id))
    for i, c in enumerate(cases):
        if c.n:
            one = ste.ste_bucket_backward(xd[i], gd[i], bucket, c.s, out=torch.empty_like(gd[i]), tie_mode=tie)
            assert_bits(one.cpu().numpy(), wants[i], ('K7 per tensor', bucket, tie, 'tensor', i, c.id))
    assert lib_cap_is_default()


# ------------------------------------------------------------------------------------------------ the mean
@pytest.mark.parametrize('n', E.MEAN_N)
def test_mean_bit_for_bit(lib, n):
    x = E.mean_data(n)
    want = E.mean_expected(x)                                                # (asserts the condition under 2^53)
    if n >= 8191:                                                            # float4s over the threads of min(ceil(n / 8192), 1024, cap) blocks
        for cap in E.CAPS:
            assert (n // 4) // (min(-(-n // 8192), 1024, cap) * 256) >= 3
    for phase in (0, 4):                                                     # the float4 loop and its leftovers, aligned and 4 bytes into a granule
        kx, xp = inp(x, phase)
        for cap in ALL_CAPS:
            m = Out(F32, 1, 0)
            with C.Capped(lib, cap):
                assert lib.qd_mean_f32(xp, n, m.ptr, *stream_tail()) == 0
            torch.cuda.synchronize()
            assert_bits(m.get(), np.array([want]), ('qd_mean_f32', n, 'phase', phase, 'cap', cap))
    assert lib_cap_is_default()
