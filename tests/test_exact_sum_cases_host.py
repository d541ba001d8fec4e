"""tests/exact_sum_cases.py without a GPU: every case is order-free (a condition on the terms, asserted in float64 and integer
arithmetic), so the numpy oracle, the C oracle, a running fp32 sum over a shuffled order and libqd_host.so all have to give the
same BITS -- and the cases aim where the case file says they do (the dispatcher's paths, the loops' trips, the partitions every
lane position meets).  This proves the cases before tests/test_hip_exact_sums.py shows them to a kernel."""
import numpy as np
import pytest

import exact_sum_cases as E
from oracle import oracle_c as oc
from oracle import oracle_np as onp
from quantized_distillation_amd import _lib

F32 = np.float32
NAN_BITS = 0x7FC0BEEF


@pytest.fixture(scope='module')
def host():
    return _lib.host()


def sentinel(count):
    return np.full(count, NAN_BITS, np.uint32).view(F32)


def host_point_grad(host, case, idx_bytes, g=None):
    g = case.g if g is None else g
    idx = np.ascontiguousarray(case.idx.astype(np.int64 if idx_bytes == 8 else np.uint8))
    out = sentinel(case.k)
    rc = host.qd_point_grad_f32(g.ctypes.data, idx.ctypes.data, idx_bytes, case.alpha.ctypes.data, case.n, case.bucket or 0, case.k,
                                out.ctypes.data, None, 0, None)
    assert rc == 0, (case.id, rc)
    return out


def assert_bits(got, want, tag):
    assert E.same_bits(np.asarray(got, F32), want), (tag,) + E.first_difference(np.asarray(got, F32), want)


def check_pg_case(host, case, thorough):
    want, t = E.pg_expected(case)                                            # (asserts the condition)
    assert np.all(case.g != 0) and np.all(t != 0)                            # a wrong alpha or bin always changes a sum
    out_c, _ = oc.point_grad(case.g, case.idx, case.alpha, case.bucket, case.k)
    assert_bits(out_c.astype(F32), want, (case.id, 'C oracle'))
    if thorough:
        out_np, _ = onp.point_grad(case.g, case.idx, case.alpha, case.bucket, case.k)
        assert_bits(out_np.astype(F32), want, (case.id, 'numpy oracle'))
        out32, _ = onp.point_grad(case.g, case.idx, case.alpha, case.bucket, case.k, dtype=F32)       # fp32 accumulation in memory order
        assert_bits(out32, want, (case.id, 'numpy oracle, fp32'))
        assert_bits(E.shuffled_fp32_sums(t, case.idx, case.k, 17), want, (case.id, 'shuffled fp32 running sum'))
    for idx_bytes in (8, 1) if case.k <= 256 else (8,):
        assert_bits(host_point_grad(host, case, idx_bytes), want, (case.id, 'libqd_host.so', idx_bytes))


# ------------------------------------------------------------------------------------------------ the helpers themselves
def test_the_condition_refuses_what_depends_on_the_order():
    t = np.array([1.0, 2.0 ** 24, -1.0], F32)                               # 2^24 + 2 units
    with pytest.raises(AssertionError):
        E.order_free(t, np.zeros(3, np.int64), 1)
    assert E.order_free(t[:2], np.array([0, 1]), 2) == (1.0, 1 << 24)
    with pytest.raises(AssertionError):
        E.order_free(np.array([0.75], F32), np.zeros(1, np.int64), 1, unit=0.5)
    assert E.unit_of(np.array([0.75, 6.0, 0.0])) == 0.25 and E.unit_of(np.zeros(3)) == 1.0
    assert E.bits(E.exact_sums(np.array([1.0, -1.0], F32), np.array([1, 1]), 3)).tolist() == [0, 0, 0]        # +0.0, also where terms cancel
    third = E.round_once_to_f32(E.fractions.Fraction(1, 3))
    assert third == F32(1.0) / F32(3.0)
    ulp = E.fractions.Fraction(1, 2 ** 23)
    assert E.round_once_to_f32(1 + ulp / 2) == F32(1.0) and E.round_once_to_f32(1 + 3 * ulp / 2) == F32(1.0) + F32(2.0 ** -22)   # ties: to even


def test_every_lane_position_meets_the_fifteen_partitions():
    assert sorted(set(E.PARTITIONS)) == E.PARTITIONS and E.PARTITIONS[0] == (0, 0, 0, 0) and E.PARTITIONS[-1] == (0, 1, 2, 3)
    for k in (5, 17, 65, 256, 1024):
        for n in (E.PG_N, E.M_BASE[-1]):
            idx, empty = E.pg_indices(n, k, 3)
            npat = min(n // 4, E.PATTERN_ROWS * 256)
            code = E.partition_code(idx[:4 * npat].reshape(-1, 4))
            i = np.arange(npat)
            assert np.array_equal(code, (i + i // 256) % 15), k             # the bins of a float4's blocks are distinct: the pattern is the planned one
            if npat >= 15 * 256:
                seen = np.zeros((256, 15), bool)
                seen[i % 256, code] = True
                assert seen.all(), k
            assert np.any(idx[:4 * npat] == 0) and np.any(idx[:4 * npat] == k - 1) and not np.any(idx == empty)
            assert idx.min() >= 0 and idx.max() == k - 1


def test_the_dispatcher_reaches_what_the_cases_aim_at():
    for k in E.PG_K:
        for idx_bytes in (8, 1) if k <= 256 else (8,):
            for bucket in E.PG_BUCKETS:
                for n in E.PG_LENGTHS:
                    path = E.pg_path(k, idx_bytes, n, bucket)
                    assert path['kernel'] == E.PG_KERNEL_OF_K[k], (k, idx_bytes, bucket)
                    assert n % 4 != 0 and (bucket is None or n % bucket != 0)       # leftovers, a ragged last bucket
                    for cap in E.CAPS:
                        geo = E.pg_geometry(path, n, k, cap)
                        assert geo['blocks'] == cap
                        if 'unrolled' in geo:                                 # two trips of the unrolled loop, then the per-lane tail
                            assert geo['unrolled'] >= 2 and geo['tail_first'] < n // 4 < geo['tail_first'] + 4 * geo['nth'], (k, cap, geo)
                        else:
                            assert geo['rounds'] >= 3, (k, cap, geo)
                    pos = E.pg_marker_positions(path, n, k, bucket, 2)
                    assert {0, 3, 4, n - 1, 4 * (n // 4) - 1, 4 * (n // 4)} <= set(pos)
    assert {n % 4 for n in E.PG_LENGTHS} == {1, 2, 3}
    # BucketWalk's splits: the edges of buckets of 7 elements fall 0, 1, 2 and 3 elements into a float4; a bucket of 100 (a
    # multiple of 4) walks without ever splitting one
    assert {(b * 7) % 4 for b in range(1, 9)} == {0, 1, 2, 3} and {(b * 100) % 4 for b in range(1, 9)} == {0}
    # the scalar kernel at each of its column widths, by every route
    widths = {}
    for k, idx_bytes, gp, ip, bucket in E.pg_any_routes():
        path = E.pg_path(k, idx_bytes, E.PG_N, bucket, gp, ip)
        assert path['kernel'] == 'any', (k, idx_bytes, gp, ip, bucket)
        widths.setdefault(path['columns'], set()).add('idx' if ip else 'bucket %d' % bucket)
    assert sorted(widths) == [32, 64, 256] and all({'idx', 'bucket 3', 'bucket 2'} <= w for w in widths.values()), widths
    # g at +4 or +12 bytes alone is no route to it: fp32 data needs four-byte alignment only, the fast kernels take it
    for k in E.PG_K:
        assert all(E.pg_path(k, 8, E.PG_N, 7, gp, 0)['kernel'] == E.PG_KERNEL_OF_K[k] for gp in E.PG_G_PHASES)
    # the large case: the full 512-block grid, every block in the unrolled loop
    path = E.pg_path(64, 1, E.PG_BIG_N, 100)
    geo = E.pg_geometry(path, E.PG_BIG_N, 64, 1 << 20)
    assert path['kernel'] == 'merged' and geo['blocks'] == 512 and geo['unrolled'] >= 1 and 2 * E.PG_BIG_N <= E.LIMIT32


# ------------------------------------------------------------------------------------------------ K6
@pytest.mark.parametrize('k', E.PG_K)
def test_point_gradient_cases(host, k):
    for bucket in E.PG_BUCKETS:
        for j, n in enumerate(E.PG_LENGTHS):
            check_pg_case(host, E.pg_case(n, k, bucket), thorough=j == 0 and bucket in (None, 7))
    check_pg_case(host, E.pg_case(E.PG_N, k, 100, scaled=True), thorough=True)
    check_pg_case(host, E.pg_case(E.PG_N, k, 256, kind='one'), thorough=False)
    for kk, idx_bytes, gp, ip, bucket in E.pg_any_routes():
        if kk == k and bucket in (2, 3):
            check_pg_case(host, E.pg_case(E.PG_N, k, bucket), thorough=False)


def test_point_gradient_large_case(host):
    case = E.pg_case(E.PG_BIG_N, 64, 100, small=True)
    assert set(np.unique(case.g)) == {-1.0, 1.0} and set(np.unique(case.alpha)) == {1.0, 2.0}
    check_pg_case(host, case, thorough=False)


@pytest.mark.parametrize('k', [4, 16, 64, 128, 256, 1024])
def test_point_gradient_one_hot_markers(host, k):
    for bucket in E.PG_BUCKETS:
        case = E.pg_case(E.PG_LENGTHS[-1], k, bucket)
        path = E.pg_path(k, 8, case.n, bucket)
        positions = sorted(set(E.pg_marker_positions(path, case.n, k, bucket, 2)) | set(E.pg_marker_positions(path, case.n, k, bucket, 1 << 20)))
        for e in positions:
            g = np.zeros(case.n, F32)
            g[e] = 1.0
            want = E.pg_marker_expected(case, e)
            assert np.count_nonzero(E.bits(want)) == 1
            assert_bits(host_point_grad(host, case, 8, g), want, (case.id, 'marker', e))


# ------------------------------------------------------------------------------------------------ K6m
def test_multi_tensor_list_is_what_the_kernel_needs():
    sizes = E.m_sizes()
    assert len(sizes) == E.M_TENSORS >= 130 and set(E.M_BASE) <= set(sizes)
    assert sizes[0] == sizes[-1] == 0 and sizes[66] == sizes[67] == 0 and sizes.count(E.M_BIG) == 1
    assert any(n >= E.M_TILE for n in sizes[128:])                          # the third ballot group owns full tiles
    assert E.M_BIG // E.M_TILE > E.M_WAVES and E.M_BIG % E.M_TILE != 0 and 2 * E.M_BIG <= E.LIMIT32
    pos = E.m_marker_positions(sizes)
    assert all(0 <= e < sizes[i] for i, e in pos) and (E.M_BIG_AT, E.M_WAVES * E.M_TILE) in pos


@pytest.mark.parametrize('bucket', E.M_BUCKETS)
@pytest.mark.parametrize('k', E.M_K)
def test_multi_tensor_cases(host, k, bucket):
    mc = E.m_case(k, bucket)                                                 # (asserts the condition tensor by tensor)
    for i in (1, 5, 7, 8, E.M_BIG_AT, 135):
        case = E.PgCase('tensor %d' % i, mc.sizes[i], k, bucket, mc.g[i], mc.idx[i], mc.alpha[i], None, 1.0)
        assert_bits(host_point_grad(host, case, 1), mc.want[i], (k, bucket, i, 'libqd_host.so'))
        out_c, _ = oc.point_grad(case.g, case.idx, case.alpha, bucket, k)
        assert_bits(out_c.astype(F32), mc.want[i], (k, bucket, i, 'C oracle'))
    for i in E.M_EMPTY:
        assert E.bits(mc.want[i]).tolist() == [0] * k


# ------------------------------------------------------------------------------------------------ K7
def host_ste(host, case, tie_mode):
    out = sentinel(case.n)
    rc = host.qd_ste_bucket_backward_f32(case.x.ctypes.data, case.g.ctypes.data, out.ctypes.data, case.n, case.bucket, case.s,
                                         0 if tie_mode == 'reference' else 1, None)
    assert rc == 0
    return out


@pytest.mark.parametrize('shape', E.ste_shapes(), ids=lambda s: '%d-%d-%d-%s' % s)
def test_ste_cases(host, shape):
    bucket, nfull, tail, what = shape
    tops = []
    for s, den in E.STE_LEVELS:
        for scale in E.STE_SCALES:
            case = E.ste_case(s, den, bucket, nfull, tail, scale)
            nb, row = E.geometry(case.n, bucket)
            for b in range(nb):                                              # a 0 and an s - 1 in every bucket of two or more
                seg = case.x[b * row:min((b + 1) * row, case.n)]
                assert seg.size < 2 or (seg.min() == 0 and seg.max() == F32(np.ldexp(float(s - 1), scale))), (case.id, b)
            for tie in E.STE_TIES:
                want, info = E.ste_expected(case, tie)                       # (asserts the condition bucket by bucket)
                tops.append(info['top'])
                assert_bits(onp.ste_complicated_backward(case.x, case.g, s, bucket, tie), want, (case.id, tie, 'numpy oracle'))
                if tie == 'reference':
                    assert_bits(oc.ste_complicated_backward(case.x, case.g, s, bucket), want, (case.id, tie, 'C oracle'))
                assert_bits(host_ste(host, case, tie), want, (case.id, tie, 'libqd_host.so'))
                if scale == 0 and what != 'one':
                    assert info['touched'] > 0 and info['unit'] >= 1.0 / ((s - 1) * den), (case.id, info)
                if scale != 0 and tie == 'true_arg' and case.n > 1:          # the sums are visible: +S and -S where g is 0
                    assert info['touched'] > 0 and np.count_nonzero(want != case.g) >= info['touched'], (case.id, info['touched'])
    assert max(tops) <= E.LIMIT32


def test_ste_shuffled_running_sums_give_the_same_bits():
    case = E.ste_case(17, 4, 513, 38, 1)
    tm = onp.ste_bucket_terms(case.x, case.g, 17, 513)
    want, info = E.ste_expected(case, 'reference')
    got_s = info['sums']
    # the terms again, summed as a shuffled fp32 running sum per bucket
    q = onp.uniform_quantize(case.x, 17, 513)['q'].reshape(-1)
    sdq = onp.scale_down(q, 513)
    aq = np.repeat(sdq['alpha'].reshape(-1), 513)[:case.n]
    bq = np.repeat(sdq['beta'].reshape(-1), 513)[:case.n]
    term = (case.g * (sdq['u'].reshape(-1)[:case.n] - ((case.x - bq).astype(F32) / aq).astype(F32)).astype(F32)).astype(F32)
    assert_bits(E.shuffled_fp32_sums(term, np.arange(case.n) // 513, tm['nb'], 5), got_s, 'bucket sums')


def test_multi_ste_list_mixes_levels_and_paths():
    levels = {E.STE_LEVELS[r][0] for r, _, _ in E.MSTE_TENSORS}
    assert levels == {5, 17, 257} and any(nf == 0 and t == 0 for _, nf, t in E.MSTE_TENSORS) and any(nf == 0 and t > 0 for _, nf, t in E.MSTE_TENSORS)


# ------------------------------------------------------------------------------------------------ the mean
@pytest.mark.parametrize('n', E.MEAN_N)
def test_mean_cases(host, n):
    x = E.mean_data(n)
    assert np.all(np.abs(x) < 1024) and np.array_equal(x * 1024, np.rint(x * 1024))
    want = E.mean_expected(x)                                                # (asserts the condition under 2^53)
    out = sentinel(1)
    assert host.qd_mean_f32(x.ctypes.data, n, out.ctypes.data, None, 0, None) == 0
    assert_bits(out, np.array([want]), ('libqd_host.so', n))
    assert_bits(np.array([oc.lib().qdo_mean_f32(oc._p(x, oc._f), n)], F32), np.array([want]), ('C oracle', n))
    assert_bits(np.array([np.mean(x, dtype=np.float64)]).astype(F32), np.array([want]), ('numpy', n))
    rng = np.random.RandomState(n % 101)
    assert_bits(np.array([np.cumsum(x[rng.permutation(n)], dtype=np.float64)[-1] / n]).astype(F32), np.array([want]), ('shuffled float64 running sum', n))
