"""tests/abs_cases.py without a GPU: the oracle's 'absmax' / 'absnorm' rules against a second, independent statement of the
same math in torch's CPU ops (oracle/torch_port.py: abs_scaling_torch_ops), on every case; and the structural claims the case
file makes about the launches it means to reach.  The reference's own code for these types raises, so two independent CPU
statements that agree are what stands behind the rules of include/qd_hip.h."""
import numpy as np
import pytest
import torch

import abs_cases as ac
import quantization
from oracle import oracle_np as onp
from oracle import torch_port


def _port_and_oracle(case):
    x = torch.from_numpy(case.x.copy())
    sub = bool(case.options.get('subtract_mean', False))
    me = case.options.get('max_element', False)
    mean = float(x.mean()) if sub else None                       # one mean for both: its summation order is not the subject
    own = torch_port.abs_scaling_torch_ops(x, case.kind, case.s, case.bucket, None, mean, me)
    norm_t = own['norm'].numpy()
    # the norm: absmax bit for bit, absnorm within the bound of the exact value and of the oracle's class
    ac.check_norm(case, norm_t, mean)
    ref = ac.norm_reference(case, mean)
    if case.kind == 'absnorm':
        ac.check_norm(case, ref.norm, mean)
    # everything else bit for bit given a common norm (the oracle's)
    port = torch_port.abs_scaling_torch_ops(x, case.kind, case.s, case.bucket, ref.norm, mean, me)
    want = ac.expect(case, ref.norm, mean)
    assert ac.bits_same(port['sign'], want['sign']) and ac.sign_same(port['sign'], want['sign']), (case.id, 'sign')
    for name in ('u', 'q', 'back'):
        assert ac.bits_same(port[name], want[name]), (case.id, name)
    return want


GROUPS = ('loop', 'many', 'single', 'option', 'nonfinite', 'scale', 'absorbed')


@pytest.mark.parametrize('group', GROUPS)
def test_oracle_agrees_with_torch_ops(group):
    count = 0
    for name, cases in ac.all_groups():
        if name != group:
            continue
        for case in cases:
            _port_and_oracle(case)
            count += 1
    assert count > 0


def test_rules_on_one_bucket():
    """The rules of the header, spelled out on the oracle (the test above ties it to torch): a NaN poisons its bucket and no
    other, sign is 0 for NaN and +-0, an infinity makes the norm +inf, u 0 or NaN, q and the way back NaN."""
    x = np.array([1.0, -2.0, np.nan, 0.5, 0.0, -0.0, 3.0, -np.inf, 1e-40, -1e-40, 2.0, 2.0], np.float32)
    x[2] = ac.NONFINITE_VALUES['nan_neg'][0]
    for kind in ac.KINDS:
        e = ac.expect(ac._case('rules', x, 6, kind))
        assert np.isnan(e['norm'][0]) and e['norm'][1] == np.inf
        assert np.array_equal(e['sign'], np.array([1, -1, 0, 1, 0, 0, 1, -1, 1, -1, 1, 1], np.float32))
        assert np.isnan(e['u'][:6]).all() and np.isnan(e['q']).all() and np.isnan(e['back']).all()
        assert np.array_equal(e['u'][6:], np.array([0, np.nan, 0, 0, 0, 0], np.float32), equal_nan=True)
    # a ragged last bucket whose last element is a NaN: the padding holds u = NaN and sign = 0
    x = np.arange(1, 8, dtype=np.float32)
    x[-1] = np.nan
    for kind in ac.KINDS:
        e = ac.expect(ac._case('pad', x, 4, kind))
        assert np.isnan(e['u'][4:]).all() and not np.isnan(e['u'][:4]).any() and np.array_equal(e['sign'][6:], [0.0, 0.0])
    # the padding enters an L2 norm
    e = ac.expect(ac._case('pad', np.array([3, 4, 0, 0, 2], np.float32), 4, 'absnorm'))
    assert np.array_equal(e['norm'], np.array([5.0, 4.0], np.float32))


def test_structural_claims():
    """What the case file says about the launches: more buckets than the capped grid has waves, planted positions outside the
    first partial block, the grid-stride trip of the partial kernel, the two-stage threshold on both sides."""
    nb = onp.bucket_geometry(ac.MANY_N, ac.MANY_BUCKET)[0]
    assert nb > 262144 and nb > ac.GRID_MAX_BLOCKS * ac.WAVES_PER_BLOCK
    assert ac.SINGLE_BIG_N > ac.PART_MAX_BLOCKS * ac.PART_PER_BLOCK and ac.SINGLE_BIG_N < 1e8
    assert ac.partial_blocks(ac.SINGLE_BIG_N) == ac.PART_MAX_BLOCKS
    assert not ac.is_two_stage(65536, None) and ac.is_two_stage(65537, None) and ac.is_two_stage(70000, 100000)
    assert not ac.is_two_stage(5000, None) and not ac.is_two_stage(70001, 256)
    for n, bucket in ac.NONFINITE_SHAPES:
        pos = ac.nonfinite_positions(n, bucket)
        assert pos['first'] == 0 and pos['last'] == n - 1
        if bucket is not None:
            nbk = onp.bucket_geometry(n, bucket)[0]
            b = pos['mid_last'] // bucket
            assert (pos['mid_last'] + 1) % bucket == 0 and (0 < b < nbk - 1 or nbk < 3), (n, bucket, pos)
        if ac.is_two_stage(n, bucket):
            assert pos['past'] > 8192 * 3 and ac.partial_block_of(pos['past'], n) != 0
            assert ac.partial_block_of(pos['last'], n) != 0 and ac.partial_blocks(n) > 1
    assert any(ac.is_two_stage(n, b) for n, b in ac.NONFINITE_SHAPES) and any(n % b for n, b in ac.NONFINITE_SHAPES if b)
    for bucket in ac.LOOP_BUCKETS:                                   # tails under one wave, one wave, more than one
        assert all(n >= 1 for n in ac.loop_lengths(bucket)) and 3 * bucket + -(-bucket // 2) in ac.loop_lengths(bucket)
    # the two-stage absorbed case: every thread of the first sweep starts on a large element
    case = list(ac.absorbed_cases())[2]
    head = ac.partial_blocks(case.x.size) * ac.PART_THREADS
    assert ac.is_two_stage(case.x.size, case.bucket) and (case.x[:head] == 16384.0).all() and (case.x[head:] == np.float32(3.9)).all()
    assert case.x.size % head == 0 and case.x.size // head == 32


def test_overflow_margins():
    """Every absnorm case is a factor four away from the edge where the order of the sum decides between a number and +inf."""
    for name, cases in ac.all_groups():
        for case in cases:
            if case.kind == 'absnorm' and name != 'loop':           # (the loop group is randn: one check per bucket size)
                assert ac.overflow_margin(case), case.id
    for bucket in ac.LOOP_BUCKETS:
        assert all(ac.overflow_margin(c) for c in ac.loop_cases('absnorm', bucket) if c.s == 8)
    sums = {c.id: float((c.x.astype(np.float64) ** 2).sum()) for c in ac.scale_cases() if '1e17' in c.id}
    assert abs(sums['scale-absnorm-1e17'] / 2.56e36 - 1) < 1e-6 and all(s < 2.0 ** 126 for s in sums.values())
    cls = {c.id: ac.norm_reference(c).cls for c in ac.scale_cases()}
    assert (cls['scale-absnorm-1e20'] == 'inf').all() and (cls['scale-absnorm-1e20-two-stage'] == 'inf').all()
    assert list(cls['scale-absnorm-1e20-middle']) == ['num', 'inf', 'num']
    assert (cls['scale-absnorm-1e17'] == 'num').all() and (cls['scale-absnorm-1e17-ragged'] == 'num').all()
    for kind in ac.KINDS:
        assert (cls['scale-%s-1e-30' % kind] == 'one').all() and (cls['scale-%s-denormal' % kind] == 'one').all()
        assert list(cls['scale-%s-zero-bucket' % kind]) == ['num', 'one', 'num']
    assert list(cls['scale-absmax-at-guard']) == ['num'] and list(cls['scale-absmax-below-guard']) == ['one']


def test_absorbed_tails_bite():
    """An fp32 running sum per lane / thread misses the norm bound on the first three absorbed-tail cases (so they can fail),
    meets it on the controls, and the oracle meets it on all of them."""
    cases = list(ac.absorbed_cases())
    for i, case in enumerate(cases):
        ref = ac.norm_reference(case)
        ratio = float(np.max(np.abs(ac.naive_lane_norm(case) - ref.norm64) / ref.norm64))
        if i < ac.ABSORBED_BITING:
            assert ratio > ac.BOUND, (case.id, ratio)
        else:
            assert ratio <= ac.BOUND, (case.id, ratio)
        assert ac.check_norm(case, ref.norm) <= 2.0 ** -23
    one = cases[0]
    lane_sum = float(ac.naive_lane_norm(one)[0] ** 2)
    assert lane_sum == 1073741824.0 and abs(float(ref_sum(one)) - 1073773905.0) < 1.0


def ref_sum(case):
    return (case.x.astype(np.float64) ** 2).sum()


@pytest.mark.parametrize('kind', ac.KINDS)
def test_cpu_tensors_still_raise(kind):
    x = torch.randn(1000)
    with pytest.raises(NotImplementedError, match='HIP device only'):
        quantization.ScalingFunction(kind, False, False, 256).scale_down(x)
    with pytest.raises(NotImplementedError, match='HIP device only'):
        quantization.uniformQuantization(x, 8, type_of_scaling=kind, bucket_size=256)
    sf = quantization.ScalingFunction(kind, False, False, 256)
    sf.tensor_sign, sf.norm_scaling = torch.ones(4, 256), torch.ones(4, 1)
    sf.original_tensor_length, sf.original_tensor_size, sf._n = 1000, x.size(), 1000
    with pytest.raises(NotImplementedError, match='HIP device only'):
        sf.inv_scale_down(torch.zeros(4, 256))
