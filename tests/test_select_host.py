"""The cases of tests/select_cases.py without a GPU: the expected answers (an integer sort of order keys) agree with numpy's
own float sort, the case conditions hold, and order_statistics on CPU tensors (np.partition) returns them -- which proves
the cases before tests/test_hip_select.py holds the device select and the device sort fallback to the same answers.
initialize_quantization_points on tensors with a NaN or an infinity, on CPU tensors, against the staged reference's own
function."""
import importlib

import numpy as np
import pytest
import torch

import quantization
import quantization.help_functions as qhf
import select_cases as S
from oracle import ref_stage

GROUP_IDS = sorted(S.GROUPS)


def test_the_case_table_is_the_documented_one():
    assert S.NAN_PAYLOADS == (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF)
    assert S.BLOCK_COUNTS == (1, 2, 3, 5, 17, 61, 64, 65, 67, 129, 256) and S.SPAN_NVEC == (0, 1, 1023, 1024, 1025, 4095, 4096, 4097)
    assert len(S.NONFINITE_IDS) == 12 and len(S.SPAN_TINY_IDS) == 9 and len(S.PREFIX_IDS) == 9 and len(S.WRAPPER_IDS) == 6
    assert [len(S.span_ids(v)) for v in S.SPAN_NVEC] == [15] + [16] * 7           # head 0..3 x tail 0..3, less n = 0
    assert sum(S.blocks_n(b) for b in S.BLOCK_COUNTS) == 659 * 16384 + 11
    heads = {off: S.head_of(off, 100) for off in range(4)}
    assert heads == {0: 0, 1: 3, 2: 2, 3: 1} and S.head_of(1, 2) == 2              # n < head
    assert len(S.PCT_SHAPES) == 12 and len(S.PCT_POISONS) == 13


def test_order_keys():
    """The key arithmetic of the expected answer on the patterns that matter: every NaN on the one largest key, above +inf's;
    -inf's key the smallest of a number; -0 directly before +0; the mapping back inverts it."""
    k = lambda b: int(S.keys_of(np.array([b], S.U32))[0])                        # noqa: E731
    assert all(k(p) == 0xFFFFFFFF for p in S.NAN_PAYLOADS) and k(S.POS_INF) == 0xFF800000 < 0xFFFFFFFF
    assert k(S.NEG_INF) == 0x007FFFFF and k(0xFF7FFFFF) == 0x00800000 and k(0x80000000) + 1 == k(0) == 0x80000000
    assert k(0x80000001) + 1 == k(0x80000000) and k(1) == k(0) + 1 and k(0x7F7FFFFF) + 1 == k(S.POS_INF)
    b = S.distinct_finite(np.random.RandomState(0), 5000)
    assert np.array_equal(S.bits_of_keys(S.keys_of(b)), b)
    assert np.isnan(S.bits_of_keys(np.array([S.NAN_KEY], S.U32)).view(np.float32)[0])


@pytest.mark.parametrize('group', GROUP_IDS)
def test_expected_answers_are_numpys_float_sort(group):
    """np.sort of the FLOATS (NaNs last whatever their sign, as the float comparison has it) gives the same values as the
    integer sort of the keys: the expected answer does not rest on the key arithmetic alone."""
    for cid in S.GROUPS[group]:
        c = S.case(cid)
        S.check_conditions(c)
        if c.ranks.size:
            S.same(np.sort(c.logical_bits().view(np.float32), kind='stable')[c.ranks], c.expected(), cid)


@pytest.mark.parametrize('group', GROUP_IDS)
def test_order_statistics_of_cpu_tensors(group):
    for cid in S.GROUPS[group]:
        c = S.case(cid)
        got = S.run(c, 'host')
        assert got.dtype == np.float32 and got.shape == c.ranks.shape, cid
        S.same(got, c.expected(), (cid, 'host'))


def test_the_comparison_rejects_what_it_must():
    """same(): a NaN where a number is expected, a number where a NaN is expected, and one differing bit all fail; +-0 pass."""
    want = np.array([0x80000000, 0x3F800000, 0x7FFFFFFF], S.U32).view(np.float32)
    S.same(np.array([0x00000000, 0x3F800000, 0xFFC00000], S.U32).view(np.float32), want)
    for bad in ([0, 0x3F800001, 0x7FC00000], [0, 0x7FC00000, 0x7FC00000], [0, 0x3F800000, 0x7F800000], [1, 0x3F800000, 0x7FC00000]):
        with pytest.raises(AssertionError):
            S.same(np.array(bad, S.U32).view(np.float32), want)


@pytest.mark.parametrize('shape', S.PCT_SHAPES, ids=S.PCT_SHAPE_IDS)
def test_percentile_points_of_nonfinite_cpu_tensors_equal_the_references(shape):
    """np.percentile (the reference's line, help_functions.py:150) returns NaN for EVERY point once the scaled tensor holds
    one NaN; one +-inf makes its bucket's scaled values NaN, so it is the same case."""
    refq = ref_stage.load()
    assert refq is not None, 'oracle/_ref is not staged (run __graft_entry__.build() where the reference exists)'
    refh = importlib.import_module(refq.__name__ + '.help_functions')
    for cid, x, bucket, k in S.percentile_cases(shape):
        t = torch.from_numpy(x)
        with np.errstate(invalid='ignore'):
            want = refh.initialize_quantization_points(t, refq.ScalingFunction('linear', False, False, bucket), k)
        got = qhf.initialize_quantization_points(t, quantization.ScalingFunction('linear', False, False, bucket), k)
        assert got.dtype == want.dtype and got.device == want.device
        S.same_points(got.numpy(), want.numpy(), cid)
        assert bool(np.isnan(want.numpy()).all()) == ('clean' not in cid), cid      # what the cases are for
        assert np.isnan(want.numpy()).any() == np.isnan(want.numpy()).all(), cid


def test_one_percentile_point_of_a_tensor_with_a_nan():
    """num_points = 1 asks for the 0th percentile only: rank n - 1 is fetched all the same, and the point is NaN."""
    x = S.percentile_input(2000, 0xFFC00000, 'middle')
    got = qhf.initialize_quantization_points(torch.from_numpy(x), quantization.ScalingFunction('linear', False, False, 256), 1)
    sf = quantization.ScalingFunction('linear', False, False, 256)
    with np.errstate(invalid='ignore'):
        want = np.percentile(sf.scale_down(torch.from_numpy(x)).view(-1)[0:2000].numpy(), np.linspace(0, 100, num=1))
    assert np.isnan(want).all()
    S.same_points(got.numpy(), want.astype(np.float32))
