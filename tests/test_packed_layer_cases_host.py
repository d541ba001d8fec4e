"""tests/packed_layer_cases.py against the oracle and against itself (no GPU): the weight value of every case is the oracle's
fake-quantized tensor bit for bit, the exact cases meet the condition that frees them of the summation order, and the
general-case bound holds for plain numpy fp32 evaluations in two different orders -- the reference alone stays inside it."""
import numpy as np
import pytest

import packed_layer_cases as P


@pytest.mark.parametrize('bits', P.BITS)
def test_weight_values_are_the_oracles(bits):
    """w from the four-operation rule == oracle_c.uniform_quantize(...)['q'] bit for bit (NaN for NaN), the stream decodes to
    the oracle's levels, and every case is the shape it says."""
    cases = P.all_cases(bits)
    assert len(cases) == 2 * len(P.SHAPES) + 2 + len(P.EXACT_SHAPES)
    for c in cases:
        wt = c.weight
        n = wt.rows * wt.cols
        assert wt.bits == bits and 2 <= wt.s <= (1 << bits) and wt.w.shape == (wt.rows, wt.cols)
        assert P.same_floats(wt.w, wt.q), wt.tag
        assert wt.packed.size == (n * bits + 7) // 8
        assert np.array_equal(P.unpack_stream(wt.packed, n, bits), wt.lev) and wt.lev.max() <= wt.s - 1
        assert wt.alpha.size == P.nbuckets(n, wt.bucket)


def test_the_list_covers_what_it_claims():
    cases = [c for b in P.BITS for c in P.all_cases(b)]
    for b in P.BITS:
        mine = [c for c in P.all_cases(b)]
        assert {c.m for c in mine} == set(P.MS) and {c.count for c in mine} == set(P.COUNTS) and {c.phase for c in mine} == set(P.PHASES)
        assert {c.weight.s for c in P.general_cases(b)} == set(P.levels_for(b))
        assert P.exact_cases(b)[0].weight.s == P.EXACT_S[b - 1] and (P.EXACT_S[b - 1] - 1) & (P.EXACT_S[b - 1] - 2) == 0
    shapes = {(c.weight.rows, c.weight.cols) for c in cases}
    assert {r for r, _ in shapes} == {1, 3, 67} and {k for _, k in shapes} == {1, 5, 32, 37, 100, 2085}
    assert {c.weight.bucket for c in cases} == {256, 64, 100, 3, None, P.BIG}
    # rows that start inside a byte / inside a word; buckets that straddle rows; several buckets in a group of four
    assert all((37 * b) % 32 for b in P.BITS) and all((37 * b) % 8 for b in (3, 5, 6, 7)) and not any((32 * b) % 32 for b in P.BITS)
    assert 256 % 37 and 256 % 100 and (67 * 37) > 256
    # the out-of-range indices are -1 and rows, nothing else
    for c in cases:
        idx = P.embedding_indices(c.weight.rows, c.count, c.seed)
        bad = idx[(idx < 0) | (idx >= c.weight.rows)]
        assert set(bad.tolist()) <= {-1, c.weight.rows} and (c.count < 5 or len(bad) == 2)
        assert c.count < 2 or len(np.unique(idx)) < idx.size


@pytest.mark.parametrize('bits', P.BITS)
def test_nonfinite_cases_hold_a_nan_bucket_an_inf_bucket_and_a_nan_in_x(bits):
    bucketed, single = P.nonfinite_cases(bits)
    a = bucketed.weight.alpha
    assert np.isnan(a[0]) and np.isinf(a[-1]) and np.isfinite(a[1:-1]).all()
    assert np.isnan(single.weight.alpha).all()
    for c in (bucketed, single):
        x, bias, _ = P.inputs_of(c)
        assert np.isnan(x[-1]).any() and np.isfinite(x[:-1]).all()
        y64, _ = P.linear_expected(c.weight.w, x, bias)
        assert np.isnan(y64[-1]).all()                                     # the NaN of x reaches its own row of y, every column
        clean_rows = np.isfinite(c.weight.w).all(axis=1)
        assert np.isfinite(y64[:-1][:, clean_rows]).all() and not np.isfinite(y64[:, ~clean_rows]).any()
    assert np.isfinite(bucketed.weight.w).all(axis=1).sum() >= 40          # other rows are unaffected


@pytest.mark.parametrize('bits', P.BITS)
def test_exact_cases_do_not_depend_on_the_order(bits):
    for c in P.exact_cases(bits):
        x, bias, _ = P.inputs_of(c)
        assert bias is not None and P.exact_condition(c.weight, x, bias)
        y64, mag = P.linear_expected(c.weight.w, x, bias)
        fwd = np.zeros((c.m, c.weight.rows), P.F32)
        for k in range(c.weight.cols):                                     # front to back, fp32, multiply then add
            fwd = fwd + x[:, k:k + 1] * c.weight.w[:, k][None, :]
        bwd = np.zeros((c.m, c.weight.rows), P.F32)
        for k in reversed(range(c.weight.cols)):
            bwd = bwd + x[:, k:k + 1] * c.weight.w[:, k][None, :]
        assert fwd.dtype == P.F32 and np.array_equal(fwd + bias, y64) and np.array_equal(bwd + bias, y64)
        assert np.array_equal(y64.astype(P.F32).astype(np.float64), y64)


def _lanes_then_tree(x, w, lanes=64):
    """fp32: `lanes` strided accumulators, column by column, then a pairwise tree."""
    m, rows = x.shape[0], w.shape[0]
    acc = np.zeros((lanes, m, rows), P.F32)
    for k in range(w.shape[1]):
        acc[(k // 4) % lanes] += x[:, k:k + 1] * w[:, k][None, :]
    while acc.shape[0] > 1:
        acc = acc[:acc.shape[0] // 2] + acc[acc.shape[0] // 2:]
    return acc[0]


@pytest.mark.parametrize('bits', (1, 4, 7))
def test_the_bound_holds_for_the_reference_alone_in_two_orders(bits):
    """Serial front to back, and 64 strided lanes + tree, both in numpy fp32 (multiply, then add): each within the bound the
    GPU test applies, with room -- the largest ratio stays below a quarter of it."""
    worst = 0.0
    for c in P.general_cases(bits):
        wt = c.weight
        x, bias, _ = P.inputs_of(c)
        y64, mag = P.linear_expected(wt.w, x, bias)
        serial = np.zeros((c.m, wt.rows), P.F32)
        for k in range(wt.cols):
            serial = serial + x[:, k:k + 1] * wt.w[:, k][None, :]
        tree = _lanes_then_tree(x, wt.w)
        for y in (serial, tree):
            if bias is not None:
                y = y + bias[None, :]
            assert y.dtype == P.F32
            worst = max(worst, P.check_linear(y, y64, mag, wt.tag))
    assert 0 < worst < 0.25 * P.TOL, worst


def test_check_linear_refuses_what_is_outside_the_bound():
    c = P.general_cases(4)[0]
    x, bias, _ = P.inputs_of(c)
    y64, mag = P.linear_expected(c.weight.w, x, bias)
    good = y64.astype(P.F32)
    P.check_linear(good, y64, mag, 'good')
    bad = good.copy()
    bad[0, 0] += P.F32(3e-6 * mag[0, 0])
    with pytest.raises(AssertionError):
        P.check_linear(bad, y64, mag, 'bad')
    bad = good.copy()
    bad[0, 0] = np.nan
    with pytest.raises(AssertionError):
        P.check_linear(bad, y64, mag, 'nan')
    want = P.embedding_expected(c.weight.w, np.array([0, -1, c.weight.rows, 2], np.int64))
    assert np.isnan(want[1]).all() and np.isnan(want[2]).all() and np.array_equal(want[3], c.weight.w[2])
    assert P.same_floats(want, want.copy()) and not P.same_floats(want, np.zeros_like(want))
