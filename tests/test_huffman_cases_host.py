"""The cases of tests/huffman_cases.py through libqd_host.so at the C ABI: the decoded floats equal the float32 formula of
include/qd_hip.h written out in numpy, bit for bit, and chunk_words equals the word counts that follow from the code lengths.
This proves the cases (every input condition is asserted by the helper) and the host reference without a GPU, before
tests/test_hip_huffman_cases.py compares the device library with them."""
import numpy as np
import pytest

import huffman_cases as H
from quantized_distillation_amd import _lib


def test_the_case_table_is_the_documented_one():
    assert H.CASE_IDS == ['deep', 'full_chunk', 'lut_edge_10', 'lut_edge_11', 'short', 'fixed8', 'fixed6', 'single', 'buckets',
                          'points', 'many', 'scan']
    for case in H.CASES.values():
        H.check_conditions(case, H.symbols(case))


@pytest.mark.parametrize('cid', H.CASE_IDS)
def test_host_codec_case(cid):
    case = H.CASES[cid]
    syms = H.symbols(case)
    res = H.run_case(case, _lib.host(), 'cpu')
    bits = H.chunk_bits(case, syms)
    want_cw = H.expected_chunk_words(case, syms)
    assert np.array_equal(np.diff(res.chunk_words.astype(np.int64)), [-(-b // 32) for b in bits])
    assert np.array_equal(res.chunk_words, want_cw) and res.chunk_words[0] == 0
    assert int(res.chunk_words[-1]) == sum(-(-b // 32) for b in bits) == len(res.words)
    if case.single >= 0:
        assert not res.chunk_words.any() and len(res.words) == 0
    assert H.same_bits(res.decoded, H.expected(case, syms))
