"""The cases of tests/huffman_cases.py through libqd_hip.so and libqd_host.so at the C ABI: the branches of
csrc/qd_huffman.hip that Gaussian weights never reach.  Device and host write the same chunk_words and
the same words, and every decode -- device of device, device of host, host of device -- equals the float32 formula of
include/qd_hip.h written out in numpy, bit for bit.  Only well-formed streams go to the device: the host stream is compared
with the word counts that follow from the code lengths before the device reads it."""
import numpy as np
import pytest
import torch

import huffman_cases as H
from quantized_distillation_amd import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.mark.parametrize('cid', H.CASE_IDS)
def test_device_codec_case(cid):
    case = H.CASES[cid]
    syms = H.symbols(case)
    want = H.expected(case, syms)
    want_cw = H.expected_chunk_words(case, syms)
    host = H.run_case(case, _lib.host(), 'cpu')
    assert np.array_equal(host.chunk_words, want_cw) and H.same_bits(host.decoded, want)
    with torch.cuda.device(DEV):
        dev = H.run_case(case, _lib.load(), DEV)
        assert np.array_equal(dev.chunk_words, want_cw)
        assert dev.chunk_words.tobytes() == host.chunk_words.tobytes() and dev.words.tobytes() == host.words.tobytes()
        assert H.same_bits(dev.decoded, want), 'device decode of the device stream'
        dev_of_host = H.run_case(case, _lib.load(), DEV, stream=(host.chunk_words, host.words))
        assert H.same_bits(dev_of_host.decoded, want), 'device decode of the host stream'
    host_of_dev = H.run_case(case, _lib.host(), 'cpu', stream=(dev.chunk_words, dev.words))
    assert H.same_bits(host_of_dev.decoded, want), 'host decode of the device stream'
    if case.single >= 0:
        assert not dev.chunk_words.any() and len(dev.words) == 0
