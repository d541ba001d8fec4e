"""tests/out16_cases.py proven without a GPU: every exact case really quantizes to {0, v} through uniformQuantization on CPU
tensors (libqd_host.so), at every bucket size and level count the device tests use, deterministic and stochastic, and the
conversion of that result with .to(dtype) shows the 16-bit pattern the table intends.  The argument checks of
MultiTensorQuantizer's out_dtype that need no device are here too."""
import numpy as np
import pytest
import torch

import out16_cases as C
import quantization
from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer

DTYPES = {'float16': torch.float16, 'bfloat16': torch.bfloat16}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize('bucket', C.BUCKETS)
def test_every_exact_case_puts_its_value_and_its_pattern_on_the_output(bucket):
    for name, v, want in C.EXACT:
        x = C.tensor_of(v)
        for s in C.LEVELS:
            for stoch in (False, True):
                q = quantization.uniformQuantization(torch.from_numpy(x.copy()), s, bucket_size=bucket, stochastic_rounding=stoch)[0]
                q = q.reshape(-1)
                assert np.array_equal(bits(q.numpy()), bits(x)), (name, bucket, s, stoch, 'the case does not quantize to {0, v}')
                for fmt, pattern in want.items():
                    p16 = C.patterns(q.to(DTYPES[fmt]))
                    assert (p16[0::2] == 0).all(), (name, fmt, 'the zeros are +0')
                    if pattern is not None:
                        assert (p16[1::2] == pattern).all(), (name, fmt, bucket, s, '0x%04X, intended 0x%04X' % (p16[1], pattern))


def test_the_table_holds_what_the_issue_lists():
    by_name = {name: (v, want) for name, v, want in C.EXACT}
    assert by_name['bf16 tie down'][0] == np.float32(1 + 2.0 ** -8) and by_name['bf16 tie up'][0] == np.float32(1 + 3 * 2.0 ** -8)
    assert by_name['fp16 tie down'][0] == np.float32(1 + 2.0 ** -11) and by_name['fp16 tie up'][0] == np.float32(1 + 3 * 2.0 ** -11)
    assert bits(by_name['bf16 first to inf'][0]) == 0x7F7FFFFF
    assert by_name['fp16 largest finite'][0] == 65504 and by_name['fp16 first to inf'][0] == 65520
    assert by_name['negative fp16 subnormal tie to zero'][1]['float16'] == 0x8000       # the sign of zero is kept
    # the intended patterns are the values they are meant to be
    as16 = lambda p, dt: torch.from_numpy(np.array([p], np.uint16).view(np.int16)).view(dt).float().item()
    assert as16(by_name['fp16 largest finite'][1]['float16'], torch.float16) == 65504.0
    assert as16(by_name['fp16 first to inf'][1]['float16'], torch.float16) == float('inf')
    assert as16(by_name['bf16 first to inf'][1]['bfloat16'], torch.bfloat16) == float('inf')
    assert as16(by_name['fp16 smallest subnormal'][1]['float16'], torch.float16) == 2.0 ** -24
    assert as16(by_name['bf16 tie up'][1]['bfloat16'], torch.bfloat16) == 1 + 2.0 ** -6
    assert as16(by_name['fp16 tie up'][1]['float16'], torch.float16) == 1 + 2.0 ** -9
    assert as16(by_name['negative bf16 largest finite'][1]['bfloat16'], torch.bfloat16) == -float(np.array([0x7F7F0000], np.uint32).view(np.float32)[0])


@pytest.mark.parametrize('bucket', [256, None])
def test_the_non_finite_cases_give_nan_where_the_bucket_holds_one(bucket):
    for name, x in C.nonfinite():
        q = quantization.uniformQuantization(torch.from_numpy(x.copy()), 16, bucket_size=bucket)[0].reshape(-1)
        nan = torch.isnan(q).numpy()
        if bucket is None:
            assert nan.all(), name
        else:
            assert nan[256:512].all() and not nan[:256].any() and not nan[512:].any(), name
        for dt in DTYPES.values():
            assert np.array_equal(torch.isnan(q.to(dt)).numpy(), nan)


def test_assert_same16_compares_patterns_and_takes_nan_for_nan():
    a = torch.tensor([1.0, -0.0, float('nan'), float('inf')]).to(torch.float16)
    C.assert_same16(a.clone(), a, 'equal')
    b = a.clone()
    b[1] = 0.0                              # +0 against -0: equal as numbers, not as patterns
    with pytest.raises(AssertionError):
        C.assert_same16(b, a, 'sign of zero')
    c = a.clone()
    c[0] = float('nan')
    with pytest.raises(AssertionError):
        C.assert_same16(c, a, 'a NaN too many')


def test_out_dtype_arguments_are_checked_before_any_device_is_needed():
    """The dtype rules of MultiTensorQuantizer come before the device check of the tensors: they can be held here."""
    x = [torch.zeros(8), torch.zeros(8)]
    with pytest.raises(TypeError, match='one dtype'):
        MultiTensorQuantizer(x, 16, 256, outputs=[torch.zeros(8, dtype=torch.float16), torch.zeros(8, dtype=torch.bfloat16)])
    with pytest.raises(TypeError, match='float32, float16 or bfloat16'):
        MultiTensorQuantizer(x, 16, 256, outputs=[torch.zeros(8, dtype=torch.float64)] * 2)
    with pytest.raises(TypeError, match='out_dtype is torch.bfloat16'):
        MultiTensorQuantizer(x, 16, 256, outputs=[torch.zeros(8)] * 2, out_dtype=torch.bfloat16)
    with pytest.raises(TypeError, match='out_dtype must be'):
        MultiTensorQuantizer(x, 16, 256, out_dtype=torch.float64)
    with pytest.raises(TypeError, match='out_dtype must be'):
        MultiTensorQuantizer(x, 16, 256, out_dtype=torch.int8)
