"""ctypes binding of libqd_infer_conv.so (C ABI: include/qd_infer_conv.h): nn.Conv2d from packed low-bit weights, an implicit
GEMM on fp32 matrix instructions.

A library of its own next to libqd_infer.so and libqd_infer_conv.so, with its own signature table.  Loaded on first use only
(the first PackedConv2d.forward); loading fails loudly when the library has not been built -- there is no fallback
implementation.
"""
import ctypes
import os

from ._lib import binding, c_int, c_p, i64

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libqd_infer_conv.so')

ABI_VERSION = 1                # QDC_ABI_VERSION of include/qd_infer_conv.h (tests/test_infer_conv_abi.py compares the two)
QDC_ERR_INVALID_ARGUMENT = -1

# symbol -> (restype, argtypes); every symbol declared in include/qd_infer_conv.h (tests/test_infer_conv_abi.py cross-checks)
SIGNATURES = {
    'qdc_abi_version': (c_int, []),
    'qdc_target_arch': (ctypes.c_char_p, []),
    'qdc_error_string': (ctypes.c_char_p, [c_int]),
    'qdc_set_grid_cap': (c_int, [c_int]),                  # test hook: blocks per launch; returns the previous cap, 0 = none
    # packed, alpha, beta, cout, cin, kh, kw, bucket, levels, bits, x, batch, h, w, stride_h, stride_w, pad_h, pad_w, bias, y, stream
    'qdc_conv2d_packed_f32': (c_int, [c_p, c_p, c_p, i64, i64, c_int, c_int, i64, c_int, c_int, c_p, i64, i64, i64, c_int, c_int, c_int, c_int,
                                      c_p, c_p, c_p]),
}

_lib = None                    # the loaded library, set by load()
load, check = binding(__name__, 'qdc', 'There is no fallback.')
