"""ctypes binding of libqd_infer_attn.so (C ABI: include/qd_infer_attn.h): one Luong global-attention step -- scores, masked
softmax and context in one launch, tanh(W_out [ctx ; x] + bias) from the packed weight on fp32 matrix instructions in another,
the concatenation never made.

A library of its own next to libqd_infer.so, libqd_infer_mm.so, libqd_infer_conv.so, libqd_infer_rnn.so and libqd_infer_gru.so,
with its own signature table.  Loaded on first use only (the first PackedGlobalAttention forward); loading fails loudly when the
library has not been built -- there is no fallback implementation.
"""
import ctypes
import os

from ._lib import binding, c_int, c_p, i64

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libqd_infer_attn.so')

ABI_VERSION = 1                # QDA_ABI_VERSION of include/qd_infer_attn.h (tests/test_infer_attn_abi.py compares the two)
QDA_ERR_INVALID_ARGUMENT = -1
CONTEXT_LDS_LIMIT = 163840     # QDA_CONTEXT_LDS_LIMIT

# symbol -> (restype, argtypes); every symbol declared in include/qd_infer_attn.h (tests/test_infer_attn_abi.py cross-checks)
SIGNATURES = {
    'qda_abi_version': (c_int, []),
    'qda_target_arch': (ctypes.c_char_p, []),
    'qda_error_string': (ctypes.c_char_p, [c_int]),
    'qda_set_grid_cap': (c_int, [c_int]),                  # test hook: blocks per launch; returns the previous cap, 0 = none
    # q, keys, values, lengths, batch, S, dim, align, ctx, stream
    'qda_attn_context_f32': (c_int, [c_p, c_p, c_p, c_p, i64, i64, i64, c_p, c_p, c_p]),
    # packed, alpha, beta, bucket, levels, bits, dim, ctx, x, batch, bias, attn_h, pre, stream
    'qda_attn_out_packed_f32': (c_int, [c_p, c_p, c_p, i64, c_int, c_int, i64, c_p, c_p, i64, c_p, c_p, c_p, c_p]),
}

_lib = None                    # the loaded library, set by load()
load, check = binding(__name__, 'qda', 'There is no fallback.')
