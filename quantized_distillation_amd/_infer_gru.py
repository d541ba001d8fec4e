"""ctypes binding of libqd_infer_gru.so (C ABI: include/qd_infer_gru.h): one GRU step from packed low-bit recurrent weights,
both products on fp32 matrix instructions, kept as two sums, and the gate arithmetic in the same launch.

A library of its own next to libqd_infer.so, libqd_infer_mm.so, libqd_infer_conv.so and libqd_infer_rnn.so, with its own
signature table.  Loaded on first use only (the first PackedGRUCell / PackedGRU forward); loading fails loudly when the library
has not been built -- there is no fallback implementation.
"""
import ctypes
import os

from ._lib import binding, c_int, c_p, i64

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libqd_infer_gru.so')

ABI_VERSION = 1                # QDG_ABI_VERSION of include/qd_infer_gru.h (tests/test_infer_gru_abi.py compares the two)
QDG_ERR_INVALID_ARGUMENT = -1

_WEIGHT = [c_p, c_p, c_p, i64, c_int, c_int]           # packed, alpha, beta, bucket, levels, bits

# symbol -> (restype, argtypes); every symbol declared in include/qd_infer_gru.h (tests/test_infer_gru_abi.py cross-checks)
SIGNATURES = {
    'qdg_abi_version': (c_int, []),
    'qdg_target_arch': (ctypes.c_char_p, []),
    'qdg_error_string': (ctypes.c_char_p, [c_int]),
    'qdg_set_grid_cap': (c_int, [c_int]),                  # test hook: blocks per launch; returns the previous cap, 0 = none
    # W_ih, W_hh, hidden, input, x, pre, h, batch, bias_ih, bias_hh, h_out, gates, stream
    'qdg_gru_cell_packed_f32': (c_int, _WEIGHT + _WEIGHT + [i64, i64, c_p, c_p, c_p, i64, c_p, c_p, c_p, c_p, c_p]),
}

_lib = None                    # the loaded library, set by load()
load, check = binding(__name__, 'qdg', 'There is no fallback.')
