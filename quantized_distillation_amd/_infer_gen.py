"""ctypes binding of libqd_infer_gen.so (C ABI: include/qd_infer_gen.h): the end of a decoder step -- the vocabulary projection
from the packed generator weight on fp32 matrix instructions, reduced in registers to (max, sum of exp, top-k) per panel of 64
words, and a second launch that combines the panels into lse, the top k and, where asked for, the log-probs.

A library of its own next to libqd_infer.so, libqd_infer_mm.so, libqd_infer_conv.so, libqd_infer_rnn.so, libqd_infer_gru.so and
libqd_infer_attn.so, with its own signature table.  Loaded on first use only (the first PackedGenerator forward); loading fails
loudly when the library has not been built -- there is no fallback implementation.
"""
import ctypes
import os

from ._lib import binding, c_int, c_p, i64

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libqd_infer_gen.so')

ABI_VERSION = 1                # QDN_ABI_VERSION of include/qd_infer_gen.h (tests/test_infer_gen_abi.py compares the two)
QDN_ERR_INVALID_ARGUMENT = -1
PANEL = 64                     # QDN_PANEL
MAX_TOPK = 16                  # QDN_MAX_TOPK

# symbol -> (restype, argtypes); every symbol declared in include/qd_infer_gen.h (tests/test_infer_gen_abi.py cross-checks)
SIGNATURES = {
    'qdn_abi_version': (c_int, []),
    'qdn_target_arch': (ctypes.c_char_p, []),
    'qdn_error_string': (ctypes.c_char_p, [c_int]),
    'qdn_set_grid_cap': (c_int, [c_int]),                  # test hook: blocks per launch; returns the previous cap, 0 = none
    'qdn_generator_work_bytes': (i64, [i64, i64, c_int]),  # V, m, k
    # packed, alpha, beta, V, dim, bucket, levels, bits, x, m, bias, lse, logp, k, top_val, top_idx, work, stream
    'qdn_generator_packed_f32': (c_int, [c_p, c_p, c_p, i64, i64, i64, c_int, c_int, c_p, i64, c_p, c_p, c_p, c_int, c_p, c_p, c_p, c_p]),
}

_lib = None                    # the loaded library, set by load()
load, check = binding(__name__, 'qdn', 'There is no fallback.')
