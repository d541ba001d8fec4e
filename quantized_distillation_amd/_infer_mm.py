"""ctypes binding of libqd_infer_mm.so (C ABI: include/qd_infer_mm.h): the Linear layer from packed low-bit weights for many
rows of x, on fp32 matrix instructions.

A library of its own next to libqd_infer.so, with its own signature table: _infer.SIGNATURES is the table of
include/qd_infer.h and stays that.  Loaded on first use only (PackedLinear with batched_from set); loading fails loudly when
the library has not been built -- there is no fallback implementation.
"""
import ctypes
import os

from ._lib import binding, c_int, c_p, i64

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libqd_infer_mm.so')

ABI_VERSION = 1                # QDM_ABI_VERSION of include/qd_infer_mm.h (tests/test_infer_mm_abi.py compares the two)
QDM_ERR_INVALID_ARGUMENT = -1

# symbol -> (restype, argtypes); every symbol declared in include/qd_infer_mm.h (tests/test_infer_mm_abi.py cross-checks)
SIGNATURES = {
    'qdm_abi_version': (c_int, []),
    'qdm_target_arch': (ctypes.c_char_p, []),
    'qdm_error_string': (ctypes.c_char_p, [c_int]),
    'qdm_set_grid_cap': (c_int, [c_int]),                  # test hook: blocks per launch; returns the previous cap, 0 = none
    'qdm_linear_packed_f32': (c_int, [c_p, c_p, c_p, i64, i64, i64, c_int, c_int, c_p, i64, c_p, c_p, c_p]),
}

_lib = None                    # the loaded library, set by load()
load, check = binding(__name__, 'qdm', 'There is no fallback: PackedLinear with batched_from=None does not need it.')
