"""ctypes binding of libqd_loss.so (C ABI: include/qd_loss.h): the distillation loss of a training step -- KL(teacher || student) at
a temperature plus the cross entropy with the labels -- and its gradient with respect to the student's logits, in one pass over the
logits (k_kd_rows) and a one-block sum over the rows (k_kd_finish).

A library of its own next to libqd_hip.so and the inference libraries, with its own signature table.  Loaded on first use only (the
first fused_kd_loss / fused_word_kd_loss call); loading fails loudly when the library has not been built -- there is no fallback
implementation.
"""
import ctypes
import os

from ._lib import binding, c_int, c_p, i64

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, 'csrc', 'loss')
LIB_PATH = os.path.join(_HERE, 'libqd_loss.so')

ABI_VERSION = 1                # QDL_ABI_VERSION of include/qd_loss.h (tests/test_loss_abi.py compares the two)
QDL_ERR_INVALID_ARGUMENT = -1

c_float = ctypes.c_float

# symbol -> (restype, argtypes); every symbol declared in include/qd_loss.h (tests/test_loss_abi.py cross-checks)
SIGNATURES = {
    'qdl_abi_version': (c_int, []),
    'qdl_target_arch': (ctypes.c_char_p, []),
    'qdl_error_string': (ctypes.c_char_p, [c_int]),
    'qdl_set_grid_cap': (c_int, [c_int]),                  # test hook: blocks per launch; returns the previous cap, 0 = none
    'qdl_wave_cols': (i64, []),                            # QDL_WAVE_COLS: the longest row one wave keeps in registers
    'qdl_lds_cols': (i64, []),                             # QDL_LDS_COLS: the longest row a workgroup keeps in LDS
    # student, teacher, target, rows, cols, temperature, kl_scale, nll_scale, ignore_index, grad, row_kl, row_nll, loss, stream
    'qdl_kd_loss_f32': (c_int, [c_p, c_p, c_p, i64, i64, c_float, c_float, c_float, i64, c_p, c_p, c_p, c_p, c_p]),
}

_lib = None                    # the loaded library, set by load()
load, check = binding(__name__, 'qdl', 'There is no fallback.')
