"""ctypes binding of libqd_infer.so (C ABI: include/qd_infer.h): Linear and Embedding from packed low-bit weights.

A library of its own next to libqd_hip.so, with its own signature table: _lib.SIGNATURES is the table of include/qd_hip.h
and stays that.  Loading fails loudly when the library has not been built -- there is no fallback implementation.
"""
import ctypes
import os
import threading

from ._lib import QdLibraryMissing, c_int, c_p, i64

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libqd_infer.so')
CSRC = os.path.join(_HERE, 'csrc', 'infer')

ABI_VERSION = 1                # QDI_ABI_VERSION of include/qd_infer.h (tests/test_infer_abi.py compares the two)
QDI_ERR_INVALID_ARGUMENT = -1

# symbol -> (restype, argtypes); every symbol declared in include/qd_infer.h (tests/test_infer_abi.py cross-checks)
SIGNATURES = {
    'qdi_abi_version': (c_int, []),
    'qdi_target_arch': (ctypes.c_char_p, []),
    'qdi_error_string': (ctypes.c_char_p, [c_int]),
    'qdi_set_grid_cap': (c_int, [c_int]),                  # test hook: blocks per launch; returns the previous cap, 0 = none
    'qdi_embedding_packed_f32': (c_int, [c_p, c_p, c_p, i64, i64, i64, c_int, c_int, c_p, i64, c_p, c_p]),
    'qdi_linear_packed_f32': (c_int, [c_p, c_p, c_p, i64, i64, i64, c_int, c_int, c_p, i64, c_p, c_p, c_p]),
}

_lib = None
_lock = threading.Lock()


def load():
    """Load libqd_infer.so (once).  Raises QdLibraryMissing if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise QdLibraryMissing(
                'quantized_distillation_amd: %s is missing. Build it first: '
                'python -c "import __graft_entry__ as g; g.build()" (needs hipcc, gfx950). '
                'There is no fallback: decode with PackedUniform.unpack() to run without it.' % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError = ABI mismatch: fail loudly
            fn.restype = res
            fn.argtypes = args
        if lib.qdi_abi_version() != ABI_VERSION:
            raise RuntimeError('libqd_infer.so has ABI version %d, this binding is written for %d: rebuild it '
                               '(python -c "import __graft_entry__ as g; g.build()")' % (lib.qdi_abi_version(), ABI_VERSION))
        _lib = lib
    return _lib


def check(code):
    """Raise for a non-zero return code of libqd_infer.so."""
    if code != 0:
        msg = load().qdi_error_string(code)
        raise RuntimeError('qd_infer: %s (code %d)' % (msg.decode() if msg else '?', code))
