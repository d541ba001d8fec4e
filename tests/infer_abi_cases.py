"""The two checks every inference library's ABI test makes (test_infer_abi.py, test_infer_mm_abi.py, test_infer_conv_abi.py,
test_infer_rnn_abi.py), once: header, binding and exports agree; no kernel uses scratch or spills.  Each test file calls them
with its own library's expectations."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols(header, prefix):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(%s_[a-z0-9_]+)\s*\(' % prefix, text)))


def check_header_binding_and_exports_agree(lib, binding, header, prefix, count):
    """lib: the loaded library; binding: its module.  The header's symbols are the binding's table and the library's exports --
    and the library exports nothing else named qd_ or qd?_, so no entry point of another library's header -- at one ABI
    version; the library says what it is built for and describes its error codes; it holds gfx950 code only."""
    syms = header_symbols(header, prefix)
    assert syms == sorted(binding.SIGNATURES) and len(syms) == count
    out = subprocess.check_output(['nm', '-D', '--defined-only', binding.LIB_PATH], text=True)
    assert sorted(set(re.findall(r' T (qd[a-z]?_[a-z0-9_]+)', out))) == syms
    define = re.search(r'#define %s_ABI_VERSION (\d+)' % prefix.upper(), open(os.path.join(ROOT, 'include', header)).read())
    assert int(define.group(1)) == binding.ABI_VERSION == getattr(lib, prefix + '_abi_version')() == 1
    assert getattr(lib, prefix + '_target_arch')() == b'gfx950'
    error_string = getattr(lib, prefix + '_error_string')
    assert error_string(0) == b'success' and b'invalid' in error_string(-1)
    blob = open(binding.LIB_PATH, 'rb').read()
    assert set(re.findall(rb'hipv4-amdgcn-amd-amdhsa--(gfx[0-9a-z]+)', blob)) == {b'gfx950'}


def check_no_kernel_uses_scratch_or_spills(binding, kernel_names, lds_limit=None, vgpr_limit=None):
    """The library's kernels are exactly kernel_names (substrings of the demangled names, one kernel each); none has a private
    segment, a spill or a dynamic stack; each stays within lds_limit bytes of LDS / vgpr_limit VGPRs where one is given."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    ks = kernel_meta.kernels(binding.LIB_PATH)
    names = ' '.join(kernel_meta.demangle([k['name'] for k in ks]).values())
    assert len(ks) == len(kernel_names) and all(n in names for n in kernel_names), names
    for k in ks:
        assert (k.get('private_segment_fixed_size', 0), k.get('vgpr_spill_count', 0), k.get('sgpr_spill_count', 0)) == (0, 0, 0), k
        assert k.get('uses_dynamic_stack') != 'true', k
        assert lds_limit is None or k['group_segment_fixed_size'] <= lds_limit, k
        assert vgpr_limit is None or k['vgpr_count'] <= vgpr_limit, k
