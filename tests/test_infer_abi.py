"""libqd_infer.so (include/qd_infer.h: Linear and Embedding from packed weights) builds for gfx950 without a GPU, loads, exports
exactly the header's symbols, keeps every kernel free of scratch and spills, and refuses bad arguments before it touches a
device; the Python layer (quantized_distillation_amd/packed_layers.py) refuses what it must before any launch.  The training
library's header stays what it was: no qdi_ symbol in include/qd_hip.h, no entry of this library in _lib.SIGNATURES."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch
from torch import nn

from quantized_distillation_amd import _infer, _lib, codec, packed_layers
from quantized_distillation_amd import build as qb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'qd_infer.h')


@pytest.fixture(scope='module')
def lib():
    qb.build_infer()
    return _infer.load()


def header_symbols():
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(qdi_[a-z0-9_]+)\s*\(', text)))


def test_header_binding_and_exports_agree(lib):
    syms = header_symbols()
    assert syms == sorted(_infer.SIGNATURES) and len(syms) == 6
    out = subprocess.check_output(['nm', '-D', '--defined-only', _infer.LIB_PATH], text=True)
    assert sorted(set(re.findall(r' T (qdi?_[a-z0-9_]+)', out))) == syms          # and nothing named qd_: no entry point of qd_hip.h
    assert int(re.search(r'#define QDI_ABI_VERSION (\d+)', open(HEADER).read()).group(1)) == _infer.ABI_VERSION == lib.qdi_abi_version() == 1
    assert lib.qdi_target_arch() == b'gfx950'
    assert lib.qdi_error_string(0) == b'success' and b'invalid' in lib.qdi_error_string(-1)


def test_the_training_library_is_untouched():
    assert 'qdi_' not in open(os.path.join(ROOT, 'include', 'qd_hip.h')).read()
    assert not [s for s in _lib.SIGNATURES if s.startswith('qdi_')]
    assert not [f for f in qb.SOURCES if 'qdi' in f or 'infer' in f]
    assert os.path.dirname(_infer.LIB_PATH) == os.path.dirname(_lib.LIB_PATH) and _infer.LIB_PATH != _lib.LIB_PATH


def test_one_device_target(lib):
    blob = open(_infer.LIB_PATH, 'rb').read()
    assert set(re.findall(rb'hipv4-amdgcn-amd-amdhsa--(gfx[0-9a-z]+)', blob)) == {b'gfx950'}


def test_no_kernel_uses_scratch_or_spills(lib):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    ks = kernel_meta.kernels(_infer.LIB_PATH)
    names = ' '.join(kernel_meta.demangle([k['name'] for k in ks]).values())
    assert len(ks) == 5 and 'k_embedding' in names and all('k_linear<%d>' % mt in names for mt in (1, 2, 4, 8)), names
    bad = [(k['name'], k.get('private_segment_fixed_size', 0), k.get('vgpr_spill_count', 0), k.get('sgpr_spill_count', 0)) for k in ks
           if k.get('private_segment_fixed_size', 0) != 0 or k.get('vgpr_spill_count', 0) != 0 or k.get('sgpr_spill_count', 0) != 0
           or k.get('uses_dynamic_stack') == 'true']
    assert not bad, bad
    assert all(k['vgpr_count'] <= 128 for k in ks), [(k['name'], k['vgpr_count']) for k in ks]


def test_grid_cap_hook(lib):
    assert lib.qdi_set_grid_cap(3) == 0 and lib.qdi_set_grid_cap(1) == 3 and lib.qdi_set_grid_cap(0) == 1 and lib.qdi_set_grid_cap(-5) == 0
    assert lib.qdi_set_grid_cap(0) == 0


def test_entry_points_check_their_arguments_before_touching_the_device(lib):
    """Every refusal of the header, with pointers that are never dereferenced: -1 without a launch (there is no device here)."""
    for name in ('qdi_embedding_packed_f32', 'qdi_linear_packed_f32'):
        res, args = _infer.SIGNATURES[name]
        assert res is ctypes.c_int
        vals = [100 if a is ctypes.c_int64 else 0 if a is ctypes.c_int else None for a in args]
        assert getattr(lib, name)(*vals) == -1, name                       # NULL pointers, non-zero sizes, zero levels and bits
    P = 4096                                                               # a well-aligned non-NULL address, never read

    def emb(packed=P, alpha=P, beta=P, rows=10, cols=8, bucket=4, levels=16, bits=4, idx=P, count=3, out=P):
        return lib.qdi_embedding_packed_f32(packed, alpha, beta, rows, cols, bucket, levels, bits, idx, count, out, None)

    def lin(packed=P, alpha=P, beta=P, rows=10, cols=8, bucket=4, levels=16, bits=4, x=P, m=3, bias=P, y=P):
        return lib.qdi_linear_packed_f32(packed, alpha, beta, rows, cols, bucket, levels, bits, x, m, bias, y, None)

    for f in (emb, lin):
        for kw in (dict(levels=1), dict(levels=257, bits=8), dict(bits=0), dict(bits=9, levels=2), dict(levels=17, bits=4),
                   dict(levels=9, bits=3), dict(levels=3, bits=1), dict(bucket=-1), dict(rows=-1), dict(cols=-1),
                   dict(packed=None), dict(alpha=None), dict(beta=None), dict(packed=P + 2), dict(alpha=P + 1), dict(beta=P + 2),
                   dict(rows=2 ** 40, cols=2 ** 40)):
            assert f(**kw) == -1, (f.__name__, kw)
    for kw in (dict(count=-1), dict(idx=None), dict(out=None), dict(idx=P + 4), dict(out=P + 2)):
        assert emb(**kw) == -1, kw
    for kw in (dict(m=-1), dict(x=None), dict(y=None), dict(x=P + 1), dict(y=P + 2), dict(bias=P + 3)):
        assert lin(**kw) == -1, kw
    # empty calls: 0 without a launch, whatever the pointers
    assert emb(count=0, idx=None, out=None) == 0 and emb(cols=0, packed=None, out=None) == 0
    assert lin(m=0, x=None, y=None) == 0 and lin(rows=0, packed=None, y=None, bias=None) == 0


def test_library_missing_is_an_error_of_its_own(monkeypatch, tmp_path):
    monkeypatch.setattr(_infer, '_lib', None)
    monkeypatch.setattr(_infer, 'LIB_PATH', str(tmp_path / 'libqd_infer.so'))
    with pytest.raises(_lib.QdLibraryMissing, match='libqd_infer.so is missing'):
        _infer.load()


# ---------------------------------------------------------------- the Python layer, before any launch
def _packed(rows=6, cols=8, s=16, bits=4, bucket=16, shape=None):
    """A PackedUniform made by hand on the CPU (pack_uniform itself is device only)."""
    n = rows * cols
    nb = 1 if (bucket is None or n < bucket) else -(-n // bucket)
    return codec.PackedUniform(torch.zeros((n * bits + 7) // 8, dtype=torch.uint8), torch.ones(nb), torch.zeros(nb),
                               shape or (rows, cols), s, bucket, bits)


def test_cpu_tensors_are_refused_by_name():
    lin, emb = nn.Linear(8, 6), nn.Embedding(6, 8)
    with pytest.raises(NotImplementedError, match='HIP device only'):
        packed_layers.PackedLinear.from_linear(lin, 16)
    with pytest.raises(NotImplementedError, match='HIP device only'):
        packed_layers.PackedEmbedding.from_embedding(emb, 16)
    pl, pe = packed_layers.PackedLinear(_packed(), torch.zeros(6)), packed_layers.PackedEmbedding(_packed())
    with pytest.raises(NotImplementedError, match='HIP device only'):
        pl(torch.zeros(3, 8))
    with pytest.raises(NotImplementedError, match='HIP device only'):
        pe(torch.zeros(3, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match='HIP device only'):
        pl.unpack()
    with pytest.raises(NotImplementedError, match='HIP device only'):
        packed_layers.pack_modules(nn.Sequential(nn.Linear(8, 6)), 16)


def test_modules_hold_buffers_and_report_their_sizes():
    pl, pe = packed_layers.PackedLinear(_packed(), torch.zeros(6)), packed_layers.PackedEmbedding(_packed(bits=3, s=5, bucket=None))
    assert sorted(n for n, _ in pl.named_buffers()) == ['alpha', 'beta', 'bias', 'packed'] and not list(pl.parameters())
    assert sorted(n for n, _ in pe.named_buffers()) == ['alpha', 'beta', 'packed']
    assert pl.nbytes == 24 + 8 * 3 + 24 == _packed().nbytes + 24 and pl.fp32_nbytes == 4 * 48 + 24
    assert pe.nbytes == 18 + 8 and pe.fp32_nbytes == 4 * 48
    assert (pl.in_features, pl.out_features, pe.num_embeddings, pe.embedding_dim) == (8, 6, 6, 8)
    assert pl.to(torch.device('cpu')) is pl and 'bits=4' in repr(pl)


def test_argument_errors_before_any_launch():
    lin, emb = nn.Linear(8, 6), nn.Embedding(6, 8)
    PL, PE = packed_layers.PackedLinear, packed_layers.PackedEmbedding
    for bad_s in (1, 257, 2.5, 'x', None, True):
        with pytest.raises(ValueError):
            PL.from_linear(lin, bad_s)
        with pytest.raises(ValueError):
            PE.from_embedding(emb, bad_s)
    for s, bits in ((16, 3), (16, 0), (16, 9), (2, True), (4, 2.0), (4, '2')):
        with pytest.raises(ValueError, match='bits'):
            PL.from_linear(lin, s, bits=bits)
    for bucket in (0, -3, 2.0, True):
        with pytest.raises(ValueError, match='[Bb]ucket'):
            PE.from_embedding(emb, 16, bucket_size=bucket)
    with pytest.raises(TypeError):
        PL.from_linear(emb, 16)
    with pytest.raises(TypeError):
        PE.from_embedding(lin, 16)
    with pytest.raises(TypeError):
        PL.from_linear(nn.Linear(8, 6).double(), 16)
    with pytest.raises(ValueError, match='max_norm'):
        PE.from_embedding(nn.Embedding(6, 8, max_norm=1.0), 16)
    with pytest.raises(TypeError):
        PL(torch.zeros(6, 8))
    with pytest.raises(ValueError, match='2-D'):
        PL(_packed(shape=(48,)))                                           # a 1-D weight
    with pytest.raises(ValueError, match='bias'):
        PL(_packed(), torch.zeros(5))
    with pytest.raises(TypeError, match='bias'):
        PL(_packed(), torch.zeros(6, dtype=torch.float64))
    with pytest.raises(ValueError, match='packed must hold'):
        PL(codec.PackedUniform(torch.zeros(5, dtype=torch.uint8), torch.ones(3), torch.zeros(3), (6, 8), 16, 16, 4))
    with pytest.raises(ValueError, match='per bucket'):
        PL(codec.PackedUniform(torch.zeros(24, dtype=torch.uint8), torch.ones(2), torch.zeros(3), (6, 8), 16, 16, 4))
    pl, pe = PL(_packed(), None), PE(_packed())
    with pytest.raises(TypeError, match='float32'):
        pl(torch.zeros(3, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match='last dimension'):
        pl(torch.zeros(3, 7))
    with pytest.raises(ValueError, match='last dimension'):
        pl(torch.zeros(()))
    with pytest.raises(TypeError):
        pl([[0.0] * 8])
    with pytest.raises(TypeError, match='int64'):
        pe(torch.zeros(3, dtype=torch.int32))
    with pytest.raises(TypeError):
        pe([1, 2])


def test_pack_modules_checks_names_and_levels_before_it_changes_anything():
    model = nn.Sequential(nn.Embedding(6, 8), nn.Linear(8, 6))
    for kw, exc in ((dict(s=16, skip=('nope',)), ValueError), (dict(s={'0': 16}), ValueError), (dict(s={'0': 16, '1': 1}), ValueError),
                    (dict(s=16, bits=3), ValueError)):
        with pytest.raises(exc):
            packed_layers.pack_modules(model, **kw)
        assert isinstance(model[0], nn.Embedding) and isinstance(model[1], nn.Linear)
    assert packed_layers.pack_modules(model, 16, skip=('0', '1')) == {}
    with pytest.raises(ValueError, match='from_linear'):
        packed_layers.pack_modules(nn.Linear(8, 6), 16)
