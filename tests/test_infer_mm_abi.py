"""libqd_infer_mm.so (include/qd_infer_mm.h: the batched Linear layer from packed weights on fp32 MFMA) builds for gfx950
without a GPU, exports exactly the header's symbols, keeps its kernel free of scratch and spills and refuses bad arguments
before it touches a device; PackedLinear validates batched_from before any launch."""
import pytest
import torch
from torch import nn

import infer_abi_cases as A
from quantized_distillation_amd import _infer_mm, codec, packed_layers
from quantized_distillation_amd import build as qb

@pytest.fixture(scope='module')
def lib():
    qb.build_infer_mm()
    return _infer_mm.load()


def test_header_binding_and_exports_agree(lib):
    A.check_header_binding_and_exports_agree(lib, _infer_mm, 'qd_infer_mm.h', 'qdm', 5)                 # and no symbol of another library's header
    assert not set(qb.INFER_MM_SOURCES) & (set(qb.SOURCES) | set(qb.INFER_SOURCES))


def test_the_kernel_uses_no_scratch_and_spills_nothing(lib):
    A.check_no_kernel_uses_scratch_or_spills(_infer_mm, ['k_linear_mm'], lds_limit=64 * 1024)


def test_refusals_and_empty_calls_without_a_device(lib):
    """Every refusal of the header (those of qd_infer.h), with pointers that are never dereferenced: -1 without a launch."""
    assert lib.qdm_set_grid_cap(3) == 0 and lib.qdm_set_grid_cap(0) == 3 and lib.qdm_set_grid_cap(-5) == 0
    P = 4096                                                               # a well-aligned non-NULL address, never read

    def lin(packed=P, alpha=P, beta=P, rows=10, cols=8, bucket=4, levels=16, bits=4, x=P, m=70, bias=P, y=P):
        return lib.qdm_linear_packed_f32(packed, alpha, beta, rows, cols, bucket, levels, bits, x, m, bias, y, None)

    for kw in (dict(levels=1), dict(levels=257, bits=8), dict(bits=0), dict(bits=9, levels=2), dict(levels=17, bits=4),
               dict(levels=9, bits=3), dict(levels=3, bits=1), dict(bucket=-1), dict(rows=-1), dict(cols=-1),
               dict(packed=None), dict(alpha=None), dict(beta=None), dict(packed=P + 2), dict(alpha=P + 1), dict(beta=P + 2),
               dict(rows=2 ** 40, cols=2 ** 40), dict(m=-1), dict(x=None), dict(y=None), dict(x=P + 1), dict(y=P + 2), dict(bias=P + 3),
               dict(m=2 ** 62), dict(m=2 ** 61, rows=1)):
        assert lin(**kw) == -1, kw
    assert lin(m=0, x=None, y=None) == 0 and lin(rows=0, packed=None, y=None, bias=None) == 0


def test_batched_from_is_validated_before_any_launch():
    n, nb = 6 * 8, 3
    pk = codec.PackedUniform(torch.zeros(n // 2, dtype=torch.uint8), torch.ones(nb), torch.zeros(nb), (6, 8), 16, 16, 4)
    PL = packed_layers.PackedLinear
    assert PL(pk).batched_from is None and PL(pk, None, batched_from=1).batched_from == 1 and PL(pk, batched_from=16).batched_from == 16
    for bad in (0, -1, 2.0, '16', True):
        with pytest.raises(ValueError, match='batched_from'):
            PL(pk, batched_from=bad)
        with pytest.raises(ValueError, match='batched_from'):
            PL.from_linear(nn.Linear(8, 6), 16, batched_from=bad)          # before the device check and before packing
        model = nn.Sequential(nn.Linear(8, 6))
        with pytest.raises(ValueError, match='batched_from'):
            packed_layers.pack_modules(model, 16, batched_from=bad)
        assert isinstance(model[0], nn.Linear)
    assert 'batched_from=16' in repr(PL(pk, batched_from=16))
