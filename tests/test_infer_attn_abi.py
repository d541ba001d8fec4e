"""libqd_infer_attn.so (include/qd_infer_attn.h: a global-attention step, its output projection from packed weights) builds for gfx950
without a GPU, exports exactly the header's symbols, keeps its kernels free of scratch and spills and refuses bad arguments before it
touches a device; PackedGlobalAttention validates before any launch."""
import pytest
import torch
from torch import nn

import infer_abi_cases as A
from quantized_distillation_amd import _infer_attn, codec, packed_layers
from quantized_distillation_amd import build as qb


@pytest.fixture(scope='module')
def lib():
    qb.build_infer_attn()
    return _infer_attn.load()


def test_header_binding_and_exports_agree(lib):
    A.check_header_binding_and_exports_agree(lib, _infer_attn, 'qd_infer_attn.h', 'qda', 6)                # and no symbol of another library's header
    others = set(qb.SOURCES).union(*(row[1] for row in qb.INFER_LIBRARIES if row[0] != 'libqd_infer_attn.so'))
    assert qb.INFER_ATTN_SOURCES == ['qda_attn.hip'] and not set(qb.INFER_ATTN_SOURCES) & others


def test_the_kernels_use_no_scratch_and_spill_nothing(lib):
    """Static LDS: k_attn_out_mm's slabs; k_attn_context's is all dynamic, held to the header's limit by the launcher (refusals below)."""
    A.check_no_kernel_uses_scratch_or_spills(_infer_attn, ['k_attn_context', 'k_attn_out_mm'], lds_limit=_infer_attn.CONTEXT_LDS_LIMIT)


def test_refusals_and_empty_calls_without_a_device(lib):
    """Every refusal of the header, with pointers that are never dereferenced: -1 without a launch."""
    assert lib.qda_set_grid_cap(3) == 0 and lib.qda_set_grid_cap(0) == 3 and lib.qda_set_grid_cap(-5) == 0
    P = 4096                                                               # a well-aligned non-NULL address, never read

    def call(fn, base, **kw):
        args = dict(base, **kw)
        return fn(*[args[k] for k in base], None)

    cx = dict(q=P, keys=2 * P, values=2 * P, lengths=3 * P, batch=3, S=9, dim=7, align=4 * P, ctx=5 * P)
    bad = [dict(batch=-1), dict(S=-1), dict(dim=-1), dict(batch=2 ** 40, S=2 ** 15, dim=2 ** 15), dict(batch=2 ** 50, dim=2 ** 14),
           dict(S=40941), dict(dim=40941), dict(S=20480, dim=20480),      # 4 (16 + dim + S) > 163840
           dict(align=P), dict(align=2 * P), dict(ctx=P), dict(ctx=2 * P), dict(ctx=4 * P), dict(values=6 * P, ctx=6 * P), dict(lengths=P + 4)]
    bad += [{k: None} for k in ('q', 'keys', 'values', 'align', 'ctx')] + [{k: P + 2} for k in ('q', 'keys', 'values', 'align', 'ctx')]
    for kw in bad:
        assert call(lib.qda_attn_context_f32, cx, **kw) == -1, kw
    for kw in (dict(batch=0), dict(S=0), dict(dim=0)):
        assert call(lib.qda_attn_context_f32, cx, q=None, keys=None, values=None, lengths=None, align=None, ctx=None, **kw) == 0, kw

    out = dict(packed=P, alpha=P, beta=P, bucket=4, levels=16, bits=4, dim=5, ctx=2 * P, x=3 * P, batch=3, bias=4 * P, attn_h=5 * P, pre=6 * P)
    bad = [dict(dim=-1), dict(batch=-1), dict(dim=2 ** 62), dict(dim=2 ** 32), dict(dim=2 ** 20, batch=2 ** 50),
           dict(levels=1), dict(levels=257, bits=8), dict(bits=0), dict(bits=9, levels=2), dict(levels=17), dict(levels=3, bits=1), dict(bucket=-1),
           dict(attn_h=2 * P), dict(attn_h=3 * P), dict(attn_h=4 * P), dict(attn_h=6 * P), dict(pre=2 * P), dict(pre=3 * P), dict(pre=4 * P)]
    bad += [{k: None} for k in ('packed', 'alpha', 'beta', 'ctx', 'x', 'attn_h')]
    bad += [{k: P + 2} for k in ('packed', 'alpha', 'beta', 'ctx', 'x', 'bias', 'attn_h', 'pre')]
    for kw in bad:
        assert call(lib.qda_attn_out_packed_f32, out, **kw) == -1, kw
    empty = dict(packed=None, alpha=None, beta=None, ctx=None, x=None, attn_h=None, pre=None, bias=None)
    assert call(lib.qda_attn_out_packed_f32, out, batch=0, **empty) == 0 and call(lib.qda_attn_out_packed_f32, out, dim=0, **empty) == 0


def _packed(rows, cols):
    n = rows * cols
    return codec.PackedUniform(torch.zeros(n // 2, dtype=torch.uint8), torch.ones(n // 16), torch.zeros(n // 16), (rows, cols), 16, 16, 4)


def test_the_module_is_validated_before_any_launch():
    PGA = packed_layers.PackedGlobalAttention
    att = PGA(_packed(8, 16), _packed(8, 8), torch.zeros(8))
    assert att.dim == 8 and att.fp32_nbytes == 4 * (128 + 8 + 64) and att.nbytes == (64 + 8 * 8 + 32) + (32 + 4 * 8)
    assert 'general' in att.extra_repr() and 'dot' in PGA(_packed(8, 16)).extra_repr()
    for args in ((_packed(8, 24),), (_packed(8, 8),), (_packed(8, 16), _packed(8, 16)), (_packed(8, 16), _packed(4, 8)),
                 (_packed(8, 16), None, torch.zeros(16))):
        with pytest.raises(ValueError):
            PGA(*args)                                                     # [dim, 3 dim]: not [ctx ; x]'s weight
    with pytest.raises(TypeError):
        PGA(nn.Linear(16, 8))
    z = torch.zeros
    i64 = z(3, dtype=torch.int64)
    packed_seq = nn.utils.rnn.pack_padded_sequence(z(5, 3, 8), [5, 3, 1])
    for query, memory, lengths, keys, err in (
            (z(3, 7), z(3, 5, 8), None, None, ValueError), (z(3, 2, 8), z(3, 5, 8), None, None, ValueError), (z(3, 8), z(2, 5, 8), None, None, ValueError),
            (z(3, 8), z(3, 5, 7), None, None, ValueError), (z(3, 8), z(3, 5, 8), None, z(3, 4, 8), ValueError), (z(3, 8), z(3, 5, 8), z(2, dtype=torch.int64), None, ValueError),
            (z(3, 8), z(3, 5, 8), z(3, dtype=torch.int32), None, TypeError), (z(3, 8), z(3, 5, 8), [5, 3, 1], None, TypeError),
            (z(3, 8, dtype=torch.float64), z(3, 5, 8), None, None, TypeError), (z(3, 8), z(3, 5, 8).double(), None, None, TypeError),
            (z(3, 8), packed_seq, None, None, TypeError), ([1.0], z(3, 5, 8), None, None, TypeError),
            (z(3, 8), z(3, 5, 8), i64, z(3, 5, 8), NotImplementedError)):
        with pytest.raises(err):
            att(query, memory, lengths, keys)                              # the last one: CPU tensors, there is no CPU path
    for args, err in (((nn.Linear(16, 8).weight, None, 16), TypeError), ((nn.Linear(16, 8), nn.Linear(8, 8), 16), ValueError),
                      ((nn.Linear(16, 8), None), TypeError), ((nn.Linear(16, 8), None, 257), ValueError), ((nn.Linear(16, 8), None, 16), NotImplementedError)):
        with pytest.raises(err):
            PGA.from_linears(*args)                                        # a biased linear_in; no s; too many levels; CPU weights have no packed form
