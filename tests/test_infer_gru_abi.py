"""libqd_infer_gru.so (include/qd_infer_gru.h: a GRU step from packed weights, both products on fp32 MFMA as two sums, gates in the same
launch) builds for gfx950 without a GPU, exports exactly the header's symbols, keeps its kernel free of scratch and spills and
refuses bad arguments before it touches a device; PackedGRUCell, PackedGRU and pack_modules(rnn=True) validate before any launch."""
import pytest
import torch
from torch import nn

import infer_abi_cases as A
from quantized_distillation_amd import _infer_gru, codec, packed_layers
from quantized_distillation_amd import build as qb


@pytest.fixture(scope='module')
def lib():
    qb.build_infer_gru()
    return _infer_gru.load()


def test_header_binding_and_exports_agree(lib):
    A.check_header_binding_and_exports_agree(lib, _infer_gru, 'qd_infer_gru.h', 'qdg', 5)                 # and no symbol of another library's header
    others = set(qb.SOURCES) | set(qb.INFER_SOURCES) | set(qb.INFER_MM_SOURCES) | set(qb.INFER_CONV_SOURCES) | set(qb.INFER_RNN_SOURCES)
    assert not set(qb.INFER_GRU_SOURCES) & others


def test_the_kernel_uses_no_scratch_and_spills_nothing(lib):
    A.check_no_kernel_uses_scratch_or_spills(_infer_gru, ['k_gru_cell_mm'], lds_limit=64 * 1024)


def test_refusals_and_empty_calls_without_a_device(lib):
    """Every refusal of the header, with pointers that are never dereferenced: -1 without a launch."""
    assert lib.qdg_set_grid_cap(3) == 0 and lib.qdg_set_grid_cap(0) == 3 and lib.qdg_set_grid_cap(-5) == 0
    P = 4096                                                               # a well-aligned non-NULL address, never read
    ih = dict(packed_ih=P, alpha_ih=P, beta_ih=P, bucket_ih=4, levels_ih=16, bits_ih=4)
    hh = dict(packed_hh=P, alpha_hh=P, beta_hh=P, bucket_hh=4, levels_hh=16, bits_hh=4)
    rest = dict(hidden=5, input=7, x=P, pre=None, h=P, batch=3, bias_ih=P, bias_hh=P, h_out=2 * P, gates=P)
    order = list(ih) + list(hh) + list(rest)

    def cell(**kw):
        args = dict(ih, **hh, **rest)
        args.update(kw)
        return lib.qdg_gru_cell_packed_f32(*[args[k] for k in order], None)

    pre_mode = dict(x=None, pre=P, bias_ih=None)
    bad = [dict(hidden=-1), dict(input=-1), dict(batch=-1), dict(hidden=2 ** 62), dict(hidden=2 ** 30, batch=2 ** 40), dict(input=2 ** 40, batch=2 ** 40),
           dict(hidden=2 ** 40, input=2 ** 40),                                                    # the element count of W_ih
           dict(x=P, pre=P, bias_ih=None), dict(x=None, pre=None), dict(x=None, pre=P), dict(h_out=P),   # both, neither, bias_ih in pre mode, h_out == h
           dict(packed_ih=None), dict(alpha_ih=None), dict(beta_ih=None), dict(pre_mode, packed_hh=None), dict(alpha_hh=None), dict(beta_hh=None)]
    for sfx in ('_ih', '_hh'):                                             # everything describe refuses, of either weight
        bad += [{'levels' + sfx: 1}, {'levels' + sfx: 257, 'bits' + sfx: 8}, {'bits' + sfx: 0}, {'bits' + sfx: 9, 'levels' + sfx: 2},
                {'levels' + sfx: 17}, {'levels' + sfx: 3, 'bits' + sfx: 1}, {'bucket' + sfx: -1},
                {'packed' + sfx: P + 2}, {'alpha' + sfx: P + 1}, {'beta' + sfx: P + 2}]
    bad += [{k: None} for k in ('h', 'h_out')] + [{k: P + 2} for k in ('x', 'h', 'bias_ih', 'bias_hh', 'h_out', 'gates')]
    bad += [dict(pre_mode, pre=P + 1), dict(pre_mode, levels_hh=1), dict(pre_mode, h=None)]
    for kw in bad:
        assert cell(**kw) == -1, kw
    assert cell(batch=0, x=None, h=None, h_out=None, gates=None) == 0
    assert cell(hidden=0, packed_hh=None, alpha_hh=None, beta_hh=None, h_out=None, gates=None) == 0
    # pre mode does not look at the W_ih arguments or at `input`
    assert cell(**dict(pre_mode, batch=0, packed_ih=None, alpha_ih=P + 1, levels_ih=0, bits_ih=77, input=-3)) == 0


def _packed(rows, cols):
    n = rows * cols
    return codec.PackedUniform(torch.zeros(n // 2, dtype=torch.uint8), torch.ones(n // 16), torch.zeros(n // 16), (rows, cols), 16, 16, 4)


def test_the_modules_are_validated_before_any_launch():
    PC, PG = packed_layers.PackedGRUCell, packed_layers.PackedGRU
    cell = PC(_packed(12, 8), _packed(12, 4), torch.zeros(12), torch.zeros(12))
    assert (cell.input_size, cell.hidden_size) == (8, 4) and cell.fp32_nbytes == 4 * (96 + 48 + 24)
    assert cell.nbytes == (48 + 6 * 8 + 48) + (24 + 3 * 8 + 48)
    for args in ((_packed(12, 8), _packed(12, 8)), (_packed(16, 8), _packed(16, 4)), (_packed(12, 8), _packed(12, 4), torch.zeros(4))):
        with pytest.raises(ValueError):
            PC(*args)                                                      # [16, 4]: an LSTM's four gates, not a GRU's three
    z = torch.zeros
    for x, h, err in ((z(3, 7), None, ValueError), (z(3, 8, 1), None, ValueError), (z(3, 8), z(3, 5), ValueError), (z(3, 8), (z(3, 4),), TypeError),
                      (z(3, 8, dtype=torch.float64), None, TypeError), ([1.0], None, TypeError), (z(3, 8), z(3, 4), NotImplementedError)):
        with pytest.raises(err):
            cell(x, h)                                                     # the last one: CPU tensors, there is no CPU path
    gru = PG([cell, PC(_packed(12, 8), _packed(12, 4)), PC(_packed(12, 8), _packed(12, 4)), PC(_packed(12, 8), _packed(12, 4))], bidirectional=True)
    assert (gru.num_layers, gru.input_size, gru.hidden_size) == (2, 8, 4) and gru.nbytes == cell.nbytes + 3 * (cell.nbytes - 96)
    lstm_cell = packed_layers.PackedLSTMCell(_packed(16, 8), _packed(16, 4))
    for cells, kw in (([], {}), ([cell], dict(bidirectional=True)), ([cell, cell], {}), ([nn.GRUCell(8, 4)], {}), ([lstm_cell], {})):
        with pytest.raises(ValueError):
            PG(cells, **kw)                                                # [cell, cell]: layer 1 takes hidden = 4 inputs, not 8
    packed_seq = nn.utils.rnn.pack_padded_sequence(z(5, 2, 8), [5, 3])
    for x, hx, err in ((packed_seq, None, TypeError), (z(5, 2, 7), None, ValueError), (z(0, 2, 8), None, ValueError), (z(5, 2, 8), z(2, 2, 4), ValueError),
                       (z(5, 2, 8), (z(4, 2, 4), z(4, 2, 4)), TypeError), (z(5, 2, 8), z(4, 2, 4), NotImplementedError)):
        with pytest.raises(err):
            gru(x, hx)
    for make, arg in ((PC.from_gru_cell, nn.LSTMCell(8, 4)), (PG.from_gru, nn.LSTM(8, 4)), (packed_layers.PackedLSTMCell.from_lstm_cell, nn.GRUCell(8, 4))):
        with pytest.raises(TypeError):
            make(arg, 16)                                                  # before the device check and before packing


def test_pack_modules_and_rnn():
    model = nn.ModuleDict(dict(enc=nn.GRU(8, 4), cell=nn.GRUCell(8, 4)))
    before = dict(model.named_modules())
    assert packed_layers.pack_modules(model, 16) == {} and dict(model.named_modules()) == before   # without rnn=True left alone
    with pytest.raises(ValueError, match='at most 256 levels'):
        packed_layers.pack_modules(model, 257, rnn=True)                   # with it they are taken, and every s is checked first
    with pytest.raises(NotImplementedError):
        packed_layers.pack_modules(model, 16, rnn=True)                    # every check passed: CPU weights have no packed form
    assert dict(model.named_modules()) == before                           # nothing was replaced
