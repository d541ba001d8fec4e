"""libqd_infer_conv.so (include/qd_infer_conv.h: nn.Conv2d from packed weights, an implicit GEMM on fp32 MFMA) builds for gfx950
without a GPU, exports exactly the header's symbols, keeps its kernel free of scratch and spills and refuses bad arguments
before it touches a device; PackedConv2d and pack_modules(conv=True) validate before any launch."""
import pytest
import torch
from torch import nn

import infer_abi_cases as A
from quantized_distillation_amd import _infer_conv, codec, packed_layers
from quantized_distillation_amd import build as qb

@pytest.fixture(scope='module')
def lib():
    qb.build_infer_conv()
    return _infer_conv.load()


def test_header_binding_and_exports_agree(lib):
    A.check_header_binding_and_exports_agree(lib, _infer_conv, 'qd_infer_conv.h', 'qdc', 5)                 # and no symbol of another library's header
    assert not set(qb.INFER_CONV_SOURCES) & (set(qb.SOURCES) | set(qb.INFER_SOURCES) | set(qb.INFER_MM_SOURCES))


def test_the_kernel_uses_no_scratch_and_spills_nothing(lib):
    A.check_no_kernel_uses_scratch_or_spills(_infer_conv, ['k_conv2d_mm'], lds_limit=80 * 1024)


def test_refusals_and_empty_calls_without_a_device(lib):
    """Every refusal of the header, with pointers that are never dereferenced: -1 without a launch."""
    assert lib.qdc_set_grid_cap(3) == 0 and lib.qdc_set_grid_cap(0) == 3 and lib.qdc_set_grid_cap(-5) == 0
    P = 4096                                                               # a well-aligned non-NULL address, never read

    def conv(packed=P, alpha=P, beta=P, cout=10, cin=3, kh=3, kw=2, bucket=4, levels=16, bits=4, x=P, batch=2, h=8, w=7, sh=1, sw=2,
             ph=1, pw=0, bias=P, y=P):
        return lib.qdc_conv2d_packed_f32(packed, alpha, beta, cout, cin, kh, kw, bucket, levels, bits, x, batch, h, w, sh, sw, ph, pw, bias, y, None)

    for kw in (dict(levels=1), dict(levels=257, bits=8), dict(bits=0), dict(bits=9, levels=2), dict(levels=17, bits=4),
               dict(levels=9, bits=3), dict(levels=3, bits=1), dict(bucket=-1), dict(cout=-1), dict(cin=-1), dict(batch=-1), dict(h=-1), dict(w=-1),
               dict(packed=None), dict(alpha=None), dict(beta=None), dict(packed=P + 2), dict(alpha=P + 1), dict(beta=P + 2),
               dict(x=None), dict(y=None), dict(x=P + 1), dict(y=P + 2), dict(bias=P + 3),
               dict(kh=0), dict(kw=0), dict(kh=-3), dict(sh=0), dict(sw=0), dict(sw=-1), dict(ph=-1), dict(pw=-1),
               dict(h=0), dict(h=1, ph=0), dict(w=1), dict(w=1, kw=4, pw=1),                       # h + 2 pad_h < kh, w + 2 pad_w < kw
               dict(cin=2 ** 62), dict(cout=2 ** 40, cin=2 ** 40),                                 # cin kh kw, and the weight's element count
               dict(batch=2 ** 40, h=2 ** 20, w=2 ** 20), dict(cin=1, cout=2 ** 20, batch=2 ** 40, h=2 ** 10, w=2 ** 11)):   # x, y
        assert conv(**kw) == -1, kw
    assert conv(batch=0, x=None, y=None) == 0 and conv(cout=0, packed=None, y=None, bias=None) == 0


def _packed(cout=6, cols=8):
    n, nb = cout * cols, cout * cols // 16
    return codec.PackedUniform(torch.zeros(n // 2, dtype=torch.uint8), torch.ones(nb), torch.zeros(nb), (cout, cols), 16, 16, 4)


def test_the_layer_is_validated_before_any_launch():
    PC = packed_layers.PackedConv2d
    layer = PC(_packed(), (2, 1), stride=2, padding=(0, 3), bias=torch.zeros(6))
    assert (layer.in_channels, layer.out_channels, layer.kernel_size, layer.stride, layer.padding) == (4, 6, (2, 1), (2, 2), (0, 3))
    assert layer.fp32_nbytes == 4 * 48 + 24 and layer.nbytes == 24 + 2 * 3 * 4 + 24 and 'kernel_size=(2, 1)' in repr(layer)
    for kw in (dict(kernel_size=0), dict(kernel_size=(2, 2, 2)), dict(kernel_size=3), dict(stride=0), dict(stride=1.0), dict(padding=-1),
               dict(padding='same'), dict(stride=True)):
        with pytest.raises(ValueError):
            PC(_packed(), **dict(dict(kernel_size=2), **kw))               # 8 columns are no multiple of 3 x 3
    with pytest.raises(ValueError):
        PC(_packed(), 2, bias=torch.zeros(5))
    for x, err in ((torch.zeros(1, 4, 5), ValueError), (torch.zeros(1, 3, 5, 5), ValueError), (torch.zeros(1, 4, 1, 5), ValueError),
                   (torch.zeros(1, 4, 5, 5, dtype=torch.float64), TypeError), ([1.0], TypeError), (torch.zeros(1, 4, 5, 5), NotImplementedError)):
        with pytest.raises(err):
            layer(x)                                                       # the last one: a CPU tensor, there is no CPU path
    for bad in (nn.Conv2d(4, 6, 3, groups=2), nn.Conv2d(4, 6, 3, dilation=2), nn.Conv2d(4, 6, 3, padding=1, padding_mode='reflect'),
                nn.Conv2d(4, 6, 3, padding='same'), nn.ConvTranspose2d(4, 6, 3)):
        with pytest.raises(ValueError):
            PC.from_conv2d(bad, 16)                                        # before the device check and before packing
        model = nn.Sequential(nn.Linear(8, 6), bad)
        if isinstance(bad, nn.Conv2d):
            with pytest.raises(ValueError):
                packed_layers.pack_modules(model, 16, conv=True)
        assert isinstance(model[0], nn.Linear) and model[1] is bad         # nothing was replaced, the Linear in front included


def test_without_conv_a_conv2d_is_left_alone():
    model = nn.Sequential(nn.Conv2d(3, 4, 3), nn.Flatten())
    assert packed_layers.pack_modules(model, 16) == {} and isinstance(model[0], nn.Conv2d)
    with pytest.raises(ValueError, match='skip'):
        packed_layers.pack_modules(model, 16, skip=('nope',), conv=True)
    assert isinstance(model[0], nn.Conv2d)
