"""libqd_infer_gen.so (include/qd_infer_gen.h: vocabulary projection, log-softmax and top-k from the packed generator weight) builds
for gfx950 without a GPU, exports exactly the header's symbols, keeps its kernels free of scratch and spills, sizes `work` as the
header says and refuses bad arguments before it touches a device; PackedGenerator validates before any launch."""
import pytest
import torch

import infer_abi_cases as A
from quantized_distillation_amd import _infer_gen, codec, packed_layers
from quantized_distillation_amd import build as qb


@pytest.fixture(scope='module')
def lib():
    qb.build_infer_gen()
    return _infer_gen.load()


def test_header_binding_and_exports_agree(lib):
    A.check_header_binding_and_exports_agree(lib, _infer_gen, 'qd_infer_gen.h', 'qdn', 6)
    others = set(qb.SOURCES).union(*(row[1] for row in qb.INFER_LIBRARIES if row[0] != 'libqd_infer_gen.so'))
    assert qb.INFER_GEN_SOURCES == ['qdn_generator.hip'] and not set(qb.INFER_GEN_SOURCES) & others
    header = open(A.os.path.join(A.ROOT, 'include', 'qd_infer_gen.h')).read()
    assert '#define QDN_PANEL %d\n' % _infer_gen.PANEL in header and '#define QDN_MAX_TOPK %d\n' % _infer_gen.MAX_TOPK in header


def test_the_kernels_use_no_scratch_and_spill_nothing(lib):
    A.check_no_kernel_uses_scratch_or_spills(_infer_gen, ['k_gen_panel_mm', 'k_gen_finish'], lds_limit=64 * 1024, vgpr_limit=128)


@pytest.mark.parametrize('V,m,k,want', (
    (1, 1, 0, 8), (64, 1, 0, 8), (65, 3, 5, 2 * 3 * 48), (32768, 64, 5, 512 * 64 * 48), (10000, 320, 16, 157 * 320 * 136), (0, 7, 5, 0), (50, 0, 5, 0),
    (-1, 1, 0, -1), (1, -1, 0, -1), (1, 1, -1, -1), (1, 1, 17, -1), (2 ** 31 - 64, 1, 0, -1), (2 ** 31 - 65, 2 ** 40, 16, -1)))
def test_work_bytes(lib, V, m, k, want):
    assert lib.qdn_generator_work_bytes(V, m, k) == want


def test_refusals_and_empty_calls_without_a_device(lib):
    """Every refusal of the header, with pointers that are never dereferenced: -1 without a launch."""
    assert lib.qdn_set_grid_cap(3) == 0 and lib.qdn_set_grid_cap(0) == 3 and lib.qdn_set_grid_cap(-5) == 0
    P = 4096                                                               # a well-aligned non-NULL address, never read
    base = dict(packed=P, alpha=2 * P, beta=3 * P, V=70, dim=5, bucket=4, levels=16, bits=4, x=4 * P, m=3, bias=5 * P, lse=6 * P, logp=7 * P, k=5,
                top_val=8 * P, top_idx=9 * P, work=10 * P)

    def call(**kw):
        args = dict(base, **kw)
        return lib.qdn_generator_packed_f32(*[args[n] for n in base], None)

    bad = [dict(V=-1), dict(dim=-1), dict(m=-1), dict(V=2 ** 31), dict(V=2 ** 30, dim=2 ** 33), dict(m=2 ** 60), dict(k=-1), dict(k=17),
           dict(levels=1), dict(levels=257, bits=8), dict(bits=0), dict(bits=9, levels=2), dict(levels=17), dict(bucket=-1), dict(top_idx=9 * P + 4)]
    bad += [{n: None} for n in ('packed', 'alpha', 'beta', 'x', 'lse', 'work', 'top_val', 'top_idx')]
    bad += [{n: P + 2} for n in ('packed', 'alpha', 'beta', 'x', 'bias', 'lse', 'logp', 'top_val', 'work')]
    bad += [{out: base[other]} for out in ('lse', 'logp', 'top_val', 'top_idx', 'work')
            for other in ('packed', 'alpha', 'beta', 'x', 'bias', 'lse', 'logp', 'top_val', 'top_idx', 'work') if other != out]
    for kw in bad:
        assert call(**kw) == -1, kw
    empty = {n: None for n in base if isinstance(base[n], int) and base[n] >= P}
    assert call(m=0, **empty) == 0 and call(V=0, **empty) == 0
    assert call(k=0, top_val=None, top_idx=None, V=0) == 0                 # k == 0: top_* are not looked at


def _packed(rows, cols):
    n = rows * cols
    return codec.PackedUniform(torch.zeros(n // 2, dtype=torch.uint8), torch.ones(n // 16), torch.zeros(n // 16), (rows, cols), 16, 16, 4)


def test_the_module_is_validated_before_any_launch():
    gen = packed_layers.PackedGenerator(_packed(8, 16), torch.zeros(8))
    assert (gen.rows, gen.cols) == (8, 16) and gen.fp32_nbytes == 4 * (128 + 8) and gen.nbytes == 64 + 8 * 8 + 32 and 'rows=8' in gen.extra_repr()
    with pytest.raises(TypeError):
        packed_layers.PackedGenerator(torch.nn.Linear(16, 8))
    with pytest.raises(ValueError):
        packed_layers.PackedGenerator(_packed(8, 16), torch.zeros(16))
    z = torch.zeros
    for x, kw, err in (([1.0], {}, TypeError), (z(3, 16, dtype=torch.float64), {}, TypeError), (z(3, 15), {}, ValueError), (z(3, 16), dict(topk=17), ValueError),
                       (z(3, 16), dict(topk=-1), ValueError), (z(3, 16), dict(topk=2.0), ValueError), (z(3, 16), {}, NotImplementedError)):
        with pytest.raises(err):
            gen(x, **kw)                                                   # the last one: CPU tensors, there is no CPU path
    for args, err in (((torch.nn.Linear(16, 8).weight, 16), TypeError), ((torch.nn.Linear(16, 8), 257), ValueError), ((torch.nn.Linear(16, 8), 16), NotImplementedError)):
        with pytest.raises(err):
            packed_layers.PackedGenerator.from_linear(*args)               # CPU weights have no packed form
