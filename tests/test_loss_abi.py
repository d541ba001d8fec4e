"""libqd_loss.so (include/qd_loss.h) builds for gfx950 without a GPU, exports exactly the header's symbols, keeps its kernels free of scratch and spills
within 160 KiB of LDS and refuses bad arguments before it touches a device; the Python functions validate before any launch; no other library's list grows."""
import pytest
import torch

import infer_abi_cases as A
from quantized_distillation_amd import _lib, _loss, kd_loss
from quantized_distillation_amd import build as qb


@pytest.fixture(scope='module')
def lib():
    qb.build_loss()
    return _loss.load()


def test_header_binding_and_exports_agree(lib):
    A.check_header_binding_and_exports_agree(lib, _loss, 'qd_loss.h', 'qdl', 7)
    header = open(A.os.path.join(A.ROOT, 'include', 'qd_loss.h')).read()
    assert '#define QDL_WAVE_COLS %d\n' % lib.qdl_wave_cols() in header and '#define QDL_LDS_COLS %d\n' % lib.qdl_lds_cols() in header
    assert 0 < lib.qdl_wave_cols() < lib.qdl_lds_cols() and 8 * lib.qdl_lds_cols() < 160 * 1024
    assert 'qdl_' not in open(A.os.path.join(A.ROOT, 'include', 'qd_hip.h')).read()
    assert not [s for s in list(_lib.SIGNATURES) + qb.SOURCES + [f for row in qb.INFER_LIBRARIES for f in row[1]] if 'qdl_' in s]


def test_the_kernels_use_no_scratch_and_spill_nothing(lib):
    rows = ['k_kd_rows<%d, %s>' % (staging, t1) for staging in (0, 1, 2) for t1 in ('true', 'false')]
    A.check_no_kernel_uses_scratch_or_spills(_loss, rows + ['k_kd_finish'], lds_limit=160 * 1024)


def test_refusals_without_a_device(lib):
    """Every refusal of the header, with pointers that are never dereferenced: -1 without a launch."""
    assert lib.qdl_set_grid_cap(3) == 0 and lib.qdl_set_grid_cap(0) == 3 and lib.qdl_set_grid_cap(-5) == 0
    P = 4096                                                               # a well-aligned non-NULL address, never read
    base = dict(student=P, teacher=2 * P, target=3 * P, rows=3, cols=7, temperature=2.0, kl_scale=0.5, nll_scale=0.5, ignore_index=-100,
                grad=4 * P, row_kl=5 * P, row_nll=6 * P, loss=7 * P)
    arrays = ('student', 'teacher', 'target', 'grad', 'row_kl', 'row_nll', 'loss')
    bad = [dict(rows=-1), dict(cols=-1), dict(cols=0), dict(rows=0, cols=0), dict(rows=2 ** 40, cols=2 ** 40), dict(rows=2 ** 31, cols=2 ** 30),
           dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float('inf')), dict(temperature=float('nan')), dict(target=3 * P + 4),
           dict(rows=0, loss=None), dict(rows=0, grad=P + 2)]
    bad += [{n: None} for n in arrays] + [{n: base[n] + 2} for n in arrays]
    bad += [{out: base[other]} for out in arrays[3:] for other in arrays if other != out]
    for kw in bad:
        args = dict(base, **kw)
        assert lib.qdl_kd_loss_f32(*[args[n] for n in base], None) == -1, kw


def test_the_python_functions_validate_before_any_launch():
    z, y = torch.zeros(3, 5), torch.zeros(3, dtype=torch.int64)
    for args, kw, err in (((z, z, y), {}, NotImplementedError), ((z, z, y), dict(batch=2), NotImplementedError),      # CPU tensors: no CPU path
                          (([0.0], z, y), {}, TypeError), ((z.double(), z, y), {}, TypeError), ((z, z.half(), y), {}, TypeError), ((z, z, y.int()), {}, TypeError),
                          ((z[0], z[0], y), {}, ValueError), ((z, z[:2], y), {}, ValueError), ((z, z, y[:2]), {}, ValueError), ((z[:, :0], z[:, :0], y), {}, ValueError),
                          ((z, z, y), dict(temperature=0.0), ValueError), ((z, z, y), dict(temperature=float('nan')), ValueError),
                          ((z, z, y), dict(teacher_weight='0.7'), TypeError), ((z, z, y), dict(batch=0), ValueError), ((z, z, y), dict(batch=2, pad=1.0), TypeError)):
        with pytest.raises(err):
            (kd_loss.fused_word_kd_loss if 'batch' in kw else kd_loss.fused_kd_loss)(*args, **kw)
