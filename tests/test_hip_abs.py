"""'absmax' / 'absnorm' scaling (csrc/qd_abs.hip) on the device, on every case of tests/abs_cases.py: through
ScalingFunction.scale_down / inv_scale_down, through uniformQuantization(type_of_scaling=...), and at the three C entry points.

The reference's own code for these types raises on every torch version, so there is no reference output: the expectations
are the oracle's (oracle/oracle_np.py), which tests/test_abs_cases_host.py holds to torch's CPU ops.  sign, u, q and the way
back are compared bit for bit GIVEN the norm and the mean the device reports (abs_cases.bits_same: the sign of a zero and the
position of a NaN count); the absmax norm is bit-exact, the absnorm norm is held to abs_cases.BOUND of the float64 value and
its ratio goes to the reduction-error log.  Two calls on one input give the same bits, the absnorm norm included."""
import numpy as np
import pytest
import torch

import abs_cases as ac
import quantization
from oracle import oracle_np as onp
from quantized_distillation_amd import _lib

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
LOG_KIND = 'a4 absnorm L2 norm'


@pytest.fixture(scope='module', autouse=True)
def _built():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    _lib.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_bits_equal(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _options(case):
    return case.options.get('max_element', False), bool(case.options.get('subtract_mean', False))


def _scale_down(case, xd):
    me, sub = _options(case)
    sf = quantization.ScalingFunction(case.kind, me, sub, case.bucket)
    u = sf.scale_down(xd)
    return sf, u


def _quantize(case, xd, in_place=False):
    me, sub = _options(case)
    return quantization.uniformQuantization(xd, case.s, type_of_scaling=case.kind, max_element=me, subtract_mean=sub,
                                            bucket_size=case.bucket, modify_in_place=in_place)


def run_api(case, xd=None, twice=True):
    """One case through the Python API.  xd: the device tensor holding case.x in some form (default: freshly allocated).
    Returns what the device gave (for the comparisons between two inputs)."""
    xd = dev(case.x) if xd is None else xd
    me, sub = _options(case)
    n = case.x.size
    nb, row, padded = onp.bucket_geometry(n, case.bucket)

    sf, u = _scale_down(case, xd)
    mean = float(sf.mean_tensor) if sub else None
    nrm = sf.norm_scaling.cpu().numpy().reshape(-1)
    assert u.shape == sf.tensor_sign.shape == (torch.Size([n]) if case.bucket is None else torch.Size([nb, row])), (case.id, u.shape)
    assert sf.norm_scaling.shape == (torch.Size([1]) if case.bucket is None else torch.Size([nb, 1]))
    ac.check_norm(case, nrm, mean, log_kind=LOG_KIND)
    want = ac.expect(case, nrm, mean)
    assert ac.sign_same(sf.tensor_sign, want['sign']), (case.id, 'sign')
    assert ac.bits_same(u, want['u']), (case.id, 'u')
    back = sf.inv_scale_down(u)
    assert back.shape == xd.shape and ac.bits_same(back, want['back']), (case.id, 'inv_scale_down')

    q, sf2 = _quantize(case, xd)
    assert ac.bits_same(sf2.norm_scaling, nrm), (case.id, 'the norm of uniformQuantization differs from scale_down')
    if sub:
        assert ac.bits_same(sf2.mean_tensor, np.float32(mean)), (case.id, 'mean')
    assert q.shape == xd.shape and ac.bits_same(q, want['q']), (case.id, 'q')
    assert ac.bits_same(xd, case.x), (case.id, 'the input was written')

    x2 = xd.clone()                                              # (keeps the strides of xd)
    if x2.is_contiguous():
        q2, sf3 = _quantize(case, x2, in_place=True)
        assert q2.data_ptr() == x2.data_ptr() and device_bits_equal(q2, q), (case.id, 'modify_in_place')
        assert device_bits_equal(x2, q) and device_bits_equal(sf3.norm_scaling, sf2.norm_scaling), (case.id, 'modify_in_place')
    else:
        with pytest.raises(ValueError, match='contiguous'):
            _quantize(case, x2, in_place=True)

    if twice:
        sf_b, u_b = _scale_down(case, xd)
        q_b, sf2_b = _quantize(case, xd)
        assert device_bits_equal(u_b, u) and device_bits_equal(sf_b.norm_scaling, sf.norm_scaling), (case.id, 'second call')
        assert device_bits_equal(sf_b.tensor_sign, sf.tensor_sign) and device_bits_equal(q_b, q), (case.id, 'second call')
        assert device_bits_equal(sf2_b.norm_scaling, sf2.norm_scaling), (case.id, 'second call')
    return dict(u=u.cpu().numpy().reshape(-1), sign=sf.tensor_sign.cpu().numpy().reshape(-1), norm=nrm,
                q=q.cpu().numpy().reshape(-1), back=back.cpu().numpy().reshape(-1))


def check_clean_buckets(case, got):
    """A non-finite case: the buckets that hold no planted element give the bits of the same call on the input with the
    planted elements replaced by 1.0."""
    if case.options.get('subtract_mean'):
        return                                                   # the mean is NaN: no bucket is clean
    mask, clean, x1 = ac.clean_elements(case)
    if not clean.any():
        return
    other = run_api(case._replace(x=x1, id=case.id + ' (planted -> 1.0)', options=dict(case.options, planted=None)), twice=False)
    row = onp.bucket_geometry(case.x.size, case.bucket)[1]
    pmask = np.repeat(clean, row)
    assert ac.bits_same(got['norm'][clean], other['norm'][clean]), (case.id, 'norm of the clean buckets')
    for name, m in (('u', pmask), ('sign', pmask), ('q', mask), ('back', mask)):
        assert ac.bits_same(got[name][m], other[name][m]), (case.id, name, 'of the clean buckets')


def run_cases(cases, **kw):
    count = 0
    for case in cases:
        got = run_api(case, **kw)
        if case.options.get('planted') is not None:
            check_clean_buckets(case, got)
        count += 1
    assert count > 0


@pytest.mark.parametrize('bucket', ac.LOOP_BUCKETS)
@pytest.mark.parametrize('kind', ac.KINDS)
def test_bucket_loop(kind, bucket):
    run_cases(ac.loop_cases(kind, bucket))


@pytest.mark.parametrize('kind', ac.KINDS)
def test_more_buckets_than_waves(kind):
    run_cases(ac.many_cases(kind))


@pytest.mark.parametrize('which', ['small', 'big'])
@pytest.mark.parametrize('kind', ac.KINDS)
def test_one_bucket(kind, which):
    run_cases(ac.single_cases(kind, which))


def three_forms(x):
    """The tensor as allocated, a view 4 bytes into an allocation, and a transposed 2-D tensor whose row-major reading is x
    (257 and 70001 are primes: their only 2-D forms are (n, 1) and its transpose, which torch counts as contiguous)."""
    n = x.size
    buf = torch.full((n + 5,), 777.0)
    buf[1:1 + n] = torch.from_numpy(x)
    yield 'own', dev(x)
    yield 'offset', buf.to(DEV)[1:1 + n]                     # (the forms of tests/test_hip_nonfinite.py)
    r = next(d for d in (40, 1) if n % d == 0)
    yield 'transposed', dev(x.reshape(r, n // r).T).t()


@pytest.mark.parametrize('form', ['own', 'offset', 'transposed'])
@pytest.mark.parametrize('kind', ac.KINDS)
def test_options(kind, form):
    """subtract_mean x max_element x modify_in_place in three tensor forms; the oracle takes the mean the device computed."""
    for case in ac.option_cases(kind):
        xd = dict(three_forms(case.x))[form]
        assert xd.data_ptr() % 16 == 4 or form != 'offset'
        assert form != 'transposed' or case.x.size != 1000 or not xd.is_contiguous()
        run_api(case, xd)


@pytest.mark.parametrize('shape', ac.NONFINITE_SHAPES, ids=lambda s: 'n%d-b%s' % s)
@pytest.mark.parametrize('kind', ac.KINDS)
def test_nonfinite(kind, shape):
    run_cases(ac.nonfinite_cases(kind, shape))


@pytest.mark.parametrize('kind', ac.KINDS)
def test_scales(kind):
    run_cases(c for c in ac.scale_cases() if c.kind == kind)


@pytest.mark.parametrize('kind', ac.KINDS)
def test_absorbed_tails(kind):
    """absnorm: the norm bound where an fp32 running sum per lane loses every small square (absmax: the same data)."""
    run_cases(ac.absorbed_cases(kind))


def run_abi(case):
    """The three C entry points on raw pointers, with qd_workspace_bytes() of scratch."""
    lib = _lib.load()
    n = case.x.size
    nb, row, padded = onp.bucket_geometry(n, case.bucket)
    wsb = int(lib.qd_workspace_bytes())
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=DEV)
    st = _lib.stream_ptr(torch.device(DEV))
    x = dev(case.x)
    k = ac.KINDS.index(case.kind)
    u, sign = (torch.full((padded,), 777.0, device=DEV) for _ in range(2))
    q, y = (torch.full((n,), 777.0, device=DEV) for _ in range(2))
    norm, norm2 = (torch.full((nb,), 777.0, device=DEV) for _ in range(2))
    b = case.bucket or 0
    assert lib.qd_scale_down_abs_f32(x.data_ptr(), u.data_ptr(), sign.data_ptr(), n, b, k, norm.data_ptr(), None, 0, 0.0,
                                     ws.data_ptr(), wsb, st) == 0
    assert lib.qd_inv_scale_abs_f32(u.data_ptr(), sign.data_ptr(), y.data_ptr(), n, b, norm.data_ptr(), None, st) == 0
    assert lib.qd_uniform_abs_f32(x.data_ptr(), q.data_ptr(), n, b, case.s, k, norm2.data_ptr(), None, 0, 0.0,
                                  ws.data_ptr(), wsb, st) == 0
    torch.cuda.synchronize()
    nrm = norm.cpu().numpy()
    ac.check_norm(case, nrm, log_kind=LOG_KIND + ' at the C ABI')
    assert device_bits_equal(norm, norm2), case.id
    want = ac.expect(case, nrm)
    assert ac.sign_same(sign, want['sign']) and ac.bits_same(u, want['u']), case.id
    assert ac.bits_same(y, want['back']) and ac.bits_same(q, want['q']), case.id
    assert ac.bits_same(x, case.x), case.id


@pytest.mark.parametrize('kind', ac.KINDS)
def test_c_entry_points(kind):
    """One non-finite case on the bucket loop, one on the two-stage path, and the absorbed tails, straight at the C ABI."""
    picked = [c for shape in (ac.NONFINITE_SHAPES[0], ac.NONFINITE_SHAPES[4]) for c in ac.nonfinite_cases(kind, shape)
              if c.id.endswith('-nan_inf-last')]
    assert len(picked) == 2
    for case in picked + list(ac.absorbed_cases(kind))[:ac.ABSORBED_BITING]:
        run_abi(case)
