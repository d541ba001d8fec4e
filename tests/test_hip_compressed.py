"""Huffman-coded checkpoints on the device (quantized_distillation_amd/compressed.py with libqd_hip.so): the one-launch
decode is bit-identical to the device quantizers, the device and the host library write byte-identical files and read
each other's, and the sizes meet the reference's accounting (tests/golden/compressed_sizes.json)."""
import json
import os

import numpy as np
import pytest
import torch

import quantization
from harness import models
from huffman_cases import _npdecode, skewed_tensor
from quantized_distillation_amd import compressed as C
from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = torch.device('cuda:0')


def same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(-1).view(torch.int32).cpu(),
                                              b.contiguous().view(-1).view(torch.int32).cpu())


def param_sets():
    torch.manual_seed(0)
    wrn = list(models.WideResNet(16, 22).parameters())
    conv = list(models.student().parameters())
    g = torch.Generator().manual_seed(7)
    rag = [torch.randn(n, generator=g) for n in (1, 37, 255, 256, 257, 1023, 1024, 1025, 100003, 0, 4097)]
    return {'wrn16_22': [p.data for p in wrn], 'convnet_student': [p.data for p in conv], 'ragged': rag}


@pytest.fixture(scope='module')
def sets():
    return {k: [t.to(DEV) for t in v] for k, v in param_sets().items()}


@pytest.mark.parametrize('name', ['wrn16_22', 'convnet_student', 'ragged'])
def test_device_uniform_round_trip_matches_the_device_quantizers(tmp_path, sets, name):
    ts = {'t%d' % i: t for i, t in enumerate(sets[name])}
    p = str(tmp_path / 'u.qd')
    rep = C.save_compressed(p, ts, s=16, bucket_size=256)
    assert rep['coding'] == 'huffman'
    out = C.load_compressed(p, device=DEV)
    for k, t in ts.items():
        assert out[k].is_cuda and same(out[k], quantization.uniformQuantization(t, 16, bucket_size=256)[0]), k
    nz = [t for t in ts.values() if t.numel()]
    mt = MultiTensorQuantizer(nz, 16, 256).quantize()
    for t, q in zip(nz, mt):
        k = [kk for kk, v in ts.items() if v is t][0]
        assert same(out[k], q), k


@pytest.mark.parametrize('name', ['convnet_student', 'ragged'])
def test_device_nonuniform_round_trip_matches_the_device_quantizer(tmp_path, sets, name):
    ts = {'t%d' % i: t for i, t in enumerate(sets[name])}
    pts = [torch.linspace(0, 1, 2 + (i % 7) * 5) for i in range(len(ts))]
    p = str(tmp_path / 'n.qd')
    C.save_compressed(p, ts, points=pts, bucket_size=100)
    out = C.load_compressed(p, device=DEV)
    for (k, t), pt in zip(ts.items(), pts):
        assert same(out[k], quantization.nonUniformQuantization(t, pt.to(DEV), bucket_size=100)[0]), k


@pytest.mark.parametrize('kind', ['uniform', 'nonuniform'])
def test_device_and_host_files_are_byte_identical_and_cross_decode(tmp_path, sets, kind):
    dev_ts = {'t%d' % i: t for i, t in enumerate(sets['convnet_student'] + sets['ragged'])}
    host_ts = {k: v.cpu() for k, v in dev_ts.items()}
    kw = dict(s=5, bucket_size=64) if kind == 'uniform' else dict(points=[[0.0, 0.1, 0.5, 0.6, 1.0]], bucket_size=None)
    pd, ph = str(tmp_path / 'd.qd'), str(tmp_path / 'h.qd')
    bn = torch.randn(9, generator=torch.Generator().manual_seed(1))
    C.save_compressed(pd, dev_ts, quantize_first_last=False, buffers={'bn': bn.to(DEV)}, **kw)
    C.save_compressed(ph, host_ts, quantize_first_last=False, buffers={'bn': bn}, **kw)
    assert open(pd, 'rb').read() == open(ph, 'rb').read()
    a = C.load_compressed(pd, device='cpu')
    b = C.load_compressed(ph, device=DEV)
    c = C.load_compressed(pd, device=DEV)
    for k in a:
        assert same(a[k], b[k]) and same(b[k], c[k]), k


def test_out_in_place_on_the_device(tmp_path, sets):
    ts = {'t%d' % i: t for i, t in enumerate(sets['convnet_student'])}
    p = str(tmp_path / 'o.qd')
    C.save_compressed(p, ts, s=4, bucket_size=256)
    out = {k: torch.empty_like(v) for k, v in ts.items()}
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    res = C.load_compressed(p, out=out)
    for k, t in ts.items():
        assert res[k].data_ptr() == ptrs[k] and same(out[k], quantization.uniformQuantization(t, 4, bucket_size=256)[0])


def test_device_file_sizes_meet_the_reference_accounting(tmp_path):
    cases = json.load(open(os.path.join(HERE, 'golden', 'compressed_sizes.json')))
    for case in cases:
        g = torch.Generator().manual_seed(case['seed'])
        ts = [(0.05 * torch.randn(*s, generator=g)).to(DEV) for s in case['shapes']]
        kw = dict(points=case['points']) if 'points' in case else dict(s=case['s'])
        p = str(tmp_path / 'm.qd')
        rep = C.save_compressed(p, {'t%d' % i: t for i, t in enumerate(ts)}, bucket_size=case['bucket_size'],
                                quantize_first_last=case['quantize_first_last'], **kw)
        n = rep['quantized_elements']
        assert rep['mean_bit_length'] == pytest.approx(case['mean_bit_length'], rel=1e-12)
        assert rep['reference_size_mb'] == pytest.approx(case['size_mb'], rel=1e-12)
        allowance = 0.1 * n / 8 + 64 * 1024 + 8 * len(ts) + rep['sections']['table'] + rep['sections']['points']
        assert rep['file_bytes'] <= case['size_mb'] * 1e6 + allowance, (case, rep)


@pytest.mark.parametrize('bucket', [None, 7, 100])
@pytest.mark.parametrize('s', [2, 3, 256])
def test_device_uniform_round_trip_at_the_ends_of_s_and_odd_buckets(tmp_path, sets, s, bucket):
    dev_ts = {'t%d' % i: t for i, t in enumerate(sets['ragged'])}
    pd, ph = str(tmp_path / 'd.qd'), str(tmp_path / 'h.qd')
    rep = C.save_compressed(pd, dev_ts, s=s, bucket_size=bucket)
    assert rep['coding'] == 'huffman'
    out = C.load_compressed(pd, device=DEV)
    for k, t in dev_ts.items():
        assert out[k].is_cuda and same(out[k], quantization.uniformQuantization(t, s, bucket_size=bucket)[0]), k
    C.save_compressed(ph, {k: v.cpu() for k, v in dev_ts.items()}, s=s, bucket_size=bucket)
    assert open(pd, 'rb').read() == open(ph, 'rb').read()
    got = _npdecode(pd)                                     # the independent numpy decoder of the documented format
    for k in dev_ts:
        assert np.array_equal(got[k].view(np.int32), out[k].cpu().numpy().view(np.int32)), k


def test_device_skewed_model_with_a_code_deeper_than_the_lookup_table(tmp_path):
    # 21 levels with counts 1, 1, 2, 4, ..., 2^19: a real Huffman code of 20 bits, the decoder's per-length search
    # (test_compressed_host.py confirms on the CPU that every element lands on its intended level)
    x, _lev, s = skewed_tensor()
    pd, ph = str(tmp_path / 'd.qd'), str(tmp_path / 'h.qd')
    rep = C.save_compressed(pd, {'w': x.to(DEV)}, s=s, bucket_size=None)
    hdr = C.read_header(pd)
    assert hdr['max_code_length'] > 10 and hdr['coding'] == 'huffman' and rep['coding'] == 'huffman'
    q = quantization.uniformQuantization(x.to(DEV), s)[0]
    assert same(C.load_compressed(pd, device=DEV)['w'], q)
    C.save_compressed(ph, {'w': x}, s=s, bucket_size=None)
    assert open(pd, 'rb').read() == open(ph, 'rb').read()
    assert same(C.load_compressed(ph, device=DEV)['w'], q) and same(C.load_compressed(pd, device='cpu')['w'], q)


def test_device_one_symbol_model_and_empty_model(tmp_path):
    pd, ph = str(tmp_path / 'd.qd'), str(tmp_path / 'h.qd')
    c = torch.full((3000,), 0.25)
    rep = C.save_compressed(pd, {'c': c.to(DEV)}, s=16, bucket_size=256)
    assert rep['code_bits'] == 0 and rep['mean_bit_length'] == 0 and rep['sections']['bitstream'] == 0
    C.save_compressed(ph, {'c': c}, s=16, bucket_size=256)
    assert open(pd, 'rb').read() == open(ph, 'rb').read()
    out = C.load_compressed(pd, device=DEV)['c']
    assert out.is_cuda and same(out, quantization.uniformQuantization(c.to(DEV), 16, bucket_size=256)[0])
    rep = C.save_compressed(pd, {'e': torch.randn(0).to(DEV)}, s=16)
    out = C.load_compressed(pd, device=DEV)['e']
    assert rep['coding'] == 'none' and out.is_cuda and out.numel() == 0


def test_device_code_longer_than_32_bits_falls_back_to_fixed_width(tmp_path):
    # the construction of test_compressed_host.py: Fibonacci level counts, the optimal code of 34 symbols is 33 bits deep
    fib = [1, 1]
    while len(fib) < 34:
        fib.append(fib[-1] + fib[-2])
    s = 34
    lev = np.repeat(np.arange(34), fib)
    np.random.default_rng(0).shuffle(lev)
    x = torch.from_numpy((lev / (s - 1)).astype(np.float32)).to(DEV)
    p = str(tmp_path / 'f.qd')
    rep = C.save_compressed(p, {'w': x}, s=s, bucket_size=None)
    assert rep['coding'] == 'fixed' and rep['max_code_length'] == 8 and C.read_header(p)['coding'] == 'fixed'
    assert same(C.load_compressed(p, device=DEV)['w'], quantization.uniformQuantization(x, s)[0])
