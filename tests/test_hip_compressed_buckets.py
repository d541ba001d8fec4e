"""save_compressed with a bucket size PER TENSOR on the device: in uniform mode the symbols, alpha and beta of the whole model
come from one launch (qd_multi_uniform_symbols_u8), the file is byte-identical to the one libqd_host.so writes from the CPU
copies, and it decodes -- on the device, on the host and through the independent numpy decoder -- to each tensor's own
uniformQuantization(t_j, s_j, bucket_size=b_j).  Last: the user's path, a per-channel model trained by DistillTrainer, saved and
loaded back to the bits it trained with."""
import numpy as np
import pytest
import torch

import quantization
from huffman_cases import _npdecode
from quantized_distillation_amd import compressed as C
from quantized_distillation_amd.multi_tensor import per_channel_bucket_sizes
from test_compressed_buckets_host import BUCKETS, LEVELS, model
from test_hip_compressed import param_sets, same

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
ENTRY = 'qd_multi_uniform_symbols_u8'


@pytest.fixture(scope='module')
def sets():
    ps = param_sets()
    return {k: [t.to(DEV) for t in ps[k]] for k in ('convnet_student', 'ragged')}


def on_device(ts):
    return {k: v.to(DEV) for k, v in ts.items()}


def test_the_device_file_is_the_hosts_and_decodes_everywhere_to_each_tensors_own_quantization(tmp_path):
    host_ts = model()
    dev_ts = on_device(host_ts)
    pd, ph = str(tmp_path / 'd.qd'), str(tmp_path / 'h.qd')
    rd = C.save_compressed(pd, dev_ts, s=LEVELS, bucket_size=BUCKETS)
    rh = C.save_compressed(ph, host_ts, s=LEVELS, bucket_size=BUCKETS)
    assert rd['symbolizer'] == ENTRY and rh['symbolizer'] == 'per_tensor'
    assert open(pd, 'rb').read() == open(ph, 'rb').read()
    assert {k: v for k, v in rd.items() if k not in ('path', 'symbolizer')} == {k: v for k, v in rh.items() if k not in ('path', 'symbolizer')}
    on_dev, on_host, ref = C.load_compressed(pd, device=DEV), C.load_compressed(pd, device='cpu'), _npdecode(pd)
    for (k, t), s, b in zip(dev_ts.items(), LEVELS, BUCKETS):
        want = quantization.uniformQuantization(t, s, bucket_size=b)[0]
        assert on_dev[k].is_cuda and same(on_dev[k], want) and same(on_host[k], want), (k, s, b)
        assert same(torch.from_numpy(np.array(ref[k])), want), (k, s, b)
    assert [e['bucket_size'] for e in C.read_header(pd)['tensors']] == BUCKETS


def test_first_and_last_raw_on_the_device(tmp_path):
    host_ts = model(seed=4)
    dev_ts = on_device(host_ts)
    pd, ph = str(tmp_path / 'd.qd'), str(tmp_path / 'h.qd')
    kw = dict(s=LEVELS[1:-1], bucket_size=BUCKETS[1:-1], quantize_first_last=False)
    rd = C.save_compressed(pd, dev_ts, buffers={'bn': torch.arange(5.0, device=DEV)}, **kw)
    C.save_compressed(ph, host_ts, buffers={'bn': torch.arange(5.0)}, **kw)
    assert rd['symbolizer'] == ENTRY and open(pd, 'rb').read() == open(ph, 'rb').read()


@pytest.mark.parametrize('b', [256, 100, 7])
def test_equal_entries_write_the_file_of_the_scalar(tmp_path, sets, b):
    ts = {'t%d' % i: t for i, t in enumerate(sets['ragged'])}
    p1, p2 = str(tmp_path / 's.qd'), str(tmp_path / 'l.qd')
    r1 = C.save_compressed(p1, ts, s=16, bucket_size=b)
    r2 = C.save_compressed(p2, ts, s=16, bucket_size=[b] * len(ts))
    assert (r1['symbolizer'], r2['symbolizer']) == ('per_tensor', ENTRY)
    assert open(p1, 'rb').read() == open(p2, 'rb').read()
    assert r1['reference_size_mb'] == r2['reference_size_mb']


@pytest.mark.parametrize('name', ['ragged', 'convnet_student'])
def test_per_channel_sizes_round_trip(tmp_path, sets, name):
    tensors = sets[name]
    if name == 'ragged':                                     # flat tensors have no channels: fold those whose size factors
        fold = {255: (15, 17), 256: (4, 64), 1023: (33, 31), 1024: (8, 128), 1025: (25, 41), 4097: (17, 241)}
        tensors = [t.view(fold[t.numel()]) if t.numel() in fold else t for t in tensors]
    sizes = per_channel_bucket_sizes(tensors)
    assert len(set(sizes)) > 2
    levels = [(2, 16, 256, 5)[i % 4] for i in range(len(tensors))]
    ts = {'t%d' % i: t for i, t in enumerate(tensors)}
    p = str(tmp_path / 'pc.qd')
    rep = C.save_compressed(p, ts, s=levels, bucket_size=sizes)
    assert rep['symbolizer'] == ENTRY
    out = C.load_compressed(p, device=DEV)
    for (k, t), s, b in zip(ts.items(), levels, sizes):
        assert out[k].shape == t.shape and same(out[k], quantization.uniformQuantization(t, s, bucket_size=b)[0]), (k, s, b)


def test_a_model_with_a_nan_bucket_and_an_infinite_bucket(tmp_path):
    host_ts = model(seed=9)
    host_ts['t0'][80] = float('nan')
    host_ts['t1'][950] = float('inf')
    host_ts['t4'][0] = float('-inf')
    dev_ts = on_device(host_ts)
    pd, ph = str(tmp_path / 'd.qd'), str(tmp_path / 'h.qd')
    assert C.save_compressed(pd, dev_ts, s=LEVELS, bucket_size=BUCKETS)['symbolizer'] == ENTRY
    C.save_compressed(ph, host_ts, s=LEVELS, bucket_size=BUCKETS)
    assert open(pd, 'rb').read() == open(ph, 'rb').read()
    out = C.load_compressed(pd, device=DEV)
    for (k, t), s, b in zip(dev_ts.items(), LEVELS, BUCKETS):
        want = quantization.uniformQuantization(t, s, bucket_size=b)[0]
        got = out[k]
        na, nb = torch.isnan(got), torch.isnan(want)
        assert torch.equal(na, nb) and same(got[~na], want[~nb]), k
    assert bool(torch.isnan(out['t0'][75:150]).all()) and bool(torch.isnan(out['t1'][900:]).all())


def test_non_uniform_mode_with_a_sequence_keeps_the_loop(tmp_path):
    dev_ts = on_device(model(seed=5))
    pts = [torch.linspace(0, 1, 2 + (i % 7) * 5) for i in range(len(dev_ts))]
    p = str(tmp_path / 'n.qd')
    rep = C.save_compressed(p, dev_ts, points=pts, bucket_size=BUCKETS)
    assert rep['symbolizer'] == 'per_tensor'
    out = C.load_compressed(p, device=DEV)
    for (k, t), pt, b in zip(dev_ts.items(), pts, BUCKETS):
        assert same(out[k], quantization.nonUniformQuantization(t, pt.to(DEV), bucket_size=b)[0]), (k, b)


def test_a_per_channel_model_trained_by_the_trainer_loads_to_the_bits_it_trained_with(tmp_path):
    from harness import models
    from harness.distill import DistillTrainer, synthetic_batch
    torch.manual_seed(0)
    student = models.student()
    n = len(list(student.parameters()))
    bits = [(8, 4, 2, 4)[i % 4] for i in range(n)]
    tr = DistillTrainer(student, models.teacher(), DEV, mode='multi', bucket_size='per_channel', num_bits=bits,
                        quantize_first_and_last_layer=False)
    for step in range(2):
        tr.step(*synthetic_batch(16, DEV, seed=step))
    tr.quantize()
    torch.cuda.synchronize()
    qi = [i for i in range(n) if tr.quantized[i]]
    assert qi == list(range(1, n - 1)) and tr.mt.entry_point == 'qd_multi_uniform_buckets_f32'
    names = [k for k, _ in tr.student.named_parameters()]
    p = str(tmp_path / 'student.qd')
    rep = C.save_compressed(p, dict(zip(names, tr.masters)), s=[tr.s_of[i] for i in qi], bucket_size=[tr.bucket_of[i] for i in qi],
                            quantize_first_last=False)
    assert rep['symbolizer'] == ENTRY and len(set(tr.bucket_of[i] for i in qi)) > 2
    out = C.load_compressed(p, device=DEV)
    for i, (k, param) in enumerate(zip(names, tr.params)):
        assert out[k].shape == param.shape and same(out[k], param.data), (i, k)      # the shadows the next forward runs on
    assert not same(out[names[1]], tr.masters[1])
