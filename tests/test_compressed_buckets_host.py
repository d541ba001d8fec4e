"""save_compressed with a bucket size PER TENSOR, on CPU tensors (libqd_host.so; no GPU): the file stores each tensor's own
bucket size and load_compressed gives back, bit for bit, what uniformQuantization / nonUniformQuantization give at that size --
the weights a per-channel model trained with.  The format and the whole read side are untouched: an independent numpy decoder
(tests/huffman_cases._npdecode) reads the same bits.  tests/test_hip_compressed_buckets.py does the same on the device, where
the symbols of the whole model come from one launch."""
import numpy as np
import pytest
import torch

import quantization
from huffman_cases import _npdecode
from quantized_distillation_amd import compressed as C

# the ten tensors: ragged rows, a row per element, n < bucket (the last bucket size is larger than its tensor), 2 .. 256 levels
SIZES = [300, 1000, 1024 + 7, 2 * 700, 5 * 37 + 3, 64, 9, 513, 2, 77]
LEVELS = [16, 4, 256, 2, 3, 16, 16, 17, 16, 5]
BUCKETS = [75, 100, 256, 700, 37, 10, 1, 256, 1, 4096]


def same(a, b):
    a, b = a.contiguous().view(-1), b.contiguous().view(-1)
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32))


def model(seed=3, sizes=SIZES):
    g = torch.Generator().manual_seed(seed)
    return {'t%d' % i: 0.3 * torch.randn(n, generator=g) for i, n in enumerate(sizes)}


def nbuckets(n, b):
    return 0 if n == 0 else -(-n // min(n, b))


def test_a_sequence_round_trips_to_each_tensors_own_quantization(tmp_path):
    ts = model()
    p = str(tmp_path / 'b.qd')
    rep = C.save_compressed(p, ts, s=LEVELS, bucket_size=BUCKETS)
    assert rep['symbolizer'] == 'per_tensor' and rep['coding'] == 'huffman'
    out = C.load_compressed(p)
    ref = _npdecode(p)
    for (k, t), s, b in zip(ts.items(), LEVELS, BUCKETS):
        want = quantization.uniformQuantization(t, s, bucket_size=b)[0]
        assert same(out[k], want), (k, s, b)
        assert same(torch.from_numpy(np.array(ref[k])), want), (k, s, b)
    hd = C.read_header(p)
    assert [e['bucket_size'] for e in hd['tensors']] == BUCKETS and [e['levels'] for e in hd['tensors']] == LEVELS
    assert hd['buckets'] == rep['buckets'] == sum(nbuckets(n, b) for n, b in zip(SIZES, BUCKETS))
    # a single bucket size does not give these weights: the capability is the sequence
    C.save_compressed(p, ts, s=LEVELS, bucket_size=256)
    other = C.load_compressed(p)
    assert not all(same(other[k], out[k]) for k in ts)


def test_a_tuple_and_numpy_integers_are_taken_like_a_list(tmp_path):
    ts = model()
    a, b = str(tmp_path / 'a.qd'), str(tmp_path / 'b.qd')
    C.save_compressed(a, ts, s=LEVELS, bucket_size=BUCKETS)
    C.save_compressed(b, ts, s=LEVELS, bucket_size=tuple(np.int64(v) for v in BUCKETS))
    assert open(a, 'rb').read() == open(b, 'rb').read()


def test_first_and_last_raw_take_a_sequence_of_the_quantized_tensors_only(tmp_path):
    ts = model()
    p = str(tmp_path / 'fl.qd')
    rep = C.save_compressed(p, ts, s=LEVELS[1:-1], bucket_size=BUCKETS[1:-1], quantize_first_last=False,
                            buffers={'bn': torch.arange(5.0)})
    out = C.load_compressed(p)
    names = list(ts)
    assert same(out[names[0]], ts[names[0]]) and same(out[names[-1]], ts[names[-1]]) and same(out['bn'], torch.arange(5.0))
    for k, s, b in zip(names[1:-1], LEVELS[1:-1], BUCKETS[1:-1]):
        assert same(out[k], quantization.uniformQuantization(ts[k], s, bucket_size=b)[0]), k
    hd = C.read_header(p)
    assert [e['bucket_size'] for e in hd['tensors']] == [None] + BUCKETS[1:-1] + [None, None]
    assert rep['quantized_elements'] == sum(SIZES[1:-1])
    with pytest.raises(ValueError, match='bucket_size'):            # one entry per QUANTIZED tensor
        C.save_compressed(p, ts, s=16, bucket_size=BUCKETS, quantize_first_last=False)


def test_non_uniform_mode_with_a_sequence(tmp_path):
    ts = model(seed=5)
    pts = [torch.linspace(0, 1, 2 + (i % 7) * 5) for i in range(len(ts))]
    p = str(tmp_path / 'n.qd')
    rep = C.save_compressed(p, ts, points=pts, bucket_size=BUCKETS)
    assert rep['symbolizer'] == 'per_tensor' and rep['mode'] == 'nonuniform'
    out = C.load_compressed(p)
    ref = _npdecode(p)
    for (k, t), pt, b in zip(ts.items(), pts, BUCKETS):
        want = quantization.nonUniformQuantization(t, pt, bucket_size=b)[0]
        assert same(out[k], want), (k, b)
        assert same(torch.from_numpy(np.array(ref[k])), want), (k, b)


@pytest.mark.parametrize('b', [256, 100, 7])
def test_equal_entries_write_the_file_of_the_scalar(tmp_path, b):
    ts = model(seed=b)
    ts['empty'] = torch.zeros(0)
    p1, p2 = str(tmp_path / 's.qd'), str(tmp_path / 'l.qd')
    r1 = C.save_compressed(p1, ts, s=LEVELS + [16], bucket_size=b)
    r2 = C.save_compressed(p2, ts, s=LEVELS + [16], bucket_size=[b] * len(ts))
    assert open(p1, 'rb').read() == open(p2, 'rb').read()
    assert r1['reference_size_mb'] == r2['reference_size_mb'] and r1['file_bytes'] == r2['file_bytes']
    assert 'symbolizer' in r1 and {k: v for k, v in r1.items() if k != 'path'} == {k: v for k, v in r2.items() if k != 'path'}


def test_a_model_with_a_nan_bucket_and_an_infinite_bucket(tmp_path):
    ts = model(seed=9)
    ts['t0'][80] = float('nan')          # bucket 1 of 4 (75 each)
    ts['t1'][950] = float('inf')         # the last bucket of t1
    ts['t4'][0] = float('-inf')
    p = str(tmp_path / 'nf.qd')
    C.save_compressed(p, ts, s=LEVELS, bucket_size=BUCKETS)
    out = C.load_compressed(p)
    for (k, t), s, b in zip(ts.items(), LEVELS, BUCKETS):
        assert same(out[k], quantization.uniformQuantization(t, s, bucket_size=b)[0]), k
    assert bool(torch.isnan(out['t0'][75:150]).all()) and not bool(torch.isnan(out['t0'][:75]).any())
    assert bool(torch.isnan(out['t1'][900:]).all()) and bool(torch.isnan(out['t4'][:37]).all())


def test_the_report_obeys_its_formulas(tmp_path):
    ts = model(seed=11)
    p = str(tmp_path / 'r.qd')
    rep = C.save_compressed(p, ts, s=LEVELS[1:-1], bucket_size=BUCKETS[1:-1], quantize_first_last=False)
    hd = C.read_header(p)
    import os
    assert rep['file_bytes'] == os.path.getsize(p) == hd['file_bytes'] == sum(rep['sections'].values())
    assert rep['sections']['alpha_beta'] == 8 * sum(nbuckets(n, b) for n, b in zip(SIZES[1:-1], BUCKETS[1:-1]))
    # code_bits: the histogram of the stored symbols under the stored code lengths
    counts = np.zeros(256, np.int64)
    for k, s, b in zip(list(ts)[1:-1], LEVELS[1:-1], BUCKETS[1:-1]):
        q, sf = quantization.uniformQuantization(ts[k], s, bucket_size=b)
        n = ts[k].numel()
        row = min(n, b)
        idx = torch.arange(n) // row
        lev = torch.round((q - sf.beta.view(-1)[idx]) / sf.alpha.view(-1)[idx] * (s - 1)).long().numpy()
        counts += np.bincount(lev, minlength=256)
    assert rep['code_bits'] == int(sum(int(c) * l for c, l in zip(counts, hd['code_lengths'])))
    assert rep['sections']['bitstream'] * 8 >= rep['code_bits']
    nsym = sum(SIZES[1:-1])
    raw = SIZES[0] + SIZES[-1]
    want = raw * 4 + rep['mean_bit_length'] * nsym / 8 + sum(n / b * 8 for n, b in zip(SIZES[1:-1], BUCKETS[1:-1]))
    assert rep['reference_size_mb'] == pytest.approx(want / 1e6, rel=1e-12)


@pytest.mark.parametrize('bad', [[256] * 9, [256] * 11, [], [256] * 9 + [0], [256] * 9 + [-1], [256] * 9 + [2.5], [256] * 9 + [True],
                                 [256] * 9 + [None], [256] * 9 + ['64'], 'per_channel', b'256', [256] * 9 + [2 ** 63]])
def test_every_invalid_sequence_is_a_value_error_that_names_the_rule(tmp_path, bad):
    with pytest.raises(ValueError, match='bucket_size must be a positive int, None, or a sequence of positive ints with one entry '
                                         'per quantized tensor'):
        C.save_compressed(str(tmp_path / 'x.qd'), model(), s=16, bucket_size=bad)


def test_the_scalar_checks_are_what_they_were(tmp_path):
    for bad in (0, -4, 2.5, True):
        with pytest.raises(ValueError, match='bucket_size must be a positive int or None'):
            C.save_compressed(str(tmp_path / 'x.qd'), model(), s=16, bucket_size=bad)
    rep = C.save_compressed(str(tmp_path / 'x.qd'), model(), s=16, bucket_size=None)
    assert rep['symbolizer'] == 'per_tensor'
