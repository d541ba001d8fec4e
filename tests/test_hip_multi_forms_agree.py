"""The forms of the one-launch uniform quantizer against EACH OTHER, through the C entry points themselves.

The other suites hold every form to the per-tensor call; MultiTensorQuantizer routes an all-equal `s` to the scalar entry
point, so none of them runs two forms on the same run-time branches of the body they share.  Here one small table goes
through every entry point that can express the same request:

    bucketed      plain == opt(no clamp, deterministic) == levels([s] * n) == buckets([b] * n, [s] * n)
                  clamp / stochastic (seed by value, seed in a device cell):  opt == levels == buckets
                  out16 (fp16, bf16) == the levels output converted on the CPU, in every option set
    no buckets    global == global_opt == global_levels, global_out16 == the converted result

Outputs are compared as bit patterns, guard bands of 777 (0x5A5A for 16 bits) included.  A few thousand elements in all."""
import ctypes

import numpy as np
import pytest
import torch

import out16_cases as C
from quantized_distillation_amd import _lib
from test_hip_multi_stochastic import Carved
from test_hip_out16 import Carved16

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED0 = 0x1234ABCD5678
CLAMP = 0.05                    # the values are 0.1 * randn: the limit cuts some of them, not all
DTYPES = {torch.float16: 1, torch.bfloat16: 2}          # QD_OUT_F16, QD_OUT_BF16 (include/qd_hip.h)

# 1024 aligned (elements 256 .. 511 span +-1e31: alpha > 2^100, so the wave of that tile takes the IEEE division and the wave
# of the next tile the bucket-invariant one); 1000: a ragged last row; 515 four bytes off 16-byte alignment; 3; empty
BUCKETED_SIZES = [1024, 1000, 515, 3, 0]
# two full tiles of 1024; a full tile and a ragged tail; the scalar path; 3; empty
GLOBAL_SIZES = [2048, 1029, 515, 3, 0]
PHASES32 = [0, 0, 1, 0, 0]      # floats past a 16-byte boundary
PHASES16 = [0, 0, 2, 0, 0]      # 16-bit elements past a 16-byte boundary: the same 4 bytes
# (clamp, stochastic, seed in a device cell)
OPTION_SETS = [(0, 0, False), (1, 0, False), (0, 1, False), (0, 1, True), (1, 1, False), (1, 1, True)]
_INPUTS = {}


def inputs(kind):
    """(Carved, the flat fp32 input buffer) of a table: built once, never written."""
    if kind not in _INPUTS:
        sizes = BUCKETED_SIZES if kind == 'bucketed' else GLOBAL_SIZES
        gen = torch.Generator(device=DEV).manual_seed(23)
        xs = [0.1 * torch.randn(n, device=DEV, generator=gen) for n in sizes]
        if kind == 'bucketed':
            xs[0][256:512:2] = -1e31
            xs[0][257:512:2] = 1e31
        c = Carved(sizes, PHASES32, xs)
        _INPUTS[kind] = (c, c.flat())
    return _INPUTS[kind]


def views(carved, flat):
    """The tensors of a Carved / Carved16 layout in `flat` (the empty one has no address to check)."""
    return [flat[o:o + n] for o, n in zip(carved.offsets, carved.sizes)]


def table(xs, qs, plan):
    """-> (the descriptor table on the device, its tile count) for inputs xs and outputs qs under `plan(host, n)`."""
    n = len(xs)
    host = (_lib.QdTensorDesc * n)()
    for i, (x, q) in enumerate(zip(xs, qs)):
        host[i].x, host[i].q, host[i].n = x.data_ptr(), q.data_ptr(), x.numel()
    tiles = plan(host, n)
    assert tiles > 0
    return _lib.upload_struct(host, torch.device(DEV)), tiles


def plan_buckets(sizes):
    def plan(host, n):
        tiles = ctypes.c_int64(0)
        _lib.check(_lib.load().qd_multi_buckets_plan(host, (ctypes.c_int64 * n)(*sizes), n, ctypes.byref(tiles)))
        return int(tiles.value)
    return plan


class Launcher(object):
    """One table, one (bucket, s): launch(form, options[, dtype]) -> the flat output buffer, guard bands checked."""

    def __init__(self, kind, bucket, s):
        self.kind, self.bucket, self.s = kind, bucket, s
        self.carved, self.x_flat = inputs(kind)
        self.n = len(self.carved.sizes)
        self.levels = torch.full((self.n,), s, dtype=torch.int32, device=DEV)
        self.buckets = None if bucket is None else torch.full((self.n,), bucket, dtype=torch.int64, device=DEV)
        self.cell = torch.tensor([SEED0], dtype=torch.int64, device=DEV)
        self.carved16 = {dt: Carved16(self.carved.sizes, PHASES16, dt) for dt in DTYPES}

    def launch(self, form, options, dtype=None):
        clamp, stoch, on_device = options
        lib, st = _lib.load(), _lib.stream_ptr(torch.device(DEV))
        out = self.carved16[dtype] if dtype else self.carved
        flat = out.flat() if dtype else out.flat(filled=False)
        xs, qs = views(self.carved, self.x_flat), views(out, flat)
        if self.kind == 'global':
            plan = lambda host, n: int(lib.qd_multi_global_plan(host, n))                       # noqa: E731
        elif form == 'buckets':
            plan = plan_buckets([self.bucket] * self.n)
        else:
            plan = lambda host, n: int(lib.qd_multi_plan(host, n, self.bucket))                 # noqa: E731
        tab, tiles = table(xs, qs, plan)
        opts = (clamp, CLAMP if clamp else 0.0, stoch, 0 if on_device else SEED0, self.cell.data_ptr() if on_device else None)
        t, lv = tab.data_ptr(), self.levels.data_ptr()
        if self.kind == 'global':
            ab = torch.empty(self.n, 2, device=DEV)
            ws = torch.empty(max(4, 2 * tiles), device=DEV)
            tail = (ab.data_ptr(), ws.data_ptr(), ws.numel() * 4, st)
            if form == 'plain':
                code = lib.qd_multi_uniform_global_f32(t, self.n, tiles, self.s, *tail)
            elif form == 'opt':
                code = lib.qd_multi_uniform_global_opt_f32(t, self.n, tiles, self.s, *opts, *tail)
            elif form == 'levels':
                code = lib.qd_multi_uniform_global_levels_f32(t, lv, self.n, tiles, *opts, *tail)
            else:
                code = lib.qd_multi_uniform_global_out16_f32(t, lv, self.n, tiles, DTYPES[dtype], *opts, *tail)
        elif form == 'plain':
            code = lib.qd_multi_uniform_f32(t, self.n, tiles, self.bucket, self.s, st)
        elif form == 'opt':
            code = lib.qd_multi_uniform_opt_f32(t, self.n, tiles, self.bucket, self.s, *opts, st)
        elif form == 'levels':
            code = lib.qd_multi_uniform_levels_f32(t, lv, self.n, tiles, self.bucket, *opts, st)
        elif form == 'buckets':
            code = lib.qd_multi_uniform_buckets_f32(t, lv, self.buckets.data_ptr(), self.n, tiles, *opts, st)
        else:
            code = lib.qd_multi_uniform_out16_f32(t, lv, self.n, tiles, self.bucket, DTYPES[dtype], *opts, st)
        _lib.check(code)
        torch.cuda.synchronize()
        assert out.untouched_outside(flat), (form, options, dtype, 'the launch wrote outside its outputs')
        return flat


def same32(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def chain(run, forms32):
    """Every option set through the fp32 forms (the plain form joins where it can express the request) and both 16-bit types."""
    result = {}
    for options in OPTION_SETS:
        clamp, stoch, _cell = options
        forms = (['plain'] if not clamp and not stoch else []) + forms32
        flats = [run.launch(form, options) for form in forms]
        assert not torch.isnan(flats[-1]).any() and (flats[-1][run.carved.inside] != 777.0).all()
        for form, flat in zip(forms[:-1], flats[:-1]):
            assert same32(flat, flats[-1]), (run.kind, run.bucket, run.s, options, '%s differs from %s' % (form, forms[-1]))
        levels = result[options] = flats[forms.index('levels')]
        want = [v.cpu() for v in views(run.carved, levels)]
        for dtype in DTYPES:
            got = views(run.carved16[dtype], run.launch('out16', options, dtype))
            for i, (g, w) in enumerate(zip(got, want)):
                C.assert_same16(g, w.to(dtype), (run.kind, run.bucket, run.s, options, dtype, 'tensor %d' % i))
    for clamp in (0, 1):                           # the same seed by value and in the device cell: the same draws ...
        assert same32(result[clamp, 1, False], result[clamp, 1, True]), (run.kind, run.bucket, run.s, clamp, 'seed cell != seed by value')
        assert not same32(result[clamp, 1, False], result[clamp, 0, False]), 'the draws are not in use'     # ... and they count
    assert not same32(result[0, 0, False], result[1, 0, False]), 'the clamp is not in use'


@pytest.mark.parametrize('s', [4, 16, 17, 256])
@pytest.mark.parametrize('bucket', [64, 128, 256, 100])
def test_bucketed_forms_agree(bucket, s):
    chain(Launcher('bucketed', bucket, s), ['opt', 'levels', 'buckets'])


@pytest.mark.parametrize('s', [4, 16, 17, 256])
def test_unbucketed_forms_agree(s):
    chain(Launcher('global', None, s), ['opt', 'levels'])


def test_the_wide_bucket_is_outside_the_fast_division_range():
    """What the bucketed table relies on: alpha of elements 256 .. 511 exceeds 2^100, alpha of the rest does not."""
    c, flat = inputs('bucketed')
    x = views(c, flat)[0].cpu().numpy()
    assert np.float32(x[256:512].max()) - np.float32(x[256:512].min()) > 2.0 ** 100
    assert np.abs(np.concatenate([x[:256], x[512:]])).max() < 1.0
