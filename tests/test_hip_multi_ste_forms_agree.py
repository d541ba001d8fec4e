"""The forms of the one-launch STE backward against EACH OTHER, through the C entry points themselves.

The other suites hold every form to the per-tensor call; MultiTensorSTE routes an all-equal `s` to the scalar entry point, so
none of them runs two forms on the same run-time branches of the tile body they share (multi_ste_tile, csrc/qd_ste.hip).  Here
one small table goes through every entry point that can express the same request, for one (bucket, s, tie_mode):

    plain(b, s) == levels(b, [s] * n) == buckets([b] * n, [s] * n) == qd_ste_bucket_backward_f32 on each tensor alone
    in16(fp16), in16(bf16)            == levels on the widened gradients, g once 8-byte aligned and once 2 bytes off

Outputs are compared as bit patterns, guard bands of 777 included, after every launch.  A few thousand elements in all.  (The
test does not depend on the kernels sharing text: it passed on the library with four written-out kernels as well.)"""
import ctypes

import numpy as np
import pytest
import torch

from quantized_distillation_amd import _lib
from test_hip_multi_stochastic import Carved
from test_hip_out16 import Carved16

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GRAD_KINDS = {torch.float16: 1, torch.bfloat16: 2}      # QD_GRAD_F16, QD_GRAD_BF16 (include/qd_hip.h)
NAN16 = {torch.float16: 0x7E00, torch.bfloat16: 0x7FC0}
TIES = {'reference': 0, 'true_arg': 1}                  # QD_STE_TIE_REFERENCE, QD_STE_TIE_TRUE_ARG
PHASES32 = [0, 0, 1, 0, 0]      # floats past a 16-byte boundary: x, the fp32 g and out of a tensor share it, so that the fp32 g is
#                                 16-byte aligned wherever x and out are and the fp32 and the 16-bit plan make the same cut
G16_PHASES = {'8-byte aligned': 4, '2 bytes off': 1}    # 16-bit elements past a 16-byte boundary, every tensor
_INPUTS = {}


def sizes_for(b):
    """3 b aligned: register tiles, the last tile partly empty; 2 b + b / 2 + 3: register tiles plus the ragged bucket on the wave
    path; b + 5 with x four bytes off 16-byte alignment: every bucket on the wave path; shorter than a bucket; empty."""
    return [3 * b, 2 * b + b // 2 + 3, b + 5, 3, 0]


def wide_bucket(b):
    """Bucket 1 of the first tensor: it alternates +-1e31, so alpha_q > 2^100 and its wave takes the IEEE division, its neighbours
    the bucket-invariant one."""
    return slice(b, 2 * b)


class Inputs(object):
    """The table of one bucket size, built once and never written: x, an fp32 gradient, and per 16-bit type a gradient, its
    widened fp32 copy and its carved 16-bit copies at both alignments."""

    def __init__(self, b):
        self.sizes = sizes_for(b)
        gen = torch.Generator(device=DEV).manual_seed(31 + b)
        xs = [0.1 * torch.randn(n, device=DEV, generator=gen) for n in self.sizes]
        xs[0][b:2 * b:2] = -1e31
        xs[0][b + 1:2 * b:2] = 1e31
        gs = [torch.randn(n, device=DEV, generator=gen) for n in self.sizes]
        self.c = Carved(self.sizes, PHASES32, xs)
        self.x = self.c.flat()
        self.g32 = Carved(self.sizes, PHASES32, gs).flat()
        self.wide, self.g16 = {}, {}
        for dt in GRAD_KINDS:
            g16 = [g.to(dt) for g in gs]
            self.wide[dt] = Carved(self.sizes, PHASES32, [g.float() for g in g16]).flat()      # widening is exact
            for name, phase in G16_PHASES.items():
                c16 = Carved16(self.sizes, [phase] * len(self.sizes), dt)
                flat = c16.flat()
                flat.view(torch.int16)[~c16.inside] = NAN16[dt]             # a guard band that is read poisons a sum
                for v, g in zip(views16(c16, flat), g16):
                    v.copy_(g)
                    assert v.numel() == 0 or v.data_ptr() % 16 == 2 * phase
                self.g16[dt, name] = (c16, flat)
        self.frozen = [t.clone() for t in self.all_inputs()]

    def all_inputs(self):
        return [self.x, self.g32] + list(self.wide.values()) + [flat for _c, flat in self.g16.values()]

    def unchanged(self):
        return all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(self.all_inputs(), self.frozen))


def inputs(b):
    if b not in _INPUTS:
        _INPUTS[b] = Inputs(b)
    return _INPUTS[b]


class Launcher(object):
    """One table, one (bucket, s, tie): launch(form, gradient views[, dtype]) -> the flat fp32 output buffer, guard bands checked."""

    def __init__(self, bucket, s, tie):
        self.inp, self.bucket, self.s, self.tie = inputs(bucket), bucket, s, TIES[tie]
        self.n = len(self.inp.sizes)
        self.levels = torch.full((self.n,), s, dtype=torch.int32, device=DEV)
        self.buckets = torch.full((self.n,), bucket, dtype=torch.int64, device=DEV)
        self.tiles = set()

    def table(self, gs, outs, form):
        lib = _lib.load()
        host = (_lib.QdSteDesc * self.n)()
        for i, (x, g, o) in enumerate(zip(self.inp.c.views(self.inp.x), gs, outs)):
            if x.numel():
                host[i].x, host[i].g, host[i].out = x.data_ptr(), g.data_ptr(), o.data_ptr()
            host[i].n = x.numel()
        tiles = ctypes.c_int64(-1)
        if form == 'buckets':
            _lib.check(lib.qd_multi_ste_buckets_plan(host, (ctypes.c_int64 * self.n)(*([self.bucket] * self.n)), self.n, ctypes.byref(tiles)))
        elif form == 'in16':
            _lib.check(lib.qd_multi_ste_in16_plan(host, self.n, self.bucket, ctypes.byref(tiles)))
        else:
            _lib.check(lib.qd_multi_ste_plan(host, self.n, self.bucket, ctypes.byref(tiles)))
        assert tiles.value > 0
        self.tiles.add(int(tiles.value))
        return _lib.upload_struct(host, torch.device(DEV)), int(tiles.value)

    def launch(self, form, gs, dtype=None):
        lib, st = _lib.load(), _lib.stream_ptr(torch.device(DEV))
        c = self.inp.c
        flat = c.flat(filled=False)
        outs = c.views(flat)
        if form == 'per tensor':
            for x, g, o in zip(c.views(self.inp.x), gs, outs):
                if x.numel():
                    _lib.check(lib.qd_ste_bucket_backward_f32(x.data_ptr(), g.data_ptr(), o.data_ptr(), x.numel(), self.bucket, self.s,
                                                              self.tie, st))
        else:
            tab, tiles = self.table(gs, outs, form)
            t, lv = tab.data_ptr(), self.levels.data_ptr()
            if form == 'plain':
                code = lib.qd_multi_ste_backward_f32(t, self.n, tiles, self.bucket, self.s, self.tie, st)
            elif form == 'levels':
                code = lib.qd_multi_ste_backward_levels_f32(t, lv, self.n, tiles, self.bucket, self.tie, st)
            elif form == 'buckets':
                code = lib.qd_multi_ste_backward_buckets_f32(t, lv, self.buckets.data_ptr(), self.n, tiles, self.tie, st)
            else:
                code = lib.qd_multi_ste_backward_in16_f32(t, lv, self.n, tiles, self.bucket, GRAD_KINDS[dtype], self.tie, st)
            _lib.check(code)
        torch.cuda.synchronize()
        assert c.untouched_outside(flat), (form, dtype, 'the launch wrote outside its outputs')
        assert not (flat[c.inside] == 777.0).any(), (form, dtype, 'elements nothing wrote')
        return flat


def views16(c16, flat):
    """The tensors of a Carved16 layout in `flat` (the empty one has no address to check)."""
    return [flat[o:o + n] for o, n in zip(c16.offsets, c16.sizes)]


def same32(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('tie', sorted(TIES))
@pytest.mark.parametrize('s', [4, 16, 17, 256])
@pytest.mark.parametrize('bucket', [64, 128, 256, 512, 1024, 100])
def test_forms_agree(bucket, s, tie):
    run = Launcher(bucket, s, tie)
    inp, c, tag = run.inp, run.inp.c, (bucket, s, tie)
    g32 = c.views(inp.g32)
    flats = {form: run.launch(form, g32) for form in ('plain', 'levels', 'buckets', 'per tensor')}
    for form in ('plain', 'buckets', 'per tensor'):
        assert same32(flats[form], flats['levels']), tag + ('%s differs from levels' % form,)
    assert not torch.isnan(flats['levels'][c.inside]).any()
    assert not same32(flats['levels'], inp.g32), tag + ('the correction at jmax / jmin is not in use',)
    for dtype in GRAD_KINDS:
        want = run.launch('levels', c.views(inp.wide[dtype]))
        assert not same32(want, inp.wide[dtype]), tag + (dtype, 'the correction at jmax / jmin is not in use')
        for name in G16_PHASES:
            c16, flat16 = inp.g16[dtype, name]
            got = run.launch('in16', views16(c16, flat16), dtype)
            assert same32(got, want), tag + (dtype, name, 'in16 differs from levels on the widened gradients')
    assert len(run.tiles) == 1, tag + ('the plans count differently', run.tiles)
    assert inp.unchanged(), tag + ('an input was written',)


@pytest.mark.parametrize('bucket', [64, 128, 256, 512, 1024, 100])
def test_the_wide_bucket_is_outside_the_fast_division_range(bucket):
    """What the table relies on: alpha of the first tensor's bucket 1 exceeds 2^100, alpha of every other bucket does not."""
    inp = inputs(bucket)
    xs = [v.cpu().numpy() for v in inp.c.views(inp.x)]
    w = wide_bucket(bucket)
    assert np.float32(xs[0][w].max()) - np.float32(xs[0][w].min()) > 2.0 ** 100
    rest = np.concatenate([xs[0][:w.start], xs[0][w.stop:]] + xs[1:])
    assert np.abs(rest).max() < 1.0
    assert [x.size for x in xs] == sizes_for(bucket) and inp.c.views(inp.x)[2].data_ptr() % 16 == 4
    assert all(v.data_ptr() % 16 == 0 for i, v in enumerate(inp.c.views(inp.x)) if i != 2 and v.numel())
