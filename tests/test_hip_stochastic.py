"""Stochastic rounding on the device (libqd_hip.so) -- tests/stochastic_cases.py at the C ABI, where qd_uniform_f32 takes the
seed directly, and through quantization.uniformQuantization: every element on its own `rnd <= p` threshold on every kernel
path at both single-bucket modes, `rnd == 0.0` at `p == 0` with the level index, independence of the decisions, the seed
sequence of the Python API and what a stochastic call does under hipGraph capture.  Every case is also run on libqd_host.so
and the two libraries' outputs compared bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import quantization
import stochastic_cases as S
from quantized_distillation_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def libs():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return S.Library('hip'), S.Library('host')


@pytest.fixture(params=[1, 0], ids=['fused', 'three-launch'])
def fused_mode(request, libs):
    """Both values of qd_set_single_fused_mode (it decides the path of one bucket of 16 Ki .. 1 Mi elements)."""
    before = libs[0].set_fused_mode(request.param)
    yield request.param
    libs[0].set_fused_mode(before)


def _agree(dev_outs, host_outs):
    assert len(dev_outs) == len(host_outs)
    for i, (d, h) in enumerate(zip(dev_outs, host_outs)):
        assert S.same_outputs(d, h), ('device and host library differ', i)


@pytest.mark.parametrize('s', [5, 17])
@pytest.mark.parametrize('n,bucket', S.SHAPES, ids=S.SHAPE_IDS)
def test_every_element_on_its_own_threshold(libs, fused_mode, n, bucket, s):
    kinds = 'ABC' if s == 5 else 'AB'
    _agree(S.check_threshold(libs[0], n, bucket, s, kinds=kinds), S.check_threshold(libs[1], n, bucket, s, kinds=kinds))


@pytest.mark.parametrize('offset', [1, 2, 3])
@pytest.mark.parametrize('n,bucket', S.OFFSET_SHAPES)
def test_threshold_cases_on_views_at_4_byte_offsets(libs, n, bucket, offset):
    _agree(S.check_threshold(libs[0], n, bucket, 5, offset=offset), S.check_threshold(libs[1], n, bucket, 5, offset=offset))


@pytest.mark.parametrize('want_lev', [False, True], ids=['q', 'q+level_idx'])
@pytest.mark.parametrize('s', [5, 16, 256])
@pytest.mark.parametrize('n,bucket', S.EDGE_GEOMETRIES, ids=S.EDGE_IDS)
def test_zero_draw_on_an_exact_level_moves_one_level_up_even_past_the_top(libs, fused_mode, n, bucket, s, want_lev):
    _agree(S.check_edges(libs[0], n, bucket, s, want_lev), S.check_edges(libs[1], n, bucket, s, want_lev))


def test_device_decisions_are_independent_across_elements_words_rows_and_seeds(libs, fused_mode):
    assert S.check_streams(libs[0]) == S.oracle_stream_statistics()


def test_successive_api_calls_on_device_tensors_follow_the_seed_schedule():
    S.check_api_sequence(DEV)


def test_stochastic_call_under_hipgraph_capture():
    """The seed is a by-value launch argument.  At the C ABI a captured qd_uniform_f32 therefore replays the draws of the seed
    it was recorded with, on whatever the input buffer holds (include/qd_hip.h says so); through the Python API, where the
    seed comes from a per-call counter the replay would never advance, the call raises during capture and records nothing --
    the capture goes on and the deterministic call next to it replays as usual.  One stream, no parallel branches."""
    n, bucket, s, seed = 4096, 256, 16, 0x1CEB00DA5EED
    rng = np.random.RandomState(3)
    x0, x1 = rng.randn(n).astype(np.float32), (rng.randn(n) * 2 - 1).astype(np.float32)
    lib = _lib.load()
    xs = torch.from_numpy(x0).to(DEV)
    qs, ab = torch.empty(n, device=DEV), torch.empty(2, n // bucket, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                      # warm-up outside the capture (lazy allocations)
        quantization.uniformQuantization(xs, s, bucket_size=bucket)
        quantization.uniformQuantization(xs, s, bucket_size=bucket, stochastic_rounding=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    import quantization.quant_functions as qf
    calls_before = qf._STOCHASTIC_CALLS[0]
    ws = _lib.workspace(torch.device(DEV))                             # (unused by a bucketed call; allocated before the capture)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert torch.cuda.is_current_stream_capturing()
        qd, _ = quantization.uniformQuantization(xs, s, bucket_size=bucket)
        with pytest.raises(RuntimeError, match='stream capture'):
            quantization.uniformQuantization(xs, s, bucket_size=bucket, stochastic_rounding=True)
        assert lib.qd_uniform_f32(xs.data_ptr(), qs.data_ptr(), n, bucket, s, ab[0].data_ptr(), ab[1].data_ptr(), None, None, 0,
                                  0.0, 1, ctypes.c_uint64(seed), ws.data_ptr(), ws.numel(), _lib.stream_ptr()) == 0
    assert qf._STOCHASTIC_CALLS[0] == calls_before, 'a refused call must not consume a seed'
    for xv in (x1, x0, x0):
        xs.copy_(torch.from_numpy(xv).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(qd.cpu().numpy(), S.onp.uniform_quantize(xv, s, bucket)['q'])
        assert np.array_equal(qs.cpu().numpy(), S.oracle(xv, s, seed, bucket)['q']), 'a replay draws what its recorded seed draws'
    # outside a capture the same API call works, and moves on to the next seed
    want_seed = qf.next_stochastic_seed(peek=True)
    q, _ = quantization.uniformQuantization(xs, s, bucket_size=bucket, stochastic_rounding=True)
    assert np.array_equal(q.cpu().numpy(), S.oracle(x0, s, want_seed, bucket)['q'])
