"""GPU tests of what the native per-call binding (csrc/qd_torch_glue.cpp) keeps for itself ACROSS calls, where a launch
outlives the Python objects that own its memory: a hipGraph replay.  The rule held here:

    a captured launch writes only memory that the graph's pool or a live Python object owns.

The common path of uniformQuantization (uniform_common: the training loops' configuration) takes alpha / beta from a 1 MiB
slab per (device, stream) that only the slab table and the ScalingFunction objects carved from it keep alive; the loops drop
the ScalingFunction, and a slab that rolls over goes back to torch's caching allocator.  A launch captured while its pair
pointed into such a slab would write, on every replay, over whoever was handed the block next -- q stays right, so no value
comparison of a single call can see it.  Pinned here: where a captured common-path call writes its pair and who owns that
memory afterwards (sentinel-filled victims allocated behind the capture are never touched), that a ScalingFunction kept from
a captured call shows the pair of the latest replay on the common path as on the general path, the per-tensor step of the
reference loop captured on a warmed-up stream and replayed while eager calls move the slab on, the slab table's eviction
branch (more than 64 streams), and the steady state of the native objects over 20000 dropped calls.

In process, single-stream graphs only.  Nothing here reads freed memory or launches on a pointer the test does not own."""
import gc
import sys

import numpy as np
import pytest
import torch

import quantization
from oracle import oracle_c as oc
from oracle import oracle_np as onp
from quantization.quant_functions import ScalingFunction
from quantized_distillation_amd import _lib, ste

import abi_contract as A
import errlog

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SLAB_BYTES = 1 << 20                 # csrc/qd_torch_glue.cpp: kSlabFloats fp32
SENT = 0x5EA1AB1E                    # what a victim holds (int32): no alpha / beta pair of the data below has these bits
FILL_BUCKET, FILL_NB = 16, 30000     # 30000 buckets = 60000 floats of alpha / beta: four calls fill a slab, 1.9 MB per tensor
FILL_N = FILL_BUCKET * FILL_NB


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    _lib.load()
    oc.build()


def host(t):
    return t.detach().cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def took_common_path(sf):
    return '_ab_slab' in sf.__dict__ or ('type_scaling' not in sf.__dict__ and '_ab' in sf.__dict__)


def ab_range(sf, nb):
    """[lo, hi): the bytes the call that built `sf` writes alpha / beta to (read BEFORE the pair is, which copies it out)."""
    if sf.__dict__.get('_ab_slab') is not None:
        lo = sf._ab_slab.data_ptr() + 4 * sf._ab_off
    else:
        lo = sf._ab.data_ptr()
    return lo, lo + 8 * nb


def overlaps(a, b):
    return a[0] < b[1] and b[0] < a[1]


def fresh_slab(x):
    """Eager common-path calls on the current stream until one opens a new slab: returns that slab's [lo, hi).  The slab then
    holds this one call's pair (60000 floats of 262144) and nothing but the slab table keeps it alive."""
    for _ in range(6):
        sf = quantization.uniformQuantization(x, 16, bucket_size=FILL_BUCKET)[1]
        assert took_common_path(sf) and sf.__dict__.get('_ab_slab') is not None
        if sf._ab_off == 0:
            lo = sf._ab_slab.data_ptr()
            assert sf._ab_slab.numel() * 4 == SLAB_BYTES
            return lo, lo + SLAB_BYTES
    raise AssertionError('six calls of 60000 floats each did not open a new 1 MiB slab')


def owner_of(rng_, graph_pool):
    """Who owns the bytes [lo, hi) according to the caching allocator: 'allocated' (inside one block that is handed out),
    'pool' (inside a segment of the graph's private pool), 'free' (inside a cached block nobody holds), 'unmapped', or None
    when this torch build's snapshot does not report addresses, block states and pool ids."""
    lo, hi = rng_
    for seg in torch.cuda.memory_snapshot():
        if not all(k in seg for k in ('address', 'total_size', 'blocks', 'segment_pool_id')):
            return None
        if not (seg['address'] <= lo and hi <= seg['address'] + seg['total_size']):
            continue
        if tuple(seg['segment_pool_id']) == tuple(graph_pool):
            return 'pool'
        at = seg['address']
        for b in seg['blocks']:
            if 'size' not in b or 'state' not in b:
                return None
            at = b.get('address', at)
            if at <= lo and hi <= at + b['size']:
                return 'allocated' if b['state'] == 'active_allocated' else 'free'
            at += b['size']
        return 'free'                                        # straddles blocks: not one live allocation
    return 'unmapped'


# ---------------------------------------------------------------- 1. who owns what a captured common-path call writes
@pytest.mark.parametrize('rollover', ['inside the capture', 'behind the capture'])
def test_captured_common_path_writes_only_memory_the_graph_or_a_live_object_owns(rollover):
    """Warm up eagerly on a side stream, capture six common-path calls on it with every ScalingFunction dropped at once (as
    the loops do), let the eager slab roll over -- inside the capture: six calls of 60000 floats, the slab takes three more;
    behind it: six calls of 10000 floats fit, five eager calls of 60000 follow -- and allocate eight 1 MiB victims on the
    stream.  No captured call may write its pair into a victim, or into memory the allocator holds for whoever comes next;
    three replays on new data give the oracle's q and leave every victim as it was.

    Before uniform_common asked whether its stream is capturing (alpha / beta carved from the slab under capture as well)
    both cases failed at the first assertion, on the first captured call: the first victim had been handed the block of
    the eager slab."""
    S = torch.cuda.Stream()
    rng = np.random.RandomState(11)
    nb = FILL_NB if rollover == 'inside the capture' else 5000
    n = FILL_BUCKET * nb
    with torch.cuda.stream(S):
        filler = torch.randn(FILL_N, device=DEV)
        eager_slab = fresh_slab(filler)
        xs = [dev(rng.randn(n).astype(np.float32)) for _ in range(6)]
    S.synchronize()
    graph = torch.cuda.CUDAGraph()
    ranges, qs, common = [], [], []
    with torch.cuda.graph(graph, stream=S):
        for x in xs:
            q, sf = quantization.uniformQuantization(x, 16, bucket_size=FILL_BUCKET)
            common.append(took_common_path(sf))
            ranges.append(ab_range(sf, nb))
            del sf
            qs.append(q)
    assert all(common)
    with torch.cuda.stream(S):
        if rollover == 'behind the capture':
            for _ in range(5):
                quantization.uniformQuantization(filler, 16, bucket_size=FILL_BUCKET)
        victims = [torch.full((SLAB_BYTES // 4,), SENT, dtype=torch.int32, device=DEV) for _ in range(8)]
    S.synchronize()
    for i, r in enumerate(ranges):
        for j, v in enumerate(victims):
            vr = (v.data_ptr(), v.data_ptr() + SLAB_BYTES)
            assert not overlaps(r, vr), ('captured call %d writes alpha / beta to [%#x, %#x), inside victim %d [%#x, %#x)%s'
                                         % (i, r[0], r[1], j, vr[0], vr[1],
                                            ': the block of the eager slab' if overlaps(vr, eager_slab) else ''))
    owners = [owner_of(r, graph.pool()) for r in ranges]
    assert all(o in (None, 'allocated', 'pool') for o in owners), (owners, [tuple(map(hex, r)) for r in ranges])
    for rep in range(3):
        data = [(rng.randn(n) * (1 + rep) + i).astype(np.float32) for i in range(6)]
        with torch.cuda.stream(S):
            for x, d in zip(xs, data):
                x.copy_(torch.from_numpy(d))
            graph.replay()
        S.synchronize()
        for i, (q, d) in enumerate(zip(qs, data)):
            want = oc.uniform_quantize(d, 16, FILL_BUCKET, want_idx=False, want_lev=False)['q']
            assert np.array_equal(host(q), want), (rep, i)
        for j, v in enumerate(victims):
            assert bool((v == SENT).all()), 'replay %d wrote into victim %d' % (rep, j)


# ---------------------------------------------------------------- 2. a kept ScalingFunction from a captured call is live
@pytest.mark.parametrize('bucket', [256, None])
def test_kept_scaling_function_of_a_captured_call_follows_the_replays_on_both_paths(bucket):
    """One common-path call and one general-path call (max_element set) captured on the same static input, both objects
    kept: after every replay alpha / beta are the oracle's for THAT replay's data on both, the inverse uses them, and the
    lazy arg indices refuse (the static input was written since).  bucket None: one bucket of 100003 elements, the
    workspace and under capture the three-launch path."""
    n, me = 100003, 2.5
    rng = np.random.RandomState(12)
    a = (rng.randn(n) * 3 + 1).astype(np.float32)
    b = (rng.randn(n) * 0.25 - 2).astype(np.float32)
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        xs = dev(rng.randn(n).astype(np.float32))
        quantization.uniformQuantization(xs, 16, bucket_size=bucket)
        quantization.uniformQuantization(xs, 16, bucket_size=bucket, max_element=me)
    S.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=S):
        qc, sfc = quantization.uniformQuantization(xs, 16, bucket_size=bucket)
        qg, sfg = quantization.uniformQuantization(xs, 16, bucket_size=bucket, max_element=me)
    assert took_common_path(sfc) and not took_common_path(sfg)
    nb, row, padded = onp.bucket_geometry(n, bucket)
    for tag, d in (('A', a), ('B', b)):
        with torch.cuda.stream(S):
            xs.copy_(torch.from_numpy(d))
            graph.replay()
        S.synchronize()
        wants = (oc.uniform_quantize(d, 16, bucket, want_idx=False, want_lev=False),
                 oc.uniform_quantize(d, 16, bucket, max_element=me, want_idx=False, want_lev=False))
        for path, q, sf, want in (('common', qc, sfc, wants[0]), ('general', qg, sfg, wants[1])):
            assert np.array_equal(host(q), want['q']), (tag, path)
            assert np.array_equal(host(sf.alpha).reshape(-1), want['alpha'].reshape(-1)), (tag, path, 'alpha is not that of this replay')
            assert np.array_equal(host(sf.beta).reshape(-1), want['beta'].reshape(-1)), (tag, path, 'beta is not that of this replay')
    assert not np.array_equal(wants[0]['alpha'], wants[1]['alpha'])            # the clamp acts: the two pairs are two pairs
    u = rng.rand(padded).astype(np.float32)
    for path, sf, want in (('common', sfc, wants[0]), ('general', sfg, wants[1])):
        assert tuple(sf.expected_tensor_size) == ((n,) if bucket is None else (nb, row))
        y = sf.inv_scale_down(dev(u).view(sf.expected_tensor_size))
        wy = onp.inv_scale_down(u.reshape(nb, row), want['alpha'].reshape(nb, 1), want['beta'].reshape(nb, 1), 0.0, n, (n,))
        assert np.array_equal(host(y).reshape(-1), wy), (path, "inv_scale_down did not use replay B's pair")
        with pytest.raises(RuntimeError, match='modified in place'):
            sf.idx_min_rows


# ---------------------------------------------------------------- 3. the per-tensor step of the reference loop, captured
# one tensor per launcher path (tests/abi_contract.py: BUCKET_PATHS, ten buckets each with a ragged last one; SINGLE_SMALL /
# SINGLE_LARGE without buckets: the last three take the workspace and, under capture, the three-launch path)
STEP_SHAPES = [(256, 9 * 256 + 1), (100, 9 * 100 + 99), (33, 9 * 33 + 2), (449, 10 * 449),
               (None, 1000), (None, 16385), (None, 300001), (None, (1 << 20) + 3)]
assert {b for b, _ in STEP_SHAPES if b} <= {b for b, _, _ in A.BUCKET_PATHS}
assert {n for b, n in STEP_SHAPES if not b} <= {n for n, _ in A.SINGLE_SMALL + A.SINGLE_LARGE}
K7_LEVELS = 16


def loop_step(w, gr, bucket):
    """What the reference loop does with one parameter tensor in one step (ref: cnn_models/conv_forward_model.py:235-266),
    every epilogue on a copy so that the static inputs stay the inputs.  Returns every tensor a kernel wrote."""
    kb = bucket or 256                                                   # K7 needs buckets (ref: quant_functions.py:332-334)
    q = quantization.uniformQuantization(w, 16, bucket_size=bucket)[0]   # common path, the ScalingFunction dropped
    wc = ste.clamp_(w.clone(), 0.5)
    gt = ste.truncated_ste_(gr.clone(), w, 0.5)
    k7 = ste.ste_bucket_backward(w, gr, kb, K7_LEVELS)
    k7g = gr.clone()
    ste.ste_bucket_backward(w, k7g, kb, K7_LEVELS, out=k7g)
    qi = quantization.uniformQuantization(w.clone(), 16, bucket_size=bucket, modify_in_place=True)[0]
    qm, sfm = quantization.uniformQuantization(w, 16, bucket_size=bucket, subtract_mean=True)
    sf = ScalingFunction('linear', False, False, bucket)
    u = sf.scale_down(w)
    y = sf.inv_scale_down(u.clone())
    return dict(q=q, clamp=wc, truncated=gt, k7=k7, k7_in_place=k7g, q_in_place=qi, q_mean=qm, mean=sfm._mean_buf,
                u=u, alpha=sf.alpha, beta=sf.beta, y=y)


def check_k7(outs, x, g, bucket, tag):
    """K7 against the float64 oracle (the terms of errlog.check_ste, computed once for the outputs of one replay): every
    position but the two touched ones per bucket is g; out[jmax_b] = g_j + S_b and out[jmin_b] = g_j - S_b are sums of the
    bucket's terms and g_j, held by errlog.check_sum to 1e-6 of the sum of their magnitudes."""
    T = onp.ste_bucket_terms(x, g, K7_LEVELS, bucket)
    starts = np.arange(T['nb'], dtype=np.int64) * T['row']
    pmax, pmin = starts + T['jmax'], starts + T['jmin']
    live = pmax != pmin                                   # a constant bucket: +S and -S cancel, nothing is touched
    touched = np.zeros(x.size, bool)
    touched[pmax[live]] = True
    touched[pmin[live]] = True
    g64 = g.astype(np.float64)
    for which, out in outs:
        assert np.array_equal(out[~touched], g[~touched]), (tag, which, 'untouched positions must equal the incoming gradient')
        o64 = out.astype(np.float64)
        for name, pos, sign in (('max', pmax[live], 1.0), ('min', pmin[live], -1.0)):
            errlog.check_sum('K7 under hipGraph replay: g_j %s S_b at the arg-%s' % ('+' if sign > 0 else '-', name), o64[pos],
                             g64[pos] + sign * T['sb'][live], T['abs_terms'][live] + np.abs(g64[pos]), tag + (which,),
                             n_terms=T['row'])


def test_the_per_tensor_step_captured_on_a_warmed_up_stream_equals_the_eager_step():
    """harness/distill.py's pattern: warm up eagerly on a stream, capture on it, replay on new weights and gradients.  Five
    replays, eager common-path calls on the same stream in between (the step itself and two 30000-bucket calls per replay:
    the slab advances and rolls over at least twice): every tensor the replay wrote equals the eager step on the same data
    bit for bit, q and the pair equal the oracle, K7 is within 1e-6 sum|terms| of the float64 oracle."""
    rng = np.random.RandomState(13)
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        filler = torch.randn(FILL_N, device=DEV)
        ws = [dev(rng.randn(n).astype(np.float32)) for _, n in STEP_SHAPES]
        gs = [dev(rng.randn(n).astype(np.float32)) for _, n in STEP_SHAPES]
        for (bucket, _), w, gr in zip(STEP_SHAPES, ws, gs):
            loop_step(w, gr, bucket)                                    # warm-up: workspaces, the stream's slab
    S.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=S):
        captured = [loop_step(w, gr, bucket) for (bucket, _), w, gr in zip(STEP_SHAPES, ws, gs)]
    offsets = []                                                         # of the filler calls' pairs in their slabs
    for rep in range(5):
        wd = [(rng.randn(n) * (0.3 + 0.2 * rep) + 0.1 * rep).astype(np.float32) for _, n in STEP_SHAPES]
        gd = [rng.randn(n).astype(np.float32) for _, n in STEP_SHAPES]
        with torch.cuda.stream(S):
            for t, d in zip(ws + gs, wd + gd):
                t.copy_(torch.from_numpy(d))
            graph.replay()
            eager = [loop_step(w, gr, bucket) for (bucket, _), w, gr in zip(STEP_SHAPES, ws, gs)]
            for _ in range(2):
                offsets.append(quantization.uniformQuantization(filler, 16, bucket_size=FILL_BUCKET)[1]._ab_off)
        S.synchronize()
        for (bucket, n), cap, eag, x, g in zip(STEP_SHAPES, captured, eager, wd, gd):
            tag = (rep, bucket, n)
            for name in cap:
                assert A._same(host(cap[name]).reshape(-1), host(eag[name]).reshape(-1)), (tag, name, 'replay != eager call')
            want = oc.uniform_quantize(x, 16, bucket, want_idx=False, want_lev=False)
            assert np.array_equal(host(cap['q']), want['q']) and np.array_equal(host(cap['q_in_place']), want['q']), tag
            assert np.array_equal(host(cap['alpha']).reshape(-1), want['alpha'].reshape(-1)), tag
            assert np.array_equal(host(cap['beta']).reshape(-1), want['beta'].reshape(-1)), tag
            check_k7([(name, host(cap[name])) for name in ('k7', 'k7_in_place')], x, g, bucket or 256, tag)
    # offsets grow inside one slab: one that does not grow is the first of a new slab
    assert sum(1 for a, b in zip(offsets, offsets[1:]) if b <= a) >= 2, ('the eager calls between the replays did not roll the slab over', offsets)


# ---------------------------------------------------------------- 4. the slab table's eviction branch
def test_slab_table_eviction_keeps_every_pair():
    """The slab table holds 64 (device, stream) entries; a 65th stream forgets the oldest, whose slab lives on through what
    was carved from it.  One common-path call on each of at least 65 distinct raw streams (every priority's pool and the
    default stream), one ScalingFunction kept per stream, then back to the first streams for more: every q, alpha and beta
    equals the oracle, and the objects kept from before the eviction still read their own pair."""
    least, greatest = torch.cuda.Stream.priority_range()
    streams, seen = [], set()
    for s in [torch.cuda.default_stream()] + [torch.cuda.Stream(priority=p) for p in range(min(least, greatest), max(least, greatest) + 1)
                                              for _ in range(32)]:
        if s.cuda_stream not in seen:
            seen.add(s.cuda_stream)
            streams.append(s)
    assert len(streams) >= 65, ('torch hands out %d distinct raw streams over priorities %d .. %d' % (len(streams), least, greatest))
    n, bucket = 700, 256
    rng = np.random.RandomState(14)
    base = rng.randn(n).astype(np.float32)
    data = [(base * (1 + i) + i).astype(np.float32) for i in range(len(streams))]
    xs = [dev(d) for d in data]
    wants = [oc.uniform_quantize(d, 16, bucket, want_idx=False, want_lev=False) for d in data]
    torch.cuda.synchronize()

    def call(i):
        with torch.cuda.stream(streams[i]):
            q, sf = quantization.uniformQuantization(xs[i], 16, bucket_size=bucket)
        assert took_common_path(sf) and sf.__dict__.get('_ab_slab') is not None
        return q, sf, sf._ab_slab.data_ptr()

    first = [call(i) for i in range(len(streams))]
    again = [call(i) for i in range(len(streams))]                 # the first stream first: its entry was forgotten, or is now
    more = [call(0) for _ in range(3)]
    torch.cuda.synchronize()
    # a stream whose entry was forgotten starts a new slab, and the old one is still alive in `first`: the two differ
    reopened = sum(1 for a, b in zip(first, again) if a[2] != b[2])
    assert reopened >= 1, 'no stream came back to a new slab: 65 streams did not overflow a table of 64'
    for what, results, idx in (('again', again, range(len(streams))), ('more', more, [0] * 3), ('kept', first, range(len(streams)))):
        for (q, sf, _), i in zip(results, idx):
            assert np.array_equal(host(q), wants[i]['q']), (what, i)
            assert np.array_equal(host(sf.alpha).reshape(-1), wants[i]['alpha'].reshape(-1)), (what, i)
            assert np.array_equal(host(sf.beta).reshape(-1), wants[i]['beta'].reshape(-1)), (what, i)


# ---------------------------------------------------------------- 5. steady state of the native objects
def test_dropped_calls_leave_no_native_object_behind():
    """20000 common-path calls with the results dropped: device memory within one slab of where it was, no reference kept
    on the class, the input or the bucket_size object (a fresh int: not one of CPython's cached small ones), no
    ScalingFunction alive."""
    x = torch.randn(5000, device=DEV)
    bucket = int('1031')
    assert took_common_path(quantization.uniformQuantization(x, 16, bucket_size=bucket)[1])
    gc.collect()
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    refs = (sys.getrefcount(ScalingFunction), sys.getrefcount(x), sys.getrefcount(bucket))
    for _ in range(20000):
        quantization.uniformQuantization(x, 16, bucket_size=bucket)
    gc.collect()
    torch.cuda.synchronize()
    assert abs(torch.cuda.memory_allocated() - mem) <= SLAB_BYTES, (mem, torch.cuda.memory_allocated())
    assert (sys.getrefcount(ScalingFunction), sys.getrefcount(x), sys.getrefcount(bucket)) == refs
    alive = [o for o in gc.get_objects() if type(o) is ScalingFunction]
    assert len(alive) == 0, ('%d ScalingFunction instances alive' % len(alive), [sorted(o.__dict__) for o in alive[:3]])
