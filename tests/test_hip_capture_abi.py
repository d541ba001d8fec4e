"""Every C-ABI entry point that launches something, recorded ONCE into a hipGraph and replayed on other data
(tests/abi_contract.py: run_case_captured, CAPTURE).  The launchers allocate nothing, never synchronise and take no host
decision from tensor contents, so every call can be recorded; what only a replay shows is a value derived from the data and
frozen into the graph as a launch argument, a workspace slot that only the recording-time call initialises, a launch plan
that differs under capture (the one-launch single-bucket kernel is refused there: three launches instead) and host memory
that is read again at replay time.  Every eager test passes in all four situations.

The cases are those of tests/test_hip_abi_contract.py -- one per launcher path of every per-call entry point, guarded buffers,
sentinel-filled outputs, the workspace at exactly its documented size -- recorded on their data (variant 0) and replayed on
variants 1 (ordinary data of another scale) and 2 (NaN, +inf, constant, 2^101- and 2^-61-scaled buckets, all-one-symbol
indices), then on 0 and 1 again, the workspace refilled with zero bytes, 0xFF bytes and the residue of larger calls in turn.
Each replay is held to the oracle through the comparison the case always had and, for variants 1 and 2, to an eager call
bit for bit.  One stream, linear graphs only; every case is warmed up eagerly first (callers must: INTEGRATION.md)."""
import numpy as np
import pytest
import torch

import abi_contract as A
import errlog
import huffman_cases as H
from quantized_distillation_amd import _lib, ste
from quantized_distillation_amd import compressed as C
from quantized_distillation_amd.multi_tensor import MultiTensorSTE

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CAPTURED_GROUP_IDS = [gid for gid in A.DEVICE_GROUP_IDS if '-mode' not in gid]      # (the give-up hooks add nothing under capture)


@pytest.mark.parametrize('gid', CAPTURED_GROUP_IDS)
def test_device_group_captured(gid):
    with torch.cuda.device(DEV):
        assert A.run_group_captured(A.GROUPS[gid], _lib.load(), DEV)


@pytest.mark.parametrize('in_place', [False, True])
@pytest.mark.parametrize('bucket', [256, 100, None])
@pytest.mark.parametrize('nt', [1, 7, 65])
def test_multi_tensor_uniform_captured(nt, bucket, in_place):
    """K9 (qd_multi_uniform_f32, qd_multi_uniform_global_f32): one launch recorded, replayed on the other variants of the
    list; without buckets the global workspace changes its fill between the replays."""
    with torch.cuda.device(DEV):
        A.run_multi_uniform_captured(nt, bucket, in_place, _lib.load(), DEV)


@pytest.mark.parametrize('bucket,k', [(256, 16), (64, 64), (1024, 2)])
@pytest.mark.parametrize('nt', [1, 7, 65])
def test_multi_tensor_diff_quant_captured(nt, bucket, k):
    """K5m (qd_multi_nearest_f32) and K6m (qd_multi_point_grad_f32), one recorded launch each; K6m's scratch changes its fill
    between the replays."""
    with torch.cuda.device(DEV):
        A.run_multi_dq_captured(nt, bucket, k, _lib.load(), DEV)


# ---------------------------------------------------------------- the two multi-tensor STE launches no other test captures
STE_SIZES, STE_BUCKET = [257, 1031, 70001, 3, 2560], 256


@pytest.mark.parametrize('form', ['levels', 'in16'])
def test_multi_ste_with_levels_and_16_bit_gradients_captured(form):
    """qd_multi_ste_backward_levels_f32 (a level count per tensor) and qd_multi_ste_backward_in16_f32 (fp16 gradients): recorded
    on variant 0, replayed on weights and gradients of variants 1, 2, 0, 1 copied into the same tensors.  Every tensor equals
    the per-call K7 on the same data bit for bit (the class's contract) and, on the ordinary data, the float64 oracle."""
    levels = [4, 16, 256, 8, 16] if form == 'levels' else 16
    s_of = (lambda i: levels[i]) if form == 'levels' else (lambda i: 16)
    gdt = torch.float32 if form == 'levels' else torch.float16
    xs = {v: [A.data(n, STE_BUCKET, 1100 + i, variant=v, finite=True) for i, n in enumerate(STE_SIZES)] for v in A.VARIANTS}
    gs = {v: [A.vary(np.random.RandomState(1200 + i).randn(n).astype(np.float32), STE_BUCKET, 1200 + i + 10 * v, min(v, 1))
              for i, n in enumerate(STE_SIZES)] for v in A.VARIANTS}                # (finite, and inside the range of fp16)
    side = A.side_stream(DEV)
    with torch.cuda.device(DEV), torch.cuda.stream(side):
        ws = [torch.from_numpy(x).to(DEV) for x in xs[0]]
        gr = [torch.from_numpy(g).to(DEV).to(gdt) for g in gs[0]]
        outs = [torch.empty(n, dtype=torch.float32, device=DEV) for n in STE_SIZES]
        mt = MultiTensorSTE(ws, gr, levels, STE_BUCKET, outs=outs)
        mt.backward(check_pointers=False)                                          # warm-up
        graph = torch.cuda.CUDAGraph()
        with A.recording(graph, DEV):
            mt.backward(check_pointers=False)
        assert mt.entry_point == 'qd_multi_ste_backward_%s_f32' % form

        def check(what, v):
            torch.cuda.synchronize()
            for t, (w, g, o) in enumerate(zip(ws, gr, outs)):
                eager = ste.ste_bucket_backward(w, g.float(), STE_BUCKET, s_of(t))
                assert torch.equal(o.view(torch.int32), eager.view(torch.int32)), (form, what, 'variant %d' % v, 'tensor %d' % t)
                if v < 2:
                    errlog.check_ste('K7m (%s) under hipGraph replay' % form, o.cpu().numpy(), xs[v][t], g.float().cpu().numpy(), s_of(t),
                                     STE_BUCKET, (form, what, t))

        for i, v in enumerate(A.REPLAY_ORDER):
            for w, g, x, gv in zip(ws, gr, xs[v], gs[v]):
                w.copy_(torch.from_numpy(x))
                g.copy_(torch.from_numpy(gv).to(gdt))
            for o in outs:
                o.fill_(float('nan'))
            graph.replay()
            check('replay %d' % i, v)
        graph.replay()                                                            # back to back: outs are no inputs
        graph.replay()
        check('two replays back to back', A.REPLAY_ORDER[-1])
        del graph


# ---------------------------------------------------------------- the Huffman codec
HUF_PAIRS = [('lut_edge_10', 'lut_edge_11'), ('fixed8', 'fixed6')]
WORD_FILL = int(np.uint32(H.WORD_SENTINEL).view(np.int32))


@pytest.mark.parametrize('pair', HUF_PAIRS, ids=['-'.join(p) for p in HUF_PAIRS])
def test_huffman_codec_captured(pair):
    """qd_huffman_encode with a capacity of one word (the sizing pass: chunk_words only, no chunk fits), qd_huffman_encode
    with the full fixed capacity and qd_huffman_decode_f32 (nwords = that capacity), three recorded calls in graphs of their
    own: two cases of tests/huffman_cases.py with equal geometry (tensor sizes, chunks) and other symbols, code lengths and
    level counts are the variants -- symbols, table and code book are rewritten in the same device buffers.  Well-formed
    streams; the reference is libqd_host.so's run of the case, the eager device run gives the same bits."""
    lib, host = _lib.load(), _lib.host()
    cases = [H.CASES[p] for p in pair]
    a = cases[0]
    assert all([(t.n, t.bucket, t.nonuniform) for t in c.tensors] == [(t.n, t.bucket, t.nonuniform) for t in a.tensors] for c in cases)
    ns, nt = [t.n for t in a.tensors], len(a.tensors)
    nchunks = sum(H.nchunks_of(t) for t in a.tensors)
    syms = [H.symbols(c) for c in cases]
    for c, s in zip(cases, syms):
        H.check_conditions(c, s)
    ref = [H.run_case(c, host, 'cpu') for c in cases]
    capacity = max(len(r.words) for r in ref) + nchunks + 1
    sym_off, sym_total = H._offsets(ns, 4)
    y_off, y_total = H._offsets(ns, 1)
    y_keep = np.ones(y_total, bool)
    for o, n in zip(y_off, ns):
        y_keep[o:o + n] = False

    def sym_image(s):
        img = np.full(sym_total, H.SYM_SENTINEL, np.uint8)
        for v, o in zip(s, sym_off):
            img[o:o + len(v)] = v
        return img

    side = A.side_stream(DEV)
    with torch.cuda.device(DEV), torch.cuda.stream(side):
        eager = [H.run_case(c, lib, DEV) for c in cases]                           # also the warm-up of both entry points
        sym_flat = torch.from_numpy(sym_image(syms[0])).to(DEV)
        y_flat = torch.full((y_total,), H.SENTINEL, dtype=torch.float32, device=DEV)
        chunk_small = torch.full((nchunks + 1,), WORD_FILL, dtype=torch.int32, device=DEV)
        words_small = torch.full((1 + 16,), WORD_FILL, dtype=torch.int32, device=DEV)
        chunk_words = torch.full((nchunks + 1,), WORD_FILL, dtype=torch.int32, device=DEV)
        words = torch.full((capacity + 16,), WORD_FILL, dtype=torch.int32, device=DEV)
        alpha, beta = (torch.from_numpy(v).to(DEV) for v in H.alpha_beta(a))

        def tables(c):
            table = (_lib.QdHufTensor * nt)()
            for j, (t, fc, fb, fp) in enumerate(zip(c.tensors, H.first_chunks(c), H.first_buckets(c), H.first_points(c))):
                e = table[j]
                e.sym, e.y = sym_flat.data_ptr() + sym_off[j], y_flat.data_ptr() + 4 * y_off[j]
                e.n, e.first_chunk, e.first_bucket, e.first_point = t.n, fc, fb, fp
                e.bucket, e.levels, e.nonuniform = t.bucket, t.levels, t.nonuniform
            return _lib.upload_struct(table, DEV), _lib.upload_struct(C.canonical_code(c.lens, c.single), DEV)

        table_d, code_d = tables(a)
        st = _lib.stream_ptr(DEV)
        sizing, encode, decode = (torch.cuda.CUDAGraph() for _ in range(3))
        with A.recording(sizing, DEV):
            rc0 = lib.qd_huffman_encode(table_d.data_ptr(), nt, nchunks, code_d.data_ptr(), chunk_small.data_ptr(), words_small.data_ptr(), 1, st)
        with A.recording(encode, DEV):
            rc1 = lib.qd_huffman_encode(table_d.data_ptr(), nt, nchunks, code_d.data_ptr(), chunk_words.data_ptr(), words.data_ptr(), capacity, st)
        with A.recording(decode, DEV):
            rc2 = lib.qd_huffman_decode_f32(words.data_ptr(), capacity, chunk_words.data_ptr(), table_d.data_ptr(), nt, nchunks, code_d.data_ptr(),
                                            alpha.data_ptr(), beta.data_ptr(), None, st)
        assert (rc0, rc1, rc2) == (0, 0, 0)
        for i, v in enumerate((1, 0, 1, None)):
            if v is not None:
                c, r, which = cases[v], ref[v], v
                sym_flat.copy_(torch.from_numpy(sym_image(syms[v])))
                t2, c2 = tables(c)
                table_d.copy_(t2)
                code_d.copy_(c2)
                for buf in (chunk_small, words_small, chunk_words, words):
                    buf.fill_(WORD_FILL)
                y_flat.fill_(H.SENTINEL)
                sizing.replay()
                encode.replay()
                decode.replay()
            else:                                                                  # twice more back to back, on what is in place
                for _ in range(2):
                    sizing.replay()
                    encode.replay()
                    decode.replay()
            torch.cuda.synchronize()
            tag = (pair, 'replay %d on %s' % (i, c.id))
            want_cw = H.expected_chunk_words(c, syms[which])
            nwords = len(r.words)
            assert np.array_equal(r.chunk_words, want_cw) and np.array_equal(eager[which].chunk_words, want_cw), tag
            assert np.array_equal(chunk_small.cpu().numpy().view(np.uint32), want_cw), (tag, 'chunk_words of the sizing pass')
            assert (words_small.cpu().numpy() == WORD_FILL).all(), (tag, 'the sizing pass wrote a chunk that does not fit its one word')
            assert np.array_equal(chunk_words.cpu().numpy().view(np.uint32), want_cw), (tag, 'chunk_words')
            w = words.cpu().numpy().view(np.uint32)
            assert np.array_equal(w[:nwords], r.words) and np.array_equal(w[:nwords], eager[which].words), (tag, 'the bitstream differs')
            assert (w[nwords:] == H.WORD_SENTINEL).all(), (tag, 'written behind the last word of the bitstream')
            y = y_flat.cpu().numpy()
            assert (y[y_keep] == np.float32(H.SENTINEL)).all(), (tag, 'written between the tensors')
            got = [y[o:o + n].copy() for o, n in zip(y_off, ns)]
            assert H.same_bits(got, H.expected(c, syms[which])) and H.same_bits(got, r.decoded) and H.same_bits(got, eager[which].decoded), tag
            assert np.array_equal(sym_flat.cpu().numpy(), sym_image(syms[which])), (tag, 'the symbols were written over')
        del sizing, encode, decode


# ---------------------------------------------------------------- the self test of the bucket-invariant division
def test_selftest_div_invariant_captured():
    """qd_selftest_div_invariant takes everything by value and generates its pairs on the device: a replay into a
    sentinel-filled result gives the counters of the eager call, no mismatch among them."""
    lib = _lib.load()
    with torch.cuda.device(DEV), torch.cuda.stream(A.side_stream(DEV)):
        st = _lib.stream_ptr(DEV)
        eager = torch.full((4,), -1, dtype=torch.int64, device=DEV)
        res = torch.full((4,), -1, dtype=torch.int64, device=DEV)
        _lib.check(lib.qd_selftest_div_invariant(0xC0FFEE, 1 << 16, 0, eager.data_ptr(), st))
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with A.recording(graph, DEV):
            rc = lib.qd_selftest_div_invariant(0xC0FFEE, 1 << 16, 0, res.data_ptr(), st)
        assert rc == 0
        for _ in range(2):
            res.fill_(-1)
            graph.replay()
            graph.replay()
            torch.cuda.synchronize()
            got = res.cpu().numpy()
            assert np.array_equal(got, eager.cpu().numpy()) and got[0] > 0 and got[1] == 0, got
        del graph


# ---------------------------------------------------------------- the control, and refused calls
def _first_case(gid):
    return [next(iter(A.cases_of(A.GROUPS[gid], _lib.load(), v))) for v in A.VARIANTS]


def _max_element_from_the_data(c, placed):
    """What no launcher does and a wrapper could: a value read from the data on the host, passed on by value -- K1's
    max_element = max |x|, a clamp that changes nothing on the data it was read from."""
    p = placed['x']
    biggest = p.buf[p.off:p.off + p.nbytes].view(torch.float32).abs().max().item()
    args = list(c.args)
    assert c.entry == 'qd_uniform_f32' and args[9] == 0
    args[9], args[10] = 1, float(biggest)
    return args


def test_the_protocol_sees_a_value_baked_into_the_graph():
    """The control that must fail: max_element computed from variant 0 on the host is frozen into the recorded launch; the
    replay on variant 1 (three times the scale) clamps where the eager call, which reads its own data, does not."""
    cv = _first_case('K1-b256-nf10')
    with torch.cuda.device(DEV):
        A.run_case_captured(cv, _lib.load(), DEV)                                      # (the same case passes as it stands)
        with pytest.raises(AssertionError, match='differ from the reference') as e:
            A.run_case_captured(cv, _lib.load(), DEV, args_for=_max_element_from_the_data)
    assert 'replay 0 on variant 1' in str(e.value)


def test_refused_calls_leave_an_open_capture_usable():
    """A handful of refused calls (QD_ERR_UNSUPPORTED, QD_ERR_INVALID_ARGUMENT, QD_ERR_WORKSPACE_TOO_SMALL) made inside an open
    capture: each returns its code and writes nothing, the capture stays valid and the call recorded behind them into the same
    graph replays correctly on every variant."""
    lib = _lib.load()
    refused = []
    for gid in ('K1-levels-only', 'K4-indices-only-refused', 'codec', 'histograms'):
        refused += [c for c in A.cases_of(A.GROUPS[gid], lib) if c.rc != 0][:3]
    assert {c.rc for c in refused} == {A.ERR_INVALID, A.ERR_WS, A.ERR_UNSUPPORTED} and len(refused) >= 10
    with torch.cuda.device(DEV):
        A.run_case_captured(_first_case('K4-b256-nf10'), lib, DEV, refused=refused)
