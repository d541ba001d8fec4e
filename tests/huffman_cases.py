"""Cases of the Huffman checkpoint codec at the C ABI (qd_huffman_encode / qd_huffman_decode_f32 of include/qd_hip.h), shared
by tests/test_huffman_cases_host.py (libqd_host.so, no GPU) and tests/test_hip_huffman_cases.py (libqd_hip.so against
libqd_host.so).  Each case is the smallest input that reaches one branch of csrc/qd_huffman.hip (DESIGN.md section 9 lists
them); `check_conditions` asserts, from the code lengths alone, that the input does reach it.  A plain helper module: no
fixtures, nothing runs on import but the case table.

Also holds `_npdecode`, the independent numpy decoder of the file format, and `skewed_tensor`, so that the host and the
device suites share them."""
import collections
import ctypes
import struct
import zlib

import numpy as np
import torch

from quantized_distillation_amd import _lib
from quantized_distillation_amd import compressed as C

CHUNK = C.CHUNK
SENTINEL = 777.0                    # between the fp32 outputs of a case
SYM_SENTINEL = 0xEE                 # between its symbol arrays
WORD_SENTINEL = 0x5A5A5A5A          # behind the last word of its bitstream

# n symbols; bucket (0 = one (alpha, beta) for the tensor); levels (s, or k for a non-uniform tensor); nonuniform; k points
Tensor = collections.namedtuple('Tensor', 'n bucket levels nonuniform k')
# lens: code length of each of the 256 symbols; single: the only symbol of a 0-bit code, else -1; draws: per tensor, the
# symbols its elements are drawn from (uniformly, one generator per case seeded with `seed`); points: all tensors' points
Case = collections.namedtuple('Case', 'id lens single tensors draws seed points')
Result = collections.namedtuple('Result', 'chunk_words words decoded')


def _lens(by_symbol):
    return list(by_symbol) + [0] * (256 - len(by_symbol))


def _uniform(n, levels, bucket=0):
    return Tensor(n, bucket, levels, 0, 0)


def _case(cid, lens, tensors, draws=None, single=-1, points=None):
    lens = _lens(lens)
    coded = [s for s, l in enumerate(lens) if l]
    draws = [list(d) if d is not None else coded for d in (draws or [None] * len(tensors))]
    assert len(draws) == len(tensors)
    return Case(cid, lens, single, list(tensors), draws, zlib.crc32(cid.encode()),
                None if points is None else np.asarray(points, dtype=np.float32))


DEEP = list(range(1, 33)) + [32]                            # 33 symbols, base[32] = 2^32 - 2
CODE16 = [2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 8, 8]   # 16 symbols, every length <= 8
MANY_SIZES = (0, 1, 5, 1024, 0, 1030)


def _build_cases():
    cases = [
        _case('deep', DEEP, [_uniform(n, 33) for n in (1024, 1025, 1)]),
        _case('full_chunk', DEEP, [_uniform(n, 33) for n in (1024, 1024, 1)], draws=[[31, 32], [0], None]),
        _case('lut_edge_10', list(range(1, 11)) + [10], [_uniform(3000, 11)]),
        _case('lut_edge_11', list(range(1, 12)) + [11], [_uniform(3000, 12)]),
        _case('short', [1, 1], [_uniform(2049, 2)]),
        _case('fixed8', [8] * 256, [_uniform(2500, 256)]),
        _case('fixed6', [6] * 64, [_uniform(2500, 34)], draws=[range(34)]),
        _case('single', [], [_uniform(n, 16, 256) for n in (0, 1, 1024, 1500)], draws=[[7]] * 4, single=7),
        _case('buckets', CODE16, [_uniform(5000, 16, b) for b in (0, 7, 100, 1000, 1024, 1025, 3000)] + [_uniform(50, 16)]),
        _case('points', CODE16, [Tensor(1500, 100, 3, 1, 3), Tensor(2100, 100, 17, 1, 17)], draws=[range(3), None],
              points=[0.0, 0.4, 1.0] + [(j / 16.0) ** 1.5 for j in range(17)]),
        # 128 tensors cycling through MANY_SIZES, then two empty ones: the first and the last tensor are empty, two empty
        # ones are adjacent, and the 1030-element tensor of the 13th cycle owns chunks 63 and 64
        _case('many', CODE16, [_uniform(MANY_SIZES[i % 6], 16, (0, 3, 256)[i % 3]) for i in range(128)] + [_uniform(0, 16)] * 2),
        _case('scan', CODE16, [_uniform(1, 16)] * 4100),
    ]
    return collections.OrderedDict((c.id, c) for c in cases)


CASES = _build_cases()
CASE_IDS = list(CASES)


# ---------------------------------------------------------------- what a case holds, computed on the host
def symbols(case):
    """The uint8 symbols of every tensor of the case."""
    rng = np.random.default_rng(case.seed)
    out = []
    for t, pool in zip(case.tensors, case.draws):
        pool = np.asarray(pool, dtype=np.uint8)
        out.append(pool[rng.integers(0, len(pool), t.n)])
    return out


def nbuckets(t):
    return 0 if t.n == 0 else (1 if t.bucket == 0 else -(-t.n // t.bucket))


def nchunks_of(t):
    return -(-t.n // CHUNK)


def _firsts(counts):
    return [int(v) for v in np.cumsum([0] + list(counts))[:-1]]


def first_buckets(case):
    return _firsts(nbuckets(t) for t in case.tensors)


def first_chunks(case):
    return _firsts(nchunks_of(t) for t in case.tensors)


def first_points(case):
    return _firsts(t.k for t in case.tensors)


def alpha_beta(case):
    """A distinct exact (alpha, beta) for every bucket, numbered through the whole case: a wrong bucket index changes the
    output."""
    b = np.arange(max(sum(nbuckets(t) for t in case.tensors), 1), dtype=np.float32)
    return (1.0 + b).astype(np.float32), (-0.5 * b).astype(np.float32)


def chunk_bits(case, syms):
    """Bits of every chunk, from the code lengths alone (none for a one-symbol code)."""
    lens = np.asarray(case.lens, dtype=np.int64)
    out = []
    for s in syms:
        l = lens[s] if case.single < 0 else np.zeros(len(s), dtype=np.int64)
        out += [int(l[e:e + CHUNK].sum()) for e in range(0, len(s), CHUNK)]
    return out


def expected_chunk_words(case, syms):
    """chunk_words of include/qd_hip.h: every chunk starts on a word of its own; the last entry is the total."""
    return np.cumsum([0] + [-(-b // 32) for b in chunk_bits(case, syms)]).astype(np.uint32)


def straddles(case, syms):
    """Codewords that end in the word after the one they start in, per chunk position: cumulative lengths only."""
    lens = np.asarray(case.lens, dtype=np.int64)
    total = 0
    for s in syms:
        for e in range(0, len(s), CHUNK):
            l = lens[s[e:e + CHUNK]]
            p = np.cumsum(l) - l
            total += int(((p % 32) + l > 32).sum())
    return total


def expected(case, syms):
    """The three float32 operations of include/qd_hip.h per element, each rounded to float32:
    uniform (sym / (levels - 1)) * alpha + beta + 0, non-uniform points[first_point + sym] * alpha + beta + 0."""
    alpha, beta = alpha_beta(case)
    out = []
    for t, s, fb, fp in zip(case.tensors, syms, first_buckets(case), first_points(case)):
        e = np.arange(t.n, dtype=np.int64)
        bk = fb + (e // t.bucket if t.bucket else 0 * e)
        a, b = alpha[bk], beta[bk]
        if t.nonuniform:
            v = case.points[fp + s.astype(np.int64)] * a
        else:
            w = s.astype(np.float32) / np.float32(t.levels - 1)
            v = w * a
        v = v + b
        v = v + np.float32(0.0)
        assert v.dtype == np.float32
        out.append(v)
    return out


def check_conditions(case, syms):
    """What keeps a case from silently missing its branch; asserted on the host before any library call."""
    lens, cid = case.lens, case.id
    assert case.single >= 0 or C._kraft_complete(lens), cid
    assert case.single < 0 or not any(lens), cid
    for t, s in zip(case.tensors, syms):
        assert len(s) == t.n and (t.n == 0 or int(s.max()) < t.levels), cid        # well-formed streams only
        assert case.single >= 0 or all(lens[int(v)] for v in np.unique(s)), cid
        assert not t.nonuniform or t.k == t.levels, cid
    drawn = set(lens[int(v)] for s in syms for v in np.unique(s))
    bits = chunk_bits(case, syms)
    chunks = [nchunks_of(t) for t in case.tensors]
    if cid == 'deep':
        assert set(range(11, 33)) <= drawn and straddles(case, syms) > 0
    if cid == 'full_chunk':
        assert bits[0] == 32 * CHUNK and bits[1:] == [CHUNK, lens[int(syms[2][0])]]
    if cid in ('lut_edge_10', 'lut_edge_11'):
        top = int(cid[-2:])
        longest = [s for s, l in enumerate(lens) if l == top]
        assert max(lens) == top and len(longest) == 2 and all((syms[0] == s).any() for s in longest)
    if cid == 'short':
        assert max(lens) < 10
    if cid in ('fixed8', 'fixed6'):
        assert len(set(l for l in lens if l)) == 1
        assert (straddles(case, syms) > 0) == (cid == 'fixed6')                     # 6-bit codes cross words, 8-bit ones never
    if cid == 'single':
        assert sum(bits) == 0 and sum(chunks) == 4
    if cid == 'buckets':
        t = [t for t in case.tensors if t.bucket == CHUNK][0]
        assert any(e % t.bucket == 0 and e % CHUNK == 0 for e in range(1, t.n))    # a bucket ends where a chunk ends
        assert any(t.bucket > CHUNK for t in case.tensors) and any(t.bucket and CHUNK % t.bucket for t in case.tensors)
    if cid == 'points':
        assert first_points(case)[1] != 0 and all(t.nonuniform for t in case.tensors)
    if cid == 'many':
        ns = [t.n for t in case.tensors]
        assert sum(chunks) > 64 and ns[0] == 0 and ns[-1] == 0 and any(a == 0 and b == 0 for a, b in zip(ns, ns[1:]))
        assert any(c and fc // 64 != (fc + c - 1) // 64 for fc, c in zip(first_chunks(case), chunks))
    if cid == 'scan':
        assert sum(chunks) > 4096


# ---------------------------------------------------------------- one case through one library
def _offsets(sizes, unit):
    """Offsets (in elements) of arrays of `sizes` elements in one flat buffer, each on a 4-byte boundary, with a gap of
    sentinels before every array and after the last; the gaps cycle so that the 16-byte alignment differs."""
    offs, o = [], 0
    for j, n in enumerate(sizes):
        o += unit * (1 + j % 3)
        offs.append(o)
        o += -(-n // unit) * unit
    return offs, o + unit


def run_case(case, lib, device, stream=None):
    """Encode the case's symbols with `lib` (_lib.load() on a HIP device, _lib.host() on the CPU) and decode the stream with
    the same library; with stream=(chunk_words, words) of another run, decode that one instead.  The symbol arrays and the
    outputs are carved out of one flat buffer each, at 4-byte offsets that are not all 16-byte aligned; the sentinels between
    them, and behind the bitstream, must be intact afterwards.  Returns Result(chunk_words, words[:nwords], decoded)."""
    device = torch.device(device)
    cuda = device.type == 'cuda'
    syms = symbols(case)
    check_conditions(case, syms)
    nt, ns = len(case.tensors), [t.n for t in case.tensors]
    nchunks = sum(nchunks_of(t) for t in case.tensors)
    st = _lib.stream_ptr(device) if cuda else None

    sym_off, sym_total = _offsets(ns, 4)
    y_off, y_total = _offsets(ns, 1)
    assert any(o % 4 for o in y_off) and any(o % 16 for o in sym_off)                # not all 16-byte aligned
    sym_image = np.full(sym_total, SYM_SENTINEL, dtype=np.uint8)
    y_keep = np.ones(y_total, dtype=bool)
    for s, so, yo in zip(syms, sym_off, y_off):
        sym_image[so:so + len(s)] = s
        y_keep[yo:yo + len(s)] = False
    sym_flat = torch.from_numpy(sym_image.copy()).to(device)
    y_flat = torch.full((y_total,), SENTINEL, dtype=torch.float32, device=device)

    table = (_lib.QdHufTensor * nt)()
    for j, (t, fc, fb, fp) in enumerate(zip(case.tensors, first_chunks(case), first_buckets(case), first_points(case))):
        e = table[j]
        e.sym, e.y = sym_flat.data_ptr() + sym_off[j], y_flat.data_ptr() + 4 * y_off[j]
        e.n, e.first_chunk, e.first_bucket, e.first_point = t.n, fc, fb, fp
        e.bucket, e.levels, e.nonuniform = t.bucket, t.levels, t.nonuniform
    code = C.canonical_code(case.lens, case.single)
    if cuda:
        table_d, code_d = _lib.upload_struct(table, device), _lib.upload_struct(code, device)
        table_p, code_p = table_d.data_ptr(), code_d.data_ptr()
    else:
        table_p, code_p = ctypes.addressof(table), ctypes.addressof(code)

    if stream is None:
        max_words = sum(chunk_bits(case, syms)) // 32 + nchunks + 1
        fill = int(np.uint32(WORD_SENTINEL).view(np.int32))
        chunk_words = torch.full((nchunks + 1,), fill, dtype=torch.int32, device=device)
        words = torch.full((max_words,), fill, dtype=torch.int32, device=device)
        _lib.check(lib.qd_huffman_encode(table_p, nt, nchunks, code_p, chunk_words.data_ptr(), words.data_ptr(), max_words, st))
        cw = chunk_words.cpu().numpy().view(np.uint32).copy()
        nwords = int(cw[-1])
        assert nwords <= max_words, (case.id, nwords, max_words)
        w_all = words.cpu().numpy().view(np.uint32)
        assert (w_all[nwords:] == WORD_SENTINEL).all(), (case.id, 'written behind the last word of the bitstream')
        w = w_all[:nwords].copy()
    else:
        cw, w = (np.ascontiguousarray(a, dtype=np.uint32) for a in stream)
        nwords = len(w)
        assert len(cw) == nchunks + 1 and int(cw[-1]) == nwords

    alpha, beta = (torch.from_numpy(a).to(device) for a in alpha_beta(case))
    points = torch.from_numpy(case.points).to(device) if case.points is not None else None
    cw_t = torch.from_numpy(cw.view(np.int32)).to(device)
    w_t = torch.from_numpy(w.view(np.int32)).to(device) if nwords else None
    _lib.check(lib.qd_huffman_decode_f32(w_t.data_ptr() if nwords else None, nwords, cw_t.data_ptr(), table_p, nt, nchunks,
                                         code_p, alpha.data_ptr(), beta.data_ptr(),
                                         points.data_ptr() if points is not None else None, st))
    y = y_flat.cpu().numpy()
    assert (y[y_keep] == np.float32(SENTINEL)).all(), (case.id, 'written between the tensors')
    assert np.array_equal(sym_flat.cpu().numpy(), sym_image), (case.id, 'the symbols were written over')
    return Result(cw, w, [y[o:o + n].copy() for o, n in zip(y_off, ns)])


def same_bits(got, want):
    """Lists of float32 arrays, equal as int32 views."""
    return len(got) == len(want) and all(a.dtype == b.dtype == np.float32 and a.shape == b.shape and
                                         np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(got, want))


# ---------------------------------------------------------------- file level
def skewed_tensor():
    """(x, level of every element, s): s = 21 levels with counts 1, 1, 2, 4, ..., 2^19 (2^20 elements, min 0, max 1, level j
    at j / 20), shuffled.  The optimal code of that histogram is 20 bits deep: a real Huffman code beyond the decoder's
    lookup table."""
    s = 21
    counts = [1] + [1 << j for j in range(20)]
    lev = np.repeat(np.arange(s), counts)
    np.random.default_rng(0).shuffle(lev)
    return torch.from_numpy((lev / (s - 1)).astype(np.float32)), lev, s


def _npdecode(path):
    """An independent decoder of the format, written from DESIGN.md section 9 (numpy + Python only)."""
    data = open(path, 'rb').read()
    (magic, version, coding, mode, chunk, ntensors, max_len, single, table_bytes, nsym, nbuckets, npoints, nraw, nchunks,
     nwords, crc, _r) = struct.unpack_from('<8sIIIIIIi7QII', data, 0)
    assert magic == b'QDHUFF\x00\x01' and chunk == 1024
    pos = 100
    entries = []
    for _ in range(ntensors):
        ln, kind, ndim = struct.unpack_from('<HBB', data, pos)
        pos += 4
        name = data[pos:pos + ln].decode()
        pos += ln
        shape = struct.unpack_from('<%dQ' % ndim, data, pos)
        pos += 8 * ndim
        numel, bucket, levels, offset, count, first_point, first_chunk = struct.unpack_from('<QQIQQQQ', data, pos)
        pos += 52
        entries.append((name, kind, shape, numel, bucket, levels, offset, first_point, first_chunk))
    o = 100 + table_bytes
    lens = list(data[o:o + 256])
    o += 256
    alpha = np.frombuffer(data, '<f4', nbuckets, o); o += 4 * nbuckets
    beta = np.frombuffer(data, '<f4', nbuckets, o); o += 4 * nbuckets
    pts = np.frombuffer(data, '<f4', npoints, o); o += 4 * npoints
    raw = np.frombuffer(data, '<f4', nraw, o); o += 4 * nraw
    cw = np.frombuffer(data, '<u4', nchunks + 1 if nchunks else 0, o); o += 4 * len(cw)
    words = np.frombuffer(data, '<u4', nwords, o)
    bitstr = ''.join(format(int(w), '032b') for w in words)
    # canonical code: (length, symbol) order
    decode, code, prev = {}, 0, 0
    for l, s in sorted((l, s) for s, l in enumerate(lens) if l):
        code <<= (l - prev)
        decode[format(code, '0%db' % l)] = s
        code += 1
        prev = l
    out = {}
    for name, kind, shape, numel, bucket, levels, offset, first_point, first_chunk in entries:
        if kind != 1:
            out[name] = raw[offset:offset + numel].reshape(shape)
            continue
        syms = []
        for c in range(-(-numel // 1024)):
            bits = bitstr[32 * int(cw[first_chunk + c]):]
            cur, i = '', 0
            while len(syms) < min(numel, 1024 * (c + 1)):
                if single >= 0:
                    syms.append(single)
                    continue
                cur += bits[i]
                i += 1
                if cur in decode:
                    syms.append(decode[cur])
                    cur = ''
        y = np.empty(numel, np.float32)
        for e, sym in enumerate(syms):
            bk = offset + (e // bucket if bucket and numel >= bucket else 0)
            a, b = alpha[bk], beta[bk]
            if mode == 0:
                v = np.float32(np.float32(sym) / np.float32(levels - 1)) * a
            else:
                v = pts[first_point + sym] * a
            y[e] = np.float32(np.float32(v + b) + np.float32(0.0))
        out[name] = y.reshape(shape)
    return out
