"""Quantized models saved and loaded in Huffman-coded form.

The reference reports the size of a quantized student (helpers/functions.py:226-262: the Huffman mean code length of
quantization/help_functions.py:157-232 per quantized weight, plus 8 B of (alpha, beta) per bucket) but saves it as a full
fp32 state_dict (cifar10_test.py:265-270).  save_compressed writes a file of that size; load_compressed reads back exactly
the tensors the quantizer produced:

    uniform      load(save(t)) == uniformQuantization(t, s, bucket_size=bucket_size)[0]
    non-uniform  load(save(t)) == nonUniformQuantization(t, points_i, bucket_size=bucket_size)[0]
    raw          load(save(t)) == t

bit for bit, on a HIP device (libqd_hip.so) or on the CPU (libqd_host.so), for a file written by either library.  The
format is specified in DESIGN.md section 9; loading never unpickles.  Symbols (the uint8 level / point index of every
quantized weight) come from the quantize kernels themselves, the histogram of the whole model gives one canonical Huffman
code (lengths built as help_functions.huffman_encode builds them), and the bitstream is written and read by
qd_huffman_encode / qd_huffman_decode_f32 (csrc/qd_huffman.hip, csrc/host/qd_host.cpp).
"""
import collections
import ctypes
import fractions
import math
import numbers
import struct
import zlib

import numpy as np
import torch

from . import _lib
from .codec import bits_for_levels
from .multi_tensor import MultiTensorSymbols
from .quantization.help_functions import huffman_encode

MAGIC = b'QDHUFF\x00\x01'
VERSION = 1
CHUNK = 1024                        # QD_HUF_CHUNK of include/qd_hip.h
MAX_CODE_LEN = 32                   # longest codeword the decoders take; a longer optimal code falls back to fixed width
# magic, version, coding, mode, chunk, ntensors, max_len, single | table_bytes, nsym, nbuckets, npoints, nraw, nchunks, nwords |
# crc32 of everything after the header, reserved
HEADER = struct.Struct('<8sIIIIIIi7QII')
ENTRY = struct.Struct('<HBB')       # name length, kind, ndim; then the name (utf-8), ndim x u64 dims, ENTRY_TAIL
ENTRY_TAIL = struct.Struct('<QQIQQQQ')   # numel, bucket (0 = none), levels, offset, count, first_point, first_chunk
CODINGS = ('none', 'huffman', 'fixed')
MODES = ('uniform', 'nonuniform')
KIND_RAW, KIND_QUANTIZED, KIND_BUFFER = 0, 1, 2
SYM_ALIGN = 16                      # every tensor's symbols start on a 16-byte boundary of the symbol buffer


# ---------------------------------------------------------------- the code
def code_lengths(counts):
    """Code length per symbol (256 entries) from the histogram of all stored symbols, built exactly as
    get_huffman_encoding_mean_bit_length builds its code (help_functions.py:213-231), and the mean bit length it reports."""
    total = int(sum(counts))
    lens = [0] * 256
    if total == 0:
        return lens, 0.0
    freq = {j: int(c) / total for j, c in enumerate(counts) if c > 0}
    code = huffman_encode(freq)
    for sym, word in code:
        lens[sym] = len(word)
    return lens, sum(freq[sym] * len(word) for sym, word in code)


def canonical_code(lens, single=-1):
    """QdHufCode (include/qd_hip.h) of a length table: codewords numbered in (length, symbol) order."""
    c = _lib.QdHufCode()
    count = [0] * 33
    for l in lens:
        if l:
            count[l] += 1
    base, first, code, pos = [0] * 33, [0] * 33, 0, 0
    for l in range(1, 33):
        code = (code + count[l - 1]) << 1 if l > 1 else 0
        base[l], first[l] = code, pos
        pos += count[l]
    order = sorted((l, s) for s, l in enumerate(lens) if l)
    nxt = list(base)
    for i, (l, s) in enumerate(order):
        c.code[s] = nxt[l]
        nxt[l] += 1
        c.sorted[i] = s
    for l in range(33):
        c.base[l], c.count[l], c.first[l] = base[l] & 0xffffffff, count[l], first[l]
    for s in range(256):
        c.len[s] = lens[s]
    c.single = single
    c.max_len = max(lens)
    return c


def _kraft_complete(lens):
    return sum(1 << (MAX_CODE_LEN - l) for l in lens if l) == 1 << MAX_CODE_LEN


# ---------------------------------------------------------------- inputs
def _named(tensors, what):
    if tensors is None:
        return []
    if isinstance(tensors, torch.nn.Module):
        items = list(tensors.named_parameters()) if what == 'tensors' else list(tensors.named_buffers())
    elif isinstance(tensors, collections.abc.Mapping):
        items = list(tensors.items())
    else:
        raise TypeError('%s must be a name -> tensor mapping or an nn.Module' % what)
    out = []
    for name, t in items:
        if not isinstance(t, torch.Tensor):
            raise TypeError('%s[%r] is not a tensor' % (what, name))
        if t.dtype != torch.float32:
            raise ValueError('%s[%r] is %s: only float32 tensors are stored' % (what, name, t.dtype))
        out.append((str(name), t.detach()))
    return out


def _point_list(points, nq):
    """One trimmed fp32 CPU tensor of sorted points per quantized tensor (one list, or a one-element list of lists, is
    shared by all of them)."""
    if isinstance(points, torch.Tensor) and points.dim() == 1:
        points = [points] * nq
    elif isinstance(points, (list, tuple)) and len(points) and all(isinstance(p, (int, float)) for p in points):
        points = [points] * nq
    points = list(points)
    if len(points) == 1:                # one list for every quantized tensor
        points = points * nq
    if len(points) != nq:
        raise ValueError('points: one list of points per quantized tensor (%d), got %d' % (nq, len(points)))
    out = []
    for p in points:
        p = torch.as_tensor(p, dtype=torch.float32).detach().cpu().reshape(-1)
        k = p.numel()
        while k > 0 and math.isinf(float(p[k - 1])) and float(p[k - 1]) > 0:     # save_quantization_points' +inf padding
            k -= 1
        p = p[:k].contiguous()
        if not 1 <= k <= 256:
            raise ValueError('a point list holds 1 .. 256 points, got %d' % k)
        if not bool(torch.isfinite(p).all()) or (k > 1 and not bool((p[1:] >= p[:-1]).all())):
            raise ValueError('quantization points must be finite and sorted ascending')
        out.append(p)
    return out


def _nbuckets(n, bucket):
    if n == 0:
        return 0
    return 1 if (bucket is None or n < bucket) else -(-n // bucket)


# ---------------------------------------------------------------- save
def save_compressed(path, tensors, *, s=None, points=None, bucket_size=256, quantize_first_last=True, buffers=None,
                    type_of_scaling='linear', stochastic_rounding=False, subtract_mean=False, max_element=False):
    """Quantize `tensors` (an ordered name -> tensor mapping, or an nn.Module's named_parameters()) and write them in
    Huffman-coded form; returns a report (section bytes, file bytes, mean code length, coding, reference_size_mb).

    Exactly one of `s` (uniform, 2 <= s <= 256 levels: one count for all, or a sequence with one entry per QUANTIZED tensor
    in the order of `tensors` -- with quantize_first_last=False the first and the last tensor have no entry) or `points`
    (non-uniform: one sorted list of at most 256 points per quantized tensor, or one list for all) is given.  bucket_size: None,
    one positive int for all, or -- as `s` -- a sequence of positive ints with one entry per quantized tensor
    (multi_tensor.per_channel_bucket_sizes(...) of the quantized tensors: the scales a per-channel model trained with); the file
    stores each tensor's own.  With a sequence, uniform mode on a HIP device takes the symbols, alpha and beta of the whole model
    from one launch (MultiTensorSymbols); the report's 'symbolizer' names it, 'per_tensor' otherwise.  quantize_first_last=False stores the first and the last tensor as raw
    fp32 (the reference's quantizeFirstLastLayer).  `buffers` (e.g. BN running statistics) are stored as raw fp32.  The
    quantizer options are the ones the training loops save with: linear scaling, deterministic rounding, no mean subtraction,
    no max_element; any other raises ValueError."""
    if type_of_scaling != 'linear' or stochastic_rounding or subtract_mean or max_element is not False:
        raise ValueError('compressed checkpoints store linear-scaled, deterministically rounded tensors without mean '
                         'subtraction or max_element')
    if (s is None) == (points is None):
        raise ValueError('give exactly one of s (uniform) or points (non-uniform)')
    b_list = None                       # the entries of a sequence bucket_size
    if bucket_size is not None and not isinstance(bucket_size, numbers.Real):
        if isinstance(bucket_size, (str, bytes)) or not hasattr(bucket_size, '__iter__'):
            raise ValueError(_BUCKET_RULE)
        b_list = list(bucket_size)
        for v in b_list:
            if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 < v < 2 ** 63:
                raise ValueError('%s, got the entry %r' % (_BUCKET_RULE, v))
        b_list = [int(v) for v in b_list]
    elif bucket_size is not None and (isinstance(bucket_size, bool) or not isinstance(bucket_size, int) or bucket_size <= 0):
        raise ValueError('bucket_size must be a positive int or None')
    s_list = None                       # the entries of a sequence s
    if s is not None:
        scalar = isinstance(s, numbers.Real)
        if not scalar and (isinstance(s, (str, bytes)) or not hasattr(s, '__iter__')):
            raise ValueError('s must be an integer in 2 .. 256, or a sequence of them with one entry per quantized tensor')
        s_list = None if scalar else list(s)
        for v in ([s] if scalar else s_list):
            if _lib.level_count(v, 's (2 .. 256 in a compressed file)') > 256:        # the shared range check first
                raise ValueError('s must be an integer in 2 .. 256, or a sequence of them with one entry per quantized tensor')
    params = _named(tensors, 'tensors')
    bufs = _named(buffers, 'buffers')
    names = [n for n, _ in params] + [n for n, _ in bufs]
    if len(set(names)) != len(names):
        raise ValueError('tensor names must be unique')
    devices = {t.device for _, t in params + bufs}
    if len(devices) > 1:
        raise ValueError('all tensors must live on one device, got %s' % sorted(str(d) for d in devices))
    dev = devices.pop() if devices else torch.device('cpu')
    if not (dev.type == 'cpu' or dev.type == 'cuda'):
        raise ValueError('tensors must live on a HIP device or on the CPU')
    T = len(params)
    quant = [i for i in range(T) if quantize_first_last or i not in (0, T - 1)]
    mode = 0 if s is not None else 1
    pts = _point_list(points, len(quant)) if mode else None
    if s_list is not None and len(s_list) != len(quant):
        raise ValueError('s has %d entries for %d quantized tensors: need one per quantized tensor' % (len(s_list), len(quant)))
    if b_list is not None and len(b_list) != len(quant):
        raise ValueError('%s: got %d entries for %d quantized tensors' % (_BUCKET_RULE, len(b_list), len(quant)))
    if mode == 0:
        s = [int(v) for v in s_list] if s_list is not None else [int(s)] * len(quant)
    if dev.type == 'cuda':
        with torch.cuda.device(dev):
            return _save(path, params, bufs, quant, mode, s, pts, bucket_size, dev, b_list)
    return _save(path, params, bufs, quant, mode, s, pts, bucket_size, dev, b_list)


_BUCKET_RULE = ('bucket_size must be a positive int, None, or a sequence of positive ints with one entry per quantized tensor '
                '(in the order of `tensors`)')


def _save(path, params, bufs, quant, mode, s, pts, bucket_size, dev, b_list=None):
    """b_list: None, or the bucket size of every quantized tensor (a sequence bucket_size); bks holds tensor j's either way."""
    cuda = dev.type == 'cuda'
    bks = b_list if b_list is not None else [bucket_size] * len(quant)
    one_launch = b_list is not None and mode == 0 and cuda and len(quant) > 0
    lib = _lib.load() if cuda else _lib.host()
    qset = set(quant)
    qx = [params[i][1].contiguous().view(-1) for i in quant]
    ns = [x.numel() for x in qx]
    nbs = [_nbuckets(n, b) for n, b in zip(ns, bks)]
    levels = s if mode == 0 else [p.numel() for p in pts]         # mode 0: s is the list of level counts, one per quantized tensor
    sym_off, o = [], 0
    for n in ns:
        sym_off.append(o)
        o += -(-n // SYM_ALIGN) * SYM_ALIGN
    nsym, nbuckets = sum(ns), sum(nbs)
    sym = torch.zeros(max(o, SYM_ALIGN), dtype=torch.uint8, device=dev)
    ab = torch.empty(2, max(nbuckets, 1), dtype=torch.float32, device=dev)
    scratch = None if one_launch else torch.empty(max(ns + [1]), dtype=torch.float32, device=dev)     # the loop's unread fp32 result
    ws = _lib.workspace(dev) if cuda else None
    wsp, wsn = (ws.data_ptr(), ws.numel()) if cuda else (None, 0)
    st = _lib.stream_ptr(dev) if cuda else None
    fb = 0
    first_bucket = []
    if one_launch:                      # symbols, alpha and beta of every tensor from one launch, written where the loop writes them
        MultiTensorSymbols(qx, levels, b_list, symbols=[sym[o:o + n] for o, n in zip(sym_off, ns)],
                           alpha_beta=(ab[0], ab[1])).encode()
    for j, x in enumerate(qx):
        first_bucket.append(fb)
        n = ns[j]
        if n and not one_launch:
            a_p, b_p = ab[0].data_ptr() + 4 * fb, ab[1].data_ptr() + 4 * fb
            bk = bks[j] or 0
            if mode == 0:               # K1 with its uint8 level output: the symbols and the alpha / beta of uniformQuantization
                _lib.check(lib.qd_uniform_f32(x.data_ptr(), scratch.data_ptr(), n, bk, levels[j], a_p, b_p,
                                              sym.data_ptr() + sym_off[j], None, 0, 0.0, 0, 0, wsp, wsn, st), lib)
            else:                       # K4 with uint8 point indices: those of nonUniformQuantization
                p = pts[j].to(dev)
                _lib.check(lib.qd_nearest_point_f32(x.data_ptr(), 0, p.data_ptr(), levels[j], 0, scratch.data_ptr(),
                                                    sym.data_ptr() + sym_off[j], 1, n, bk, a_p, b_p, None, 0, 0.0, wsp, wsn, st), lib)
        fb += nbs[j]
    # histogram of every stored symbol (the zero padding between tensors is taken off symbol 0)
    pad = sym.numel() - nsym
    if cuda:
        hist = torch.empty(256, dtype=torch.int64, device=dev)
        _lib.check(lib.qd_histogram_u8_ws(sym.data_ptr(), sym.numel(), 256, hist.data_ptr(), wsp, wsn, st), lib)
        counts = hist.cpu().numpy().astype(np.int64)
    else:
        counts = np.bincount(sym.numpy(), minlength=256).astype(np.int64)
    counts[0] -= pad
    lens, mean_bits = code_lengths(counts)
    single = -1
    if nsym == 0:
        coding = 0
    elif max(lens) <= MAX_CODE_LEN:
        coding = 1
        if int((counts > 0).sum()) == 1:
            single = int(np.nonzero(counts)[0][0])
    else:                               # the optimal code is longer than the decoders take: fixed-width level indices
        coding = 2
        bits = bits_for_levels(max(levels))
        lens = [bits] * (1 << bits) + [0] * (256 - (1 << bits))
    code_bits = int(sum(int(c) * l for c, l in zip(counts, lens))) if single < 0 else 0

    chunks = [-(-n // CHUNK) for n in ns]
    first_chunk = list(np.cumsum([0] + chunks)[:-1]) if chunks else []
    nchunks = int(sum(chunks))
    words_np = np.zeros(0, dtype=np.uint32)
    chunk_np = np.zeros(0, dtype=np.uint32)
    if nchunks:
        max_words = code_bits // 32 + nchunks + 1
        if max_words >= 1 << 32:
            raise ValueError('the bitstream exceeds the 32-bit word offsets of the format')
        table = (_lib.QdHufTensor * len(quant))()
        for j in range(len(quant)):
            e = table[j]
            e.sym, e.n, e.first_chunk = sym.data_ptr() + sym_off[j], ns[j], int(first_chunk[j])
        code = canonical_code(lens, single)
        chunk_words = torch.empty(nchunks + 1, dtype=torch.int32, device=dev)
        words = torch.empty(max_words, dtype=torch.int32, device=dev)
        if cuda:
            table_d = _lib.upload_struct(table, dev)
            code_d = _lib.upload_struct(code, dev)
            _lib.check(lib.qd_huffman_encode(table_d.data_ptr(), len(quant), nchunks, code_d.data_ptr(), chunk_words.data_ptr(),
                                             words.data_ptr(), max_words, st), lib)
        else:
            _lib.check(lib.qd_huffman_encode(ctypes.addressof(table), len(quant), nchunks, ctypes.addressof(code),
                                             chunk_words.data_ptr(), words.data_ptr(), max_words, None), lib)
        chunk_np = chunk_words.cpu().numpy().view(np.uint32)
        nwords = int(chunk_np[-1])
        if nwords > max_words:
            raise RuntimeError('qd_huffman_encode: %d words for a buffer of %d' % (nwords, max_words))
        words_np = words[:nwords].cpu().numpy().view(np.uint32)

    # the file
    ab_np = ab[:, :nbuckets].cpu().numpy() if nbuckets else np.zeros((2, 0), np.float32)
    pts_np = np.concatenate([p.numpy() for p in pts]) if (mode and pts) else np.zeros(0, np.float32)
    first_point = list(np.cumsum([0] + levels)[:-1]) if mode else [0] * len(quant)
    raw_list = [(name, t, KIND_RAW) for i, (name, t) in enumerate(params) if i not in qset] + \
               [(name, t, KIND_BUFFER) for name, t in bufs]
    raw_off, r = {}, 0
    for name, t, _k in raw_list:
        raw_off[name] = r
        r += t.numel()
    nraw = r
    qpos = {i: j for j, i in enumerate(quant)}
    entries = []
    for i, (name, t) in enumerate(params):
        if i in qset:
            j = qpos[i]
            entries.append((name, KIND_QUANTIZED, tuple(t.shape), ns[j], bks[j] or 0, levels[j], first_bucket[j], nbs[j],
                            int(first_point[j]), int(first_chunk[j])))
        else:
            entries.append((name, KIND_RAW, tuple(t.shape), t.numel(), 0, 0, raw_off[name], t.numel(), 0, 0))
    for name, t in bufs:
        entries.append((name, KIND_BUFFER, tuple(t.shape), t.numel(), 0, 0, raw_off[name], t.numel(), 0, 0))
    table_b = _pack_table(entries)
    raw_np = np.concatenate([t.contiguous().view(-1).cpu().numpy() for _n, t, _k in raw_list]) if raw_list else np.zeros(0, np.float32)
    body = [table_b, bytes(bytearray(lens)), ab_np[0].astype('<f4').tobytes(), ab_np[1].astype('<f4').tobytes(),
            pts_np.astype('<f4').tobytes(), raw_np.astype('<f4').tobytes(),
            chunk_np.astype('<u4').tobytes(), words_np.astype('<u4').tobytes()]
    crc = 0
    for b in body:
        crc = zlib.crc32(b, crc)
    header = HEADER.pack(MAGIC, VERSION, coding, mode, CHUNK, len(entries), max(lens), single, len(table_b), nsym, nbuckets,
                         len(pts_np), nraw, nchunks, len(words_np), crc, 0)
    with open(path, 'wb') as f:
        f.write(header)
        for b in body:
            f.write(b)

    # the report
    n_raw_params = sum(t.numel() for _n, t, k in raw_list if k == KIND_RAW)
    n_buf = sum(t.numel() for _n, t, k in raw_list if k == KIND_BUFFER)
    sections = collections.OrderedDict([
        ('header', HEADER.size), ('table', len(table_b)), ('code_lengths', 256), ('alpha_beta', 8 * nbuckets),
        ('points', 4 * len(pts_np)), ('raw', 4 * n_raw_params), ('buffers', 4 * n_buf),
        ('chunk_offsets', len(body[6])), ('bitstream', len(body[7]))])
    if b_list is not None:              # the reference's bucket term per tensor, summed exactly: [b] * T gives the scalar's value
        bucket_term = float(sum(fractions.Fraction(n, b) for n, b in zip(ns, b_list)) * 8)
    else:
        bucket_term = nsym / bucket_size * 8 if bucket_size is not None else 0
    ref = n_raw_params * 4 + mean_bits * nsym / 8 + bucket_term
    return {'path': str(path), 'sections': sections, 'file_bytes': sum(sections.values()), 'coding': CODINGS[coding],
            'mode': MODES[mode], 'mean_bit_length': mean_bits, 'code_bits': code_bits, 'quantized_elements': nsym,
            'buckets': nbuckets, 'chunks': nchunks, 'max_code_length': max(lens),
            'reference_size_mb': ref / 1e6,
            'symbolizer': MultiTensorSymbols.ENTRY_POINT if one_launch else 'per_tensor'}


def _pack_table(entries):
    out = bytearray()
    for name, kind, shape, numel, bucket, levels, offset, count, first_point, first_chunk in entries:
        nb = name.encode('utf-8')
        if len(nb) > 0xffff or len(shape) > 255:
            raise ValueError('tensor name or rank too large for the table: %r' % name)
        out += ENTRY.pack(len(nb), kind, len(shape)) + nb + struct.pack('<%dQ' % len(shape), *shape)
        out += ENTRY_TAIL.pack(numel, bucket, levels, offset, count, first_point, first_chunk)
    out += b'\0' * (-len(out) % 4)
    return bytes(out)


# ---------------------------------------------------------------- read
class _File(object):
    pass


def _bad(msg):
    raise ValueError('not a valid compressed checkpoint: %s' % msg)


def _parse(data, check_crc=True):
    if len(data) < HEADER.size:
        _bad('shorter than its header')
    (magic, version, coding, mode, chunk, ntensors, max_len, single, table_bytes, nsym, nbuckets, npoints, nraw, nchunks,
     nwords, crc, _res) = HEADER.unpack_from(data, 0)
    if magic != MAGIC or version != VERSION:
        _bad('bad magic or version')
    if coding >= len(CODINGS) or mode >= len(MODES) or chunk != CHUNK or max_len > MAX_CODE_LEN or table_bytes % 4:
        _bad('bad header fields')
    f = _File()
    f.coding, f.mode, f.single, f.nsym, f.nbuckets, f.npoints, f.nraw, f.nchunks, f.nwords = \
        coding, mode, single, nsym, nbuckets, npoints, nraw, nchunks, nwords
    sizes = [table_bytes, 256, 4 * nbuckets, 4 * nbuckets, 4 * npoints, 4 * nraw, 4 * (nchunks + 1) if nchunks else 0, 4 * nwords]
    if HEADER.size + sum(sizes) != len(data):
        _bad('size %d does not match its header (%d)' % (len(data), HEADER.size + sum(sizes)))
    offs = np.cumsum([HEADER.size] + sizes).tolist()
    f.sections = collections.OrderedDict(zip(('table', 'code_lengths', 'alpha', 'beta', 'points', 'raw', 'chunk_offsets',
                                              'bitstream'), zip(offs[:-1], sizes)))
    if check_crc and zlib.crc32(memoryview(data)[HEADER.size:]) != crc:
        _bad('checksum mismatch (corrupted or truncated)')
    # the table
    pos, end = HEADER.size, HEADER.size + table_bytes
    f.entries = []
    try:
        for _ in range(ntensors):
            ln, kind, ndim = ENTRY.unpack_from(data, pos)
            pos += ENTRY.size
            name = bytes(data[pos:pos + ln]).decode('utf-8')
            pos += ln
            shape = struct.unpack_from('<%dQ' % ndim, data, pos)
            pos += 8 * ndim
            numel, bucket, levels, offset, count, first_point, first_chunk = ENTRY_TAIL.unpack_from(data, pos)
            pos += ENTRY_TAIL.size
            f.entries.append(dict(name=name, kind=kind, shape=tuple(shape), numel=numel, bucket=bucket, levels=levels,
                                  offset=offset, count=count, first_point=first_point, first_chunk=first_chunk))
    except (struct.error, UnicodeDecodeError):
        _bad('truncated tensor table')
    if pos > end or any(data[pos:end]):
        _bad('tensor table overruns its section')
    f.lens = list(bytes(data[offs[1]:offs[1] + 256]))
    _validate(f)
    return f


def _validate(f):
    sq = nb = npt = ch = 0
    raw_seen = 0
    for e in f.entries:
        if e['kind'] not in (KIND_RAW, KIND_QUANTIZED, KIND_BUFFER) or int(np.prod(e['shape'], dtype=np.int64)) != e['numel']:
            _bad('bad entry %r' % e['name'])
        if e['kind'] == KIND_QUANTIZED:
            n = e['numel']
            bucket = e['bucket'] or None
            if (e['offset'], e['count'], e['first_chunk']) != (nb, _nbuckets(n, bucket), ch):
                _bad('inconsistent offsets of %r' % e['name'])
            if not 1 <= e['levels'] <= 256 or (f.mode == 0 and e['levels'] < 2):
                _bad('bad levels of %r' % e['name'])
            if f.mode == 1:
                if e['first_point'] != npt:
                    _bad('inconsistent points of %r' % e['name'])
                npt += e['levels']
            nb += e['count']
            ch += -(-n // CHUNK)
            sq += n
        else:
            if e['offset'] != raw_seen or e['count'] != e['numel']:
                _bad('inconsistent raw offsets of %r' % e['name'])
            raw_seen += e['numel']
    if (sq, nb, ch, raw_seen) != (f.nsym, f.nbuckets, f.nchunks, f.nraw) or (f.mode == 1 and npt != f.npoints):
        _bad('table does not match the header')
    if f.coding == 0 and f.nsym:
        _bad('quantized elements without a code')
    if f.coding:
        if f.single >= 0:
            if f.single > 255 or any(f.lens) or f.nwords:
                _bad('bad one-symbol code')
        elif not _kraft_complete(f.lens):
            _bad('code lengths do not form a complete prefix code')


def read_header(path):
    """Names, shapes, kinds, coding and section sizes of a compressed checkpoint, without decoding it."""
    with open(path, 'rb') as fh:
        data = fh.read()
    f = _parse(data, check_crc=False)
    kinds = {KIND_RAW: 'raw', KIND_QUANTIZED: 'quantized', KIND_BUFFER: 'buffer'}
    return {'coding': CODINGS[f.coding], 'mode': MODES[f.mode], 'chunk': CHUNK, 'max_code_length': max(f.lens),
            'code_lengths': f.lens, 'quantized_elements': f.nsym, 'buckets': f.nbuckets, 'chunks': f.nchunks,
            'file_bytes': len(data), 'sections': collections.OrderedDict((k, v[1]) for k, v in f.sections.items()),
            'tensors': [{'name': e['name'], 'shape': e['shape'], 'kind': kinds[e['kind']], 'numel': e['numel'],
                         'bucket_size': e['bucket'] or None, 'levels': e['levels'] if e['kind'] == KIND_QUANTIZED else None}
                        for e in f.entries]}


def _targets(out):
    if out is None:
        return None
    if isinstance(out, torch.nn.Module):
        d = collections.OrderedDict(out.named_parameters())
        d.update(out.named_buffers())
        return d
    if isinstance(out, collections.abc.Mapping):
        return out
    raise TypeError('out must be a name -> tensor mapping or an nn.Module')


def load_compressed(path, device=None, out=None):
    """name -> fp32 tensor of a compressed checkpoint, in the original shapes (parameters, then buffers).  device: where to
    decode (None: the device of `out`, else the CPU); a HIP device decodes with libqd_hip.so in one launch, the CPU with
    libqd_host.so.  out: a state dict or module whose existing contiguous fp32 tensors are written in place."""
    with open(path, 'rb') as fh:
        data = fh.read()
    f = _parse(data)
    targets = _targets(out)
    if device is None:
        device = next(iter(targets.values())).device if targets else torch.device('cpu')
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    if device.type not in ('cuda', 'cpu'):
        raise ValueError('decode on a HIP device or on the CPU')
    res = collections.OrderedDict()
    for e in f.entries:
        if targets is not None:
            if e['name'] not in targets:
                raise ValueError('out has no tensor %r' % e['name'])
            t = targets[e['name']]
            t = t.data if isinstance(t, torch.nn.Parameter) else t
            if (t.dtype != torch.float32 or t.device != device or not t.is_contiguous() or tuple(t.shape) != e['shape']):
                raise ValueError('out[%r] must be a contiguous float32 tensor of shape %s on %s' % (e['name'], e['shape'], device))
        else:
            t = torch.empty(e['shape'], dtype=torch.float32, device=device)
        res[e['name']] = t
    if device.type == 'cuda':
        with torch.cuda.device(device):
            _decode(f, data, res, device)
    else:
        _decode(f, data, res, device)
    return res


def _decode(f, data, res, device):
    cuda = device.type == 'cuda'
    lib = _lib.load() if cuda else _lib.host()
    start = f.sections['alpha'][0]
    body = torch.frombuffer(bytearray(data[start:]) if len(data) > start else bytearray(4), dtype=torch.uint8)
    if cuda:
        body = body.to(device)

    def sect(name):
        o, n = f.sections[name]
        return body[o - start:o - start + n].view(torch.float32 if name in ('alpha', 'beta', 'points', 'raw') else torch.int32)

    raw = sect('raw')
    for e in f.entries:
        if e['kind'] != KIND_QUANTIZED and e['numel']:
            res[e['name']].view(-1).copy_(raw[e['offset']:e['offset'] + e['numel']])
    q = [e for e in f.entries if e['kind'] == KIND_QUANTIZED]
    if not f.nchunks:
        return
    alpha, beta, pts = sect('alpha'), sect('beta'), sect('points')
    chunk_words, words = sect('chunk_offsets'), sect('bitstream')
    cw = np.frombuffer(data, dtype='<u4', count=f.nchunks + 1, offset=f.sections['chunk_offsets'][0])
    d = np.diff(cw.astype(np.int64))
    if cw[0] != 0 or int(cw[-1]) != f.nwords or (d < 0).any() or (d > CHUNK).any():
        _bad('bad chunk offsets')
    table = (_lib.QdHufTensor * len(q))()
    for j, e in enumerate(q):
        t = table[j]
        t.y, t.n, t.first_chunk, t.first_bucket = res[e['name']].data_ptr(), e['numel'], e['first_chunk'], e['offset']
        t.first_point, t.bucket, t.levels, t.nonuniform = e['first_point'], e['bucket'], e['levels'], f.mode
        if e['bucket'] and e['numel'] < e['bucket']:
            t.bucket = 0
    code = canonical_code(f.lens, f.single)
    ptr = lambda x: x.data_ptr() if x.numel() else None      # noqa: E731
    if cuda:
        table_d = _lib.upload_struct(table, device)
        code_d = _lib.upload_struct(code, device)
        _lib.check(lib.qd_huffman_decode_f32(ptr(words), f.nwords, chunk_words.data_ptr(), table_d.data_ptr(), len(q), f.nchunks,
                                             code_d.data_ptr(), alpha.data_ptr(), beta.data_ptr(), ptr(pts),
                                             _lib.stream_ptr(device)), lib)
        _lib.mark_written([res[e['name']] for e in q])
    else:
        _lib.check(lib.qd_huffman_decode_f32(ptr(words), f.nwords, chunk_words.data_ptr(), ctypes.addressof(table), len(q),
                                             f.nchunks, ctypes.addressof(code), alpha.data_ptr(), beta.data_ptr(), ptr(pts), None), lib)
