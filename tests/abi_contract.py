"""The memory contract of the C ABI (include/qd_hip.h), held at every entry point outside the Huffman codec and the
multi-tensor STE (tests/huffman_cases.py and tests/test_hip_multi_ste.py hold those two): shared by
tests/test_abi_contract_host.py (libqd_host.so, no GPU) and tests/test_hip_abi_contract.py (libqd_hip.so, and both libraries
against each other).  A plain helper module: no fixtures, nothing runs on import but the table of groups.

What the header promises and no value comparison through the Python API can see:
  - fp32 data pointers need 4-byte alignment and nothing more: every array of a call sits at its own 16-byte phase;
  - outputs hold exactly n / num_buckets / qd_padded_length(n, bucket) elements: every array lies in a flat buffer of its own
    between two guard bands (GUARD bytes), outputs are pre-filled with a sentinel no arithmetic produces, and the guards of
    inputs hold values that change a result they are read into (NaN and +-3e38 for floats, a valid index for indices);
  - the workspace needs no initialisation: every call runs on a workspace of zero bytes, of 0xFF bytes and of the residue of
    larger calls of other entry points, and must give the same bits each time; the workspace has exactly the documented size
    and guards of its own, one byte less must return QD_ERR_WORKSPACE_TOO_SMALL with every output untouched;
  - "may alias" and "optional outputs may be NULL" give the out-of-place / all-outputs result.

A Case is ONE call: the entry point, its arguments in the header's order (scalars, Ref(name) of a placed array, None, WS /
WSB / STREAM) and `expect`, the reference of every written array -- oracle/oracle_c.py and oracle/oracle_np.py, the functions
the parity suite compares with, plain numpy where the oracle has none.  A Group is the list of cases that reach one path of
one launcher (csrc/qd_plan.h: plan_transform; every group names the kernel(s) it reaches, and tests/test_transform_plan.py
holds the plan to that); the two test files parametrise over groups.  Everything is compared bit for bit; the K6 sums go
through errlog.check_sum (their three runs must still agree bit for bit).

Every generator takes a `variant`: 0 is the data above, 1 and 2 are the same cases -- tags, entry points, shapes, phases, by-value
arguments -- on other array contents (vary()).  run_case_captured records the call of a case once, on variant 0, into a hipGraph
and replays it on the others (tests/test_hip_capture_abi.py); CAPTURE, at the end, is the ledger of where each entry point of
the header is captured."""
import collections
import math

import numpy as np
import torch

import errlog
from oracle import oracle_c as oc
from oracle import oracle_np as onp
from quantized_distillation_amd import _lib

GUARD = 64                           # bytes of guard band on both sides of every array
F_SENT = 0x7FC5A5A5                  # a quiet NaN with a payload of its own: no arithmetic produces it
B_SENT = 0xEE                        # uint8 / int64 / uint64 outputs: 0xEE bytes (int64 -1229782938247303442: never an index or a count)
ERR_INVALID, ERR_WS, ERR_UNSUPPORTED = -1, -2, -3

F32, U8, I64, U64, F64 = (np.dtype(t) for t in ('float32', 'uint8', 'int64', 'uint64', 'float64'))

Arr = collections.namedtuple('Arr', 'role dtype data n phase guard valid_max')
Ref = collections.namedtuple('Ref', 'name')
Sum = collections.namedtuple('Sum', 'want abs_terms kind')          # an output compared through errlog.check_sum
Near = collections.namedtuple('Near', 'want rtol')                  # the absnorm norm (the bound of test_abs_scaling_intended_math)
WS, WSB, STREAM = 'WS', 'WSB', 'STREAM'
Case = collections.namedtuple('Case', 'tag entry arrays args expect ws_bytes uses_ws rc fused_mode')
Group = collections.namedtuple('Group', 'id entry path make host')


def inp(data, phase=0, guard='float'):
    """An input: `data` at `phase` bytes into a 16-byte granule; guard 'float' (NaN, 3e38, NaN, -3e38), 'grad' (+-3e38), or
    ('index', v): the valid index v."""
    data = np.ascontiguousarray(data)
    return Arr('in', data.dtype, data, data.size, phase, guard, None)


def inout(data, phase=0, guard='float'):
    """An input the call may write (an aliased output, K8's w and grad)."""
    data = np.ascontiguousarray(data)
    return Arr('inout', data.dtype, data, data.size, phase, guard, None)


def out(dtype, n, phase=0, valid_max=None):
    """An output of n elements, pre-filled with the sentinel.  valid_max: the largest value a uint8 output may hold (the
    sentinel check runs only where it is below B_SENT)."""
    return Arr('out', np.dtype(dtype), None, int(n), phase, 'sentinel', valid_max)


def case(tag, entry, arrays, args, expect, ws_bytes=None, uses_ws=False, rc=0, fused_mode=None):
    """uses_ws: the call carves the workspace (libqd_hip.so), so one byte less than the documented size must be refused."""
    return Case(tag, entry, collections.OrderedDict(arrays), list(args), expect, ws_bytes, uses_ws, rc, fused_mode)


# ---------------------------------------------------------------- placement
def _pattern(arr):
    if arr.role == 'out':
        return np.array([F_SENT], np.uint32).view(F32) if arr.dtype == F32 else np.full(1, B_SENT, U8).repeat(arr.dtype.itemsize).view(arr.dtype)
    g = arr.guard
    if g == 'float':
        big = 3e38 if arr.dtype == F32 else 1e308
        return np.array([np.nan, big, np.nan, -big], arr.dtype)
    if g == 'grad':
        return np.array([3e38, -3e38], arr.dtype)
    assert g[0] == 'index', g
    return np.array([g[1]], arr.dtype)


class Placed(object):
    """One array inside a flat buffer of its own: GUARD bytes (at least) before and behind it, the payload `phase` bytes into
    a 16-byte granule.  `image` is what the buffer held before the call."""

    def __init__(self, arr, device):
        self.arr = arr
        isz = arr.dtype.itemsize
        self.nbytes = arr.n * isz
        total = GUARD + 32 + self.nbytes + GUARD + 16
        self.buf = torch.empty(total, dtype=torch.uint8, device=device)
        base = self.buf.data_ptr()
        self.off = GUARD + (-(base + GUARD)) % 16 + arr.phase
        assert (base + self.off - arr.phase) % 16 == 0 and self.off >= GUARD and total - self.off - self.nbytes >= GUARD
        pat = _pattern(arr)
        img = np.full(total, B_SENT, np.uint8)
        s = self.off % isz
        cnt = (total - s) // isz
        first = (self.off - s) // isz
        img[s:s + cnt * isz] = pat[(np.arange(cnt) - first) % len(pat)].view(np.uint8)
        if arr.data is not None:
            img[self.off:self.off + self.nbytes] = arr.data.reshape(-1).view(np.uint8)
        self.image = img
        self.buf.copy_(torch.from_numpy(img.copy()))
        self.ptr = base + self.off

    def fill(self, data_bytes):
        """(the workspace) new contents of the payload, guards unchanged."""
        self.image[self.off:self.off + self.nbytes] = data_bytes
        self.buf.copy_(torch.from_numpy(self.image.copy()))

    def reload(self, arr):
        """(a replay) the contents of `arr`, the same array of another variant, in the SAME buffer at the same address: its
        data, or the sentinel for an output; guards unchanged."""
        old = self.arr
        assert (arr.role, arr.dtype, arr.n, arr.phase, arr.guard) == (old.role, old.dtype, old.n, old.phase, old.guard)
        self.arr = arr
        if arr.data is not None:
            payload = arr.data.reshape(-1).view(np.uint8)
        else:
            payload = np.resize(_pattern(arr).view(np.uint8), self.nbytes)
        self.fill(payload)

    def read(self, tag, name):
        """The payload after the call; the guards must hold what they held, an input all of it."""
        got = self.buf.cpu().numpy()
        lo, hi = self.off, self.off + self.nbytes
        assert np.array_equal(got[:lo], self.image[:lo]), (tag, name, 'written in front of the array', self._where(got, 0, lo))
        assert np.array_equal(got[hi:], self.image[hi:]), (tag, name, 'written behind the array', self._where(got, hi, len(got)))
        if self.arr.role == 'in':
            assert np.array_equal(got[lo:hi], self.image[lo:hi]), (tag, name, 'an input was written over')
        return got[lo:hi].copy().view(self.arr.dtype)

    def _where(self, got, lo, hi):
        bad = np.nonzero(got[lo:hi] != self.image[lo:hi])[0]
        return 'bytes %d .. %d relative to the array' % (lo + bad[0] - self.off, lo + bad[-1] - self.off) if len(bad) else ''

    def untouched(self, payload):
        return np.array_equal(payload.view(np.uint8), self.image[self.off:self.off + self.nbytes])

    def assert_no_sentinel(self, payload, tag, name):
        assert_no_sentinel(self.arr, payload, tag, name)


def assert_no_sentinel(a, payload, tag, name):
    """Every element of the output `payload` (described by the Arr `a`) was written."""
    if a.role != 'out' or len(payload) == 0:
        return
    if a.dtype == F32:
        left = payload.view(np.uint32) == F_SENT
    elif a.dtype == U8:
        if a.valid_max is None or a.valid_max >= B_SENT:
            return
        left = payload == B_SENT
    else:
        left = (payload.view(np.uint8).reshape(-1, a.dtype.itemsize) == B_SENT).all(axis=1)
    assert not left.any(), (tag, name, '%d elements never written, first at %d' % (left.sum(), np.nonzero(left)[0][0]))


# ---------------------------------------------------------------- the workspace and what larger calls leave in it
_residue = {}


def _hostile(n, seed):
    rng = np.random.RandomState(seed)
    g = (rng.randn(n) * 1e37).astype(np.float32)
    g[::7] = 3e38
    g[3::11] = -3e38
    return g


def residue_image(lib, device):
    """The bytes a full-size workspace holds after larger calls of the entry points that carve it: K6 (k = 1024: the whole
    partial-row region), the single-bucket arg-min/max, the mean and the three-launch K1 (in place, so never fused), each over
    300001 elements of +-3e38 and 1e37-scale values -- inf and NaN partials, large int64 positions."""
    device = torch.device(device)
    key = device.type
    if key in _residue:
        return _residue[key]
    nbytes = int(lib.qd_workspace_bytes())
    if device.type != 'cuda':
        img = ((np.arange(nbytes) * 37 + 11) % 251).astype(np.uint8)        # libqd_host.so takes no scratch from the caller
    else:
        n, k = 300001, 1024
        st = _lib.stream_ptr(device)
        ws = torch.full((nbytes,), 0x3C, dtype=torch.uint8, device=device)
        g = torch.from_numpy(_hostile(n, 1)).to(device)
        idx = torch.from_numpy(np.random.RandomState(2).randint(0, k, n).astype(np.int64)).to(device)
        one = torch.full((1,), 3e38, device=device)
        gp = torch.empty(k, device=device)
        ai = torch.empty(2, dtype=torch.int64, device=device)
        _lib.check(lib.qd_point_grad_f32(g.data_ptr(), idx.data_ptr(), 8, one.data_ptr(), n, 0, k, gp.data_ptr(), ws.data_ptr(), nbytes, st))
        _lib.check(lib.qd_bucket_argminmax_f32(g.data_ptr(), n, 0, None, 0, 0.0, ai.data_ptr(), ai.data_ptr() + 8, ws.data_ptr(), nbytes, st))
        _lib.check(lib.qd_mean_f32(g.data_ptr(), n, gp.data_ptr(), ws.data_ptr(), nbytes, st))
        _lib.check(lib.qd_uniform_f32(g.data_ptr(), g.data_ptr(), n, 0, 16, None, None, None, None, 0, 0.0, 0, 0, ws.data_ptr(), nbytes, st))
        torch.cuda.synchronize(device)
        img = ws.cpu().numpy().copy()
    _residue[key] = img
    return img


FILLS = ('zero', 'ff', 'residue')


def _ws_bytes(fill, nbytes, lib, device):
    if fill == 'zero':
        return np.zeros(nbytes, np.uint8)
    if fill == 'ff':
        return np.full(nbytes, 0xFF, np.uint8)
    return np.resize(residue_image(lib, device), nbytes)


# ---------------------------------------------------------------- one case through one library
def _call(c, lib, device, placed, ws, ws_bytes, sync=True, args=None):
    """sync=False: the call only, no host synchronisation (inside a stream capture there can be none); args: instead of
    c.args."""
    argv = []
    for a in (c.args if args is None else args):
        if isinstance(a, Ref):
            argv.append(placed[a.name].ptr)
        elif a is WS:
            argv.append(ws.ptr if ws is not None else None)
        elif a is WSB:
            argv.append(ws_bytes)
        elif a is STREAM:
            argv.append(_lib.stream_ptr(device) if device.type == 'cuda' else None)
        elif isinstance(a, np.ndarray):                    # a HOST array (the ranks of K10)
            argv.append(a.ctypes.data)
        else:
            argv.append(a)
    rc = getattr(lib, c.entry)(*argv)
    if sync and device.type == 'cuda':
        torch.cuda.synchronize(device)
    return rc


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _compare(c, name, got, want):
    if isinstance(want, Sum):
        errlog.check_sum(want.kind, got, want.want, want.abs_terms, (c.entry, c.tag), n_terms=None)
    elif isinstance(want, Near):
        assert np.allclose(got, want.want, rtol=want.rtol, atol=0), (c.entry, c.tag, name)
    else:
        want = np.ascontiguousarray(want).reshape(-1)
        assert want.dtype == got.dtype and want.shape == got.shape, (c.entry, c.tag, name, want.dtype, got.dtype, want.shape, got.shape)
        if not _same(got, want):
            diff = (got.view(np.uint8).reshape(len(got), -1) != want.view(np.uint8).reshape(len(want), -1)).any(axis=1)
            if want.dtype.kind == 'f':                     # a NaN for a NaN: the header leaves its sign and payload open
                diff &= ~(np.isnan(got) & np.isnan(want))  # (no case of variant 0 expects one; replay and eager call are
            bad = np.nonzero(diff)[0]                      # compared with _same, payloads included)
            if len(bad) == 0:
                return
            raise AssertionError((c.entry, c.tag, name, '%d of %d elements differ from the reference, first at %d: %r != %r'
                                  % (len(np.unique(bad)), len(got), bad[0], got[bad[0]], want[bad[0]])))


def run_case(c, lib, device, fills=FILLS):
    """Place the arrays of the case, call the entry point once per workspace fill and hold it to the contract.  Returns the
    written arrays (name -> payload) of the first fill; the others gave the same bits."""
    device = torch.device(device)
    tag = (c.entry, c.tag)
    nbytes = c.ws_bytes if c.ws_bytes is not None else int(lib.qd_workspace_bytes())
    has_ws = any(a is WS for a in c.args)                  # not `in`: an argument may be a numpy array (the ranks of K10)
    ws_arr = Arr('ws', U8, None, nbytes, 0, 'sentinel', None)
    want = None
    first = None
    prev_mode = lib.qd_set_single_fused_mode(c.fused_mode) if c.fused_mode is not None else None
    try:
        for fill in (fills if has_ws else fills[:1]):
            placed = collections.OrderedDict((name, Placed(a, device)) for name, a in c.arrays.items())
            ws = None
            if has_ws:
                ws = Placed(ws_arr._replace(role='out'), device)
                ws.fill(_ws_bytes(fill, nbytes, lib, device))
            if c.rc == 0 and c.uses_ws and device.type == 'cuda':
                # one byte below the documented minimum: refused before anything is written
                rc = _call(c, lib, device, placed, ws, nbytes - 1)
                assert rc == ERR_WS, (tag, fill, 'a workspace one byte short returned %d' % rc)
                for name, p in placed.items():
                    assert p.untouched(p.read(tag, name)), (tag, name, 'written by a refused call')
            rc = _call(c, lib, device, placed, ws, nbytes)
            assert rc == c.rc, (tag, fill, 'returned %d, expected %d' % (rc, c.rc))
            if c.rc != 0:
                _assert_untouched(placed, ws, tag)
                return collections.OrderedDict()
            if want is None:
                want = c.expect()
            got = _held(c, placed, ws, want)
            if first is None:
                first = got
            else:
                for name in got:
                    assert _same(got[name], first[name]), (tag, name, 'differs between workspace fills %s and %s' % (fills[0], fill))
    finally:
        if prev_mode is not None:
            lib.qd_set_single_fused_mode(prev_mode)
    return first


def _assert_untouched(placed, ws, tag):
    """After a refused call: guards and payloads as they were."""
    if ws is not None:
        ws.read(tag, 'workspace')
    for name, p in placed.items():
        assert p.untouched(p.read(tag, name)), (tag, name, 'written by a refused call')


def _held(c, placed, ws, want):
    """After a call (or a replay) of the case `c`: guards intact around every array and the workspace, inputs unchanged, no
    sentinel left in an output, outputs equal to `want` (c.expect()) through the comparison of their kind.  Returns the written
    arrays, name -> payload."""
    tag = (c.entry, c.tag)
    if ws is not None:
        ws.read(tag, 'workspace')
    got = collections.OrderedDict()
    for name, p in placed.items():
        payload = p.read(tag, name)
        if p.arr.role != 'in':
            p.assert_no_sentinel(payload, tag, name)
            got[name] = payload
    assert set(want) <= set(got), (tag, sorted(want), sorted(got))
    for name, w in want.items():
        _compare(c, name, got[name], w.fn(got['norm']) if isinstance(w, AfterNorm) else w)
    for name in got:                                       # an 'inout' array the case expects nothing of stays as it was
        if name not in want:
            assert placed[name].untouched(got[name]), (tag, name, 'written, and the case expects no change')
    return got


def run_group(group, lib, device, fills=FILLS, keep_mode=True, variant=0):
    """Every case of the group through `lib`; keep_mode=False runs the cases of a qd_set_single_fused_mode group in the
    library's only mode (libqd_host.so has no such switch)."""
    return [(c, run_case(c if keep_mode else c._replace(fused_mode=None), lib, device, fills)) for c in cases_of(group, lib, variant)]


def same_results(a, b):
    """Two run_group results (of the two libraries): the same arrays, bit for bit."""
    assert len(a) == len(b)
    for (ca, ra), (cb, rb) in zip(a, b):
        assert ca.tag == cb.tag and list(ra) == list(rb), (ca.tag, cb.tag)
        for name in ra:
            if ca.entry == 'qd_point_grad_f32':
                continue                                        # fp32 sums in another order: each is held to the oracle
            assert _same(ra[name], rb[name]), (ca.entry, ca.tag, name, 'libqd_hip.so and libqd_host.so differ')


# ---------------------------------------------------------------- record once, replay on other data
REPLAY_ORDER = (1, 2, 0, 1)                  # the variants a recorded launch is replayed on; replay i takes FILLS[i % 3]
_side = {}


def side_stream(device):
    """The one stream every captured call of this module is made on."""
    device = torch.device(device)
    if device not in _side:
        _side[device] = torch.cuda.Stream(device)
    return _side[device]


class recording(object):
    """torch.cuda.graph(graph, stream=side_stream(device)) without the gc.collect() and empty_cache() of its __enter__ (20 ms
    per capture, and the codec group alone records 900): device-wide synchronise, begin the capture on the side stream, end
    it on the way out.  Nothing is allocated inside: every buffer is placed before."""

    def __init__(self, graph, device):
        self.graph, self.ctx = graph, torch.cuda.stream(side_stream(device))

    def __enter__(self):
        torch.cuda.synchronize()
        self.ctx.__enter__()
        self.graph.capture_begin()

    def __exit__(self, *exc):
        self.graph.capture_end()
        self.ctx.__exit__(*exc)


def _place(c, device, lib, fill):
    """The arrays of the case and its workspace (None without one) at exactly its documented size, as run_case places them."""
    placed = collections.OrderedDict((name, Placed(a, device)) for name, a in c.arrays.items())
    ws = None
    nbytes = c.ws_bytes if c.ws_bytes is not None else int(lib.qd_workspace_bytes())
    if any(a is WS for a in c.args):
        ws = Placed(Arr('out', U8, None, nbytes, 0, 'sentinel', None), device)
        ws.fill(_ws_bytes(fill, nbytes, lib, device))
    return placed, ws, nbytes


def _same_outputs(a, b, tag, what):
    assert list(a) == list(b), (tag, what)
    for name in a:
        assert _same(a[name], b[name]), (tag, name, what)


def run_case_captured(c_variants, lib, device, args_for=None, refused=()):
    """Record the call of a case ONCE, on variant 0, and replay it on the other variants: c_variants = the same case of
    variants 0, 1, 2 (cases_of).  What a replay can get wrong and no eager call shows: a value derived from the data on the
    host and frozen into the graph as a launch argument, a workspace slot that only the recording-time call (or nobody)
    initialises, a launch plan that differs under capture, host memory read again at replay time.

      1. every call is made on side_stream(device); one eager warm-up call of variant 0 into the placed buffers;
      2. the call is recorded (and not run), host arrays (the ranks of K10) from a copy that is overwritten and dropped at once;
      3. replays on variants 1, 2, 0, 1 written into the SAME buffers: inputs rewritten, outputs back to their sentinel, the
         workspace payload to the next of FILLS; each is held to the checks of run_case (_held) against ITS variant's expect();
      4. variants 1 and 2 also run eagerly into a second set of buffers: replay and eager call agree bit for bit (K6's sums,
         the absnorm norm and NaN payloads included: the launches are deterministic and share their geometry -- where the
         eager call takes the one-launch single-bucket kernel and the captured one cannot, both equal the oracle bit for bit);
      5. two more replays back to back, nothing in between, on what the last one left: for a case without in-place
         arrays the bits of the last replay again, for every case the bits of two more eager calls on the eager buffers;
      6. the graph is dropped.

    args_for(c, placed) -> argument list, called on the host BEFORE the recording and before every eager call (default:
    c.args): the control of tests/test_hip_capture_abi.py derives a by-value argument from the data there.
    refused: cases with rc != 0, called inside the open capture in front of the recorded call: each returns its code and
    writes nothing (now or at a replay), and the capture goes on."""
    device = torch.device(device)
    c0 = c_variants[0]
    tag = (c0.entry, c0.tag)
    assert c0.rc == 0 and c0.fused_mode is None and device.type == 'cuda', tag
    args_for = args_for or (lambda c, placed: c.args)
    wants, eager1 = {}, None
    residue_image(lib, device)                            # (its own launches and synchronisation: never inside a capture)
    with torch.cuda.stream(side_stream(device)):
        placed, ws, nbytes = _place(c0, device, lib, FILLS[-1])
        turned_down = [(r,) + _place(r, device, lib, FILLS[0]) for r in refused]
        assert _call(c0, lib, device, placed, ws, nbytes, args=args_for(c0, placed)) == 0, (tag, 'warm-up')
        for name, p in placed.items():
            p.reload(c0.arrays[name])
        rec_args = [a.copy() if isinstance(a, np.ndarray) else a for a in args_for(c0, placed)]
    graph = torch.cuda.CUDAGraph()
    with recording(graph, device):
        codes = [_call(r, lib, device, rp, rws, rn, sync=False) for r, rp, rws, rn in turned_down]
        rc = _call(c0, lib, device, placed, ws, nbytes, sync=False, args=rec_args)
    for a in rec_args:
        if isinstance(a, np.ndarray):
            a.fill(-1)                                    # frozen at record time: the replays must not look here again
    del rec_args
    assert rc == 0, (tag, 'the recorded call returned %d' % rc)
    for (r, rp, rws, rn), code in zip(turned_down, codes):
        assert code == r.rc, ((r.entry, r.tag), 'inside a capture: returned %d, expected %d' % (code, r.rc))
    with torch.cuda.stream(side_stream(device)):
        for i, v in enumerate(REPLAY_ORDER):
            c = c_variants[v]
            rtag = tag + ('replay %d on variant %d' % (i, v),)
            for name, p in placed.items():
                p.reload(c.arrays[name])
            if ws is not None:
                ws.fill(_ws_bytes(FILLS[i % len(FILLS)], nbytes, lib, device))
            graph.replay()
            torch.cuda.synchronize(device)
            if v not in wants:
                wants[v] = c.expect()
            got = _held(c._replace(tag=rtag[1:]), placed, ws, wants[v])
            if v != 0 and i < 2:
                ep, ews, _ = _place(c, device, lib, FILLS[(i + 1) % len(FILLS)])
                assert _call(c, lib, device, ep, ews, nbytes, args=args_for(c, ep)) == 0, rtag
                eager = _held(c._replace(tag=rtag[1:] + ('eager',)), ep, ews, wants[v])
                _same_outputs(got, eager, rtag, 'the replay and the eager call differ')
                if v == REPLAY_ORDER[-1]:
                    eager1 = (c, ep, ews)
        for r, rp, rws, rn in turned_down:
            _assert_untouched(rp, rws, (r.entry, r.tag, 'refused inside the capture'))
        graph.replay()
        graph.replay()
        torch.cuda.synchronize(device)
        if ws is not None:
            ws.read(tag, 'workspace')
        again = collections.OrderedDict((name, p.read(tag, name)) for name, p in placed.items() if p.arr.role != 'in')
        if not any(p.arr.role == 'inout' for p in placed.values()):
            _same_outputs(again, got, tag, 'two replays back to back differ from the replay before them')
        c, ep, ews = eager1
        for _ in range(2):
            assert _call(c, lib, device, ep, ews, nbytes, args=args_for(c, ep)) == 0, tag
        if ews is not None:
            ews.read(tag, 'workspace')
        thrice = collections.OrderedDict((name, p.read(tag, name)) for name, p in ep.items() if p.arr.role != 'in')
        _same_outputs(again, thrice, tag, 'three replays in a row differ from three eager calls in a row')
    del graph
    return got


def run_group_captured(group, lib, device):
    """Every case of the group through run_case_captured.  Its refused cases (rc != 0) record nothing: each is called inside
    the open capture of the next case that does (of K1's first group where the group has none)."""
    cases = list(zip(*(cases_of(group, lib, v) for v in VARIANTS)))
    pending, done = [], 0
    for cv in cases:
        if cv[0].rc != 0:
            pending.append(cv[0])
            continue
        run_case_captured(cv, lib, device, refused=pending)
        pending, done = [], done + 1
    if pending:
        first = next(iter(GROUPS.values()))
        run_case_captured([next(iter(cases_of(first, lib, v))) for v in VARIANTS], lib, device, refused=pending)
    return done + len(pending)


# ---------------------------------------------------------------- inputs
VARIANTS = (0, 1, 2)
BIG, SMALL = 2.0 ** 101, 2.0 ** -61         # alpha outside [2^-60, 2^100]: the IEEE division instead of the bucket-invariant one
FLAVOURS = ('big', 'small', 'nan', 'inf', 'const')
FINITE_FLAVOURS = ('big', 'small', 'const', 'dup')


def vary(x, bucket, seed, variant, finite=False, big=BIG, small=SMALL):
    """Other contents for the array `x` of a case, same shape and type: what a recorded launch is replayed on.
    variant 0: x itself.  variant 1: ordinary data from another seed, scaled by 3 and shifted by 1.  variant 2: the same
    with "path-flipping" buckets -- one scaled by 2^101 and one by 2^-61 (the per-wave choice between the bucket-invariant
    and the IEEE division flips against the recorded run), one with a NaN, one with +inf, one constant (alpha < 1e-10);
    finite=True (inputs whose reference is undefined for NaN / inf: sums): scaled, constant and duplicated buckets only.
    Five or more buckets: the first four and the LAST (the ragged one) get one flavour each, rotated by the seed; fewer:
    every bucket gets one."""
    if variant == 0:
        return x
    n = x.size
    rng = np.random.RandomState((seed * 3 + 104729 * variant) % (1 << 31))
    y = (rng.randn(n) * 3 + 1).astype(np.float32)
    if variant == 1 or n == 0:
        return y
    row = bucket if bucket and n >= bucket else n
    nb = -(-n // row)
    fl = FINITE_FLAVOURS if finite else FLAVOURS
    targets = list(range(nb)) if nb < 5 else [0, 1, 2, 3, nb - 1]
    for j, b in enumerate(targets):
        s = y[b * row:min(n, (b + 1) * row)]
        f = fl[(seed + j) % len(fl)]
        if f == 'big':
            s *= np.float32(big)
        elif f == 'small':
            s *= np.float32(small)
        elif f == 'nan':
            s[len(s) // 2] = np.nan
        elif f == 'inf':
            s[len(s) // 3] = np.inf
        elif f == 'const':
            s[:] = s[0]
        else:
            s[1::2] = s[0::2][:len(s[1::2])]
    return y


def data(n, bucket, seed, const_bucket=True, scale=1.0, variant=0, **how):
    """randn with a few exact ties (two equal maxima and two equal minima in the first bucket, repeated values elsewhere) and,
    from three buckets on, a second bucket of equal values (the alpha < 1e-10 guard).  variant 1 / 2: vary() of it."""
    if variant:
        return vary(np.empty(n, np.float32), bucket, seed, variant, **how)
    x = (np.random.RandomState(seed).randn(n) * scale).astype(np.float32)
    row = bucket if bucket and n >= bucket else n
    if row >= 8:
        first = x[:row]
        first[row // 2] = first.max()
        first[row // 2 + 1] = first.min()
    if n >= 16:
        x[n - 5] = x[n - 9]
        x[5] = x[2]
    if const_bucket and bucket and n >= 3 * bucket:
        x[bucket:2 * bucket] = np.float32(0.25)
    return x


def nbuckets(n, bucket):
    return 1 if (not bucket or n < bucket) else -(-n // bucket)


def padded(n, bucket):
    return n if (not bucket or n < bucket) else -(-n // bucket) * bucket


PHASES = ((0, 4), (8, 12), (4, 4))          # (x, out): aligned x with out at +4; two different non-zero phases; the same one
SIDE = (12, 8, 4)                           # alpha / beta / idx ... of the same three runs: never the phase of x


def lengths(bucket, nfull, tail=2):
    """n % bucket == 0, a last bucket of `tail` (1 .. 3) elements, a last bucket one short of full."""
    return (nfull * bucket, nfull * bucket + tail, nfull * bucket + bucket - 1)


def points(k, seed=7):
    p = np.sort(np.random.RandomState(seed + k).rand(k)).astype(np.float32)
    p[0], p[-1] = 0.0, 1.0
    return p


def _vmean(mean, variant):
    """The device scalar `mean` of a case (an input array like any other): another exact value per variant."""
    return mean if mean is None or not variant else float(np.float32(mean * (1 + 2 * variant) - 0.5))


# ---------------------------------------------------------------- K1: qd_uniform_f32
def k1(tag, x, bucket, levels=16, px=0, pq=4, ps=12, alias=False, want_ab=True, lev_phase=None, mean=None, me=None,
       stochastic=0, seed=0, fused_mode=None, q_null=False, rc=0, variant=0):
    n = x.size
    nb = nbuckets(n, bucket)
    mean = _vmean(mean, variant)
    arrays = [('x', (inout if alias else inp)(x, px))]
    if not alias and not q_null:
        arrays.append(('q', out(F32, n, pq)))
    if want_ab:
        arrays += [('alpha', out(F32, nb, ps)), ('beta', out(F32, nb, (ps + 8) % 16))]
    if lev_phase is not None:
        arrays.append(('lev', out(U8, n, lev_phase, levels - 1)))
    if mean is not None:
        arrays.append(('mean', inp(np.array([mean], np.float32), 8)))
    args = [Ref('x'), None if q_null else Ref('x' if alias else 'q'), n, bucket, levels, Ref('alpha') if want_ab else None,
            Ref('beta') if want_ab else None, Ref('lev') if lev_phase is not None else None,
            Ref('mean') if mean is not None else None, int(me is not None), float(me or 0.0), stochastic, seed, WS, WSB, STREAM]

    def expect():
        kw = dict(max_element=me if me is not None else False, subtract_mean=mean is not None, mean=mean)
        if stochastic:
            rand = np.zeros(padded(n, bucket), np.float32)
            rand[:n] = onp.philox4x32_7_uniform(seed, n)
            with np.errstate(invalid='ignore'):            # (variant 2: inf - inf, 0 x inf in the numpy statement)
                r = onp.uniform_quantize_stochastic(x, levels, rand, bucket or None, **kw)
        else:
            r = oc.uniform_quantize(x, levels, bucket or None, want_idx=False, **kw)
        w = {} if q_null else {'x' if alias else 'q': r['q']}
        if want_ab:
            w.update(alpha=np.asarray(r['alpha'], np.float32).reshape(-1), beta=np.asarray(r['beta'], np.float32).reshape(-1))
        if lev_phase is not None:
            w['lev'] = r['lev'].reshape(-1)[:n].astype(np.uint8)
        return w
    return case(tag, 'qd_uniform_f32', arrays, args, expect, uses_ws=_single_ws(n, bucket), rc=rc, fused_mode=fused_mode)


def _single_ws(n, bucket):
    """The launcher carves the workspace for one bucket of more than 16384 elements (csrc/qd_plan.h: kSingleSmallN)."""
    return nbuckets(n, bucket) == 1 and n > 16384


# ---------------------------------------------------------------- K2 / K3
def k2(tag, x, bucket, px=0, pq=4, ps=12, alias=False, mean=None, me=None, fused_mode=None, variant=0):
    n = x.size
    mean = _vmean(mean, variant)
    nb, npad = nbuckets(n, bucket), padded(n, bucket)
    assert not alias or npad == n
    arrays = [('x', (inout if alias else inp)(x, px))]
    if not alias:
        arrays.append(('u', out(F32, npad, pq)))
    arrays += [('alpha', out(F32, nb, ps)), ('beta', out(F32, nb, (ps + 8) % 16))]
    if mean is not None:
        arrays.append(('mean', inp(np.array([mean], np.float32), 4)))
    args = [Ref('x'), Ref('x' if alias else 'u'), n, bucket, Ref('alpha'), Ref('beta'), Ref('mean') if mean is not None else None,
            int(me is not None), float(me or 0.0), WS, WSB, STREAM]

    def expect():
        r = oc.scale_down(x, bucket or None, max_element=me if me is not None else False, subtract_mean=mean is not None, mean=mean)
        u = np.concatenate([r['u'], np.full(npad - n, r['u'][-1], np.float32)])      # padding: the scaled last element
        return {'x' if alias else 'u': u, 'alpha': r['alpha'], 'beta': r['beta']}
    return case(tag, 'qd_scale_down_f32', arrays, args, expect, uses_ws=_single_ws(n, bucket), fused_mode=fused_mode)


def k3(tag, n, bucket, seed, pu=0, py=4, ps=12, alias=False, mean=None, variant=0):
    nb, npad = nbuckets(n, bucket), padded(n, bucket)
    rng = np.random.RandomState(seed + 5000 * variant)
    u = rng.rand(npad).astype(np.float32)
    alpha = (np.abs(rng.randn(nb)) + 0.1).astype(np.float32)
    beta = rng.randn(nb).astype(np.float32)
    mean = _vmean(mean, variant)
    if variant:
        u, beta = u * np.float32(3.0) + np.float32(1.0), beta * np.float32(3.0) + np.float32(1.0)
    if variant == 2:                                  # plain IEEE u alpha + beta: NaN / inf propagate, 0 x inf = NaN
        u[npad // 2], u[npad // 3], u[0] = np.nan, np.inf, 0.0
        alpha[0] *= np.float32(BIG)
        alpha[-1] *= np.float32(SMALL)
        if nb > 2:
            alpha[1], beta[2] = np.inf, -np.inf
            u[2 * bucket:3 * bucket] = u[2 * bucket]
    arrays = [('u', (inout if alias else inp)(u, pu)), ('alpha', inp(alpha, ps)), ('beta', inp(beta, (ps + 8) % 16))]
    if not alias:
        arrays.append(('y', out(F32, n, py)))
    if mean is not None:
        arrays.append(('mean', inp(np.array([mean], np.float32), 12)))
    args = [Ref('u'), Ref('u' if alias else 'y'), n, bucket, Ref('alpha'), Ref('beta'), Ref('mean') if mean is not None else None, STREAM]

    def expect():
        row = bucket if nb > 1 else npad
        y = onp.inv_scale_down(u.reshape(nb, row), alpha.reshape(nb, 1), beta.reshape(nb, 1), mean or 0.0, n, (n,))
        if alias:
            return {'u': np.concatenate([y, u[n:]])}                 # the padding behind y[n-1] is not part of y
        return {'y': y}
    return case(tag, 'qd_inv_scale_f32', arrays, args, expect)


# ---------------------------------------------------------------- K4: qd_nearest_point_f32
def k4(tag, x, bucket, k=16, mode=0, idx_bytes=8, prescaled=0, px=0, pq=4, ps=12, pidx=0, alias=False, want_idx=True, q_null=False,
       fused_mode=None, rc=0, variant=0):
    n = x.size
    nb = nbuckets(n, bucket)
    pts = points(k, seed=7 + 100 * variant)
    sd = oc.scale_down(x, bucket or None) if prescaled else None
    src = sd['u'] if prescaled else x
    arrays = [('x', (inout if alias else inp)(src, px)), ('points', inp(pts, 8))]
    if not alias and not q_null:
        arrays.append(('q', out(F32, n, pq)))
    if want_idx:
        arrays.append(('idx', out(I64 if idx_bytes == 8 else U8, n, pidx, k - 1)))
    if prescaled:
        arrays += [('alpha', inp(sd['alpha'], ps)), ('beta', inp(sd['beta'], (ps + 8) % 16))]
    else:
        arrays += [('alpha', out(F32, nb, ps)), ('beta', out(F32, nb, (ps + 8) % 16))]
    args = [Ref('x'), prescaled, Ref('points'), k, mode, None if q_null else Ref('x' if alias else 'q'),
            Ref('idx') if want_idx else None, idx_bytes, n, bucket, Ref('alpha'), Ref('beta'), None, 0, 0.0, WS, WSB, STREAM]

    def expect():
        w = {}
        if prescaled:
            idx = (onp.assign_distance if mode == 0 else onp.assign_midpoint)(src, pts)
            row = bucket if nb > 1 else n
            a, b = np.repeat(sd['alpha'], row)[:n], np.repeat(sd['beta'], row)[:n]
            with np.errstate(invalid='ignore'):                # (variant 2: 0 x inf, inf - inf)
                q = ((pts[idx] * a).astype(np.float32) + b).astype(np.float32) + np.float32(0.0)
        else:
            r = oc.nonuniform_quantize(x, pts, bucket or None, 'distance' if mode == 0 else 'midpoint')
            idx, q = r['idx'].reshape(-1), r['q'].reshape(-1)
            w.update(alpha=r['alpha'], beta=r['beta'])
        if not q_null:
            w['x' if alias else 'q'] = q
        if want_idx:
            w['idx'] = idx.astype(np.int64 if idx_bytes == 8 else np.uint8)
        return w
    uses_ws = _single_ws(n, bucket) and not (prescaled and q_null)
    return case(tag, 'qd_nearest_point_f32', arrays, args, expect, uses_ws=uses_ws and rc == 0, rc=rc, fused_mode=fused_mode)


# ---------------------------------------------------------------- the launcher paths of K1 / K2 / K4 (run_transform)
class Path(str):
    """The explanatory text of a launcher path, and as data the kernel(s) it names: `kernels` is what qd_transform_plan must
    return for every case of the group, for K1 / K2 / K4 (mode 0 / 1 / 2) -- one pattern with %d for the mode, or one per mode;
    ' ; ' separates the launches of a sequence.  tests/test_transform_plan.py holds the plan to it; the text is for the reader."""

    def __new__(cls, kernels, text):
        self = str.__new__(cls, text)
        self.kernels = kernels
        return self

    def kernels_of(self, mode):
        pat = self.kernels if isinstance(self.kernels, str) else self.kernels[mode]
        return [k.replace('%d', str(mode)) for k in pat.split(' ; ')]


# (bucket, full buckets, path): plan_transform of csrc/qd_plan.h with 4-byte aligned x / out
BUCKET_PATHS = [
    (64, 10, Path('k_bucket_vec<%d,16,1,4>', 'k_bucket_vec<16,1,4>: 16 buckets per wave tile, ten buckets = one partial tile + the tail block')),
    (128, 10, Path('k_bucket_vec<%d,16,2,2>', 'k_bucket_vec<16,2,2>')),
    (256, 10, Path('k_bucket_vec<%d,16,4,1>', 'k_bucket_vec<16,4,1>')),
    (512, 10, Path('k_bucket_vec<%d,64,2,2>', 'k_bucket_vec<64,2,2>')),
    (1024, 10, Path('k_bucket_vec<%d,64,4,1>', 'k_bucket_vec<64,4,1>')),
    (2048, 10, Path('k_bucket_vec<%d,64,8,1>', 'k_bucket_vec<64,8,1>')),
    (100, 21, Path('k_bucket_chunk<%d,8>', 'k_bucket_chunk: bq = 25 float4, m = 16 buckets per chunk: one whole chunk + 5 leftover full buckets')),
    (36, 61, Path('k_bucket_chunk<%d,8>', 'k_bucket_chunk: bq = 9, m = 56 (48 .. 63 lanes, one bucket each): one chunk + 5 buckets')),
    (33, 65, Path('k_bucket_chunk_any<%d,8>', 'k_bucket_chunk_any: m = 60 buckets per chunk with the lead-in: one chunk + 5 buckets')),
    (7, 261, Path('k_bucket_chunk_any<%d,8>', 'k_bucket_chunk_any: m = 256 (a lane reduces whole buckets alone): one chunk + 5 buckets')),
    (447, 6, Path('k_bucket_chunk_any<%d,8>',
                  'k_bucket_chunk_any: the largest bucket it takes (257 .. 447, no multiple of 4: m = 4 with the lead-in): one chunk + 2 buckets')),
    (509, 6, Path('k_bucket_wave_any<%d,3,1>',
                  'k_bucket_wave_any (nf_max = 127 + 2 + 7): sizes from 448 that are no multiple of 4 return from the wave kernel first, so the '
                  'm < 4 branch of k_bucket_chunk_any once written for 506 .. 511 was dead and is gone (DESIGN.md, findings)')),
    (449, 6, Path(('k_bucket_wave_any<%d,2,1>', 'k_bucket_wave_any<%d,3,1>', 'k_bucket_wave_any<%d,3,1>'),
                  'k_bucket_wave_any: not a multiple of 4, >= 448: nf_max = 112 + 2 + 7')),
    (513, 6, Path('k_bucket_wave_any<%d,3,1>', 'k_bucket_wave_any: the first size above 512')),
    (1000, 6, Path('k_bucket_wave_any<%d,5,1>', 'k_bucket_wave_any: a multiple of 4 that is no multiple of 32 (lead-in from the 128-byte line)')),
    (4097, 5, Path(('k_bucket_wave_any<%d,5,4>', 'k_bucket_wave_any<%d,6,4>', 'k_bucket_wave_any<%d,6,4>'),
                   'k_bucket_wave_any: four waves per bucket (nf_max = 1024 + 2 + 7 = 1033: K1 V = 5, K2 / K4 V = 6, G = 4), odd size')),
    (20000, 3, Path(('k_bucket_wave_any<%d,24,4>', 'k_bucket_wave_any<%d,32,4>', 'k_bucket_generic<%d>'),
                    'k_bucket_wave_any V > 16 (K1: 24, K2: 32; K4: k_bucket_generic): the short last bucket goes to block 0')),
    (100, 3, Path('k_bucket_groups<%d,16>', 'k_bucket_groups<16>: bucket <= 256 with fewer full buckets (3) than a chunk holds (16)')),
    (300, 3, Path('k_bucket_groups<%d,64>', 'k_bucket_groups<64>: 257 .. 16384 (bq = 75, m = 4) with 3 full buckets')),
    (40000, 2, Path('k_bucket_generic<%d>', 'k_bucket_generic: a bucket above 32768')),
]
SINGLE_SMALL = [(1000, Path('k_bucket_generic<%d>', 'k_bucket_generic, one block')),
                (16384, Path('k_bucket_generic<%d>', 'k_bucket_generic, one block: the largest')),
                (16385, Path('k_single_fused<%d,1,4>', 'k_single_fused<V = 1>: the smallest tensor that takes the workspace'))]
SINGLE_LARGE = [(300001, Path('k_single_fused<%d,4,4>', 'k_single_fused<V = 4>')),
                ((1 << 20) + 3, Path('k_minmax_partial ; k_single_apply<%d>', 'k_minmax_partial + k_single_apply (above kFusedMaxN)')),
                ((8 << 20) + 5, Path('k_minmax_partial ; k_minmax_final ; k_single_apply<%d>',
                                     'k_minmax_partial + k_minmax_final + k_single_apply (above 8 Mi elements)'))]
FUSED_MODES = [(0, 'three launches'), (2, 'every block gives up'), (3, 'blocks with blockIdx % 7 == 3 give up'), (4, 'one block gives up')]


def _sweep(make, bucket, nfull, seed, v=0):
    """The three lengths of a bucketed path, each at the three phase combinations."""
    for li, n in enumerate(lengths(bucket, nfull, 1 + (seed + bucket) % 3)):
        x = data(n, bucket, seed + li, variant=v)
        for pi, ((px, pq), ps) in enumerate(zip(PHASES, SIDE)):
            yield make('n=%d x+%d out+%d' % (n, px, pq), x, bucket, px=px, pq=pq, ps=ps, variant=v)


def _transform_groups(name, entry, make, seed):
    groups = []
    for bucket, nfull, path in BUCKET_PATHS:
        groups.append(Group('%s-b%d-nf%d' % (name, bucket, nfull), entry, path,
                            (lambda v=0, b=bucket, f=nfull: _sweep(make, b, f, seed, v)), True))

    def tiny(v=0):
        for n in (1, 2, 3, 5, 255, 257):
            for (px, pq), ps in zip(PHASES[:2], SIDE):
                yield make('n=%d bucket 256 x+%d out+%d' % (n, px, pq), data(n, 256, seed + n, variant=v), 256, px=px, pq=pq, ps=ps, variant=v)
        for n in (1, 2, 3, 5):
            yield make('n=%d no bucket' % n, data(n, 0, seed + n, variant=v), 0, px=4, pq=8, ps=0, variant=v)
    groups.append(Group(name + '-tiny', entry, 'n in {1, 2, 3, 5, bucket - 1, bucket + 1}: one short bucket (k_bucket_generic) / two', tiny, True))
    for n, path in SINGLE_SMALL:
        groups.append(Group('%s-single-%d' % (name, n), entry, path,
                            (lambda v=0, n=n: (make('n=%d x+%d out+%d' % (n, px, pq), data(n, 0, seed + n % 97, variant=v), 0, px=px, pq=pq,
                                                    ps=ps, variant=v) for (px, pq), ps in zip(PHASES, SIDE))), True))
    for n, path in SINGLE_LARGE:
        groups.append(Group('%s-single-%d' % (name, n), entry, path,
                            (lambda v=0, n=n: iter([make('n=%d x+0 out+4' % n, data(n, 0, seed + n % 97, variant=v), 0, px=0, pq=4, ps=12,
                                                         variant=v)])), True))
    for mode, path in FUSED_MODES:
        groups.append(Group('%s-single-70001-mode%d' % (name, mode), entry, 'qd_set_single_fused_mode(%d): %s' % (mode, path),
                            (lambda v=0, m=mode: iter([make('n=70001 mode %d' % m, data(70001, 0, seed + 3, variant=v), 0, px=0, pq=4, ps=12,
                                                            fused_mode=m, variant=v)])),
                            False))
    return groups


def _k4_default(tag, x, bucket, **kw):
    return k4(tag, x, bucket, k=16, mode=0, idx_bytes=8, **kw)


K_SWEEP = (2, 32, 33, 64, 65, 256, 1000)        # byte staging (k <= 32), coarse / fine table (k > 32 midpoint, > 64 vector), uint8 limit
K4_SHAPES = [(256, 10 * 256 + 3), (100, 21 * 100 + 99), (33, 65 * 33 + 2), (1000, 6000 + 1), (0, 1000), (0, 70001)]


def _k1_extra(v=0):
    for bucket, n in ((256, 2563), (33, 65 * 33 + 2), (1000, 6001), (0, 1000), (0, 70001)):
        x = data(n, bucket, 40 + bucket, variant=v)
        yield k1('stochastic n=%d bucket %d' % (n, bucket), x, bucket, px=4, pq=8, ps=0, stochastic=1, seed=0x1234567890ABCDEF)
        yield k1('mean + clamp n=%d bucket %d' % (n, bucket), x, bucket, px=8, pq=4, ps=0, mean=float(np.float32(0.0625)), me=0.8, variant=v)
        yield k1('in place n=%d bucket %d' % (n, bucket), x, bucket, px=4, ps=8, alias=True)
        yield k1('no alpha / beta n=%d bucket %d' % (n, bucket), x, bucket, px=0, pq=12, want_ab=False)
        for lp in (0, 4, 8, 12, 1, 2, 3):
            yield k1('level_idx +%d n=%d bucket %d' % (lp, n, bucket), x, bucket, levels=256 if lp == 0 else 16, px=0, pq=4, ps=12, lev_phase=lp)


def _k1_levels_only(v=0):
    x = data(2563, 256, 50, variant=v)
    yield k1('levels only, x at +4: QD_ERR_UNSUPPORTED', x, 256, px=4, lev_phase=0, q_null=True, rc=ERR_UNSUPPORTED)
    yield k1('levels only, bucket 100: QD_ERR_UNSUPPORTED', x, 100, px=0, lev_phase=0, q_null=True, rc=ERR_UNSUPPORTED)
    for lp in (0, 4, 8, 12):
        yield k1('levels only, level_idx +%d' % lp, x, 256, px=0, lev_phase=lp, q_null=True)
    yield k1('levels only, no alpha / beta', x, 256, px=0, lev_phase=0, q_null=True, want_ab=False)


def _k2_extra(v=0):
    for bucket, n in ((256, 2560), (100, 2100), (33, 65 * 33), (1000, 6000), (0, 1000), (0, 70001)):
        x = data(n, bucket, 60 + bucket, variant=v)
        yield k2('in place n=%d bucket %d' % (n, bucket), x, bucket, px=4, ps=8, alias=True)
        yield k2('mean + clamp n=%d bucket %d' % (n, bucket), x, bucket, px=8, pq=4, ps=0, mean=float(np.float32(0.0625)), me=0.8, variant=v)


def _k4_k(prescaled):
    def make(v=0):
        for si, (bucket, n) in enumerate(K4_SHAPES):
            x = data(n, bucket, 70 + si, variant=v)
            for ki, k in enumerate(K_SWEEP):
                for mode in (0, 1):
                    for ib in ((8, 1) if k <= 256 else (8,)):
                        px, pq = PHASES[(si + ki + mode) % 3]
                        yield k4('k=%d mode %d idx%d n=%d bucket %d x+%d out+%d' % (k, mode, ib, n, bucket, px, pq), x, bucket, k=k,
                                 mode=mode, idx_bytes=ib, prescaled=prescaled, px=px, pq=pq, ps=SIDE[ki % 3],
                                 pidx=0 if ib == 8 else (0, 4, 8, 12)[(ki + mode) % 4], variant=v)
    return make


def _k4_extra(v=0):
    for si, (bucket, n) in enumerate(K4_SHAPES):
        x = data(n, bucket, 80 + si, variant=v)
        yield k4('in place n=%d bucket %d' % (n, bucket), x, bucket, k=16, px=4, ps=8, alias=True, variant=v)
        yield k4('no idx n=%d bucket %d' % (n, bucket), x, bucket, k=40, mode=1, px=0, pq=12, want_idx=False, variant=v)
        yield k4('int64 idx at +8 n=%d bucket %d' % (n, bucket), x, bucket, k=16, px=0, pq=4, pidx=8, variant=v)
        for pidx in (1, 2, 3):
            yield k4('uint8 idx at +%d n=%d bucket %d' % (pidx, n, bucket), x, bucket, k=16, idx_bytes=1, px=8, pq=12, pidx=pidx, variant=v)
        if bucket == 0 or bucket >= 4:
            for ib in (8, 1):
                yield k4('indices only idx%d n=%d bucket %d' % (ib, n, bucket), x, bucket, k=40, mode=1, idx_bytes=ib, prescaled=1,
                         px=4, pidx=0 if ib == 8 else 12, q_null=True, variant=v)


def _k4_indices_only_refused(v=0):
    x = data(2563, 256, 90, variant=v)
    yield k4('indices only, int64 idx at +8: QD_ERR_INVALID_ARGUMENT', x, 256, k=16, prescaled=1, pidx=8, q_null=True, rc=ERR_INVALID)
    yield k4('indices only, uint8 idx at +1: QD_ERR_INVALID_ARGUMENT', x, 256, k=16, idx_bytes=1, prescaled=1, pidx=1, q_null=True, rc=ERR_INVALID)
    yield k4('indices only, buckets of 3 elements: QD_ERR_INVALID_ARGUMENT', data(300, 3, 91, variant=v), 3, k=16, prescaled=1, q_null=True, rc=ERR_INVALID)
    yield k4('indices only, n = 3: QD_ERR_INVALID_ARGUMENT', data(3, 0, 92, variant=v), 0, k=16, prescaled=1, q_null=True, rc=ERR_INVALID)


# ---------------------------------------------------------------- the smaller per-call entry points
def _k3_cases(v=0):
    for bucket, nfull in ((256, 10), (33, 9), (1000, 3)):
        for li, n in enumerate(lengths(bucket, nfull)):
            for (pu, py), ps in zip(PHASES, SIDE):
                yield k3('n=%d bucket %d u+%d y+%d' % (n, bucket, pu, py), n, bucket, 100 + li, pu=pu, py=py, ps=ps,
                         mean=0.125 if li == 1 else None, variant=v)
            yield k3('in place n=%d bucket %d' % (n, bucket), n, bucket, 110 + li, pu=4, ps=0, alias=True, variant=v)
    for n in (1, 2, 3, 5, 255, 257):
        yield k3('n=%d bucket 256' % n, n, 256, 120 + n, pu=8, py=4, ps=0, variant=v)
    yield k3('n=5000 no bucket', 5000, 0, 130, pu=4, py=12, ps=8, variant=v)
    yield k3('in place n=5000 no bucket', 5000, 0, 131, pu=12, ps=4, alias=True, variant=v)


def _prep(x, mean, me):
    v = x - np.float32(mean or 0.0)
    if me is not None:
        v = np.clip(v, np.float32(-me), np.float32(me))
    return v.astype(np.float32)


def argminmax(tag, x, bucket, px, pa, mean=None, me=None, variant=0):
    n = x.size
    mean = _vmean(mean, variant)
    nb = nbuckets(n, bucket)
    arrays = [('x', inp(x, px)), ('argmin', out(I64, nb, pa)), ('argmax', out(I64, nb, (pa + 8) % 16))]
    if mean is not None:
        arrays.append(('mean', inp(np.array([mean], np.float32), 12)))
    args = [Ref('x'), n, bucket, Ref('mean') if mean is not None else None, int(me is not None), float(me or 0.0), Ref('argmin'),
            Ref('argmax'), WS, WSB, STREAM]

    def expect():
        v = _prep(x, mean, me)
        row = bucket if nb > 1 else n
        lo = np.arange(nb) * row
        return {'argmin': np.array([np.argmin(v[a:a + row]) for a in lo], np.int64),
                'argmax': np.array([np.argmax(v[a:a + row]) for a in lo], np.int64)}
    return case(tag, 'qd_bucket_argminmax_f32', arrays, args, expect, uses_ws=nb == 1 and n > 65536)


def _argminmax_cases(v=0):
    for bucket, nfull in ((256, 10), (33, 9), (64, 5), (1000, 3)):
        for li, n in enumerate(lengths(bucket, nfull)):
            yield argminmax('n=%d bucket %d' % (n, bucket), data(n, bucket, 140 + li, variant=v), bucket, (0, 4, 8)[li], (0, 8, 0)[li],
                            mean=0.0625 if li == 2 else None, me=0.8 if li == 2 else None, variant=v)
    for n in (1, 2, 3, 5, 255, 257):
        yield argminmax('n=%d bucket 256' % n, data(n, 256, 150 + n, variant=v), 256, 12, 0)
    yield argminmax('n=65536 no bucket: one chunk', data(65536, 0, 160, variant=v), 0, 4, 0)
    yield argminmax('n=65537 no bucket: two chunks', data(65537, 0, 161, variant=v), 0, 8, 8)
    yield argminmax('n=200003 no bucket: four chunks, mean + clamp', data(200003, 0, 162, variant=v), 0, 12, 0, mean=0.0625, me=0.8, variant=v)


def mean_case(n, px, pm, variant=0):
    x = data(n, 0, 170 + n % 13, variant=variant, finite=True)          # (a sum: finite values only)
    arrays = [('x', inp(x, px)), ('mean', out(F32, 1, pm))]

    def expect():
        return {'mean': np.array([math.fsum(x.astype(np.float64).tolist()) / n], np.float64).astype(np.float32)}
    return case('n=%d x+%d mean+%d' % (n, px, pm), 'qd_mean_f32', arrays, [Ref('x'), n, Ref('mean'), WS, WSB, STREAM], expect, uses_ws=True)


def _mean_cases(v=0):
    for n in (1, 1023, 70001):
        for px, pm in ((0, 4), (8, 12), (4, 4), (12, 0)):
            yield mean_case(n, px, pm, v)


K6_PAIRS = [(100, 4), (100, 600), (1000, 4), (1000, 600), (100, 64), (100, 100), (33, 16), (256, 600), (0, 700), (256, 1024),
            (1000, 1024), (100, 128), (1000, 256), (7, 16), (5, 4), (6, 200), (3, 16), (2, 4), (256, 100), (0, 100), (256, 300),
            (0, 300)]


def k6(tag, n, bucket, k, idx_bytes, pg, pidx, pa, pout, variant=0):
    rng = np.random.RandomState(k * 7 + bucket + n + 7000 * variant)
    g = rng.randn(n).astype(np.float32)
    idx = rng.randint(0, k, size=n).astype(np.int64)
    nb = nbuckets(n, bucket)
    alpha = (np.abs(rng.randn(nb)) + 0.1).astype(np.float32)
    if variant:                                        # gradients and alpha stay finite: errlog.check_sum keeps its meaning
        g = vary(g, bucket, k * 7 + bucket + n, variant, finite=True)
    if variant == 2:
        idx[:] = k // 2                                # every term in ONE bin
    arrays = [('g', inp(g, pg, 'grad')), ('idx', inp(idx if idx_bytes == 8 else idx.astype(np.uint8), pidx, ('index', k - 1))),
              ('alpha', inp(alpha, pa)), ('grad_points', out(F32, k, pout))]
    args = [Ref('g'), Ref('idx'), idx_bytes, Ref('alpha'), n, bucket, k, Ref('grad_points'), WS, WSB, STREAM]

    def expect():
        want, absum = oc.point_grad(g, idx, alpha, bucket or None, k)
        return {'grad_points': Sum(want, absum, 'K6 point gradient at the C ABI (bucket %d, k = %d)' % (bucket, k))}
    return case(tag, 'qd_point_grad_f32', arrays, args, expect, uses_ws=True)


def _k6_cases(bucket, k):
    def make(v=0):
        # qd_point_grad_f32 (csrc/qd_reductions.hip) picks its kernel from k, the alignment of g and idx and whether there is
        # one bucket (nb == 1) or several of a power-of-two / other size; n enters only through nb and the grid, blocks_for(n, 2048)
        # (1024 per block in the scalar kernel), i.e. one partial row or several for the fold.  6151 = 3 * 2048 + 7: four blocks,
        # and several buckets with a ragged last one at every bucket size of the table (1000: 6 + 151, 256: 24 + 7, 100: 61 + 51);
        # n = 1 and 5 below are the nb == 1, one-block end of the bucketed pairs.
        n = 6151
        yield k6('int64 n=%d' % n, n, bucket, k, 8, 0, 0, 4, 12, v)
        yield k6('int64 at +8, g at +4 n=%d' % n, n, bucket, k, 8, 4, 8, 12, 8, v)
        if k <= 256:
            yield k6('uint8 n=%d' % n, n, bucket, k, 1, 8, 4, 0, 4, v)
            yield k6('uint8 at +1 n=%d' % n, n, bucket, k, 1, 12, 1, 8, 0, v)
        for small in (1, 5):
            yield k6('n=%d' % small, small, bucket, k, 8, 4, 0, 12, 8, v)
    return make


def _k8_cases(v=0):
    for n in (1, 5, 50001):
        rng = np.random.RandomState(180 + n + 8000 * v)
        w = rng.randn(n).astype(np.float32)
        g = rng.randn(n).astype(np.float32)
        if v:                                                         # w: NaN stays / keeps the gradient, +-inf clamps / zeroes it
            w, g = vary(w, 1000, 180 + n, v) * np.float32(0.125), vary(g, 1000, 190 + n, v, finite=True)
            if v == 2 and n > 4:
                w[1], w[3] = -np.inf, np.float32(-0.5)
        w[n // 2] = np.float32(0.5)                                   # |w| == limit: kept by both
        for pw, pg in PHASES:
            yield case('clamp n=%d w+%d' % (n, pw), 'qd_clamp_f32', [('w', inout(w, pw))], [Ref('w'), n, 0.5, STREAM],
                       (lambda w=w: {'w': np.clip(w, np.float32(-0.5), np.float32(0.5))}))
            yield case('truncated STE n=%d w+%d grad+%d' % (n, pw, pg), 'qd_truncated_ste_f32', [('w', inp(w, pw)), ('grad', inout(g, pg, 'grad'))],
                       [Ref('w'), Ref('grad'), n, 0.5, STREAM], (lambda w=w, g=g: {'grad': np.where(np.abs(w) > np.float32(0.5), np.float32(0.0), g)}))


# ---------------------------------------------------------------- device only: absmax / absnorm
def abs_case(op, tag, x, bucket, kind, px, pq, ps, mean=None, me=None, variant=0):
    """op 0: qd_uniform_abs_f32, 1: qd_scale_down_abs_f32, 2: qd_inv_scale_abs_f32 (on the oracle's u, sign and norm)."""
    n = x.size
    mean = _vmean(mean, variant)
    nb, npad = nbuckets(n, bucket), padded(n, bucket)
    name = ('absmax', 'absnorm')[kind]
    opts = dict(max_element=False if me is None else me, subtract_mean=mean is not None, mean=mean)
    ref = onp.scale_down_abs(x, bucket or None, name, **opts)
    norm_want = ref['norm'].reshape(-1) if kind == 0 else Near(ref['norm'].reshape(-1), 2e-6)
    mean_arr = [('mean', inp(np.array([mean], np.float32), 4))] if mean is not None else []
    m = Ref('mean') if mean is not None else None
    tail = [int(me is not None), float(me or 0.0), WS, WSB, STREAM]
    if op == 0:
        arrays = [('x', inp(x, px)), ('q', out(F32, n, pq)), ('norm', out(F32, nb, ps))] + mean_arr
        args = [Ref('x'), Ref('q'), n, bucket, 8, kind, Ref('norm'), m] + tail
        ent = 'qd_uniform_abs_f32'
    elif op == 1:
        arrays = [('x', inp(x, px)), ('u', out(F32, npad, pq)), ('sign', out(F32, npad, (pq + 8) % 16)), ('norm', out(F32, nb, ps))] + mean_arr
        args = [Ref('x'), Ref('u'), Ref('sign'), n, bucket, kind, Ref('norm'), m] + tail
        ent = 'qd_scale_down_abs_f32'
    else:
        arrays = [('u', inp(ref['u'].reshape(-1), px)), ('sign', inp(ref['sign'].reshape(-1), (px + 8) % 16)), ('y', out(F32, n, pq)),
                  ('norm', inp(ref['norm'].reshape(-1), ps))] + mean_arr
        args = [Ref('u'), Ref('sign'), Ref('y'), n, bucket, Ref('norm'), m, STREAM]
        ent = 'qd_inv_scale_abs_f32'

    def expect():
        if op == 2:
            return {'y': onp.inv_scale_down_abs(ref['u'], ref['sign'], ref['norm'], ref['mean'], n, (n,))}
        if op == 1:
            return {'norm': norm_want, 'u': AfterNorm(lambda nrm: onp.scale_down_abs(x, bucket or None, name, norm=nrm, **opts)['u'].reshape(-1)),
                    'sign': ref['sign'].reshape(-1)}
        return {'norm': norm_want,
                'q': AfterNorm(lambda nrm: onp.uniform_quantize_abs(x, 8, bucket or None, name, norm=nrm, **opts)['q'].reshape(-1))}
    return case(tag, ent, arrays, args, expect)           # (the header states no minimum for the two-stage norm's scratch)


class AfterNorm(object):
    """An output that is exact GIVEN the norm the library wrote (absnorm: a sum of squares in another order)."""

    def __init__(self, fn):
        self.fn = fn


def _abs_cases(op, kind):
    def make(v=0):
        for n, bucket in ((2560, 256), (2563, 256), (2560 + 255, 256), (5000, 0), (65537, 0), (5, 256), (1, 0)):
            # variant 2: finite (the norm goes through np.allclose and AfterNorm), scaled by 2^+-40: a sum of squares near 2^100,
            # and a norm below 1e-10, which is replaced by 1
            x = data(n, bucket, 200 + n % 31, variant=v, finite=True, big=2.0 ** 40, small=2.0 ** -40)
            x[::97] = 0.0
            for ci, ((px, pq), ps) in enumerate(zip(PHASES, SIDE)):
                with_prep = ci == 1
                yield abs_case(op, 'n=%d bucket %d x+%d out+%d%s' % (n, bucket, px, pq, ' mean + clamp' if with_prep else ''), x, bucket,
                               kind, px, pq, ps, mean=0.0625 if with_prep else None, me=0.8 if with_prep and op != 2 else None, variant=v)
    return make


# ---------------------------------------------------------------- device only: packed codec
def pack_bits(lev, bits):
    """Element e in bits [e*bits, (e+1)*bits) of the stream, little endian inside a byte (include/qd_hip.h)."""
    lev = np.asarray(lev, np.uint8)
    per = 8 // bits
    pad = np.zeros(-(-len(lev) // per) * per, np.uint8)
    pad[:len(lev)] = lev
    outb = np.zeros(len(pad) // per, np.uint8)
    for j in range(per):
        outb |= (pad[j::per] << np.uint8(j * bits)).astype(np.uint8)
    return outb


def _codec_cases(v=0):
    for bits in (1, 2, 4, 8):
        levels = 1 << bits
        for bucket in (64, 256, 2048):
            for n in (10 * bucket, 10 * bucket + 3, 10 * bucket + bucket - 1, 5):
                if n < bucket and bucket != 256:
                    continue
                x = data(n, bucket, 300 + bits + n % 17, variant=v)
                nb = nbuckets(n, bucket)
                nbytes = (n * bits + 7) // 8
                r = oc.uniform_quantize(x, levels, bucket, want_idx=False)
                lev = r['lev'].reshape(-1)[:n].astype(np.uint8)
                want_packed = pack_bits(lev, bits)
                lev_in = lev if v < 2 else np.full(n, levels - 1, np.uint8)      # variant 2: all one symbol
                want_lev_packed = pack_bits(lev_in, bits)
                for pp in (0, 4, 8, 12):
                    if n >= bucket:
                        yield case('pack bits %d bucket %d n=%d packed+%d' % (bits, bucket, n, pp), 'qd_pack_uniform_f32',
                                   [('x', inp(x, 0)), ('packed', out(U8, nbytes, pp)), ('alpha', out(F32, nb, 4)), ('beta', out(F32, nb, 12))],
                                   [Ref('x'), n, bucket, levels, bits, Ref('packed'), Ref('alpha'), Ref('beta'), STREAM],
                                   (lambda w=want_packed, r=r: {'packed': w, 'alpha': r['alpha'], 'beta': r['beta']}))
                    if pp == 0 and n >= bucket:
                        yield case('pack without alpha / beta bits %d bucket %d n=%d' % (bits, bucket, n), 'qd_pack_uniform_f32',
                                   [('x', inp(x, 0)), ('packed', out(U8, nbytes, 8))],
                                   [Ref('x'), n, bucket, levels, bits, Ref('packed'), None, None, STREAM], (lambda w=want_packed: {'packed': w}))
                    for plev in ((0, 1, 2, 3) if pp == 0 else (pp,)):
                        yield case('pack levels bits %d n=%d levels+%d packed+%d' % (bits, n, plev, pp), 'qd_pack_levels_u8',
                                   [('lev', inp(lev_in, plev, ('index', levels - 1))), ('packed', out(U8, nbytes, pp))],
                                   [Ref('lev'), n, bits, Ref('packed'), STREAM], (lambda w=want_lev_packed: {'packed': w}))
                    for ub in (bucket, 0, 100):
                        ru = r if ub == bucket else oc.uniform_quantize(x, levels, ub or None, want_idx=False)
                        wp = pack_bits(ru['lev'].reshape(-1)[:n].astype(np.uint8), bits)
                        yield case('unpack bits %d bucket %d n=%d packed+%d y+%d' % (bits, ub, n, pp, (pp + 4) % 16), 'qd_unpack_uniform_f32',
                                   [('packed', inp(wp, pp, ('index', levels - 1))), ('alpha', inp(ru['alpha'], 8)), ('beta', inp(ru['beta'], 4)),
                                    ('y', out(F32, n, (pp + 4) % 16))],
                                   [Ref('packed'), n, ub, levels, bits, Ref('alpha'), Ref('beta'), Ref('y'), STREAM],
                                   (lambda ru=ru: {'y': ru['q'].reshape(-1)}))
    x = data(2563, 256, 310, variant=v)
    yield case('pack, x at +4: QD_ERR_UNSUPPORTED', 'qd_pack_uniform_f32', [('x', inp(x, 4)), ('packed', out(U8, 2563, 0))],
               [Ref('x'), 2563, 256, 16, 8, Ref('packed'), None, None, STREAM], None, rc=ERR_UNSUPPORTED)
    yield case('pack, packed at +1: QD_ERR_UNSUPPORTED', 'qd_pack_uniform_f32', [('x', inp(x, 0)), ('packed', out(U8, 2563, 1))],
               [Ref('x'), 2563, 256, 16, 8, Ref('packed'), None, None, STREAM], None, rc=ERR_UNSUPPORTED)
    yield case('pack, bucket 100: QD_ERR_UNSUPPORTED', 'qd_pack_uniform_f32', [('x', inp(x, 0)), ('packed', out(U8, 2563, 0))],
               [Ref('x'), 2563, 100, 16, 8, Ref('packed'), None, None, STREAM], None, rc=ERR_UNSUPPORTED)


# ---------------------------------------------------------------- device only: histograms
def hist_ws_sizes(rows, lib):
    """Room for zero, one and three per-block rows of `rows` uint64 counters, and the full workspace."""
    return [8 * rows - 8, 8 * rows, 3 * 8 * rows, int(lib.qd_workspace_bytes())]


def _hist_cases(lib, v=0):
    for n in (1, 1000, 70001):
        for k in (2, 16, 256):
            rng = np.random.RandomState(400 + n % 11 + k + 9000 * v)
            idx8 = rng.randint(0, k, n).astype(np.uint8)
            if v == 2:
                idx8[:] = k - 1                                         # all one symbol
            want8 = np.bincount(idx8, minlength=k).astype(np.uint64)
            for pi in (0, 1, 2, 3, 4, 8, 12):
                yield case('u8 n=%d k=%d idx+%d' % (n, k, pi), 'qd_histogram_u8', [('idx', inp(idx8, pi, ('index', k - 1))), ('hist', out(U64, k, 8 * (pi % 2)))],
                           [Ref('idx'), n, k, Ref('hist'), STREAM], (lambda w=want8: {'hist': w}))
            for wi, wsb in enumerate(hist_ws_sizes(k, lib)):
                # without room for one row the entry point falls back to the form without a workspace (qd_codec.hip)
                yield case('u8_ws n=%d k=%d ws %d bytes' % (n, k, wsb), 'qd_histogram_u8_ws', [('idx', inp(idx8, (0, 4, 1, 8)[wi], ('index', k - 1))), ('hist', out(U64, k, 8))],
                           [Ref('idx'), n, k, Ref('hist'), WS, WSB, STREAM], (lambda w=want8: {'hist': w}), ws_bytes=wsb)
            idx64 = rng.randint(0, k, n).astype(np.int64)
            if n > 2:
                idx64[n // 2] = -1
                idx64[n // 3] = k
            if v == 2:
                idx64[:] = k // 2
            inside = (idx64 >= 0) & (idx64 < k)
            want64 = np.concatenate([np.bincount(idx64[inside], minlength=k), [np.count_nonzero(~inside)]]).astype(np.uint64)
            m = k
            edges = np.linspace(0.0, 1.0, m).astype(np.float64)
            val = rng.rand(n).astype(np.float32)
            val[::5] = edges[rng.randint(0, m, len(val[::5]))].astype(np.float32)   # exact hits of an edge
            if v == 1:
                val = val * np.float32(1.5) - np.float32(0.25)                      # below the first edge and above the last
            elif v == 2:
                val[:] = np.float32(edges[m // 2])                                  # all one value, on an edge; one NaN (c = m)
                val[n // 2] = np.nan if n > 2 else val[0]
            wantd = np.bincount(np.digitize(val.astype(np.float64), edges), minlength=m + 1).astype(np.uint64)
            for wi, wsb in enumerate(hist_ws_sizes(k + 1, lib)):
                small = wsb < 8 * (k + 1)
                yield case('i64 n=%d k=%d ws %d bytes' % (n, k, wsb), 'qd_histogram_i64', [('idx', inp(idx64, (0, 8, 0, 8)[wi], ('index', k - 1))), ('hist', out(U64, k + 1, 0))],
                           [Ref('idx'), n, k, Ref('hist'), WS, WSB, STREAM], None if small else (lambda w=want64: {'hist': w}), ws_bytes=wsb,
                           rc=ERR_WS if small else 0)
                yield case('digitize n=%d m=%d ws %d bytes' % (n, m, wsb), 'qd_digitize_histogram_f32',
                           [('v', inp(val, (0, 4, 8, 12)[wi])), ('edges', inp(edges, 8 * (wi % 2))), ('hist', out(U64, m + 1, 8))],
                           [Ref('v'), n, Ref('edges'), m, Ref('hist'), WS, WSB, STREAM], None if small else (lambda w=wantd: {'hist': w}), ws_bytes=wsb,
                           rc=ERR_WS if small else 0)
    for n in (1, 1000, 70001, 2560):                                  # n = 1: nfull == 0, the whole tensor is the tail
        for levels in (2, 16, 256):
            bucket = 256
            x = data(n, bucket, 420 + levels, variant=v)
            r = oc.uniform_quantize(x, levels, bucket, want_idx=False)
            wantl = np.bincount(r['lev'].reshape(-1)[:n], minlength=levels).astype(np.uint64)
            q = r['q'].reshape(-1)
            m = levels
            edges = np.linspace(0.0, 1.0, m).astype(np.float64)
            u = oc.scale_down(q, bucket)['u']
            wants = np.bincount(np.digitize(u.astype(np.float64), edges), minlength=m + 1).astype(np.uint64)
            for wi, wsb in enumerate(hist_ws_sizes(levels, lib)):                    # rows of `levels` counters
                small_l = wsb < 8 * levels
                yield case('level n=%d levels %d ws %d bytes' % (n, levels, wsb), 'qd_level_histogram_f32', [('x', inp(x, 0)), ('hist', out(U64, levels, 8 * (wi % 2)))],
                           [Ref('x'), n, bucket, levels, Ref('hist'), WS, WSB, STREAM], None if small_l else (lambda w=wantl: {'hist': w}), ws_bytes=wsb,
                           rc=ERR_WS if small_l else 0)
            for wi, wsb in enumerate(hist_ws_sizes(m + 1, lib)):                     # rows of m + 1 counters
                small_s = wsb < 8 * (m + 1)
                yield case('scale + digitize n=%d m=%d ws %d bytes' % (n, m, wsb), 'qd_scale_digitize_histogram_f32',
                           [('q', inp(q, 0)), ('edges', inp(edges, 8 * (wi % 2))), ('hist', out(U64, m + 1, 8))],
                           [Ref('q'), n, bucket, Ref('edges'), m, Ref('hist'), WS, WSB, STREAM], None if small_s else (lambda w=wants: {'hist': w}), ws_bytes=wsb,
                           rc=ERR_WS if small_s else 0)
    x = data(2563, 256, 430, variant=v)
    edges = np.linspace(0.0, 1.0, 16)
    yield case('level histogram, x at +4: QD_ERR_UNSUPPORTED', 'qd_level_histogram_f32', [('x', inp(x, 4)), ('hist', out(U64, 16, 0))],
               [Ref('x'), 2563, 256, 16, Ref('hist'), WS, WSB, STREAM], None, rc=ERR_UNSUPPORTED)
    yield case('level histogram, bucket 100: QD_ERR_UNSUPPORTED', 'qd_level_histogram_f32', [('x', inp(x, 0)), ('hist', out(U64, 16, 0))],
               [Ref('x'), 2563, 100, 16, Ref('hist'), WS, WSB, STREAM], None, rc=ERR_UNSUPPORTED)
    yield case('scale + digitize, q at +8: QD_ERR_UNSUPPORTED', 'qd_scale_digitize_histogram_f32', [('q', inp(x, 8)), ('edges', inp(edges, 0)), ('hist', out(U64, 17, 0))],
               [Ref('q'), 2563, 256, Ref('edges'), 16, Ref('hist'), WS, WSB, STREAM], None, rc=ERR_UNSUPPORTED)
    yield case('scale + digitize, bucket 100: QD_ERR_UNSUPPORTED', 'qd_scale_digitize_histogram_f32', [('q', inp(x, 0)), ('edges', inp(edges, 0)), ('hist', out(U64, 17, 0))],
               [Ref('q'), 2563, 100, Ref('edges'), 16, Ref('hist'), WS, WSB, STREAM], None, rc=ERR_UNSUPPORTED)


# ---------------------------------------------------------------- device only: K10
def _k10_cases(m):
    """One group per m: the workspace of m = 32 is 32 MiB, placed and read back once per fill."""
    def make(lib, v=0):
        for n in (1, 5, 70001):
            x = data(n, 0, 500 + n % 7, variant=v, finite=True)
            if v == 2 and n > 4:                                      # duplicates and a NaN (it orders last: ranks[-1] is n - 1)
                x[n // 2:] = x[:n - n // 2]
                x[n // 3] = np.nan
            if n > 4:
                x[1] = np.float32(-0.0)
                x[3] = np.float32(0.0)
            srt = np.sort(x, kind='stable')                           # -0 (at 1) stays before +0 (at 3), the header's order
            rng = np.random.RandomState(510 + m + n % 5)
            ranks = np.sort(rng.randint(0, n, m)).astype(np.int64)
            if m > 1:
                ranks[1] = ranks[0]                                   # a repeated rank
                ranks[-1] = n - 1
            wsb = int(lib.qd_order_stats_workspace_bytes(m))
            for px in (0, 4, 8, 12):
                yield case('n=%d m=%d x+%d' % (n, m, px), 'qd_order_stats_f32', [('x', inp(x, px)), ('out', out(F32, m, (px + 4) % 16))],
                           [Ref('x'), n, ranks, m, Ref('out'), WS, WSB, STREAM], (lambda s=srt, r=ranks: {'out': s[r]}), ws_bytes=wsb, uses_ws=True)
    return make


# ---------------------------------------------------------------- the table
def _build_groups():
    g = []
    g += _transform_groups('K1', 'qd_uniform_f32', k1, 1000)
    g.append(Group('K1-extra', 'qd_uniform_f32', 'stochastic rounding, mean + clamp, in place, NULL alpha / beta, level_idx at byte phases', _k1_extra, True))
    g.append(Group('K1-levels-only', 'qd_uniform_f32', 'q == NULL: the 8-bit pack kernel; its stricter requirements are refused', _k1_levels_only, False))
    g += _transform_groups('K2', 'qd_scale_down_f32', k2, 2000)
    g.append(Group('K2-extra', 'qd_scale_down_f32', 'u == x at n % bucket == 0, mean + clamp', _k2_extra, True))
    g += _transform_groups('K4', 'qd_nearest_point_f32', _k4_default, 3000)
    g.append(Group('K4-k-raw', 'qd_nearest_point_f32', 'k in K_SWEEP x both assign modes x idx_bytes, prescaled == 0', _k4_k(0), True))
    g.append(Group('K4-k-prescaled', 'qd_nearest_point_f32', 'the same with prescaled != 0 (k_nearest_prescaled_stream / single apply)', _k4_k(1), True))
    g.append(Group('K4-extra', 'qd_nearest_point_f32', 'q == x, idx == NULL, misaligned idx (k_bucket_groups), indices only', _k4_extra, True))
    g.append(Group('K4-indices-only-refused', 'qd_nearest_point_f32', 'the documented requirements of the indices-only form', _k4_indices_only_refused, False))
    g.append(Group('K3', 'qd_inv_scale_f32', 'k_inv_scale<false> (row % 4 == 0 or one bucket) and <true>', _k3_cases, True))
    g.append(Group('argminmax', 'qd_bucket_argminmax_f32', 'k_argminmax per bucket; one bucket above 65536 elements: chunks + k_arg_final', _argminmax_cases, True))
    g.append(Group('mean', 'qd_mean_f32', 'k_sum_partial + k_mean_final', _mean_cases, True))
    for bucket, k in K6_PAIRS:
        g.append(Group('K6-b%d-k%d' % (bucket, k), 'qd_point_grad_f32', 'the (bucket, k) pair of test_point_gradient_deterministic_and_within_1e6_on_every_path',
                       _k6_cases(bucket, k), True))
    g.append(Group('K8', 'qd_clamp_f32 / qd_truncated_ste_f32', 'n in {1, 5, 50001}', _k8_cases, True))
    for op, name in enumerate(('uniform', 'scale_down', 'inv_scale')):
        for kind in (0, 1):
            g.append(Group('abs-%s-%s' % (name, ('absmax', 'absnorm')[kind]), 'qd_%s_abs_f32' % name,
                           'bucket 256 whole / ragged (padded u, sign), one bucket at 5000 and 65537 (two-stage), mean + clamp', _abs_cases(op, kind), False))
    g.append(Group('codec', 'qd_pack_uniform_f32 / qd_pack_levels_u8 / qd_unpack_uniform_f32', 'bits 1, 2, 4, 8; a partly filled last byte; byte phases', _codec_cases, False))
    g.append(Group('histograms', 'the five histogram entry points and qd_histogram_u8', 'workspace room for 0, 1, 3 rows and the full size', _hist_cases, False))
    for m in (1, 2, 32):
        g.append(Group('K10-m%d' % m, 'qd_order_stats_f32', 'n in {1, 5, 70001}, repeated ranks, x at every phase', _k10_cases(m), False))
    return collections.OrderedDict((x.id, x) for x in g)


GROUPS = _build_groups()
HOST_GROUP_IDS = [i for i, x in GROUPS.items() if x.host]
DEVICE_GROUP_IDS = list(GROUPS)
NEEDS_LIB = ('histograms', 'K10-m1', 'K10-m2', 'K10-m32')              # their workspace sizes come from the library


def cases_of(group, lib, variant=0):
    """The cases of the group; variant 1 / 2: the same tags, entry points, shapes, phases and by-value arguments on other array
    contents (vary()), what a launch recorded on variant 0 is replayed on."""
    return group.make(lib, variant) if group.id in NEEDS_LIB else group.make(variant)


# ---------------------------------------------------------------- device only: the multi-tensor launches (K9, K5m, K6m)
class Flat(object):
    """The tensors of one column of a descriptor table carved out of ONE flat device buffer: tensor i starts `phases[i]` bytes
    into a 16-byte granule, at least GUARD bytes behind the one before; what lies between them is guard (the sentinel for
    outputs, hostile values for inputs), as in Placed."""

    def __init__(self, sizes, dtype, device, role, arrays=None, guard='float', phases=None, valid_max=None):
        self.dtype, self.sizes = np.dtype(dtype), list(sizes)
        isz = self.dtype.itemsize
        phases = phases or [(0, 4, 8, 12)[(i + 1) % 4] for i in range(len(sizes))]
        self.arr = Arr(role, self.dtype, None, 0, 0, guard if role != 'out' else 'sentinel', valid_max)
        self.offs, off = [], 0
        for n, ph in zip(sizes, phases):
            off = -(-(off + GUARD) // 16) * 16 + ph
            self.offs.append(off)
            off += n * isz
        total = off + GUARD + 16
        self.buf = torch.empty(total + 16, dtype=torch.uint8, device=device)
        assert self.buf.data_ptr() % 16 == 0
        pat = _pattern(self.arr)
        img = np.resize(pat, (total + 16) // isz + 1).view(np.uint8)[:total + 16].copy()
        self.inside = np.zeros(total + 16, bool)
        for i, (o, n) in enumerate(zip(self.offs, sizes)):
            self.inside[o:o + n * isz] = True
            if arrays is not None:
                img[o:o + n * isz] = np.ascontiguousarray(arrays[i], self.dtype).view(np.uint8)
        self.image = img
        self.buf.copy_(torch.from_numpy(img.copy()))

    def views(self):
        tdt = {'float32': torch.float32, 'uint8': torch.uint8}[self.dtype.name]
        return [self.buf[o:o + n * self.dtype.itemsize].view(tdt) for o, n in zip(self.offs, self.sizes)]

    def read(self, tag, name):
        got = self.buf.cpu().numpy()
        bad = np.nonzero((got != self.image) & ~self.inside)[0]
        assert len(bad) == 0, (tag, name, 'written between the tensors, first at byte %d' % (bad[0] if len(bad) else -1))
        if self.arr.role == 'in':
            assert np.array_equal(got, self.image), (tag, name, 'an input was written over')
        outs = [got[o:o + n * self.dtype.itemsize].copy().view(self.dtype) for o, n in zip(self.offs, self.sizes)]
        if self.arr.role == 'out':
            for i, o in enumerate(outs):
                assert_no_sentinel(self.arr, o, tag, '%s[%d]' % (name, i))
        return outs


# Zero-length tensors sit between the others (the plans give them no tile and, in K6m, one partial row nobody writes or reads):
# one alone, the first, two in a row and the last of a list.
EMPTY_65 = (0, 20, 21, 40, 64)
MULTI_LISTS = {1: [70001], 7: [1, 0, 257, 70001, 0, 1000, 3],
               65: [0 if i in EMPTY_65 else 70001 if i == 63 else 1 + (i * 37) % 300 if i % 3 else 300 + (i * 911) % 9000 for i in range(65)]}


def _ws_view(ws):
    return ws.buf[ws.off:ws.off + ws.nbytes].view(torch.float32)


def run_multi_uniform(nt, bucket, in_place, lib, device, s=16):
    """qd_multi_uniform_f32 (bucket > 0) / qd_multi_uniform_global_f32 (bucket None) on a plan built by
    quantized_distillation_amd.multi_tensor over carved views: every tensor equals the per-tensor oracle bit for bit."""
    from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer
    # (this and run_multi_dq put carved buffers behind the plan classes' own attributes -- _scratch, alpha_beta, scaled, indices,
    # _tiles / _blocks, _table, _plan() -- as tests/test_hip_multi_ste.py does: a change of those names has to be followed here)
    device = torch.device(device)
    sizes = MULTI_LISTS[nt]
    tag = ('K9', nt, bucket, in_place)
    xs = [data(n, bucket or 0, 600 + i) for i, n in enumerate(sizes)]
    fx = Flat(sizes, F32, device, 'inout' if in_place else 'in', xs)
    fq = fx if in_place else Flat(sizes, F32, device, 'out', phases=[(0, 4, 8, 12)[(i + 3) % 4] for i in range(nt)])
    mt = MultiTensorQuantizer(fx.views(), s, bucket, outputs=fq.views())
    wants = [oc.uniform_quantize(x, s, bucket, want_idx=False, want_lev=False) for x in xs]
    results = []
    for fill in (FILLS if bucket is None else FILLS[:1]):
        if not in_place:
            fq.buf.copy_(torch.from_numpy(fq.image.copy()))
        else:
            fx.buf.copy_(torch.from_numpy(fx.image.copy()))
        if bucket is None:
            nbytes = max(mt._tiles, 1) * 2 * 4
            ws = Placed(Arr('out', U8, None, nbytes, 0, 'sentinel', None), device)
            ws.fill(_ws_bytes(fill, nbytes, lib, device))
            ab = Placed(out(F32, 2 * nt, 4), device)
            mt._scratch = _ws_view(ws)
            mt.alpha_beta = ab.buf[ab.off:ab.off + ab.nbytes].view(torch.float32).view(nt, 2)
            rc = lib.qd_multi_uniform_global_f32(mt._table.data_ptr(), nt, mt._tiles, s, ab.ptr, ws.ptr, nbytes - 1, _lib.stream_ptr(device))
            torch.cuda.synchronize(device)
            assert rc == ERR_WS and ab.untouched(ab.read(tag, 'alpha_beta')), (tag, rc)
        outs = mt.quantize(check_pointers=False)
        torch.cuda.synchronize(device)
        assert [o.data_ptr() for o in outs] == [v.data_ptr() for v in fq.views()]
        got = fq.read(tag, 'q')
        if not in_place:
            fx.read(tag, 'x')
        for i, (g, w) in enumerate(zip(got, wants)):
            assert _same(g, w['q'].reshape(-1)), (tag, fill, 'tensor %d of %d elements differs from the oracle' % (i, sizes[i]))
        if bucket is None:
            ws.read(tag, 'workspace')
            abv = ab.read(tag, 'alpha_beta')
            ab.assert_no_sentinel(abv, tag, 'alpha_beta')
            # an empty tensor's row is written too: (alpha, beta) of the min / max over no element, (+inf, -inf) -> alpha < 1e-10 -> 1,
            # beta = min = +inf (k_mg_fold); nothing reads it
            want_ab = np.array([[w['alpha'][0], w['beta'][0]] if n else [1.0, np.inf] for w, n in zip(wants, sizes)], np.float32).reshape(-1)
            assert _same(abv, want_ab), (tag, fill, 'alpha_beta')
        results.append(got)
    for r in results[1:]:
        assert all(_same(a, b) for a, b in zip(r, results[0])), (tag, 'differs between workspace fills')


def run_multi_dq(nt, bucket, k, lib, device):
    """qd_multi_nearest_f32 and qd_multi_point_grad_f32 on a plan of MultiTensorDiffQuant whose every column -- u, q, idx,
    grad -- is a carved view, `points` and grad_points sit between guards and the scratch has exactly total_blocks * k floats."""
    from quantized_distillation_amd.multi_tensor import MultiTensorDiffQuant
    device = torch.device(device)
    sizes = MULTI_LISTS[nt]
    tag = ('K5m/K6m', nt, bucket, k)
    xs = [data(n, bucket, 700 + i) for i, n in enumerate(sizes)]
    gs = [np.random.RandomState(800 + i).randn(n).astype(np.float32) for i, n in enumerate(sizes)]
    pts = np.stack([points(k, seed=900 + i) for i in range(nt)])
    fq = Flat(sizes, F32, device, 'out')
    fg = Flat(sizes, F32, device, 'in', gs, guard='grad', phases=[(0, 4, 8, 12)[(i + 2) % 4] for i in range(nt)])
    mt = MultiTensorDiffQuant([torch.from_numpy(x).to(device) for x in xs], fq.views(), fg.views(), k, bucket)
    sds = [oc.scale_down(x, bucket) for x in xs]
    fu = Flat(sizes, F32, device, 'in', [sd['u'] for sd in sds], phases=[(0, 4, 8, 12)[(i + 3) % 4] for i in range(nt)])
    fi = Flat(sizes, U8, device, 'out', phases=[(0, 4, 8, 12)[i % 4] for i in range(nt)], valid_max=k - 1)
    for got, sd in zip(mt.scaled, sds):
        assert _same(got.cpu().numpy(), sd['u']), (tag, 'scale_down differs from the oracle')
    mt.scaled, mt.indices = fu.views(), fi.views()
    mt._plan()
    pp = Placed(inp(pts.reshape(-1), 4), device)
    wants = [oc.nonuniform_quantize(x, p, bucket, 'midpoint') for x, p in zip(xs, pts)]
    mt.forward(pp.buf[pp.off:pp.off + pp.nbytes].view(torch.float32).view(nt, k))
    torch.cuda.synchronize(device)
    pp.read(tag, 'points')
    fu.read(tag, 'u')
    for i, (q, ix, w) in enumerate(zip(fq.read(tag, 'q'), fi.read(tag, 'idx'), wants)):
        assert _same(q, w['q'].reshape(-1)) and _same(ix, w['idx'].reshape(-1).astype(np.uint8)), (tag, 'forward: tensor %d (%d elements)' % (i, sizes[i]))
    fi.arr = fi.arr._replace(role='in')                       # the backward sweep only reads them
    fi.image = fi.buf.cpu().numpy()
    nbytes = max(mt._blocks * k, 1) * 4
    results = []
    for fill in FILLS:
        ws = Placed(Arr('out', U8, None, nbytes, 0, 'sentinel', None), device)
        ws.fill(_ws_bytes(fill, nbytes, lib, device))
        gp = Placed(out(F32, nt * k, 8), device)
        gp_view = gp.buf[gp.off:gp.off + gp.nbytes].view(torch.float32).view(nt, k)
        rc = lib.qd_multi_point_grad_f32(mt._table.data_ptr(), nt, mt._blocks, bucket, k, gp.ptr, ws.ptr, nbytes - 1, _lib.stream_ptr(device))
        torch.cuda.synchronize(device)
        assert rc == ERR_WS and gp.untouched(gp.read(tag, 'grad_points')), (tag, rc)
        mt._scratch = _ws_view(ws)
        mt.backward(out=gp_view)
        torch.cuda.synchronize(device)
        ws.read(tag, 'workspace')
        fg.read(tag, 'grad')
        fi.read(tag, 'idx')
        got = gp.read(tag, 'grad_points')
        gp.assert_no_sentinel(got, tag, 'grad_points')
        for i, (g, w, sd) in enumerate(zip(gs, wants, sds)):
            want, absum = oc.point_grad(g, w['idx'], sd['alpha'], bucket, k)
            errlog.check_sum('K6m point gradient at the C ABI', got[i * k:(i + 1) * k], want, absum, tag + (i,))
        results.append(got)
    for r in results[1:]:
        assert _same(r, results[0]), (tag, 'differs between workspace fills')


# ---------------------------------------------------------------- the multi-tensor launches, recorded once and replayed
def _flat_reload(flat, arrays=None):
    """(a replay) new contents for every tensor of the column -- or, for outputs, the sentinel again -- in the same buffer."""
    isz = flat.dtype.itemsize
    if flat.arr.role == 'out':
        pat = _pattern(flat.arr)
        img = np.resize(pat, len(flat.image) // isz + 1).view(np.uint8)[:len(flat.image)].copy()
        flat.image[flat.inside] = img[flat.inside]
    else:
        for o, n, a in zip(flat.offs, flat.sizes, arrays):
            flat.image[o:o + n * isz] = np.ascontiguousarray(a, flat.dtype).view(np.uint8)
    flat.buf.copy_(torch.from_numpy(flat.image.copy()))


def _same_as_oracle(got, want):
    """Bit for bit, a NaN for a NaN (_compare)."""
    want = np.ascontiguousarray(want).reshape(-1)
    if want.size == 0 or _same(got, want):
        return _same(got, want)
    return got.dtype == want.dtype and got.shape == want.shape and bool(
        ((got.view(np.uint8).reshape(len(got), -1) == want.view(np.uint8).reshape(len(want), -1)).all(axis=1)
         | ((np.isnan(got) & np.isnan(want)) if want.dtype.kind == 'f' else False)).all())


def _rows_same(a, b):
    return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


def run_multi_uniform_captured(nt, bucket, in_place, lib, device, s=16):
    """run_multi_uniform under the protocol of run_case_captured: ONE launch of K9 recorded on variant 0 of the list, replayed
    on variants 1, 2, 0, 1 written into the same flat buffers (without buckets: the global workspace refilled with the next
    of FILLS and alpha_beta back to its sentinel), every tensor against the per-tensor oracle, variants 1 and 2 against an
    eager launch of a second plan over a second set of buffers bit for bit, then two replays back to back."""
    from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer
    device = torch.device(device)
    sizes = MULTI_LISTS[nt]
    tag = ('K9 captured', nt, bucket, in_place)
    xs = {v: [data(n, bucket or 0, 600 + i, variant=v) for i, n in enumerate(sizes)] for v in VARIANTS}
    residue_image(lib, device)

    def plan(x0):
        fx = Flat(sizes, F32, device, 'inout' if in_place else 'in', x0)
        fq = fx if in_place else Flat(sizes, F32, device, 'out', phases=[(0, 4, 8, 12)[(i + 3) % 4] for i in range(nt)])
        mt = MultiTensorQuantizer(fx.views(), s, bucket, outputs=fq.views())
        ws = ab = None
        if bucket is None:
            ws = Placed(Arr('out', U8, None, max(mt._tiles, 1) * 2 * 4, 0, 'sentinel', None), device)
            ab = Placed(out(F32, 2 * nt, 4), device)
            mt._scratch = _ws_view(ws)
            mt.alpha_beta = ab.buf[ab.off:ab.off + ab.nbytes].view(torch.float32).view(nt, 2)
        return fx, fq, mt, ws, ab

    def load(p, v, fill):
        fx, fq, mt, ws, ab = p
        _flat_reload(fx, xs[v])
        if not in_place:
            _flat_reload(fq)
        if ws is not None:
            ws.fill(_ws_bytes(fill, ws.nbytes, lib, device))
            ab.reload(ab.arr)

    def read(p, v, rtag, check=True):
        fx, fq, mt, ws, ab = p
        got = fq.read(rtag, 'q')
        if not in_place:
            fx.read(rtag, 'x')
        abv = None
        if ws is not None:
            ws.read(rtag, 'workspace')
            abv = ab.read(rtag, 'alpha_beta')
            ab.assert_no_sentinel(abv, rtag, 'alpha_beta')
        if check:
            wants = [oc.uniform_quantize(x, s, bucket, want_idx=False, want_lev=False) for x in xs[v]]
            for i, (g, w) in enumerate(zip(got, wants)):
                assert _same_as_oracle(g, w['q']), (rtag, 'tensor %d of %d elements differs from the reference' % (i, sizes[i]))
            if abv is not None:
                want_ab = np.array([[w['alpha'][0], w['beta'][0]] if n else [1.0, np.inf] for w, n in zip(wants, sizes)], np.float32)
                assert _same_as_oracle(abv, want_ab), (rtag, 'alpha_beta differs from the reference')
        return got + ([abv] if abv is not None else [])

    with torch.cuda.stream(side_stream(device)):
        p = plan(xs[0])
        p[2].quantize(check_pointers=False)                    # warm-up
    graph = torch.cuda.CUDAGraph()
    with recording(graph, device):
        p[2].quantize(check_pointers=False)
    with torch.cuda.stream(side_stream(device)):
        eager1 = None
        for i, v in enumerate(REPLAY_ORDER):
            rtag = tag + ('replay %d on variant %d' % (i, v),)
            load(p, v, FILLS[i % len(FILLS)])
            graph.replay()
            torch.cuda.synchronize(device)
            got = read(p, v, rtag)
            if v != 0 and i < 2:
                e = plan(xs[v])
                load(e, v, FILLS[(i + 1) % len(FILLS)])
                e[2].quantize(check_pointers=False)
                torch.cuda.synchronize(device)
                assert _rows_same(got, read(e, v, rtag + ('eager',))), (rtag, 'the replay and the eager launch differ')
                if v == REPLAY_ORDER[-1]:
                    eager1 = e
        graph.replay()
        graph.replay()
        torch.cuda.synchronize(device)
        again = read(p, REPLAY_ORDER[-1], tag, check=False)
        if not in_place:
            assert _rows_same(again, got), (tag, 'two replays back to back differ from the replay before them')
        eager1[2].quantize(check_pointers=False)
        eager1[2].quantize(check_pointers=False)
        torch.cuda.synchronize(device)
        assert _rows_same(again, read(eager1, REPLAY_ORDER[-1], tag, check=False)), (tag, 'three replays differ from three eager launches')
    del graph


def run_multi_dq_captured(nt, bucket, k, lib, device):
    """run_multi_dq under the same protocol: K5m (qd_multi_nearest_f32) and K6m (qd_multi_point_grad_f32) recorded as ONE
    launch each into graphs of their own, on variant 0, and replayed on the other variants: u, points, alpha and the
    gradients are rewritten in place, q, idx and grad_points go back to their sentinel, K6m's scratch (exactly
    total_blocks * k floats) takes the next of FILLS.  The data stays finite (K6m's sums go through errlog.check_sum)."""
    from quantized_distillation_amd.multi_tensor import MultiTensorDiffQuant
    device = torch.device(device)
    sizes = MULTI_LISTS[nt]
    tag = ('K5m/K6m captured', nt, bucket, k)
    # neither sweep divides (u is scaled already): the scales only have to keep every g alpha and their sums inside fp32
    xs = {v: [data(n, bucket, 700 + i, variant=v, finite=True, big=2.0 ** 60, small=2.0 ** -60) for i, n in enumerate(sizes)] for v in VARIANTS}
    gs = {v: [vary(np.random.RandomState(800 + i).randn(n).astype(np.float32), bucket, 800 + i, v, finite=True, big=2.0 ** 30, small=2.0 ** -30)
              for i, n in enumerate(sizes)] for v in VARIANTS}
    pts = {v: np.stack([points(k, seed=900 + i + 50 * v) for i in range(nt)]) for v in VARIANTS}
    sds = {v: [oc.scale_down(x, bucket) for x in xs[v]] for v in VARIANTS}
    wants = {v: [oc.nonuniform_quantize(x, p, bucket, 'midpoint') for x, p in zip(xs[v], pts[v])] for v in VARIANTS}
    residue_image(lib, device)

    def plan(v):
        fq = Flat(sizes, F32, device, 'out')
        fg = Flat(sizes, F32, device, 'in', gs[v], guard='grad', phases=[(0, 4, 8, 12)[(i + 2) % 4] for i in range(nt)])
        mt = MultiTensorDiffQuant([torch.from_numpy(x).to(device) for x in xs[v]], fq.views(), fg.views(), k, bucket)
        fu = Flat(sizes, F32, device, 'in', [sd['u'] for sd in sds[v]], phases=[(0, 4, 8, 12)[(i + 3) % 4] for i in range(nt)])
        fi = Flat(sizes, U8, device, 'out', phases=[(0, 4, 8, 12)[i % 4] for i in range(nt)], valid_max=k - 1)
        mt.scaled, mt.indices = fu.views(), fi.views()
        mt._plan()
        pp = Placed(inp(pts[v].reshape(-1), 4), device)
        ws = Placed(Arr('out', U8, None, max(mt._blocks * k, 1) * 4, 0, 'sentinel', None), device)
        gp = Placed(out(F32, nt * k, 8), device)
        mt._scratch = _ws_view(ws)
        return dict(fq=fq, fg=fg, fu=fu, fi=fi, mt=mt, pp=pp, ws=ws, gp=gp,
                    pts=pp.buf[pp.off:pp.off + pp.nbytes].view(torch.float32).view(nt, k),
                    gpv=gp.buf[gp.off:gp.off + gp.nbytes].view(torch.float32).view(nt, k))

    def load(p, v, fill):
        _flat_reload(p['fu'], [sd['u'] for sd in sds[v]])
        _flat_reload(p['fg'], gs[v])
        _flat_reload(p['fq'])
        p['fi'].arr = p['fi'].arr._replace(role='out')
        _flat_reload(p['fi'])
        p['pp'].reload(inp(pts[v].reshape(-1), 4))
        p['gp'].reload(p['gp'].arr)
        p['ws'].fill(_ws_bytes(fill, p['ws'].nbytes, lib, device))
        for sf, sd in zip(p['mt'].scalings, sds[v]):                 # the table points at these two tensors
            sf.alpha.copy_(torch.from_numpy(np.asarray(sd['alpha'], np.float32).reshape(tuple(sf.alpha.shape))))
            sf.beta.copy_(torch.from_numpy(np.asarray(sd['beta'], np.float32).reshape(tuple(sf.beta.shape))))

    def read_forward(p, v, rtag, check=True):
        p['pp'].read(rtag, 'points')
        p['fu'].read(rtag, 'u')
        q, ix = p['fq'].read(rtag, 'q'), p['fi'].read(rtag, 'idx')
        if check:
            for i, (a, b, w) in enumerate(zip(q, ix, wants[v])):
                assert _same_as_oracle(a, w['q']) and _same(b, w['idx'].reshape(-1).astype(np.uint8)), \
                    (rtag, 'forward: tensor %d (%d elements) differs from the reference' % (i, sizes[i]))
        p['fi'].arr = p['fi'].arr._replace(role='in')               # the backward sweep only reads them
        p['fi'].image = p['fi'].buf.cpu().numpy()
        return q + ix

    def read_backward(p, v, rtag, check=True):
        p['ws'].read(rtag, 'workspace')
        p['fg'].read(rtag, 'grad')
        p['fi'].read(rtag, 'idx')
        got = p['gp'].read(rtag, 'grad_points')
        p['gp'].assert_no_sentinel(got, rtag, 'grad_points')
        if check:
            for i, (g, w, sd) in enumerate(zip(gs[v], wants[v], sds[v])):
                want, absum = oc.point_grad(g, w['idx'], sd['alpha'], bucket, k)
                errlog.check_sum('K6m point gradient under hipGraph replay', got[i * k:(i + 1) * k], want, absum, rtag + (i,))
        return [got]

    def eager(p):
        p['mt'].forward(p['pts'])
        p['mt'].backward(out=p['gpv'])
        torch.cuda.synchronize(device)

    with torch.cuda.stream(side_stream(device)):
        p = plan(0)
        eager(p)                                                      # warm-up
    fwd, bwd = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with recording(fwd, device):
        p['mt'].forward(p['pts'])
    with recording(bwd, device):
        p['mt'].backward(out=p['gpv'])
    with torch.cuda.stream(side_stream(device)):
        for i, v in enumerate(REPLAY_ORDER):
            rtag = tag + ('replay %d on variant %d' % (i, v),)
            load(p, v, FILLS[i % len(FILLS)])
            fwd.replay()
            torch.cuda.synchronize(device)
            got = read_forward(p, v, rtag)
            bwd.replay()
            torch.cuda.synchronize(device)
            got = got + read_backward(p, v, rtag)
            if v != 0 and i < 2:
                e = plan(v)
                load(e, v, FILLS[(i + 1) % len(FILLS)])
                e['mt'].forward(e['pts'])
                torch.cuda.synchronize(device)
                other = read_forward(e, v, rtag + ('eager',))
                e['mt'].backward(out=e['gpv'])
                torch.cuda.synchronize(device)
                other = other + read_backward(e, v, rtag + ('eager',))
                assert _rows_same(got, other), (rtag, 'the replay and the eager launches differ')
        for _ in range(2):                                            # back to back: no input is written by either sweep
            fwd.replay()
            bwd.replay()
        torch.cuda.synchronize(device)
        v = REPLAY_ORDER[-1]
        p['fi'].arr = p['fi'].arr._replace(role='out')
        again = read_forward(p, v, tag, check=False) + read_backward(p, v, tag, check=False)
        assert _rows_same(again, got), (tag, 'two replays back to back differ from the replay before them')
    del fwd, bwd


# ---------------------------------------------------------------- the capture ledger
HIST_ENTRIES = ('qd_histogram_u8', 'qd_histogram_u8_ws', 'qd_level_histogram_f32', 'qd_digitize_histogram_f32', 'qd_histogram_i64',
                'qd_scale_digitize_histogram_f32')         # (the one group whose `entry` is prose)


def _captured_here():
    here = collections.OrderedDict()
    for gid, g in GROUPS.items():
        if '-mode' in gid:                                 # the qd_set_single_fused_mode hooks add nothing under capture
            continue
        for entry in (HIST_ENTRIES if gid == 'histograms' else g.entry.split(' / ')):
            here.setdefault(entry, []).append(gid)
    here.update([('qd_multi_uniform_f32', ['test_multi_tensor_uniform_captured']),
                 ('qd_multi_uniform_global_f32', ['test_multi_tensor_uniform_captured']),
                 ('qd_multi_nearest_f32', ['test_multi_tensor_diff_quant_captured']),
                 ('qd_multi_point_grad_f32', ['test_multi_tensor_diff_quant_captured']),
                 ('qd_multi_ste_backward_levels_f32', ['test_multi_ste_with_levels_and_16_bit_gradients_captured']),
                 ('qd_multi_ste_backward_in16_f32', ['test_multi_ste_with_levels_and_16_bit_gradients_captured']),
                 ('qd_huffman_encode', ['test_huffman_codec_captured']),
                 ('qd_huffman_decode_f32', ['test_huffman_codec_captured']),
                 ('qd_selftest_div_invariant', ['test_selftest_div_invariant_captured'])])
    return here


# Every entry point of include/qd_hip.h (_lib.SIGNATURES) in exactly one column (tests/test_abi_contract_host.py holds the table
# to that, so a new entry point without a stance fails without a GPU):
#   'here'             recorded once and replayed on other data by tests/test_hip_capture_abi.py: the groups of this module
#                      (run_group_captured), or the named test function of that file;
#   'elsewhere'        (file, test function, what the file says of it): a capture test that existed before;
#   'launches nothing' plans, queries, hooks and size helpers: host code only;
#   'not capturable'   by contract: (reason, file, test that pins the documented behaviour).  A key 'entry: argument' is the
#                      stance of one argument of an entry point that has a column of its own.
CAPTURE = collections.OrderedDict([
    ('here', _captured_here()),
    ('elsewhere', collections.OrderedDict([
        ('qd_ste_bucket_backward_f32', ('test_hip_capture_lifetime.py', 'test_the_per_tensor_step_captured_on_a_warmed_up_stream_equals_the_eager_step',
                                        'ste.ste_bucket_backward')),
        ('qd_multi_uniform_opt_f32', ('test_hip_multi_stochastic.py',
                                      'test_device_seed_is_advanced_on_the_stream_and_a_captured_launch_draws_anew_at_every_replay',
                                      'qd_multi_uniform_opt_f32')),
        ('qd_multi_uniform_global_opt_f32', ('test_hip_multi_stochastic.py',
                                             'test_device_seed_is_advanced_on_the_stream_and_a_captured_launch_draws_anew_at_every_replay',
                                             'qd_multi_uniform_global_opt_f32')),
        ('qd_multi_uniform_levels_f32', ('test_hip_multi_levels.py', 'test_a_captured_launch_with_a_mixed_list_draws_anew_at_every_replay',
                                         'qd_multi_uniform_levels_f32')),
        ('qd_multi_uniform_global_levels_f32', ('test_hip_multi_levels.py', 'test_a_captured_launch_with_a_mixed_list_draws_anew_at_every_replay',
                                                'qd_multi_uniform_global_levels_f32')),
        ('qd_multi_uniform_out16_f32', ('test_hip_out16.py', 'test_a_captured_launch_draws_anew_at_every_replay', 'qd_multi_uniform_out16_f32')),
        ('qd_multi_uniform_global_out16_f32', ('test_hip_out16.py', 'test_a_captured_launch_draws_anew_at_every_replay',
                                               'qd_multi_uniform_global_out16_f32')),
        ('qd_multi_ste_backward_f32', ('test_hip_multi_ste.py', 'test_captures_and_replays_in_a_single_stream_graph', 'MultiTensorSTE')),
        ('qd_multi_uniform_buckets_f32', ('test_hip_multi_buckets.py', 'test_one_captured_step_of_quantize_and_ste_replays_as_two_eager_steps',
                                          'qd_multi_uniform_buckets_f32')),
        ('qd_multi_ste_backward_buckets_f32', ('test_hip_multi_buckets.py', 'test_one_captured_step_of_quantize_and_ste_replays_as_two_eager_steps',
                                               'qd_multi_ste_backward_buckets_f32')),
        ('qd_multi_uniform_symbols_u8', ('test_hip_symbols.py', 'test_one_captured_encode_replays_on_the_inputs_of_the_moment', 'MultiTensorSymbols')),
        ('qd_multi_nearest_out16_f32', ('test_hip_dq16.py', 'test_one_graph_of_forward_and_backward_replays_to_the_eager_bits',
                                        'qd_multi_nearest_out16_f32')),
        ('qd_multi_point_grad_in16_f32', ('test_hip_dq16.py', 'test_one_graph_of_forward_and_backward_replays_to_the_eager_bits',
                                          'qd_multi_point_grad_in16_f32')),
    ])),
    ('launches nothing', ('qd_abi_version', 'qd_target_arch', 'qd_error_string', 'qd_workspace_bytes', 'qd_set_single_fused_mode', 'qd_set_grid_cap',
                          'qd_num_buckets', 'qd_padded_length', 'qd_transform_plan', 'qd_multi_plan', 'qd_multi_global_plan', 'qd_multi_ste_plan',
                          'qd_multi_ste_in16_plan', 'qd_multi_buckets_plan', 'qd_multi_ste_buckets_plan', 'qd_multi_symbols_plan', 'qd_multi_dq_plan',
                          'qd_packed_bytes', 'qd_order_stats_workspace_bytes')),
    ('not capturable', collections.OrderedDict([
        ('qd_uniform_f32: seed', ('a by-value seed is frozen into the launch, every replay rounds with the same draws: the Python layer refuses',
                                  'test_hip_stochastic.py', 'test_stochastic_call_under_hipgraph_capture')),
        ('qd_multi_uniform_opt_f32: seed', ('the same by-value seed (a seed cell on the device is advanced by the launch and is capturable)',
                                            'test_hip_multi_stochastic.py', 'test_by_value_seed_is_refused_during_capture')),
    ])),
])
