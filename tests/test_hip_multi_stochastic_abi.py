"""The memory contract of qd_multi_uniform_global_opt_f32 and qd_multi_uniform_opt_f32 at the C ABI, with the helpers of
tests/abi_contract.py: every tensor at its own 16-byte phase in shared flat buffers with guard bands between them, outputs
pre-filled with a sentinel, the workspace at exactly total_tiles * 8 bytes and filled with zero bytes, 0xFF bytes and the
residue of larger calls (its contents are irrelevant), one byte less refused with nothing written.  The yardstick is
qd_uniform_f32 per tensor at seed + i, as the header states."""
import numpy as np
import pytest
import torch

import abi_contract as A
from quantized_distillation_amd import _lib
from quantized_distillation_amd.multi_tensor import MultiTensorQuantizer

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SEED = 0xFFFFFFFFFFFFFFFE            # tensor 2 and the ones behind it wrap past 2^64
S = 16


def _per_tensor(lib, x, bucket, clamp, me, stoch, seed):
    """qd_uniform_f32 on a copy of x in a buffer of its own: (q, alpha[0], beta[0])."""
    n = x.size
    xd = torch.from_numpy(x).to(DEV)
    q = torch.empty_like(xd)
    nb = lib.qd_num_buckets(n, bucket or 0)
    ab = torch.empty(2 * nb, device=DEV)
    ws = torch.empty(lib.qd_workspace_bytes(), dtype=torch.uint8, device=DEV)
    _lib.check(lib.qd_uniform_f32(xd.data_ptr(), q.data_ptr(), n, bucket or 0, S, ab.data_ptr(), ab.data_ptr() + 4 * nb, None, None,
                                  clamp, me, stoch, seed & 0xFFFFFFFFFFFFFFFF, ws.data_ptr(), ws.numel(), _lib.stream_ptr(DEV)))
    torch.cuda.synchronize(DEV)
    return q.cpu().numpy(), float(ab[0]), float(ab[nb])


@pytest.mark.parametrize('in_place', [False, True], ids=['out_of_place', 'in_place'])
@pytest.mark.parametrize('stoch,clamp', [(1, 0), (1, 1), (0, 1)])
@pytest.mark.parametrize('bucket', [256, None])
@pytest.mark.parametrize('nt', [7, 65])
def test_multi_tensor_uniform_with_options(nt, bucket, stoch, clamp, in_place):
    lib = _lib.load()
    me = 0.5                                     # (A.data: values of order one)
    sizes = A.MULTI_LISTS[nt]
    tag = ('K9 options', nt, bucket, stoch, clamp, in_place)
    with torch.cuda.device(DEV):
        xs = [A.data(n, bucket or 0, 600 + i) for i, n in enumerate(sizes)]
        fx = A.Flat(sizes, A.F32, DEV, 'inout' if in_place else 'in', xs)
        fq = fx if in_place else A.Flat(sizes, A.F32, DEV, 'out', phases=[(0, 4, 8, 12)[(i + 3) % 4] for i in range(nt)])
        mt = MultiTensorQuantizer(fx.views(), S, bucket, outputs=fq.views())          # the plan and the table; the launches below are ours
        wants = [_per_tensor(lib, x, bucket, clamp, me, stoch, SEED + i) if x.size else None for i, x in enumerate(xs)]
        cell = A.Placed(A.inp(np.array([SEED], np.uint64), 8, guard=('index', 0)), DEV)            # the device seed word, read only
        results = []
        for fill, seed_cell in zip(A.FILLS if bucket is None else A.FILLS[:2], (None, cell.ptr, None)):
            (fq if not in_place else fx).buf.copy_(torch.from_numpy((fq if not in_place else fx).image.copy()))
            seed = SEED if seed_cell is None else 12345          # with a cell the by-value seed is not used
            st = _lib.stream_ptr(DEV)
            if bucket is None:
                nbytes = max(mt._tiles, 1) * 2 * 4
                ws = A.Placed(A.Arr('out', A.U8, None, nbytes, 0, 'sentinel', None), DEV)
                ws.fill(A._ws_bytes(fill, nbytes, lib, DEV))
                ab = A.Placed(A.out(A.F32, 2 * nt, 4), DEV)
                rc = lib.qd_multi_uniform_global_opt_f32(mt._table.data_ptr(), nt, mt._tiles, S, clamp, me, stoch, seed, seed_cell,
                                                         ab.ptr, ws.ptr, nbytes - 1, st)
                torch.cuda.synchronize(DEV)
                assert rc == A.ERR_WS and ab.untouched(ab.read(tag, 'alpha_beta')), (tag, rc)
                if not in_place:
                    assert all(np.array_equal(o.view(np.uint32), np.full(o.size, A.F_SENT, np.uint32))
                               for o in [v.cpu().numpy() for v in fq.views()]), (tag, 'a refused call wrote an output')
                rc = lib.qd_multi_uniform_global_opt_f32(mt._table.data_ptr(), nt, mt._tiles, S, clamp, me, stoch, seed, seed_cell,
                                                         ab.ptr, ws.ptr, nbytes, st)
            else:
                rc = lib.qd_multi_uniform_opt_f32(mt._table.data_ptr(), nt, mt._tiles, bucket, S, clamp, me, stoch, seed, seed_cell, st)
            torch.cuda.synchronize(DEV)
            assert rc == 0, (tag, rc)
            got = fq.read(tag, 'q')
            if not in_place:
                fx.read(tag, 'x')
            cell.read(tag, 'seed_cell')
            for i, (g, w) in enumerate(zip(got, wants)):
                if w is not None:
                    assert A._same(g, w[0]), (tag, fill, 'tensor %d of %d elements differs from qd_uniform_f32 at seed + %d' % (i, sizes[i], i))
            if bucket is None:
                ws.read(tag, 'workspace')
                abv = ab.read(tag, 'alpha_beta')
                ab.assert_no_sentinel(abv, tag, 'alpha_beta')
                want_ab = np.array([[w[1], w[2]] if w is not None else [1.0, np.inf] for w in wants], np.float32).reshape(-1)
                assert A._same(abv, want_ab), (tag, fill, 'alpha_beta')
            results.append(got)
        for r in results[1:]:
            assert all(A._same(a, b) for a, b in zip(r, results[0])), (tag, 'differs between workspace fills / seed sources')
