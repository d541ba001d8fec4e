"""Writes tests/golden/abi_contract_variant0.json: one SHA-256 per case of tests/abi_contract.py over what the case feeds the
entry point -- every placed input (name, dtype, phase, bytes), the shape, type and phase of every output, the by-value arguments
and the host arrays (the ranks of K10).  Run at the commit BEFORE the case generators took a `variant` argument, so that
tests/test_abi_contract_host.py can hold variant 0 to the data every earlier test saw:

    python tests/golden/gen_abi_contract_digests.py            (needs the built libraries, no GPU)

Uses only what the module had at that commit (GROUPS, cases_of), so it runs unchanged on either side of the change."""
import collections
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import abi_contract as A                                   # noqa: E402
from quantized_distillation_amd import _lib                # noqa: E402


def case_digest(c):
    h = hashlib.sha256()
    h.update(repr((c.entry, c.tag, c.ws_bytes, c.uses_ws, c.rc, c.fused_mode)).encode())
    for name, a in c.arrays.items():
        h.update(repr((name, a.role, a.dtype.str, a.n, a.phase, a.guard, a.valid_max)).encode())
        if a.data is not None:
            h.update(np.ascontiguousarray(a.data).tobytes())
    for v in c.args:
        if isinstance(v, np.ndarray):
            h.update(repr(('host', v.dtype.str, v.shape)).encode())
            h.update(np.ascontiguousarray(v).tobytes())
        else:
            h.update(repr(v).encode())
    return h.hexdigest()


def group_digests(group, lib):
    """'<index> <tag>' -> digest, in the order the group yields its cases."""
    return collections.OrderedDict(('%d %s' % (i, c.tag), case_digest(c)) for i, c in enumerate(A.cases_of(group, lib)))


def main():
    lib = _lib.load()
    out = collections.OrderedDict((gid, group_digests(g, lib)) for gid, g in A.GROUPS.items())
    path = os.path.join(HERE, 'abi_contract_variant0.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=0, separators=(',', ':'))
        f.write('\n')
    print('wrote %s: %d groups, %d cases' % (path, len(out), sum(len(v) for v in out.values())))


if __name__ == '__main__':
    main()
