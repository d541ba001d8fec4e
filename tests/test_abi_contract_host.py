"""The groups of tests/abi_contract.py whose entry points libqd_host.so has (_lib.HOST_SYMBOLS), on CPU buffers: every array at
its own 16-byte phase between guard bands, outputs pre-filled with a sentinel, against the oracle bit for bit.  Proves the
cases and the host library -- whose AVX-512 / AVX2 / SSE2 clones have masked tails of their own -- without a GPU, before
tests/test_hip_abi_contract.py holds libqd_hip.so to the same table."""
import pytest

import abi_contract as A
from quantized_distillation_amd import _lib


def test_the_group_table_names_host_entry_points_only():
    for gid in A.HOST_GROUP_IDS:
        for entry in A.GROUPS[gid].entry.split(' / '):
            assert entry in _lib.HOST_SYMBOLS, (gid, entry)
    assert len(set(A.DEVICE_GROUP_IDS)) == len(A.DEVICE_GROUP_IDS) and set(A.HOST_GROUP_IDS) < set(A.DEVICE_GROUP_IDS)


@pytest.mark.parametrize('gid', A.HOST_GROUP_IDS)
def test_host_group(gid):
    assert A.run_group(A.GROUPS[gid], _lib.host(), 'cpu')
