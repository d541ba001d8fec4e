"""Every group of tests/abi_contract.py through libqd_hip.so at the C ABI: each array of a call at its own 16-byte phase between
guard bands, outputs pre-filled with a sentinel, the workspace at exactly its documented size and filled with zero bytes, 0xFF
bytes and the residue of larger calls -- against the oracle bit for bit, the three runs against each other, and, where
libqd_host.so has the entry point, the two libraries against each other in the same carved layout."""
import pytest
import torch

import abi_contract as A
from quantized_distillation_amd import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.mark.parametrize('gid', A.DEVICE_GROUP_IDS)
def test_device_group(gid):
    group = A.GROUPS[gid]
    with torch.cuda.device(DEV):
        dev = A.run_group(group, _lib.load(), DEV)
    assert dev
    if group.host or '-mode' in gid:                         # (the give-up hooks exist on the device only: same result in every mode)
        host = A.run_group(group, _lib.host(), 'cpu', fills=A.FILLS[:1], keep_mode=False)
        A.same_results(dev, host)


@pytest.mark.parametrize('in_place', [False, True])
@pytest.mark.parametrize('bucket', [256, 100, None])
@pytest.mark.parametrize('nt', [1, 7, 65])
def test_multi_tensor_uniform(nt, bucket, in_place):
    """K9, bucketed and global (three workspace fills, alpha_beta between guards): lists of 1, 7 and 65 tensors of 1 .. 70001
    elements, every tensor at its own phase in the shared flat buffers, guards between all of them."""
    with torch.cuda.device(DEV):
        A.run_multi_uniform(nt, bucket, in_place, _lib.load(), DEV)


@pytest.mark.parametrize('bucket,k', [(256, 16), (64, 64), (1024, 2)])
@pytest.mark.parametrize('nt', [1, 7, 65])
def test_multi_tensor_diff_quant(nt, bucket, k):
    """K5m forward and K6m backward on carved columns, the scratch at exactly total_blocks * k floats."""
    with torch.cuda.device(DEV):
        A.run_multi_dq(nt, bucket, k, _lib.load(), DEV)
