"""The groups of tests/abi_contract.py whose entry points libqd_host.so has (_lib.HOST_SYMBOLS), on CPU buffers: every array at
its own 16-byte phase between guard bands, outputs pre-filled with a sentinel, against the oracle bit for bit.  Proves the
cases and the host library -- whose AVX-512 / AVX2 / SSE2 clones have masked tails of their own -- without a GPU, before
tests/test_hip_abi_contract.py holds libqd_hip.so to the same table.

Also the CPU side of tests/test_hip_capture_abi.py (a launch recorded on variant 0 of a case and replayed on variants 1 and 2):
the three variants of every group differ in array contents and in nothing else, variant 0 is the data every earlier test saw
(tests/golden/abi_contract_variant0.json, written at the commit before the generators took a variant), variants 1 and 2 of
the host groups pass through libqd_host.so against their own expect() -- the new data lies inside the oracle's domain -- and
the capture ledger names every entry point of the header exactly once."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest

import abi_contract as A
from quantized_distillation_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))


def test_the_group_table_names_host_entry_points_only():
    for gid in A.HOST_GROUP_IDS:
        for entry in A.GROUPS[gid].entry.split(' / '):
            assert entry in _lib.HOST_SYMBOLS, (gid, entry)
    assert len(set(A.DEVICE_GROUP_IDS)) == len(A.DEVICE_GROUP_IDS) and set(A.HOST_GROUP_IDS) < set(A.DEVICE_GROUP_IDS)


@pytest.mark.parametrize('gid', A.HOST_GROUP_IDS)
def test_host_group(gid):
    assert A.run_group(A.GROUPS[gid], _lib.host(), 'cpu')


# ---------------------------------------------------------------- the data variants
def _digests():
    spec = importlib.util.spec_from_file_location('gen_abi_contract_digests', os.path.join(HERE, 'golden', 'gen_abi_contract_digests.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _shape_of(c):
    """Everything of a case but the contents of its arrays."""
    arrays = [(name, a.role, a.dtype.str, a.n, a.phase, a.guard, a.valid_max) for name, a in c.arrays.items()]
    args = [('host', v.dtype.str, v.shape, v.tobytes()) if isinstance(v, np.ndarray) else v for v in c.args]
    return (c.tag, c.entry, arrays, args, c.ws_bytes, c.uses_ws, c.rc, c.fused_mode, c.expect is None)


def test_variant_0_is_the_data_of_the_parent_commit():
    with open(os.path.join(HERE, 'golden', 'abi_contract_variant0.json')) as f:
        want = json.load(f)
    gen, lib = _digests(), _lib.load()                  # (loading libqd_hip.so needs no GPU: the workspace sizes of two groups)
    assert list(want) == list(A.GROUPS)
    for gid, group in A.GROUPS.items():
        got = gen.group_digests(group, lib)
        assert list(got) == list(want[gid]), (gid, 'other cases, or another order')
        changed = [t for t in got if got[t] != want[gid][t]]
        assert not changed, (gid, 'variant 0 is no longer the data the fixture was written from', changed[:3])


@pytest.mark.parametrize('gid', A.DEVICE_GROUP_IDS)
def test_variants_agree_in_everything_but_contents(gid):
    lib = _lib.load()
    v0, v1, v2 = ([c for c in A.cases_of(A.GROUPS[gid], lib, v)] for v in A.VARIANTS)
    assert len(v0) == len(v1) == len(v2) > 0
    differ = {1: 0, 2: 0}
    for c0, c1, c2 in zip(v0, v1, v2):
        assert _shape_of(c0) == _shape_of(c1) == _shape_of(c2), (gid, c0.tag)
        for v, c in ((1, c1), (2, c2)):
            differ[v] += any(a.data is not None and a.data.size and not A._same(a.data, c0.arrays[name].data) for name, a in c.arrays.items())
    assert differ[1] and differ[2], (gid, 'a variant with the contents of variant 0', differ)
    if all(c.rc == 0 for c in v0):                       # (a refused case may be one element: nothing to vary)
        assert differ[1] >= len(v0) // 2 and differ[2] >= len(v0) // 2, (gid, differ, len(v0))


@pytest.mark.parametrize('variant', [1, 2])
@pytest.mark.parametrize('gid', A.HOST_GROUP_IDS)
def test_host_group_on_the_variants(gid, variant):
    """One workspace fill: libqd_host.so takes no scratch."""
    got = A.run_group(A.GROUPS[gid], _lib.host(), 'cpu', fills=A.FILLS[:1], variant=variant)
    assert got


# ---------------------------------------------------------------- the capture ledger
def test_every_entry_point_has_exactly_one_capture_stance():
    """A new entry point of include/qd_hip.h without a stance on capture fails here, without a GPU."""
    named = [e for column in A.CAPTURE.values() for e in column if ':' not in e]
    assert sorted(named) == sorted(_lib.SIGNATURES), (sorted(set(_lib.SIGNATURES) - set(named)), sorted(set(named) - set(_lib.SIGNATURES)),
                                                      sorted(e for e in set(named) if named.count(e) > 1))
    for key in A.CAPTURE['not capturable']:                 # the stance of one ARGUMENT of an entry point listed above
        assert ':' not in key or key.split(':')[0] in named, key


def test_the_capture_ledger_points_at_what_exists():
    lib = _lib.load()
    of_group = {gid: {c.entry for c in A.cases_of(g, lib)} for gid, g in A.GROUPS.items()}
    for entry, where in A.CAPTURE['here'].items():
        assert where, entry
        for gid in where:
            if gid in A.GROUPS:
                assert entry in of_group[gid] and '-mode' not in gid, (entry, gid)
            else:                                        # a test function of tests/test_hip_capture_abi.py
                _assert_test_mentions(entry, 'test_hip_capture_abi.py', gid, entry)
    for entry, (fname, test, mention) in A.CAPTURE['elsewhere'].items():
        _assert_test_mentions(entry, fname, test, mention)
    for entry, (reason, fname, test) in A.CAPTURE['not capturable'].items():
        assert reason and '\n' not in reason
        _assert_test_mentions(entry, fname, test, None)
    # every group is replayed, but for the hook groups (they add nothing under capture)
    replayed = {gid for where in A.CAPTURE['here'].values() for gid in where}
    assert {gid for gid in A.GROUPS if '-mode' not in gid} <= replayed


def _assert_test_mentions(entry, fname, test, mention):
    with open(os.path.join(HERE, fname)) as f:
        text = f.read()
    assert re.search(r'^def %s\(' % re.escape(test), text, re.M), (entry, fname, test, 'no such test function')
    assert mention is None or mention in text, (entry, fname, 'does not mention %s' % mention)
