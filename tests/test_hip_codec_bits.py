"""The packed codec at 3, 5, 6 and 7 bits per level index on the device (tests/codec_bits_cases.py): the three entry points
between guard bands against the numpy reference of the stream and the oracle's levels, bit for bit -- every fused bucket
size, ragged tails, every word phase of `packed`, byte phases of the levels, bucket geometries of the decode; the later
trips of the grid-stride loops under qd_set_grid_cap; the fused pack against qd_uniform_f32 + qd_pack_levels_u8 and the 3-bit
against the 4-bit stream of the same levels; NaN, +-inf and constant buckets; every new width recorded into a graph and
replayed on other data; codec.pack_uniform(bits=...)."""
import numpy as np
import pytest
import torch

import abi_contract as A
import codec_bits_cases as B
from quantized_distillation_amd import _lib, codec

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def run(c, lib):
    with torch.cuda.device(DEV):
        return A.run_case(c, lib, DEV)


# ---------------------------------------------------------------- 1. the memory contract
@pytest.mark.parametrize('bucket', B.FUSED_BUCKETS)
@pytest.mark.parametrize('bits', B.NEW_BITS)
def test_fused_pack_between_guards(lib, bits, bucket):
    """qd_pack_uniform_f32: k_pack_vec on ten full buckets + k_pack_tail on 0, 3 and bucket - 1 more elements; 2^bits levels
    and a count that does not fill the width; `packed` at every word of a 16-byte granule; with and without alpha / beta."""
    ran = 0
    for c in B.pack_cases(bits, bucket):
        got = run(c, lib)
        assert len(got['packed']) == B.packed_bytes(c.args[1], bits)
        ran += 1
    assert ran == 48


@pytest.mark.parametrize('bits', B.NEW_BITS)
def test_pack_levels_between_guards(lib, bits):
    """qd_pack_levels_u8: 5, 31, 32, 33 and 2563 symbols of the whole uint8 range (masked to `bits` bits), the levels at every
    byte phase, `packed` at +0 ... +3."""
    for c in B.levels_cases(bits):
        run(c, lib)


@pytest.mark.parametrize('bucket', B.UNPACK_BUCKETS)
@pytest.mark.parametrize('bits', B.NEW_BITS)
def test_unpack_between_guards(lib, bits, bucket):
    """qd_unpack_uniform_f32: k_unpack (bucket 256) and k_unpack_any (no buckets, 100, 3: a group of four crosses two
    buckets), n % 4 != 0, y at every 4-byte phase, 0xFF bytes behind the stream; equal to the oracle's q bit for bit."""
    for c in B.unpack_cases(bits, bucket):
        run(c, lib)


def test_refusals_write_nothing(lib):
    """What the entry points refuse at the new widths (pointers and lengths as for a valid call): nothing is written."""
    x, r, lev = B.quantized(2563, 256, 8, 1)
    for tag, bits, levels, bucket, px, pp, rc in (('levels 9 at 3 bits', 3, 9, 256, 0, 0, A.ERR_INVALID),
                                                  ('bucket 100 at 3 bits', 3, 8, 100, 0, 0, A.ERR_UNSUPPORTED),
                                                  ('x at +4 at 5 bits', 5, 32, 256, 4, 0, A.ERR_UNSUPPORTED),
                                                  ('packed at +1 at 7 bits', 7, 128, 256, 0, 1, A.ERR_UNSUPPORTED)):
        run(A.case(tag, 'qd_pack_uniform_f32', [('x', A.inp(x, px)), ('packed', A.out(A.U8, 2563, pp))],
                   [A.Ref('x'), 2563, bucket, levels, bits, A.Ref('packed'), None, None, A.STREAM], None, rc=rc), lib)
    run(A.case('unpack, packed at +2 at 6 bits', 'qd_unpack_uniform_f32',
               [('packed', A.inp(lev, 2, ('index', 0))), ('alpha', A.inp(r['alpha'], 0)), ('beta', A.inp(r['beta'], 0)), ('y', A.out(A.F32, 2563, 0))],
               [A.Ref('packed'), 2563, 256, 64, 6, A.Ref('alpha'), A.Ref('beta'), A.Ref('y'), A.STREAM], None, rc=A.ERR_UNSUPPORTED), lib)


# ---------------------------------------------------------------- 2. later trips
def under_caps(lib, c):
    """The case under the default grid and under caps of 1 and 2 blocks: the reference's bits (run_case) and the same bits
    as the uncapped call."""
    base = run(c, lib)
    for cap in (1, 2):
        prev = lib.qd_set_grid_cap(cap)
        try:
            got = run(c, lib)
        finally:
            lib.qd_set_grid_cap(prev)
        assert list(got) == list(base)
        for name in got:
            assert got[name].tobytes() == base[name].tobytes(), (c.tag, name, cap)
    assert lib.qd_set_grid_cap(-1) == 1 << 20


@pytest.mark.parametrize('bits', B.NEW_BITS)
def test_later_trips_of_the_grid_stride_loops(lib, bits):
    nfull, bucket, rest = B.TRIP_PACK
    under_caps(lib, B.pack_case(bits, 1 << bits, bucket, nfull * bucket + rest, 0, True))
    for plev in (0, 1):                                            # the 16-byte loads, and the byte path
        under_caps(lib, B.levels_case(bits, B.TRIP_LEVELS_N, plev, 0))
    for ub in (256, 100):                                          # k_unpack, k_unpack_any
        under_caps(lib, B.unpack_case(bits, 1 << bits, ub, B.TRIP_UNPACK_N, 0, 4))


# ---------------------------------------------------------------- 3. agreement between paths
@pytest.mark.parametrize('bits', B.NEW_BITS)
def test_fused_pack_equals_quantize_then_pack_levels(lib, bits):
    n, bucket = 10 * 256 + 255, 256
    for levels in B.level_counts(bits):
        x = torch.from_numpy(A.data(n, bucket, 40 + bits)).to(DEV)
        nbytes = int(lib.qd_packed_bytes(n, bits))
        fused = torch.full((nbytes,), 0xEE, dtype=torch.uint8, device=DEV)
        two = torch.full((nbytes,), 0xEE, dtype=torch.uint8, device=DEV)
        lev = torch.empty(n, dtype=torch.uint8, device=DEV)
        q = torch.empty_like(x)
        ws = _lib.workspace(DEV)
        with torch.cuda.device(DEV):
            st = _lib.stream_ptr()
            assert lib.qd_pack_uniform_f32(x.data_ptr(), n, bucket, levels, bits, fused.data_ptr(), None, None, st) == 0
            assert lib.qd_uniform_f32(x.data_ptr(), q.data_ptr(), n, bucket, levels, None, None, lev.data_ptr(), None, 0, 0.0, 0, 0,
                                      ws.data_ptr(), ws.numel(), st) == 0
            assert lib.qd_pack_levels_u8(lev.data_ptr(), n, bits, two.data_ptr(), st) == 0
        assert torch.equal(fused, two), (bits, levels)
        assert np.array_equal(B.unpack_stream(fused.cpu().numpy(), n, bits), lev.cpu().numpy())


def test_the_3_bit_and_the_4_bit_stream_of_8_levels_decode_to_the_same_floats(lib):
    for bucket, n in ((256, 2563), (100, 2563), (None, 1000)):
        x = torch.from_numpy(A.data(n, bucket or 0, 55)).to(DEV)
        p3, p4 = codec.pack_uniform(x, 8, bucket, bits=3), codec.pack_uniform(x, 8, bucket, bits=4)
        assert p3.packed.numel() == (3 * n + 7) // 8 and p4.packed.numel() == (n + 1) // 2
        assert torch.equal(p3.unpack().view(torch.int32), p4.unpack().view(torch.int32)), bucket


# ---------------------------------------------------------------- 4. non-finite and constant buckets
@pytest.mark.parametrize('bits', B.NEW_BITS)
def test_nan_inf_and_constant_buckets(lib, bits):
    bucket, levels = 256, 1 << bits
    x = B.nonfinite_input(bucket)
    n = x.size
    got = run(B.pack_case(bits, levels, bucket, n, 0, True, x=x), lib)            # the oracle's levels, alpha and beta
    lev = B.unpack_stream(got['packed'], n, bits)
    assert not lev[bucket:2 * bucket].any() and not lev[5 * bucket:].any()       # a NaN bucket packs zeros
    assert np.isnan(got['alpha'][[1, 5]]).all() and got['alpha'][3] == 1.0       # the constant bucket: alpha -> 1
    assert not lev[3 * bucket:4 * bucket].any() and lev[:bucket].max() == levels - 1 and lev[4 * bucket:5 * bucket].max() == levels - 1
    with np.errstate(invalid='ignore'):
        r = B.oc.uniform_quantize(x, levels, bucket, want_idx=False)
    y = run(A.case('unpack the non-finite buckets, bits %d' % bits, 'qd_unpack_uniform_f32',
                   [('packed', A.inp(got['packed'], 0, ('index', 0xFF))), ('alpha', A.inp(got['alpha'], 8)), ('beta', A.inp(got['beta'], 4)),
                    ('y', A.out(A.F32, n, 4))],
                   [A.Ref('packed'), n, bucket, levels, bits, A.Ref('alpha'), A.Ref('beta'), A.Ref('y'), A.STREAM],
                   (lambda: {'y': r['q'].reshape(-1)})), lib)['y']
    nan_buckets = np.isnan(np.concatenate([y, np.zeros(-n % bucket, np.float32)]).reshape(-1, bucket)).any(axis=1)
    assert list(nan_buckets) == [False, True, True, False, False, True]          # NaN, +-inf (inf - inf) and the NaN tail only
    assert np.isnan(y[bucket:2 * bucket]).all() and np.isnan(y[5 * bucket:]).all()
    assert np.array_equal(y[3 * bucket:4 * bucket], x[3 * bucket:4 * bucket])


# ---------------------------------------------------------------- 5. graph capture
@pytest.mark.parametrize('bits', B.NEW_BITS)
def test_recorded_once_and_replayed_on_other_data(lib, bits):
    levels = B.PARTIAL_LEVELS[bits] if bits in (5, 7) else 1 << bits
    with torch.cuda.device(DEV):
        A.run_case_captured([B.pack_case(bits, levels, 256, 10 * 256 + 3, 4, True, v) for v in A.VARIANTS], lib, DEV)
        A.run_case_captured([B.levels_case(bits, 10 * 256 + 3, 1, 0, v) for v in A.VARIANTS], lib, DEV)
        A.run_case_captured([B.unpack_case(bits, levels, 256, 10 * 256 + 3, 0, 4, v) for v in A.VARIANTS], lib, DEV)
        A.run_case_captured([B.unpack_case(bits, levels, 100, 10 * 256 + 3, 8, 12, v) for v in A.VARIANTS], lib, DEV)


# ---------------------------------------------------------------- 6. Python
S_AND_BITS = ((5, 3), (8, 3), (3, 5), (17, 5), (32, 5), (33, 6), (64, 6), (65, 7), (128, 7))


@pytest.mark.parametrize('s,bits', S_AND_BITS)
def test_pack_uniform_with_bits(s, bits):
    """pack_uniform(x, s, bucket, bits=b).unpack() is uniformQuantization(x, s, bucket)[0] bit for bit on both of its paths:
    the fused kernel (bucket 256) and quantize + pack_levels (bucket 100, no buckets, a view 4 bytes into a granule)."""
    import quantization
    n = 10 * 256 + 3
    base = torch.from_numpy(A.data(n + 1, 256, 60 + s)).to(DEV)
    assert base.data_ptr() % 16 == 0
    for x, bucket in ((base[:n].clone(), 256), (base[:n].clone(), 100), (base[:n].clone(), None), (base[1:], 256)):
        assert (x.data_ptr() % 16 == 4) == (x.data_ptr() == base.data_ptr() + 4)
        pk = codec.pack_uniform(x.view(11, 233), s, bucket, bits=bits)
        want = quantization.uniformQuantization(x.view(11, 233), s, bucket_size=bucket)[0]
        got = pk.unpack()
        assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32)), (s, bits, bucket)
        buckets = 1 if bucket is None else -(-n // bucket)
        assert pk.bits == bits and pk.packed.numel() == (n * bits + 7) // 8
        assert pk.nbytes == (n * bits + 7) // 8 + 8 * buckets


def test_pack_uniform_bits_argument():
    x = torch.from_numpy(A.data(2563, 256, 3)).to(DEV)
    for bad in (0, 9, True, -1, 3.0, '3'):
        with pytest.raises(ValueError, match='from 1 to 8'):
            codec.pack_uniform(x, 2, 256, bits=bad)
    for s, bits in ((9, 3), (33, 5), (65, 6), (129, 7), (3, 1)):
        with pytest.raises(ValueError, match='hold s levels'):
            codec.pack_uniform(x, s, 256, bits=bits)
    assert codec.pack_uniform(x, 8, 256).bits == 4                 # bits=None: bits_for_levels, as before
    assert codec.pack_uniform(x, 5, 256).bits == 4 and codec.pack_uniform(x, 17, 256).bits == 8
    assert codec.pack_uniform(x, 8, 256, bits=codec.min_bits_for_levels(8)).bits == 3
