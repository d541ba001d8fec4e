"""tests/codec_bits_cases.py held on the CPU: its numpy reference of the packed stream against abi_contract.pack_bits (the
widths that had one) and against its own inverse, what every shape of the case list is there for, the argument checks of the
three codec entry points of libqd_hip.so at the widths 3, 5, 6 and 7 (no launch: this runs without a GPU), and
codec.min_bits_for_levels."""
import numpy as np
import pytest

import abi_contract as A
import codec_bits_cases as B
from quantized_distillation_amd import _lib
from quantized_distillation_amd import build as qb
from quantized_distillation_amd import codec


@pytest.fixture(scope='module')
def lib():
    qb.build_extension()
    return _lib.load()


# ---------------------------------------------------------------- the reference
@pytest.mark.parametrize('bits', B.OLD_BITS)
def test_reference_equals_pack_bits_where_an_element_lies_inside_a_byte(bits):
    for n in (0, 1, 5, 8, 9, 2563):
        lev = np.random.RandomState(n + bits).randint(0, 1 << bits, n).astype(np.uint8)
        assert np.array_equal(B.pack_stream(lev, bits), A.pack_bits(lev, bits)), (bits, n)


@pytest.mark.parametrize('bits', range(1, 9))
def test_reference_round_trips_and_pads_with_zero_bits(bits):
    for n in (0, 1, 2, 3, 5, 7, 8, 9, 31, 32, 33, 2563):
        lev = np.random.RandomState(100 + n + bits).randint(0, 1 << bits, n).astype(np.uint8)
        lev[-3:] = (1 << bits) - 1                                 # all ones in front of the padding
        stream = B.pack_stream(lev, bits)
        assert stream.dtype == np.uint8 and len(stream) == B.packed_bytes(n, bits) == (n * bits + 7) // 8
        assert np.array_equal(B.unpack_stream(stream, n, bits), lev), (bits, n)
        used = n * bits - 8 * (len(stream) - 1)                    # bits of the last byte that belong to an element
        if n and used < 8:
            assert stream[-1] >> used == 0, (bits, n, 'the unused high bits of the last byte are zero')


def test_reference_states_the_format_bit_by_bit():
    """Bit i of the stream is bit i & 7 of byte i >> 3; element e holds its index LSB first in stream bits [e b, (e + 1) b)."""
    for bits in range(1, 9):
        lev = np.random.RandomState(bits).randint(0, 1 << bits, 77).astype(np.uint8)
        stream = B.pack_stream(lev, bits)
        for e in range(77):
            got = 0
            for j in range(bits):
                i = e * bits + j
                got |= ((int(stream[i >> 3]) >> (i & 7)) & 1) << j
            assert got == lev[e], (bits, e)


# ---------------------------------------------------------------- what the shapes are there for
@pytest.mark.parametrize('bits', B.NEW_BITS)
def test_every_shape_is_there_for_a_reason(bits):
    assert not any(B.straddles_byte(64, b) for b in B.OLD_BITS) and B.straddles_byte(64, bits) and B.straddles_word(64, bits)
    assert B.PARTIAL_LEVELS[bits] == (1 << (bits - 1)) + 1       # the smallest count that needs the width
    # fused pack: every fused bucket size; a whole-byte end, a partial last byte, the longest ragged row
    for bucket in B.FUSED_BUCKETS:
        ns = B.pack_lengths(bucket)
        assert [n % bucket for n in ns] == [0, 3, bucket - 1] and all(n // bucket == 10 for n in ns)
        assert (bucket * bits) % 32 == 0                           # a bucket row is whole words
        assert any(B.partial_last_byte(n, bits) for n in ns) and all(B.straddles_word(n, bits) for n in ns)
        tags = [c.tag for c in B.pack_cases(bits, bucket)]
        assert len(tags) == len(set(tags)) == 2 * 3 * 4 * 2
        for levels in B.level_counts(bits):
            for pp in B.PACKED_PHASES:
                assert sum('levels %d ' % levels in t and t.endswith('packed+%d' % pp) for t in tags) == 3
                assert sum('levels %d ' % levels in t and 'packed+%d without' % pp in t for t in tags) == 3
    # the ragged tail of 3 elements: already there an element straddles a byte (3 bits: element 2 holds stream bits 6 .. 8)
    assert B.straddles_byte(3, bits)
    # pack_levels: below one group of 32 levels, one short of it, exactly one, one more, and many with a ragged end
    assert B.LEVEL_NS == (5, 31, 32, 33, 2563)
    assert [n // 32 for n in B.LEVEL_NS] == [0, 0, 1, 1, 80] and B.straddles_byte(5, bits)
    assert any(B.partial_last_byte(n, bits) for n in B.LEVEL_NS)
    assert any(B.partial_last_byte(n, bits) and n % 32 for n in B.LEVEL_NS)
    assert len(list(B.levels_cases(bits))) == len(B.LEVEL_NS) * 7
    # unpack: a partial last group of four in every n; a last 32-bit word that is partial (read byte by byte) in at least one
    assert all(n % 4 for n in B.UNPACK_NS)
    assert any(B.packed_bytes(n, bits) % 4 for n in B.UNPACK_NS)
    assert any(B.partial_last_byte(n, bits) for n in B.UNPACK_NS)
    assert B.UNPACK_BUCKETS == (256, 0, 100, 3)
    for bucket in B.UNPACK_BUCKETS:
        tags = [c.tag for c in B.unpack_cases(bits, bucket)]
        assert len(tags) == len(set(tags)) == 2 * len(B.UNPACK_NS) * 7
        for py in B.Y_PHASES:
            assert any(t.endswith('packed+0 y+%d' % py) for t in tags)
    # the later trips: a thread / wave of a grid of one or two blocks comes round at least three times
    nfull, bucket, rest = B.TRIP_PACK
    assert -(-nfull // 4) >= 3 * 2 * 4                             # tiles of four buckets over 2 blocks x 4 waves
    assert B.TRIP_LEVELS_N // 32 >= 3 * 2 * 256 and B.TRIP_LEVELS_N % 32 and B.partial_last_byte(B.TRIP_LEVELS_N, bits)
    assert -(-B.TRIP_UNPACK_N // 4) >= 3 * 2 * 256 and B.TRIP_UNPACK_N % 4


def test_case_expectations_are_the_reference_of_the_oracle_levels():
    """One case of each entry point, read back through the reference's inverse."""
    c = B.pack_case(3, 8, 64, 643, 0, True)
    w = c.expect()
    x, r, lev = B.quantized(643, 64, 8, B._seed(3, 643))
    assert np.array_equal(B.unpack_stream(w['packed'], 643, 3), lev) and lev.max() == 7 and len(w['packed']) == 242
    assert c.args[1:5] == [643, 64, 8, 3]
    c = B.levels_case(5, 33, 1, 0)
    assert np.array_equal(B.unpack_stream(c.expect()['packed'], 33, 5), B.levels_input(5, 33) & 31)
    assert B.levels_input(5, 33).max() > 31                        # the mask is exercised
    c = B.unpack_case(7, 65, 3, 2563, 0, 4)
    assert c.arrays['alpha'].n == 855 and c.expect()['y'].shape == (2563,)


# ---------------------------------------------------------------- libqd_hip.so without a GPU: the argument checks
@pytest.mark.parametrize('bits', B.NEW_BITS)
def test_an_empty_tensor_is_accepted_at_the_new_widths(lib, bits):
    """n == 0 returns 0 without a launch at every width the format has (QD_ERR_INVALID_ARGUMENT before the widths 3, 5, 6, 7)."""
    levels = 1 << bits
    assert lib.qd_pack_uniform_f32(None, 0, 256, levels, bits, None, None, None, None) == 0
    assert lib.qd_pack_uniform_f32(None, 0, 2048, B.PARTIAL_LEVELS[bits], bits, None, None, None, None) == 0
    assert lib.qd_pack_levels_u8(None, 0, bits, None, None) == 0
    assert lib.qd_unpack_uniform_f32(None, 0, 256, levels, bits, None, None, None, None) == 0
    assert lib.qd_unpack_uniform_f32(None, 0, 100, levels, bits, None, None, None, None) == 0
    assert lib.qd_packed_bytes(0, bits) == 0 and lib.qd_packed_bytes(3, bits) == (3 * bits + 7) // 8


def test_widths_outside_one_to_eight_and_too_many_levels_are_refused(lib):
    for bits in (0, 9, -1):
        assert lib.qd_pack_uniform_f32(None, 0, 256, 2, bits, None, None, None, None) == A.ERR_INVALID, bits
        assert lib.qd_pack_levels_u8(None, 0, bits, None, None) == A.ERR_INVALID, bits
        assert lib.qd_unpack_uniform_f32(None, 0, 256, 2, bits, None, None, None, None) == A.ERR_INVALID, bits
    for bits, levels in ((3, 9), (5, 33), (6, 65), (7, 129)):
        assert lib.qd_pack_uniform_f32(None, 0, 256, levels, bits, None, None, None, None) == A.ERR_INVALID, bits
        assert lib.qd_unpack_uniform_f32(None, 0, 256, levels, bits, None, None, None, None) == A.ERR_INVALID, bits
        assert lib.qd_pack_uniform_f32(None, 0, 256, levels - 1, bits, None, None, None, None) == 0, bits


def test_pack_refuses_other_bucket_sizes_at_the_new_widths(lib):
    for bits in B.NEW_BITS:
        assert lib.qd_pack_uniform_f32(None, 0, 100, 1 << bits, bits, None, None, None, None) == A.ERR_UNSUPPORTED, bits
    # in the order of the checks: the width comes first
    assert lib.qd_pack_uniform_f32(None, 0, 100, 8, 9, None, None, None, None) == A.ERR_INVALID


# ---------------------------------------------------------------- codec.min_bits_for_levels
def test_min_bits_for_levels():
    want = {2: 1, 3: 2, 4: 2, 5: 3, 8: 3, 9: 4, 16: 4, 17: 5, 32: 5, 33: 6, 64: 6, 65: 7, 128: 7, 129: 8, 256: 8}
    for s, b in want.items():
        assert codec.min_bits_for_levels(s) == b, s
    for s in range(2, 257):
        b = codec.min_bits_for_levels(s)
        assert (1 << (b - 1)) < s <= (1 << b) and b <= codec.bits_for_levels(s)
    assert codec.min_bits_for_levels(16.0) == 4                    # _lib.level_count: an integral float is its integer
    with pytest.raises(ValueError, match='at most 256 levels'):
        codec.min_bits_for_levels(257)
    with pytest.raises(ValueError, match='at most 256 levels'):
        codec.bits_for_levels(257)
    for bad in (1, 0, -3, 2.5, True, '8', None, float('nan'), 2 ** 31):
        with pytest.raises(ValueError, match='must be an integer >= 2'):
            codec.min_bits_for_levels(bad)
    # the default of pack_uniform has not moved
    assert [codec.bits_for_levels(s) for s in (2, 3, 5, 8, 16, 17, 64, 128, 256)] == [1, 2, 4, 4, 4, 8, 8, 8, 8]
