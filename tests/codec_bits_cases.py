"""The packed codec at the widths whose elements straddle bytes (3, 5, 6 and 7 bits): the case list and a numpy reference of
the stream, shared by tests/test_codec_bits_cases_host.py (no GPU: the reference against itself and against
abi_contract.pack_bits, what every shape below is there for, the argument checks of libqd_hip.so) and
tests/test_hip_codec_bits.py (libqd_hip.so on the device).  A plain helper module on the harness of tests/abi_contract.py.

The stream (include/qd_hip.h): bit i is bit i & 7 of byte i >> 3, element e holds its index LSB first in stream bits
[e b, (e + 1) b), the unused high bits of the last byte are zero.  pack_stream writes exactly that sentence with
np.unpackbits / np.packbits(bitorder='little'); expected levels are the oracle's (oracle_c.uniform_quantize(...)['lev']), as in
abi_contract._codec_cases."""
import functools

import numpy as np

from abi_contract import F32, STREAM, U8, Ref, case, data, inp, nbuckets, out
from oracle import oracle_c as oc

NEW_BITS = (3, 5, 6, 7)
OLD_BITS = (1, 2, 4, 8)
PARTIAL_LEVELS = {3: 5, 5: 17, 6: 33, 7: 65}            # a count that does not fill the width (the smallest that needs it)
FUSED_BUCKETS = (64, 128, 256, 512, 1024, 2048)
PACKED_PHASES = (0, 4, 8, 12)
LEVEL_NS = (5, 31, 32, 33, 10 * 256 + 3)                # qd_pack_levels_u8: below, at and above one group of 32 levels
LEVEL_PHASES = (0, 1, 2, 3)
UNPACK_BUCKETS = (256, 0, 100, 3)                       # k_unpack; k_unpack_any: none, no power of two, several per group of four
UNPACK_NS = (10 * 256 + 3, 10 * 256 + 255, 5)           # n % 4 != 0: a partial last group
Y_PHASES = (0, 4, 8, 12)
# later trips (qd_set_grid_cap 1 and 2): 199 buckets of 256 + 255 elements, 2500 groups of 32 levels + 17, 20003 elements
TRIP_PACK = (199, 256, 255)
TRIP_LEVELS_N = 32 * 2500 + 17
TRIP_UNPACK_N = 20003


# ---------------------------------------------------------------- the reference
def pack_stream(lev, bits):
    """The packed stream of the level indices `lev` at `bits` bits each: ceil(n bits / 8) bytes."""
    lev = np.asarray(lev).astype(np.uint8).reshape(-1, 1)
    stream_bits = np.unpackbits(lev, axis=1, bitorder='little')[:, :bits].reshape(-1)       # element e: bits [e b, (e + 1) b), LSB first
    return np.packbits(stream_bits, bitorder='little')                                      # zero-padded to a whole byte


def unpack_stream(stream, n, bits):
    """The n level indices of a stream (uint8): the inverse of pack_stream."""
    stream_bits = np.unpackbits(np.asarray(stream, np.uint8), bitorder='little')[:n * bits].reshape(n, bits)
    wide = np.zeros((n, 8), np.uint8)
    wide[:, :bits] = stream_bits
    return np.packbits(wide, axis=1, bitorder='little').reshape(-1)


def packed_bytes(n, bits):
    return (n * bits + 7) // 8


# what a shape is there for
def straddles_byte(n, bits):
    """Some element of the n has its bits in two bytes."""
    return any((e * bits) // 8 != ((e + 1) * bits - 1) // 8 for e in range(min(n, 64)))


def straddles_word(n, bits):
    """Some element has its bits in two 32-bit words."""
    return any((e * bits) // 32 != ((e + 1) * bits - 1) // 32 for e in range(min(n, 64)))


def partial_last_byte(n, bits):
    return (n * bits) % 8 != 0


def pack_lengths(bucket):
    """Ten full buckets: none, three and bucket - 1 elements behind them (the tail kernel's shortest and longest row)."""
    return (10 * bucket, 10 * bucket + 3, 10 * bucket + bucket - 1)


def level_counts(bits):
    return (1 << bits, PARTIAL_LEVELS[bits])


# ---------------------------------------------------------------- inputs and what the oracle makes of them, computed once
@functools.lru_cache(maxsize=None)
def quantized(n, bucket, levels, seed, variant=0):
    """(x, the oracle's result, its levels as uint8) of data(n, bucket or 256, seed) quantized with `bucket` (0: none)."""
    x = data(n, bucket or 256, seed, variant=variant)
    with np.errstate(invalid='ignore'):
        r = oc.uniform_quantize(x, levels, bucket or None, want_idx=False)
    lev = r['lev'].reshape(-1)[:n].astype(np.uint8)
    for a in (x, lev, r['alpha'], r['beta'], r['q']):
        a.flags.writeable = False                       # shared among the tests: nobody changes it
    return x, r, lev


def _seed(bits, n):
    return 700 + bits + n % 17


# ---------------------------------------------------------------- the cases
def pack_case(bits, levels, bucket, n, pp, with_ab, variant=0, x=None):
    """One qd_pack_uniform_f32 call; x: instead of data() (the non-finite buckets)."""
    if x is None:
        x, r, lev = quantized(n, bucket, levels, _seed(bits, n), variant)
    else:
        with np.errstate(invalid='ignore'):
            r = oc.uniform_quantize(x, levels, bucket, want_idx=False)
        lev = r['lev'].reshape(-1)[:n].astype(np.uint8)
    nb = nbuckets(n, bucket)
    want = pack_stream(lev, bits)
    assert len(want) == packed_bytes(n, bits)
    tag = 'pack bits %d levels %d bucket %d n=%d packed+%d%s' % (bits, levels, bucket, n, pp, '' if with_ab else ' without alpha / beta')
    if with_ab:
        return case(tag, 'qd_pack_uniform_f32',
                    [('x', inp(x, 0)), ('packed', out(U8, len(want), pp)), ('alpha', out(F32, nb, 4)), ('beta', out(F32, nb, 12))],
                    [Ref('x'), n, bucket, levels, bits, Ref('packed'), Ref('alpha'), Ref('beta'), STREAM],
                    (lambda: {'packed': want, 'alpha': r['alpha'], 'beta': r['beta']}))
    return case(tag, 'qd_pack_uniform_f32', [('x', inp(x, 0)), ('packed', out(U8, len(want), pp))],
                [Ref('x'), n, bucket, levels, bits, Ref('packed'), None, None, STREAM], (lambda: {'packed': want}))


def pack_cases(bits, bucket, variant=0):
    for levels in level_counts(bits):
        for n in pack_lengths(bucket):
            for pp in PACKED_PHASES:
                for with_ab in (True, False):
                    yield pack_case(bits, levels, bucket, n, pp, with_ab, variant)


def levels_input(bits, n, variant=0):
    """Symbols of the whole uint8 range: the entry point masks them to `bits` bits.  variant 2: all one symbol."""
    lev = np.random.RandomState(900 + bits + n % 13 + 77 * variant).randint(0, 256, n).astype(np.uint8)
    if variant == 2:
        lev[:] = 0xFF
    return lev


def levels_case(bits, n, plev, pp, variant=0):
    lev = levels_input(bits, n, variant)
    want = pack_stream(lev & np.uint8((1 << bits) - 1), bits)
    return case('pack levels bits %d n=%d levels+%d packed+%d' % (bits, n, plev, pp), 'qd_pack_levels_u8',
                [('lev', inp(lev, plev, ('index', 0xFF))), ('packed', out(U8, len(want), pp))],
                [Ref('lev'), n, bits, Ref('packed'), STREAM], (lambda: {'packed': want}))


def levels_cases(bits, variant=0):
    """`lev` at +0 ... +3 with `packed` word aligned (the 16-byte loads at +0, the byte path else), and `packed` at +1 ... +3."""
    for n in LEVEL_NS:
        for plev in LEVEL_PHASES:
            yield levels_case(bits, n, plev, 0, variant)
        for pp in (1, 2, 3):
            yield levels_case(bits, n, 0, pp, variant)


def unpack_case(bits, levels, bucket, n, pp, py, variant=0):
    x, r, lev = quantized(n, bucket, levels, _seed(bits, n), variant)
    stream = pack_stream(lev, bits)
    return case('unpack bits %d levels %d bucket %d n=%d packed+%d y+%d' % (bits, levels, bucket, n, pp, py), 'qd_unpack_uniform_f32',
                [('packed', inp(stream, pp, ('index', 0xFF))), ('alpha', inp(r['alpha'], 8)), ('beta', inp(r['beta'], 4)),
                 ('y', out(F32, n, py))],
                [Ref('packed'), n, bucket, levels, bits, Ref('alpha'), Ref('beta'), Ref('y'), STREAM],
                (lambda: {'y': r['q'].reshape(-1)}))


def unpack_cases(bits, bucket, variant=0):
    """Every 4-byte phase of y with `packed` at +0, and `packed` at +4, +8 and +12 (a stream whose 32-bit words sit at every
    word of a 16-byte granule); the bytes behind the stream hold 0xFF: a read past its end shows in the last elements."""
    for levels in level_counts(bits):
        for n in UNPACK_NS:
            for py in Y_PHASES:
                yield unpack_case(bits, levels, bucket, n, 0, py, variant)
            for pp in PACKED_PHASES[1:]:
                yield unpack_case(bits, levels, bucket, n, pp, (pp + 4) % 16, variant)


def nonfinite_input(bucket=256):
    """Five buckets and a ragged sixth: ordinary, one NaN, +inf and -inf, constant (alpha -> 1), ordinary, and a tail with a NaN."""
    n = 5 * bucket + 77
    x = (np.random.RandomState(31).randn(n) * 2).astype(np.float32)
    x[bucket + 9] = np.nan
    x[2 * bucket + 3], x[2 * bucket + 100] = np.inf, -np.inf
    x[3 * bucket:4 * bucket] = np.float32(0.375)
    x[5 * bucket + 70] = np.nan
    return x
