"""Stochastic rounding on CPU tensors (libqd_host.so) and in the oracle itself -- tests/stochastic_cases.py without a GPU:
known answers for the generator, every element on its own `rnd <= p` threshold, `rnd == 0.0` at `p == 0` with the level index,
independence of the decisions between elements, words, rows and successive seeds, and the sequence of seeds of the Python API."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import stochastic_cases as S
from oracle import oracle_np as onp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Random123's known-answer vectors for philox4x32_10 (kat_vectors of the Random123 distribution): counter, key, result.
# Confirmed against an implementation that is not this project's, the round function of rocRAND's
# rocrand_philox4x32_10.h (tests/native/philox_kat.cpp; test_philox_core_against_rocrand_round_function runs it).
PHILOX4X32_10_KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.fixture(scope='module')
def lib():
    return S.Library('host')


# ---------------------------------------------------------------------------------------------- the generator
def test_philox_core_known_answers_at_10_rounds():
    for counter, key, want in PHILOX4X32_10_KAT:
        got = tuple(int(w[0]) for w in onp.philox4x32(counter, key, 10))
        assert got == want, (['%08x' % w for w in got], ['%08x' % w for w in want])
    # the same as arrays: three counters and three keys in one call
    c = [np.array([v[0][i] for v in PHILOX4X32_10_KAT], np.uint64) for i in range(4)]
    k = [np.array([v[1][i] for v in PHILOX4X32_10_KAT], np.uint64) for i in range(2)]
    got = np.stack(onp.philox4x32(c, k, 10), axis=1)
    assert np.array_equal(got, np.array([v[2] for v in PHILOX4X32_10_KAT], np.uint64))


def test_philox_core_against_rocrand_round_function():
    """The published vectors and 64 seeded (counter, key) pairs through rocRAND's ten rounds on the host."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    exe = os.path.join(ROOT, 'build', 'philox_kat')
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call([hipcc, '--cuda-host-only', '-O1', os.path.join(ROOT, 'tests', 'native', 'philox_kat.cpp'), '-o', exe])
    rng = np.random.RandomState(1)
    cases = [v[0] + v[1] for v in PHILOX4X32_10_KAT] + [tuple(int(w) for w in rng.randint(0, 1 << 32, 6, dtype=np.uint64))
                                                         for _ in range(64)]
    out = subprocess.run([exe] + ['%x' % w for c in cases for w in c], capture_output=True, text=True, timeout=60, check=True)
    theirs = [tuple(int(w, 16) for w in line.split()) for line in out.stdout.splitlines()]
    assert theirs[:3] == [v[2] for v in PHILOX4X32_10_KAT]
    ours = [tuple(int(w[0]) for w in onp.philox4x32(c[:4], c[4:], 10)) for c in cases]
    assert theirs == ours


def test_draws_are_the_seven_round_core_with_the_documented_counter_key_and_conversion():
    """philox4x32_7_uniform, spelled out element by element from the core: counter (e >> 2, 0, 0x51ed270b, 0x2545f491), key
    (seed low, seed high), word e & 3, top 24 bits times 2^-24 -- a multiple of 2^-24 below 1."""
    seed = 0xFEDCBA9876543210
    d = onp.philox4x32_7_uniform(seed, 1003)
    for e in (0, 1, 2, 3, 4, 7, 510, 1002):
        w = onp.philox4x32((e >> 2, 0, 0x51ed270b, 0x2545f491), (seed & 0xFFFFFFFF, seed >> 32), 7)[e & 3][0]
        assert d[e] == np.float32(int(w) >> 8) * np.float32(2.0 ** -24)
    assert np.all(d < 1.0) and np.all(d >= 0.0) and np.array_equal(d * 2.0 ** 24, np.round(d * 2.0 ** 24))
    big = onp.philox4x32_7_words(seed, 8, first=1 << 34)                 # the high counter word: elements past 2^34
    w = onp.philox4x32((0, 1, 0x51ed270b, 0x2545f491), (seed & 0xFFFFFFFF, seed >> 32), 7)
    assert [int(v) for v in big[:4]] == [int(v[0]) for v in w]


def test_host_generator_draws_the_oracles_numbers_on_65536_elements(lib):
    """Every draw of libqd_host.so's generator, read off the decisions: x = d / 4 with s = 5 puts each element on its own
    threshold (level 1), x = nextafter(d) / 4 one float below it (level 0) -- a draw that differs from the oracle's in any
    bit flips its element in one of the two."""
    S.check_threshold(lib, 1 << 16, 4096, 5, kinds='AB')
    S.check_threshold(lib, 1 << 16, None, 5, kinds='AB')


# ---------------------------------------------------------------------------------------------- rnd <= p by equality
def test_the_fixed_seed_meets_the_conditions_of_the_threshold_cases():
    S.check_seed_conditions()


@pytest.mark.parametrize('s', [5, 17])
@pytest.mark.parametrize('n,bucket', S.SHAPES, ids=S.SHAPE_IDS)
def test_every_element_on_its_own_threshold(lib, n, bucket, s):
    S.check_threshold(lib, n, bucket, s, kinds='ABC' if s == 5 else 'AB')


@pytest.mark.parametrize('offset', [1, 2, 3])
@pytest.mark.parametrize('n,bucket', S.OFFSET_SHAPES)
def test_threshold_cases_on_views_at_4_byte_offsets(lib, n, bucket, offset):
    S.check_threshold(lib, n, bucket, 5, offset=offset)


# ---------------------------------------------------------------------------------------------- rnd == 0.0 at p == 0
def test_recorded_zero_draws_are_zero_draws():
    pairs = S.edge_pairs()
    assert len(pairs) >= 4 and all(p['element'] < 4096 for p in pairs) and len(set(p['element'] & 3 for p in pairs)) == 4
    for p in pairs:
        words = onp.philox4x32_7_words(p['seed'], p['element'] + 1)
        assert int(words[p['element']]) == p['word'] < 256
        assert S.draws(p['seed'], p['element'] + 1)[p['element']] == 0.0


@pytest.mark.parametrize('want_lev', [False, True], ids=['q', 'q+level_idx'])
@pytest.mark.parametrize('s', [5, 16, 256])
@pytest.mark.parametrize('n,bucket', S.EDGE_GEOMETRIES, ids=S.EDGE_IDS)
def test_zero_draw_on_an_exact_level_moves_one_level_up_even_past_the_top(lib, n, bucket, s, want_lev):
    S.check_edges(lib, n, bucket, s, want_lev)


# ---------------------------------------------------------------------------------------------- independence
def test_oracle_decisions_are_independent_across_elements_words_rows_and_seeds():
    """The generator and the seed schedule themselves: every z below 4 (profiles/stochastic_streams.txt holds these numbers)."""
    z = S.oracle_stream_statistics()
    assert len(z) == 10 + 3 + 6 + 3
    worst = max(z, key=lambda k: abs(z[k]))
    assert abs(z[worst]) <= S.Z_FINDING, (worst, z[worst])
    with open(os.path.join(ROOT, 'profiles', 'stochastic_streams.txt')) as f:
        assert f.read() == S.format_statistics(z), 'profiles/stochastic_streams.txt is stale: python tests/stochastic_cases.py'


def test_host_decisions_are_independent_across_elements_words_rows_and_seeds(lib):
    S.check_streams(lib)


def test_successive_api_calls_on_cpu_tensors_follow_the_seed_schedule():
    S.check_api_sequence('cpu')
