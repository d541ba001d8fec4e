"""Cases of the one-launch differentiable-quantization sweeps on a 16-bit student (qd_multi_nearest_out16_f32 /
qd_multi_point_grad_in16_f32, MultiTensorDiffQuant with fp16 / bf16 outputs and gradients).  Nothing runs on import;
tests/test_dq16_cases_host.py proves the tables on the CPU, tests/test_hip_dq16.py runs them on the device.

Forward.  The rounding table is out16_cases.EXACT: a tensor of 0 and v scales to u in {0, 1}, and a points row that starts at 0
and ends at 1 puts exactly {0, v} on the fp32 output ({v, +0} for a negative v: alpha = -v, beta = v, so u = 0 -> 0 * alpha + v
and u = 1 -> alpha + v = +0), whatever lies between the two points -- so the conversion of the store meets the table's ties,
overflows, subnormals and signed zeros.  The yardstick of every device test is the fp32 launch followed by .cpu().to(dtype).

Backward.  16-bit gradients travel as uint16 patterns (ste_in16_cases); the yardstick is the fp32 launch on the widened
gradients in freshly allocated buffers, bit for bit, or the exact sums of exact_sum_cases.m_case, whose gradients (+-1, +-2, +-3)
are 16-bit numbers."""
import numpy as np

from exact_sum_cases import m_case                                   # noqa: F401  (the 137-tensor list with its exact sums)
from out16_cases import EXACT, assert_same16, nonfinite, tensor_of   # noqa: F401
from ste_in16_cases import FORMATS, INF16, NAN16, WIDENING, to_patterns, torch_dtype, widen   # noqa: F401

F32 = np.float32
KIND = {'float16': 1, 'bfloat16': 2}                     # QD_OUT_F16 = QD_GRAD_F16, QD_OUT_BF16 = QD_GRAD_BF16 (include/qd_hip.h)
FWD_BUCKETS = (64, 100, 128, 256, None)                  # the five forms of the forward kernel: rows 64 / 128 / 256, generic, flat
FWD_K = (2, 4, 17, 256)
BWD_K = (4, 16, 64, 65, 256)                             # registers | four waves of LDS columns | one wave of LDS columns
BWD_BUCKETS = (256, 100, None)                           # shift, division, one alpha: with BWD_K all six instantiations
PHASES = tuple(range(0, 16, 2))                          # bytes into a 16-byte granule: every 2-byte phase
MIN_TILES = 37                                           # under a cap of 3 blocks (12 waves): at least three trips per wave
FLAT_TILE = GRAD_TILE = 1024


def points_row(k):
    """k sorted points from exactly 0 to exactly 1."""
    p = np.linspace(0.0, 1.0, k).astype(F32)
    p[0], p[-1] = F32(0.0), F32(1.0)
    return p


def exact_tensors():
    """(name, x) of the whole forward table: the 22 rounding cases, then the two non-finite tensors."""
    return [(name, tensor_of(v)) for name, v, _ in EXACT] + nonfinite()


def forward_tiles(n, bucket):
    """What qd_multi_dq_plan counts for one tensor: four buckets a tile, or 1024 elements without buckets."""
    if n == 0:
        return 0
    if bucket is None:
        return -(-n // FLAT_TILE)
    row = min(n, bucket)
    return -(-(-(-n // row)) // 4)


def sizes(bucket):
    """Element counts of the random list: empty, 1, 3, around one gradient tile, tensors of several forward tiles with a ragged
    last bucket, a tensor of full buckets only; padded until the forward tiles are at least MIN_TILES and no multiple of 4;
    a trailing empty tensor."""
    B = bucket or FLAT_TILE
    out = [0, 1, 3, 1023, 1024, 1025, 9 * B + 3, 8 * B, 4 * B + B // 2 + 1]
    pad = [5 * B + 7, B + 2, 2 * 1024 + 1000]
    i = 0
    while True:
        total = sum(forward_tiles(n, bucket) for n in out)
        if total >= MIN_TILES and total % 4:
            break
        out.append(pad[i % 3])
        i += 1
    return out + [0]


def random_list(bucket, k, fmt, seed=0):
    """[(masters fp32, gradient patterns)] of sizes(bucket) and a [ntensors, k] array of sorted points in [0, 1]."""
    ns = sizes(bucket)
    ts = []
    for i, n in enumerate(ns):
        rng = np.random.RandomState(1000 * seed + 31 * i + (bucket or 7))
        ts.append((rng.randn(n).astype(F32), to_patterns(rng.randn(n).astype(F32), fmt)))
    rng = np.random.RandomState(seed + k)
    pts = np.sort(rng.rand(len(ns), k).astype(F32), axis=1)
    return ts, pts


def with_widening_patterns(ts, fmt):
    """The gradient patterns of random_list with the WIDENING table written over them, in the main tiles and in the remainder
    (n mod 1024 elements) of the tensors that have both: the finite rows (subnormals, the smallest normal, the largest finite,
    -0) into the first such tensor, +-inf into the second, a NaN into the third."""
    table = [p for p, _ in WIDENING[fmt]]
    finite, infs = table[:5], table[5:]
    groups = [finite, infs, [NAN16[fmt]]]
    out, at = [], 0
    for x, g in ts:
        g = g.copy()
        n = g.size
        if n > GRAD_TILE and n % GRAD_TILE and at < len(groups):
            pats = groups[at]
            at += 1
            full = n // GRAD_TILE * GRAD_TILE
            main = (np.arange(2 * len(pats) + 3) * 37 + 5) % full           # several lanes of several quadruples
            rest = full + (np.arange(len(pats) + 1) * 3) % (n - full)
            for j, e in enumerate(np.concatenate([main, rest, [n - 1]])):
                g[e] = pats[j % len(pats)]
        out.append((x, g))
    assert at == len(groups), 'the list has too few tensors with full tiles and a remainder'
    return out
