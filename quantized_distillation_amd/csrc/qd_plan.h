// qd_plan.h -- which kernel a single-tensor transform call reaches, and with what launch geometry: ONE pure function.
//
// plan_transform() takes numbers only (mode, n, bucket, alignment facts, k, ...) and returns a TransformPlan: the kernel
// family and template arguments of every launch, its grid, block size and dynamic LDS, and the values the kernels index with
// (m, nchunks, nbk, nvec, amask, the effective `fine`).  run_transform<MODE>() of qd_transform.h derives the inputs from its
// pointers, plans, and launches what the plan says; qd_transform_plan() (include/qd_hip.h) returns the same plan with the
// kernel names spelled out, so tests/test_transform_plan.py holds the kernels' capacity contracts and the family boundaries
// for every bucket size on a machine without a GPU.
//
// Plain C++17: no HIP header, no runtime call (g++ -std=c++17 -fsyntax-only compiles it).  Under hipcc the few functions the
// kernels share with the plan (point_table_bytes, stage8) are __host__ __device__.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define QD_HD __host__ __device__
#else
#define QD_HD
#endif

namespace qd {

enum Mode { MODE_QDQ = 0, MODE_SCALE = 1, MODE_NEAREST = 2 };

// ---- constants the kernels and the plan share -------------------------------------------------------------------------
constexpr int kMaxPoints = 1024;        // LDS table of quantization points
constexpr int kPartialBlocks = 1024;    // stage-1 blocks of every two-stage reduction
constexpr int kCells = 256;             // uniform grid over [0,1] that narrows the midpoint search (k > 32)
constexpr int kSmallTable = 32;
constexpr int kFineCells = 2048;        // the fine cell table (PointStore, qd_points.h)
// Grid cap of the kernels that build the fine table, in blocks per CU (6 are resident next to 26.6 KB of LDS).  Measured, K5
// k = 256 at bucket 256 / 1000, 64 Mi elements (round 2's narrowed search: 117 / 144 us): 6 -> 102 / 110 us (every resident
// block builds its table at the same moment, nothing to overlap it with), 12 -> 98 / 105, 24 -> 95 / 102, 48 -> 101 / 111,
// uncapped (a table per 16 KB of data) -> 106 / 117.  (A compile-time constant; tools/ build variants of it for A/B runs.)
#ifndef QD_FINE_BLOCKS_PER_CU
#define QD_FINE_BLOCKS_PER_CU 24
#endif
constexpr int kFineBlocksPerCu = QD_FINE_BLOCKS_PER_CU;
constexpr size_t kCoarseTableBytes = (size_t)2 * kMaxPoints * sizeof(float) + (size_t)2 * (kCells + 4) * sizeof(int);   // 10272
QD_HD constexpr size_t point_table_bytes(int k, int fine = 0) {
    return k <= kSmallTable ? (size_t)2 * kSmallTable * sizeof(float)
                            : kCoarseTableBytes + (fine ? (size_t)kFineCells * 8 : 0);
}
// float4 per lane a chunk holds.  Measured at 64 Mi elements, bucket 100 / 36 / 300 / 1000 / 2000 (the one-bucket-
// per-lane-group kernels: 145 / 211 / 167 / 114 / 122 us): 16 -> 123 / 123 / 128 / 122 / 120 us (195 VGPRs,
// two waves per SIMD: the load and the compute phase of a wave do not overlap); 8 -> 100 / 100 / 103 / 108 / 108;
// 4 -> 124 / 131 / 130 / 118 / 121.  Bucket 12 / 4: 101 / 112 us instead of 571 / 1616.
constexpr int kChunkV = 8;
constexpr int64_t kSingleSmallN = 16384;               // one bucket up to here: one block of k_bucket_generic does both passes
// Measured on MI355X (docs/history/profiles/r02_k1g_fused.txt): a device-scope round trip costs 1.5-2 us, so the barrier adds ~3.5 us
// to a kernel -- about what a kernel boundary costs -- and the load and store phases of the register-resident kernel do
// not overlap, while the three-launch path's second read is served by the 256 MiB Infinity Cache.  One launch wins only
// where the call is launch-bound: up to 1 Mi elements (GPU time 7.8 vs 9.7 us at 0.1 M, 10.8 vs 10.9 at 0.8 M; one host
// launch instead of two); at 2.8 M / 5.3 M elements it measured 22 / 21 us against 16 / 17.5 us.
constexpr int64_t kFusedMaxN = (int64_t)1 << 20;
constexpr int64_t kFoldLaunchN = (int64_t)8 << 20;     // above 32 MB: thousands of apply blocks, the partials are folded once in a launch of its own
constexpr int kStreamU = 4;                            // float4s per lane in flight in k_nearest_prescaled_stream
constexpr int kDefaultGridCap = 1 << 20;               // one wave-tile per wave streams fastest: the cap only bounds the grid dimension

inline void geometry(int64_t n, int64_t bucket, int64_t& nb, int64_t& row) {       // help_functions.py:67-94
    if (bucket <= 0 || n < bucket) { nb = 1; row = n; return; }
    row = bucket;
    nb = (n + bucket - 1) / bucket;
}

// k_bucket_chunk_any stages level / point indices that fit a byte in LDS behind the values: the kernel carves its LDS by
// this, the plan sizes it by this
QD_HD constexpr bool stage8(int mode, bool lev8, bool idx, int k) {
    return (mode == MODE_QDQ && lev8) || (mode == MODE_NEAREST && idx && k <= 32);
}

// with the fine cell table the grid is capped (the kernels loop): the table is built once per resident block, not per tile
inline int fine_grid_cap(int fine, int cus) { return fine ? kFineBlocksPerCu * cus : (1 << 30); }

// ---- one list per kernel family: the plan's selection and the launcher's instantiation both expand it -------------------
// k_bucket_vec<MODE, LPB, V, U>, X(row, lanes per bucket, float4 per lane, buckets per lane group and tile): row = LPB x V x 4
// (4096, 8192: k_bucket_wave_any with two / four waves per bucket -- 8192: 91.2 vs 95.5 us as 32 float4 per lane)
#define QD_VEC_SHAPES(X)                                                                                              \
    X(64, 16, 1, 4)                                                                                                   \
    X(128, 16, 2, 2)                                                                                                  \
    X(256, 16, 4, 1)                                                                                                  \
    X(512, 64, 2, 2)                                                                                                  \
    X(1024, 64, 4, 1)                                                                                                 \
    X(2048, 64, 8, 1)
// k_bucket_wave_any<MODE, V, G>, X(float4 per lane, waves per bucket), in first-fit order: the first shape with
// nf_max <= 64 * G * V.  One wave per bucket up to 8 rounds (2048 elements), then two (up to 4096) and four waves per bucket.
// The hot mode has rounds in steps of one; above 8192 elements more float4s per lane again (8200 / 10000 / 16384 / 20000 took
// 148 / 182 / 155 / 284 us on the two-pass kernels).
#define QD_WAVE_SHAPES_QDQ(X)                                                                                         \
    X(2, 1) X(3, 1) X(4, 1) X(5, 1) X(6, 1) X(7, 1) X(8, 1)                                                           \
    X(5, 2) X(6, 2) X(7, 2) X(8, 2)                                                                                   \
    X(5, 4) X(6, 4) X(7, 4) X(8, 4) X(9, 4)                                                                           \
    X(12, 4) X(16, 4) X(24, 4) X(32, 4)
// scale_down, nearest point: fewer instances
#define QD_WAVE_SHAPES_SCALE(X)                                                                                       \
    X(3, 1) X(5, 1) X(8, 1) X(6, 2) X(8, 2) X(6, 4) X(9, 4) X(16, 4) X(32, 4)
// more than 9 float4s per lane: not in the nearest-point mode -- its point search keeps too much live and the compiler
// demotes the float4 array to scratch memory (272 / 528 bytes per lane); buckets above 9216 elements take the two-pass
// kernels in that mode
#define QD_WAVE_SHAPES_NEAREST(X)                                                                                     \
    X(3, 1) X(5, 1) X(8, 1) X(6, 2) X(8, 2) X(6, 4) X(9, 4)
// k_single_fused<MODE, V, W>, X(index, float4 per lane, waves per SIMD), tried in this order
#define QD_FUSED_SHAPES(X) X(0, 1, 4) X(1, 4, 4)
constexpr int kFusedShapes = 2;

// ---- the plan -------------------------------------------------------------------------------------------------------
enum Family {
    FAM_VEC,                 // k_bucket_vec<MODE, a = LPB, b = V, c = U>
    FAM_CHUNK,               // k_bucket_chunk<MODE, a = kChunkV>
    FAM_CHUNK_ANY,           // k_bucket_chunk_any<MODE, a = kChunkV>
    FAM_WAVE_ANY,            // k_bucket_wave_any<MODE, a = V, b = G>
    FAM_GROUPS,              // k_bucket_groups<MODE, a = LANES>
    FAM_GENERIC,             // k_bucket_generic<MODE>
    FAM_FUSED,               // k_single_fused<MODE, a = V, b = W>
    FAM_MINMAX_PARTIAL,      // k_minmax_partial
    FAM_MINMAX_FINAL,        // k_minmax_final
    FAM_SINGLE_APPLY,        // k_single_apply<MODE>
    FAM_PRESCALED_STREAM     // k_nearest_prescaled_stream<a = TWO>
};

struct Launch {
    int family;              // Family
    int a, b, c;             // its template arguments after MODE
    int blocks, threads;
    size_t lds;              // dynamic LDS bytes
};

struct PlanInput {
    int mode;                // Mode
    int64_t n, bucket;       // n > 0
    int data_misalign;       // (x | out) & 15: the fp32 data pointers need 4-byte alignment
    int side_bytes;          // the level (MODE_QDQ: 1) or index output (MODE_NEAREST: 1 or 8) asked for; 0: none
    int side_misalign;       // its address & 15: level_idx needs 4 bytes, an int64 idx 16 (the pre-scaled stream: a uint8 idx 4)
    int k, assign_mode;      // MODE_NEAREST
    bool prescaled;          // MODE_NEAREST: x is already u, alpha / beta are inputs
    bool q_null;             // MODE_NEAREST: indices only
    bool fused_ok;           // the one-launch single-bucket kernel may be tried: not switched off, not in place
    int cus;                 // compute units of the device
    int grid_cap;            // kDefaultGridCap, or what qd_set_grid_cap() set (QD_TUNING builds: QD_GRID_CAP)
};

struct TransformPlan {
    int64_t nb, row;         // geometry()
    int64_t nvec;            // leading full buckets of the vector kernel (0: every other kernel)
    int fine;                // the kernel builds and uses the fine cell table
    int m;                   // chunk kernels: buckets per chunk
    int64_t nchunks;         // chunk kernels: whole chunks
    int64_t nbk;             // k_bucket_wave_any: buckets [0, nbk) are its own, the rest block 0's scalar path
    int64_t amask;           // k_bucket_wave_any: ~31, the 128-byte line
    int nlaunch;             // 0: no kernel serves the call (indices only without the pre-scaled stream)
    Launch launch[3];        // in order
    // one bucket of kSingleSmallN .. kFusedMaxN elements: k_single_fused of QD_FUSED_SHAPES index i needs fused_blocks[i] blocks
    // RESIDENT (the launcher asks the occupancy, and whether the stream is capturing); launch[] is what runs otherwise.
    int64_t fused_blocks[kFusedShapes];      // 0: not to be tried
    size_t fused_lds;
    bool needs_workspace;    // the launches use the caller's scratch buffer
    bool copies_ab;          // pre-scaled single bucket: (alpha, beta) are copied into the scratch slot k_single_apply reads
    int nparts;              // min / max partials k_minmax_partial leaves (its blocks)
    bool ab_ready;           // k_single_apply finds (alpha, beta) in the scratch slot (copied, or folded by k_minmax_final); else it folds nparts partials
};

// The grid of a launch that is sized from the problem: ceil(items / per_block) blocks, at least 1, at most the launch
// site's own cap (kNoOwnCap: none) and the grid cap -- kDefaultGridCap, or what qd_set_grid_cap() set.  Every such launch
// goes through this one function: the plan below with its input's grid_cap, the launchers through grid_blocks()
// (qd_common.h), which passes the hook's value.
constexpr int64_t kNoOwnCap = (int64_t)1 << 30;
inline int capped_blocks(int64_t items, int64_t per_block, int64_t own_cap, int64_t grid_cap) {
    int64_t b = (items + per_block - 1) / per_block;
    const int64_t cap = own_cap < grid_cap ? own_cap : grid_cap;
    if (b > cap) b = cap;
    return (int)(b < 1 ? 1 : b);
}

// lanes of a chunk kernel that reduce side by side: above 64 buckets a lane reduces whole buckets alone, below that 64 / m
// lanes share one, so m is rounded down to a power of two -- except 48 .. 63, one lane per bucket
inline int chunk_lane_rule(int m, int p2) {
    if (m >= 64) return m;
    while (p2 * 2 <= m) p2 *= 2;
    return (m < 48 || p2 == m) ? p2 : m;
}

inline TransformPlan plan_transform(const PlanInput& in) {
    TransformPlan pl = {};
    geometry(in.n, in.bucket, pl.nb, pl.row);
    const int mode = in.mode;
    const bool nearest = mode == MODE_NEAREST;
    const int64_t n = in.n, row = pl.row, nb = pl.nb;
    pl.fine = (nearest && in.k > 32 && in.assign_mode == 1 /* QD_ASSIGN_MIDPOINT */) ? 1 : 0;
    const int fine_cap = fine_grid_cap(pl.fine, in.cus);
    const size_t tb = nearest ? point_table_bytes(in.k, pl.fine) : 0;       // dynamic LDS of every launch: the point table
    const size_t tbc = nearest ? point_table_bytes(in.k, 0) : 0;            // the chunk kernels': always the coarse table
    const bool data_ok = (in.data_misalign & 3) == 0;
    const bool side = in.side_bytes != 0;
    const bool side_ok = !side || (nearest ? (in.side_bytes != 8 || (in.side_misalign & 15) == 0) : (in.side_misalign & 3) == 0);
    const bool aligned = data_ok && side_ok;
    auto one = [&pl](int family, int a, int b, int c, int blocks, int threads, size_t lds) {
        pl.launch[pl.nlaunch++] = Launch{family, a, b, c, blocks, threads, lds};
    };
    // grid(items, per_block, own_cap): capped_blocks() under the input's grid cap; `fine_cap` is the own cap of the kernels
    // that build the fine table
    auto grid = [&in](int64_t items, int64_t per_block, int64_t own_cap) { return capped_blocks(items, per_block, own_cap, in.grid_cap); };

    // K5 at any bucket size from 4 elements: the pre-processed forward as a plain stream (qd_nearest.hip).  One bucket with a
    // q output: the single-bucket apply kernel already is a plain stream.
    if (nearest && in.prescaled && n >= 4 && row >= 4 && !(nb <= 1 && !in.q_null) && data_ok &&
        (!side || (in.side_misalign & (in.side_bytes == 8 ? 15 : 3)) == 0)) {
        one(FAM_PRESCALED_STREAM, (row & 3) != 0, 0, 0, grid(n >> 2, 256 * kStreamU, fine_cap), 256, tb);
        return pl;                                      // one 4 KiB tile per wave
    }
    if (in.q_null) return pl;                           // (n < 4, a bucket below 4 elements, or a misaligned base): nothing serves it

    if (nb == 1) {                                      // ---- one bucket spanning the tensor
        if (n <= kSingleSmallN) {
            one(FAM_GENERIC, 0, 0, 0, 1, 1024, tb);
            return pl;
        }
        pl.needs_workspace = true;
        const bool prescaled = nearest && in.prescaled;
        if (!prescaled && in.fused_ok && aligned && n <= kFusedMaxN) {
            const int64_t lanes = ((n >> 2) + 255) / 256;              // blocks needed at one float4 per lane
#define QD_FUSED_BLOCKS(I, V, W) pl.fused_blocks[I] = (lanes + V - 1) / V;     /* >= 1: n > kSingleSmallN */
            QD_FUSED_SHAPES(QD_FUSED_BLOCKS)
#undef QD_FUSED_BLOCKS
            pl.fused_lds = tb;
        }
        if (prescaled) {
            pl.copies_ab = pl.ab_ready = true;
        } else {
            pl.nparts = grid(n, 256 * 4 * 8, kPartialBlocks);
            one(FAM_MINMAX_PARTIAL, 0, 0, 0, pl.nparts, 256, 0);
            pl.ab_ready = n > kFoldLaunchN;
            if (pl.ab_ready) one(FAM_MINMAX_FINAL, 0, 0, 0, 1, 256, 0);
        }
        one(FAM_SINGLE_APPLY, 0, 0, 0, grid(n, 256 * 4 * 4, fine_cap), 256, tb);
        return pl;
    }

    // ---- more than one bucket
    const int64_t nfull = n / row;                      // leading full buckets
    if (aligned) {
#define QD_PLAN_VEC(ROW, LPB, V, U)                                                                                   \
        if (row == ROW) {                                                                                             \
            pl.nvec = nfull;                                                                                          \
            const int64_t bpw = (64 / LPB) * U;                                                                       \
            /* the vector kernel hides the narrowed search behind 7 waves per SIMD up to 64 points (99 us against 104 us with */ \
            /* the fine table on a capped grid); the kernels with fewer resident waves gain from 33 points on */     \
            if (in.k <= 64) pl.fine = 0;                                                                              \
            const int blocks = grid((nfull + bpw - 1) / bpw, 4, kNoOwnCap) + 1;           /* +1: the block that owns the tail */ \
            one(FAM_VEC, LPB, V, U, pl.fine && blocks > fine_cap ? fine_cap : blocks, 256, nearest ? point_table_bytes(in.k, pl.fine) : 0); \
        }
        QD_VEC_SHAPES(QD_PLAN_VEC)
#undef QD_PLAN_VEC
        if (pl.nlaunch) return pl;
    }
    if (aligned && row > 256 && row <= 32768 && (row > 512 || ((row & 3) != 0 && row >= 448))) {
        // one wave per bucket, any size (k_bucket_wave_any): sizes above 512, and sizes from 448 that are not a multiple of 4
        // (multiples of 4 up to 512 stay with the chunk kernel: 300 -> 90 us against 127 us here; the vector sizes 512 /
        // 1024 / 2048 were taken above).  The lane -> float4 mapping starts at the 128-byte line (32 elements) at or below
        // the bucket (measured against 16- and 64-element boundaries: docs/history/profiles/r02_tune_kernels.txt).
        // float4s a wave may have to hold: the bucket's own, +2 for a split first / last one, +7 for the lead-in from the line
        const int nf_max = (int)(row >> 2) + ((row & 3) ? 2 : 0) + ((row & 31) ? 7 : 0);
        int V = 0, G = 0;
#define QD_FIRST_FIT(V_, G_) if (!V && nf_max <= 64 * G_ * V_) { V = V_; G = G_; }
        if (mode == MODE_QDQ) { QD_WAVE_SHAPES_QDQ(QD_FIRST_FIT) }
        else if (mode == MODE_SCALE) { QD_WAVE_SHAPES_SCALE(QD_FIRST_FIT) }
        else { QD_WAVE_SHAPES_NEAREST(QD_FIRST_FIT) }
#undef QD_FIRST_FIT
        if (V) {
            // every bucket, the short last one included (the float4 that would reach past the end of the tensor is fetched as
            // x[n-4 .. n-1] and rotated: nothing outside the tensor is read, whatever the alignment of the base); the instances
            // with more than 16 float4s per lane have no registers to spare for that and leave the buckets whose last float4
            // crosses the end of the tensor to block 0's scalar path
            pl.nbk = nb;
            if (V > 16)
                while (pl.nbk > 0 && ((((pl.nbk * row < n ? pl.nbk * row : n) + 3) >> 2) << 2) > n) --pl.nbk;
            pl.amask = ~(int64_t)31;
            one(FAM_WAVE_ANY, V, G, 0, grid(pl.nbk > 0 ? pl.nbk : 1, 4 / G, fine_cap), 256, tb);
            return pl;
        }
    }
    if (aligned && (row & 3) == 0 && row <= (int64_t)kChunkV * 256) {
        // as many whole buckets as fit the chunk's kChunkV * 64 float4 (<= 256: the (alpha, beta) table), not the next power of
        // two below it: bucket 36 fills 504 of the 512 float4 with m = 56 instead of 288 with m = 32
        int m = (int)((kChunkV * 64) / (row >> 2));
        if (m > 256) m = 256;
        m = chunk_lane_rule(m, 1);
        if (nfull / m > 0) {
            pl.m = m;
            pl.nchunks = nfull / m;
            pl.fine = 0;                                // the chunk kernels stage data in LDS: coarse table
            // two waves per block: pairs, (alpha, beta), 1/alpha
            one(FAM_CHUNK, kChunkV, 0, 0, grid(pl.nchunks, 2, kNoOwnCap) + 1 /* the block that owns the tail */, 128,
                (size_t)2 * (kChunkV * 64 + 256 + 128) * 8 + tbc);
            return pl;
        }
    }
    constexpr int kChunkAnyRoom = kChunkV * 256 - 28;   // elements of a chunk less the lead-in to the 128-byte line
    if (aligned && (row & 3) != 0 && row * 4 <= kChunkAnyRoom) {
        // m: a multiple of 4 (chunks start 16-byte aligned), as many buckets as fit next to the lead-in: bucket 33 fills 1980 of
        // the 2048 elements with m = 60 instead of 1056 with m = 32.
        // (No upper limit on m: the kernel keeps no per-bucket table; bucket sizes 1, 2, 3, 5, 7 fill the chunk too.  Above 64
        // buckets every lane reduces whole buckets alone: a multiple of 64 keeps all lanes busy in every round -- bucket 7:
        // 102 us with m = 256, 107-110 us with m = 288.)
        // The kernel is only ever planned WITH the lead-in (its `lead` argument is always 1): at the sizes where fewer than four
        // buckets fit next to it (506 .. 511) k_bucket_wave_any has returned above -- no multiple of 4 and >= 448 -- so the
        // launcher's former `lead = 0` branch was dead, and the condition above now says so.
        int m = (int)(kChunkAnyRoom / row) & ~3;         // >= 4
        if (m >= 64) m &= ~63;
        m = chunk_lane_rule(m, 4);
        if (nfull / m > 0) {
            pl.m = m;
            pl.nchunks = nfull / m;
            pl.fine = 0;
            // two waves: the staged chunk, + a byte per element when level / point indices (<= 255) are asked for
            one(FAM_CHUNK_ANY, kChunkV, 0, 0, grid(pl.nchunks, 2, kNoOwnCap) + 1, 128,
                (size_t)2 * (kChunkV * 256 + (stage8(mode, side, side, in.k) ? kChunkV * 64 : 0)) * 4 + tbc);
            return pl;
        }
    }
    // misaligned, or too few full buckets for one chunk, or (nearest point) a bucket above 9216 elements: two passes, the
    // second from L1 / L2
    if (row <= 256) one(FAM_GROUPS, 16, 0, 0, grid(nb, 16, fine_cap), 256, tb);          // 16 buckets per block, a DPP row each
    else if (row <= 16384) one(FAM_GROUPS, 64, 0, 0, grid(nb, 4, fine_cap), 256, tb);    // 4 buckets per block, one wave each
    else one(FAM_GENERIC, 0, 0, 0, grid(nb, 1, fine_cap), 1024, tb);
    return pl;
}

// ---- the kernel's name as tools/launch_coverage.py short_name spells it, from the family and arguments the launcher switches on
inline char* put_str(char* o, const char* s) { while (*s) *o++ = *s++; return o; }
inline char* put_int(char* o, int v) {
    char tmp[12];
    int nd = 0;
    do { tmp[nd++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (nd) *o++ = tmp[--nd];
    return o;
}
constexpr int kKernelNameBytes = 40;
inline void kernel_name(int mode, const Launch& L, char out[kKernelNameBytes]) {
    static const char* const base[] = {"k_bucket_vec", "k_bucket_chunk", "k_bucket_chunk_any", "k_bucket_wave_any", "k_bucket_groups",
                                       "k_bucket_generic", "k_single_fused", "k_minmax_partial", "k_minmax_final", "k_single_apply",
                                       "k_nearest_prescaled_stream"};
    static const int nargs[] = {3, 1, 1, 2, 1, 0, 2, -1, -1, 0, -2};      // after MODE; -1: no template; -2: one bool
    char* o = put_str(out, base[L.family]);
    const int na = nargs[L.family];
    if (na == -2) o = put_str(o, L.a ? "<true>" : "<false>");
    if (na >= 0) {
        const int args[3] = {L.a, L.b, L.c};
        *o++ = '<';
        o = put_int(o, mode);
        for (int i = 0; i < na; ++i) { *o++ = ','; o = put_int(o, args[i]); }
        *o++ = '>';
    }
    *o = 0;
}

}  // namespace qd
