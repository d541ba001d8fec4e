// qd_multi_uniform.h -- the bodies the kernels of qd_multi_uniform.hip and qd_multi_uniform_out16.hip are instantiations of, and
// what their entry points share on the host.  Private to those two files (qd_multi.h stays free of qd_element.h).
//
//   device   qdq4              four components through qdq / qdq_tab / qdq_stochastic / qdq_stochastic_tab: the ONE place that picks
//            reg_row           a full bucket row in registers: load, clamp, min / max, alpha / beta, division split, quantize, store
//            bucketed_tile     a tile of the launches with one bucket size: the bucket of each DPP row, reg_row or the row path
//            mg_minmax_tile    no buckets, phase 1: min / max of a tile of kTile elements
//            mg_apply_tile     no buckets, phase 3: a tile under its tensor's (alpha, beta)
//   host     multi_args_ok, workspace_ok, dispatch
//
// Compile-time parameters say what a kernel is: CLAMP (Prep::me is in use), STOCH (stochastic rounding) and the output element O
// (float, _Float16, __bf16: the store and the alignment it needs).  Every instantiation sees the text of its own kernel and
// nothing of the others'.  A kernel keeps the loop over its wave's tiles, the tile -> tensor search and where its level count
// comes from; the rest of a tile is one call.
#pragma once

#include <initializer_list>
#include <type_traits>

#include "qd_element.h"        // bucket_lanes, KParams, Prep, transform<MODE_QDQ>
#include "qd_launch.h"         // launch geometry
#include "qd_multi.h"

namespace {

// The first seed of a launch: the by-value argument, or the device word when there is one (a kernel argument, so the load
// is a scalar one; the kernel never writes the cell).  Tensor ti of the table draws with seed0 + ti (its position, empty tensors
// included); element e of it takes word e & 3 of Philox block e >> 2 as in every other kernel.
__device__ __forceinline__ uint64_t first_seed(uint64_t seed, const uint64_t* __restrict__ seed_cell) {
    return seed_cell ? *seed_cell : seed;
}

// ---- the output element: four results of a lane as one non-temporal store, and what the vector paths ask of the pointers ----
// fp32: x and q 16-byte aligned (float4 loads, float4 stores).  16 bits: x 16-byte aligned, q 8-byte aligned (a lane stores its
// four results as 8 bytes: store4_nt, qd_multi.h).
// quad_ptr: the lane's first four elements of the row at `row`, the lane's place in it l; store_quad: four results, `quads` groups
// of four elements further on
__device__ __forceinline__ f4* quad_ptr(float* row, int l) { return (f4*)row + l; }
template <typename O> __device__ __forceinline__ O* quad_ptr(O* row, int l) { return row + l * 4; }
__device__ __forceinline__ void store_quad(const f4& r, f4* dst, int quads) { stg_nt(r, dst + quads); }
template <typename O> __device__ __forceinline__ void store_quad(const f4& r, O* dst, int quads) { store4_nt(r, dst + quads * 4); }
// one element on the scalar path of mg_apply_tile: fp32 outputs through the descriptor's own pointers, 16-bit outputs through
// ldg / stg -- not the same machine code (flat against global accesses), and each output type keeps the one it was measured with
__device__ __forceinline__ float load_one(const float* x, int64_t i, float*) { return x[i]; }
template <typename O> __device__ __forceinline__ float load_one(const float* x, int64_t i, O*) { return ldg(x + i); }
__device__ __forceinline__ void store_one(float r, float* q, int64_t i) { q[i] = r; }
template <typename O> __device__ __forceinline__ void store_one(float r, O* q, int64_t i) { stg((O)r, q + i); }
template <typename O>
__device__ __forceinline__ bool vector_aligned(const QdTensorDesc& d) {
    if constexpr (std::is_same<O, float>::value) return ((((uintptr_t)d.x) | ((uintptr_t)d.q)) & 15) == 0;
    else return ((((uintptr_t)d.x) & 15) | (((uintptr_t)d.q) & 7)) == 0;
}

// ---- four components of one float4 ----
// STOCH at compile time, use_tab (<= 16 levels: the level table held by a DPP row, which is active as a whole wherever this is
// called with use_tab) at run time; FAST: the bucket-invariant division with y = 1 / a (qd_common.h).
template <bool FAST, int STOCH>
__device__ __forceinline__ f4 qdq4(const f4& v, float a, float b, float sm1, const float (&rnd)[4], float& lev, bool use_tab,
                                   float tab, float y) {
    auto quad = [&](auto one) {
        f4 r;
        r.x = one(v.x, rnd[0]); r.y = one(v.y, rnd[1]); r.z = one(v.z, rnd[2]); r.w = one(v.w, rnd[3]);
        return r;
    };
    if (STOCH && use_tab) return quad([&](float e, float u) { return qdq_stochastic_tab<FAST>(e, a, b, sm1, 0.0f, u, lev, tab, y); });
    if (STOCH) return quad([&](float e, float u) { return qdq_stochastic<FAST>(e, a, b, sm1, 0.0f, u, lev, y); });
    if (use_tab) return quad([&](float e, float) { return qdq_tab<FAST>(e, a, b, sm1, 0.0f, lev, tab, y); });
    return quad([&](float e, float) { return qdq<FAST>(e, a, b, sm1, 0.0f, lev, y); });
}

// ---- one full bucket row of 64 V elements, held by the 16 lanes of a DPP row (l: the lane's place in it) ----
// x + lo 16-byte aligned, out + lo as vector_aligned says.  On this path an element index is a multiple of 4: one Philox block
// per float4.
template <int V, bool CLAMP, int STOCH, typename O>
__device__ __forceinline__ void reg_row(const float* x, O* out, int64_t lo, int l, const Prep& pp, float sm1, bool use_tab,
                                        float tab, uint64_t seed_t) {
    const f4* src = (const f4*)(x + lo) + l;
    f4 v[V];
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = ldg_nt(src + j * 16);   // masters: read once
    if (CLAMP) {
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = prep4(v[j], pp);    // the clamp comes before the bucket's min / max
    }
    float mn = pmin4(v[0]), mx = pmax4(v[0]);      // NaN-propagating
#pragma unroll
    for (int j = 1; j < V; ++j) { mn = pmin(mn, pmin4(v[j])); mx = pmax(mx, pmax4(v[j])); }
    mn = row16_min(mn); mx = row16_max(mx);
    float a, b, lev;
    alpha_beta(mn, mx, a, b);
    auto dst = quad_ptr(out + lo, l);
    const uint64_t blk0 = (uint64_t)(lo >> 2) + (uint64_t)l;      // Philox block of this lane's first float4
    // rows of the wave that took this branch: all in the proven range -> bucket-invariant division (qd_common.h)
    const bool fdiv = !__any(!fastdiv_ok(a));
    auto body = [&](auto fast_c) {
        constexpr bool FAST = decltype(fast_c)::value;
        const float y = FAST ? 1.0f / a : 0.0f;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float rnd[4] = {0.f, 0.f, 0.f, 0.f};
            if (STOCH) philox_uniform4(seed_t, blk0 + (uint64_t)(j * 16), rnd);
            store_quad(qdq4<FAST, STOCH>(v[j], a, b, sm1, rnd, lev, use_tab, tab, y), dst, j * 16);
        }
    };
    if (fdiv) body(std::true_type{}); else body(std::false_type{});
}

// The KParams of the row paths (bucket_lanes, bucket_lanes4, bucket_row16_o16): tensor d in rows of `row`, nb of them.  The
// 16-bit row path stores through its own pointer.
template <typename O>
__device__ __forceinline__ KParams row_params(const QdTensorDesc& d, int64_t row, int64_t nb, float me, float sm1, int stochastic,
                                              uint64_t seed_t) {
    KParams p;
    p.x = d.x; p.out = std::is_same<O, float>::value ? d.q : nullptr; p.n = d.n;
    p.row = row;
    p.nb = nb;
    p.alpha = nullptr; p.beta = nullptr; p.mean = nullptr; p.me = me; p.sm1 = sm1; p.lev8 = nullptr;
    p.idx = nullptr; p.idx_bytes = 0; p.pts = nullptr; p.k = 0; p.assign_mode = 0; p.prescaled = 0;
    p.stochastic = stochastic; p.seed = seed_t; p.nvec = 0;
    return p;
}

// bucket_lanes<MODE_QDQ, 16> (qd_element.h) with a 16-bit store: a DPP row processes one arbitrary bucket [lo, hi) with scalar
// accesses in two passes -- the ragged last bucket, short buckets, odd bucket sizes, pointers that the register path does not
// take.  The same reduction, the same transform<MODE_QDQ>; q needs 2-byte alignment only.  No alpha / beta / level outputs: the
// multi-tensor launches have none.
template <typename O>
__device__ __forceinline__ void bucket_row16_o16(const KParams& p, O* __restrict__ q, int64_t lo, int64_t hi, int l, const Prep& pp) {
    float mn = INFINITY, mx = -INFINITY;
    bool nan = false;
    for (int64_t i = lo + l; i < hi; i += 16) {
        const float v = prep(ldg(p.x + i), pp);
        mn = fminf(mn, v); mx = fmaxf(mx, v);
        nan |= (v != v);
    }
    mn = row16_min(mn); mx = row16_max(mx);
    if (group_any<16>(nan)) { mn = NAN; mx = NAN; }
    float a, b;
    alpha_beta(mn, mx, a, b);
    for (int64_t i = lo + l; i < hi; i += 16) {
        const float v = prep(ldg(p.x + i), pp);
        float rnd = 0.0f;
        if (p.stochastic) {
            float r4[4];
            philox_uniform4(p.seed, (uint64_t)i >> 2, r4);
            rnd = r4[i & 3];
        }
        float side = 0.0f;
        const float y = transform<MODE_QDQ>(p, nullptr, v, a, b, pp.mean, rnd, side);
        stg((O)y, q + i);
    }
}

// ---- what a wave derives from a level count: sm1, and for <= 16 levels (use_tab) its entry of the level table, tab = (float)
// (lane & 15) / sm1 -- the correctly rounded division of k_bucket_vec.  Once per wave where sm1 is a kernel argument; where it is
// levels[ti] (read with the descriptor from the index owner_of returns: wave-uniform, a scalar load), whenever the wave moves on
// to another tensor -- a scalar branch, the tiles of one tensor that a wave takes in a row share it.  An entry < 2 gives sm1 <= 0:
// wrong values in that tensor's output and nothing else (sm1 is never an address; the table lookup of qdq_tab is a cross-lane
// read).
struct Levels {
    float sm1, tab;
    bool use_tab;
};
__device__ __forceinline__ Levels levels_of(float sm1, int lane) {
    Levels lv;
    lv.sm1 = sm1;
    lv.use_tab = sm1 <= 15.0f;
    lv.tab = (float)(lane & 15) / sm1;
    return lv;
}

// ---- bucketed, one bucket size for the launch: tile t of tensor d in k_multi_uniform, _opt, _lv and _o16 ----
// A tile = 4 buckets of one tensor = one wave iteration; a DPP row owns a bucket.  Full ROW-element buckets of a tensor that is
// vector_aligned take reg_row, everything else the row path (bucket_lanes<16>; 16 bits: bucket_row16_o16).  Both give the same bits.
template <int ROW, bool CLAMP, int STOCH, typename O>
__device__ __forceinline__ void bucketed_tile(const QdTensorDesc d, int64_t t, int64_t bucket, const Levels& lv, float me,
                                              uint64_t seed_t) {
    const int lane = threadIdx.x & 63;
    const int sub = lane >> 4, l = lane & 15;
    Prep pp;
    pp.mean = 0.0f;
    pp.me = me;
    const int64_t row = d.n < bucket ? d.n : bucket;
    const KParams p = row_params<O>(d, row, (d.n + row - 1) / row, me, lv.sm1, STOCH, seed_t);
    const int64_t bkt = (t - d.first_tile) * 4 + sub;
    if (bkt >= p.nb) return;
    const int64_t lo = bkt * p.row;
    const int64_t hi = lo + p.row < p.n ? lo + p.row : p.n;
    const bool fast = ROW > 0 && (hi - lo) == ROW && p.row == ROW && vector_aligned<O>(d);
    if (fast) {
        reg_row<(ROW > 0 ? ROW / 64 : 1), CLAMP, STOCH>(p.x, (O*)d.q, lo, l, pp, lv.sm1, lv.use_tab, lv.tab, seed_t);
    } else {
        if constexpr (std::is_same<O, float>::value) bucket_lanes<MODE_QDQ, 16>(p, nullptr, bkt, lo, hi, l, pp);
        else bucket_row16_o16<O>(p, (O*)d.q, lo, hi, l, pp);
    }
}

// ---- no buckets (kTile, the elements of a wave tile: qd_multi.h) ----
// phase 1: min / max of tile t of tensor d (CLAMP: of the clamped values) -> part[2 * t], part[2 * t + 1]
template <bool CLAMP>
__device__ __forceinline__ void mg_minmax_tile(const QdTensorDesc d, int64_t t, float* part, float me) {
    const int lane = threadIdx.x & 63;
    Prep pp;
    pp.mean = 0.0f;
    pp.me = me;
    const int64_t lo = (t - d.first_tile) * kTile;
    const int64_t hi = lo + kTile < d.n ? lo + kTile : d.n;
    float mn = INFINITY, mx = -INFINITY;
    bool nan = false;
    if (hi - lo == kTile && ((((uintptr_t)d.x) & 15) == 0)) {
        const f4* src = (const f4*)(d.x + lo) + lane;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f4 v = ldg(src + j * 64);                 // plain loads: phase 3 re-reads from L2 / MALL
            if (CLAMP) v = prep4(v, pp);
            mn = fminf(mn, fminf(fminf(v.x, v.y), fminf(v.z, v.w)));
            mx = fmaxf(mx, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
            nan |= has_nan4(v);
        }
    } else {
        for (int64_t i = lo + lane; i < hi; i += 64) {
            const float v = CLAMP ? prep(d.x[i], pp) : d.x[i];
            mn = fminf(mn, v); mx = fmaxf(mx, v); nan |= (v != v);
        }
    }
    mn = wave_min(mn); mx = wave_max(mx);
    if (group_any<64>(nan)) { mn = NAN; mx = NAN; }       // NaN poisons the tile and, in phase 2, the tensor
    if (lane == 0) { part[2 * t] = mn; part[2 * t + 1] = mx; }
}

// phase 3: tile t of tensor d (the ti-th of the table) under the tensor's single (alpha, beta) = ab[ti], with its level count and,
// STOCH, its draws under seed_t -- one Philox block per float4, block = element index in the tensor >> 2.  The IEEE division, no
// level table.
template <bool CLAMP, int STOCH, typename O>
__device__ __forceinline__ void mg_apply_tile(const QdTensorDesc d, int ti, int64_t t, const float* ab, float sm1, float me,
                                              uint64_t seed_t) {
    const int lane = threadIdx.x & 63;
    Prep pp;
    pp.mean = 0.0f;
    pp.me = me;
    const float a = ab[2 * ti], b = ab[2 * ti + 1];
    const int64_t lo = (t - d.first_tile) * kTile;
    const int64_t hi = lo + kTile < d.n ? lo + kTile : d.n;
    O* const q = (O*)d.q;                       // n elements of the output type (include/qd_hip.h)
    float lev;
    if (hi - lo == kTile && vector_aligned<O>(d)) {
        const f4* src = (const f4*)(d.x + lo) + lane;
        auto dst = quad_ptr(q + lo, lane);
        const uint64_t blk0 = (uint64_t)(lo >> 2) + (uint64_t)lane;
        f4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ldg_nt(src + j * 64);
        __builtin_amdgcn_sched_barrier(0);          // all four loads in flight before the first use
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f4 c = CLAMP ? prep4(v[j], pp) : v[j];
            float rnd[4] = {0.f, 0.f, 0.f, 0.f};
            if (STOCH) philox_uniform4(seed_t, blk0 + (uint64_t)(j * 64), rnd);
            store_quad(qdq4<false, STOCH>(c, a, b, sm1, rnd, lev, false, 0.0f, 0.0f), dst, j * 64);
        }
    } else {
        for (int64_t i = lo + lane; i < hi; i += 64) {
            const float c = CLAMP ? prep(load_one(d.x, i, q), pp) : load_one(d.x, i, q);
            if (STOCH) {
                float r4[4];
                philox_uniform4(seed_t, (uint64_t)i >> 2, r4);
                store_one(qdq_stochastic(c, a, b, sm1, 0.0f, r4[i & 3], lev), q, i);
            } else {
                store_one(qdq(c, a, b, sm1, 0.0f, lev), q, i);
            }
        }
    }
}

// ---- host: what every launch entry point refuses, and the choice of the instantiation ----
// The one argument check.  An entry point passes what its signature has and a value that passes for the rest (bucket 1, levels
// 2, clamp 0, no seed cell, QD_OUT_F16); `arrays`: the device arrays and outputs it requires, each non-null and aligned to its
// element.  clamp != 0 needs a positive limit (not NaN); me: the limit the kernels see, +inf when the clamp is off.
struct Required { const void* p; uintptr_t align_mask; };
inline bool multi_args_ok(const QdTensorDesc* table, int ntensors, int64_t total_tiles, int64_t bucket, int levels,
                          std::initializer_list<Required> arrays, int clamp, float max_element, const uint64_t* seed_cell, float& me,
                          int out_kind = QD_OUT_F16) {
    me = clamp ? max_element : INFINITY;
    if (!table || ntensors <= 0 || total_tiles < 0 || bucket <= 0 || levels < 2) return false;
    for (const Required& r : arrays)
        if (!r.p || (((uintptr_t)r.p) & r.align_mask)) return false;
    if (out_kind != QD_OUT_F16 && out_kind != QD_OUT_BF16) return false;
    if (clamp && !(max_element > 0.0f)) return false;
    if (seed_cell && (((uintptr_t)seed_cell) & 7)) return false;
    return true;
}

// the workspace of the launches without buckets: (min, max) per tile, 16-byte aligned
inline bool workspace_ok(const void* workspace, size_t workspace_bytes, int64_t total_tiles) {
    return workspace && !(((uintptr_t)workspace) & 15) && workspace_bytes >= (size_t)total_tiles * 2 * sizeof(float);
}

// launch(ROW, STOCH, OUT) with the three as std::integral_constant<int, ...>: ROW = bucket where a register body exists (256, 128,
// 64), else 0; STOCH = 0 / 1; OUT = out_kind.  A launch that has no use for one of them ignores it.
template <typename Launch>
inline void dispatch(int64_t bucket, int stochastic, int out_kind, Launch launch) {
    auto with_out = [&](auto row, auto stoch) {
        if (out_kind == QD_OUT_BF16) launch(row, stoch, std::integral_constant<int, QD_OUT_BF16>{});
        else launch(row, stoch, std::integral_constant<int, QD_OUT_F16>{});
    };
    auto with_stoch = [&](auto row) {
        if (stochastic) with_out(row, std::integral_constant<int, 1>{});
        else with_out(row, std::integral_constant<int, 0>{});
    };
    if (bucket == 256) with_stoch(std::integral_constant<int, 256>{});
    else if (bucket == 128) with_stoch(std::integral_constant<int, 128>{});
    else if (bucket == 64) with_stoch(std::integral_constant<int, 64>{});
    else with_stoch(std::integral_constant<int, 0>{});
}

}  // namespace
