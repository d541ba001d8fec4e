// qd_bucket_vec_kernels.h -- the bucket kernels in which a wave streams SEVERAL buckets at a time and holds them in registers
// or LDS, one pass over HBM: k_bucket_vec (the vector sizes, a DPP row or a wave per bucket), k_bucket_chunk (any multiple
// of 4) and k_bucket_chunk_any (any size).  The kernels with one lane group, wave or block per bucket: qd_bucket_row_kernels.h.
#pragma once

#include "qd_element.h"        // KParams, the transforms and side stores, make_prep, the row routines of the tails

#include <type_traits>

using namespace qd;

namespace {

// ---- vector path: LPB lanes per bucket, V float4 per lane: bucket = LPB*V*4 elements ---------
// LPB == 16: a DPP row owns a bucket; LPB == 64: the whole wave owns a bucket (large buckets).
// U = consecutive buckets each lane group handles per tile, so that a wave always streams 4 KiB
// per tile (U*V == 4 float4 per lane in flight) whatever the bucket size.

// wave-uniform facts about the call that the per-bucket code branches on
struct VecFlags {
    bool prescaled;   // NEAREST with u, alpha, beta given
    bool prep_on;     // mean subtraction / clamp requested
    bool use_tab;     // QDQ, deterministic, <= 16 levels: level / (s-1) from the per-row table
    bool use_tab_s;   // same for the stochastic branch
    float tab;        // this lane's table entry: (lane & 15) / (s-1)
};

// The transform + store half of vec_bucket for one code variant: VAR 0 = deterministic with the per-row level table
// (<= 16 levels), 1 = stochastic with the table, 2 = generic transform<MODE>; FAST = bucket-invariant division.
template <int MODE, int LPB, int V, int VAR, bool FAST>
__device__ __forceinline__ void vec_apply(const KParams& p, const PointTable* T, const Prep& pp, const VecFlags& fl,
                                          f4 (&v)[V], int64_t e0, float a, float b) {
    // The seed goes through an opaque (empty) asm per instantiation: without it LLVM hoists the code the variants share --
    // the whole Philox draw of the stochastic and generic variants -- in front of the variant dispatch, where the
    // deterministic path executes it too (that is what round 1's kernel did: 12 of its 32 VALU instructions per element
    // were an unused random draw).
    uint32_t seed_lo = (uint32_t)p.seed, seed_hi = (uint32_t)(p.seed >> 32);
    if (MODE == MODE_QDQ && VAR != 0) asm volatile("; seed of variant %2" : "+s"(seed_lo), "+s"(seed_hi) : "n"(VAR * 2 + (FAST ? 1 : 0)));
    const uint64_t seed = (uint64_t)seed_lo | ((uint64_t)seed_hi << 32);
    uint32_t ctr_lo = (uint32_t)e0, ctr_hi = (uint32_t)((uint64_t)e0 >> 32);         // same for the counter (round 1 is seed-free)
    if (MODE == MODE_QDQ && VAR != 0) asm volatile("; counter of variant %2" : "+v"(ctr_lo), "+v"(ctr_hi) : "n"(VAR * 2 + (FAST ? 1 : 0)));
    const uint64_t ctr0 = (uint64_t)ctr_lo | ((uint64_t)ctr_hi << 32);
    f4* dst = (f4*)(p.out + e0);
    const float y = FAST ? 1.0f / a : 0.0f;             // RN(1/alpha): one IEEE division per bucket and lane
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int64_t e = e0 + (int64_t)j * LPB * 4;
        float rnd[4] = {0.f, 0.f, 0.f, 0.f};
        if (MODE == MODE_QDQ && VAR != 0 && p.stochastic) philox_uniform4(seed, (ctr0 + (uint64_t)j * LPB * 4) >> 2, rnd);
        float side[4];
        f4 r;
        if (MODE == MODE_QDQ && VAR == 0) {
            r.x = qdq_tab<FAST>(v[j].x, a, b, p.sm1, pp.mean, side[0], fl.tab, y);
            r.y = qdq_tab<FAST>(v[j].y, a, b, p.sm1, pp.mean, side[1], fl.tab, y);
            r.z = qdq_tab<FAST>(v[j].z, a, b, p.sm1, pp.mean, side[2], fl.tab, y);
            r.w = qdq_tab<FAST>(v[j].w, a, b, p.sm1, pp.mean, side[3], fl.tab, y);
        } else if (MODE == MODE_QDQ && VAR == 1) {
            r.x = qdq_stochastic_tab<FAST>(v[j].x, a, b, p.sm1, pp.mean, rnd[0], side[0], fl.tab, y);
            r.y = qdq_stochastic_tab<FAST>(v[j].y, a, b, p.sm1, pp.mean, rnd[1], side[1], fl.tab, y);
            r.z = qdq_stochastic_tab<FAST>(v[j].z, a, b, p.sm1, pp.mean, rnd[2], side[2], fl.tab, y);
            r.w = qdq_stochastic_tab<FAST>(v[j].w, a, b, p.sm1, pp.mean, rnd[3], side[3], fl.tab, y);
        } else {
            r = transform_f4<MODE, FAST>(p, T, v[j], a, b, pp.mean, rnd, side, y);
        }
        // MODE_SCALE: the whole-tile and partial-tile copies of this loop are merged by the compiler, and the merged store
        // loses its !nontemporal flag (qd_common.h store_nt_pinned)
        if (MODE == MODE_SCALE) store_nt_pinned((QD_AS_GLOBAL f4*)dst + j * LPB, r);
        else __builtin_nontemporal_store(r, dst + j * LPB);
        store_side4_row<MODE>(p, e, side);
    }
}

// One bucket held in registers by its LPB lanes (v[0..V): this lane's float4s, already loaded): reduce, transform,
// store.  The ONLY copy of the per-bucket arithmetic of the vector kernels: both loop shapes of k_bucket_vec call it.
template <int MODE, int LPB, int V>
__device__ __forceinline__ void vec_bucket(const KParams& p, const PointTable* T, const Prep& pp, const VecFlags& fl,
                                           f4 (&v)[V], int64_t bkt, int uu, int l, float& a_keep, float& b_keep) {
    constexpr int ROW = LPB * V * 4;
    const int64_t e0 = bkt * ROW + (int64_t)l * 4;     // first element of this lane
    float a, b;
    if (fl.prescaled) {
        a = p.alpha[bkt]; b = p.beta[bkt];
    } else {
        if (MODE != MODE_QDQ || fl.prep_on) {
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = prep4(v[j], pp);
        }
        float mn = pmin4(v[0]), mx = pmax4(v[0]);           // NaN-propagating: a NaN element makes both NaN
#pragma unroll
        for (int j = 1; j < V; ++j) { mn = pmin(mn, pmin4(v[j])); mx = pmax(mx, pmax4(v[j])); }
        if (LPB == 16) { mn = row16_min(mn); mx = row16_max(mx); }
        else { mn = wave_min(mn); mx = wave_max(mx); }
        alpha_beta(mn, mx, a, b);
        if (l == uu) { a_keep = a; b_keep = b; }       // lane uu of the group keeps bucket uu's pair
    }
    // quantize-dequantize consumes only the LEVEL of u, so the bucket-invariant division form is exact there (qd_common.h);
    // wave-uniform choice: every bucket of the wave must be in the proven range.  The transform loop is instantiated per
    // (variant, division form) and chosen ONCE per bucket: with the flags tested inside the loop the compiler no longer
    // unswitched it and the kernel executed 37.9 M instead of 33.9 M VALU wave-instructions (docs/history/profiles/r02_sq_counters.txt).
    const bool fast = MODE == MODE_QDQ && !__any(!fastdiv_ok(a));
    if (MODE == MODE_SCALE) {
        unsigned key = 0xFFFFFFFFu;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            key = min(key, min(scale_numerator_key(v[j].x, b), scale_numerator_key(v[j].y, b)));
            key = min(key, min(scale_numerator_key(v[j].z, b), scale_numerator_key(v[j].w, b)));
        }
        if (!__any(!scale_fast_ok(a, key))) vec_apply<MODE, LPB, V, 2, true>(p, T, pp, fl, v, e0, a, b);
        else vec_apply<MODE, LPB, V, 2, false>(p, T, pp, fl, v, e0, a, b);
    } else if (MODE != MODE_QDQ) vec_apply<MODE, LPB, V, 2, false>(p, T, pp, fl, v, e0, a, b);
    else if (fast) {
        if (fl.use_tab) vec_apply<MODE, LPB, V, 0, true>(p, T, pp, fl, v, e0, a, b);
        else if (fl.use_tab_s) vec_apply<MODE, LPB, V, 1, true>(p, T, pp, fl, v, e0, a, b);
        else vec_apply<MODE, LPB, V, 2, true>(p, T, pp, fl, v, e0, a, b);
    } else {
        if (fl.use_tab) vec_apply<MODE, LPB, V, 0, false>(p, T, pp, fl, v, e0, a, b);
        else if (fl.use_tab_s) vec_apply<MODE, LPB, V, 1, false>(p, T, pp, fl, v, e0, a, b);
        else vec_apply<MODE, LPB, V, 2, false>(p, T, pp, fl, v, e0, a, b);
    }
}

template <int MODE, int LPB, int V, int U>
__global__ __launch_bounds__(256) void k_bucket_vec(KParams p) {
    PointStore Ts;
    PointTable Tc;
    const PointTable* T = &Tc;                             // (read only in the nearest-point mode)
    if (MODE == MODE_NEAREST) load_points(Tc, Ts, p.pts, p.k, p.fine);

    constexpr int BPW = (64 / LPB) * U;           // buckets per wave tile
    constexpr int ROW = LPB * V * 4;              // elements per bucket.  CONTRACT (plan_transform, held by tests/test_transform_plan.py): p.row == ROW
    const int lane = threadIdx.x & 63;
    const int sub = lane / LPB;                   // which lane group of the wave
    const int l = lane % LPB;                     // lane inside the bucket
    const Prep pp = make_prep(p.mean, p.me);
    // wave-uniform shortcuts of the common configuration (no mean, no clamp, <= 16 levels, deterministic): they
    // take the kernel from ~43 to ~30 VALU instructions per element, which keeps it HBM-bound on boxes whose
    // sustained clock is lower (measured: 88 us vs 85.8 us for the leaner kbench kernel on the same box)
    // (MODE_QDQ only, so that the code generated for the other modes is untouched: the point-search kernels are
    // sensitive to it -- K5 at k = 256 went from 112 to 124 us when these branches were compiled into them.)
    VecFlags fl;
    fl.prescaled = (MODE == MODE_NEAREST && p.prescaled);
    fl.prep_on = MODE != MODE_QDQ || p.mean != nullptr || p.me != INFINITY;
    fl.use_tab = MODE == MODE_QDQ && !p.stochastic && p.sm1 <= 15.0f;
    fl.use_tab_s = MODE == MODE_QDQ && p.stochastic && p.sm1 <= 15.0f;
    fl.tab = MODE == MODE_QDQ ? (float)(lane & 15) / p.sm1 : 0.0f;

    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t ntiles = (p.nvec + BPW - 1) / BPW;

    // One loop shape around the one vec_bucket(): whole tiles unpredicated (all loads, then the buckets), the last,
    // partial tile bucket by bucket.
    for (int64_t t = wave; t < ntiles; t += nwaves) {
        const int64_t bkt0 = t * BPW + (int64_t)sub * U;          // first of this group's U buckets
        float a_keep = 0.0f, b_keep = 0.0f;
        if (bkt0 + U <= p.nvec) {
            // whole group in range (every tile but possibly the last): unpredicated.  All loads first, then the buckets
            // one after the other.
            f4 v[U][V];
#pragma unroll
            for (int uu = 0; uu < U; ++uu) {
                const f4* src = (const f4*)(p.x + (bkt0 + uu) * ROW + (int64_t)l * 4);
#pragma unroll
                for (int j = 0; j < V; ++j) v[uu][j] = __builtin_nontemporal_load(src + j * LPB);
            }
#pragma unroll
            for (int uu = 0; uu < U; ++uu) vec_bucket<MODE, LPB, V>(p, T, pp, fl, v[uu], bkt0 + uu, uu, l, a_keep, b_keep);
        } else {
            for (int uu = 0; uu < U; ++uu) {
                if (bkt0 + uu < p.nvec) {
                    f4 v[V];
                    const f4* src = (const f4*)(p.x + (bkt0 + uu) * ROW + (int64_t)l * 4);
#pragma unroll
                    for (int j = 0; j < V; ++j) v[j] = __builtin_nontemporal_load(src + j * LPB);
                    vec_bucket<MODE, LPB, V>(p, T, pp, fl, v, bkt0 + uu, uu, l, a_keep, b_keep);
                }
            }
        }
        // alpha/beta of the group's U buckets: lanes 0..U-1 write U consecutive floats (one store
        // instruction per array per tile instead of U single-lane stores)
        if (!fl.prescaled && l < U && bkt0 + l < p.nvec) {
            if (p.alpha) p.alpha[bkt0 + l] = a_keep;
            if (p.beta) p.beta[bkt0 + l] = b_keep;
        }
    }

    // buckets after the vector part (the ragged last bucket): one DPP row each, last block
    if (blockIdx.x == 0) {                                    // (the first block, which starts first: the tail overlaps the bulk)
        tail_buckets<MODE>(p, T, p.nvec, pp);
    }
}

// ---- chunk path: bucket sizes that are a multiple of 4 but not one of the vector sizes ----------
// (100, 1000, 36, 4096, ...).  A wave streams a CHUNK of m consecutive buckets (m a power of two, m * row / 4
// <= VMAX * 64 float4) with fully coalesced 16-byte loads -- lane i holds float4 i, i + 64, ... of the chunk,
// whatever the bucket boundaries are -- and keeps it in registers: one pass over HBM.  The per-float4 (min,
// max) go through LDS, where lane groups of 64 / m lanes reduce one bucket each; (alpha, beta) of the chunk's
// buckets come back through an LDS table.  Every chunk starts at a multiple of row * 4 bytes, so alignment
// only needs row % 4 == 0.  The buckets after the last whole chunk are done by the last block, a DPP row each.
template <int MODE, int VMAX>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(1, 4)))   // the chunk lives in registers
void k_bucket_chunk(KParams p, int m, int64_t nchunks) {
    PointStore Ts;
    PointTable Tc;
    const PointTable* T = &Tc;                             // (read only in the nearest-point mode)
    if (MODE == MODE_NEAREST) load_points(Tc, Ts, p.pts, p.k, p.fine);
    // dynamic LDS: [point table (nearest-point mode)] then per wave: pairs[VMAX * 64], ab[256], 1/alpha[256]
    float2* chunk_lds = (float2*)(qd_dyn_lds + (MODE == MODE_NEAREST ? point_table_bytes(p.k) : 0));
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // CONTRACT (plan_transform, held by tests/test_transform_plan.py for every bucket size): row % 4 == 0, 1 <= m <= 256 (ab, yt),
    // m * row / 4 <= VMAX * 64 (pr, v[]), m < 64 -> m a power of two or 48 .. 63 (G below), nchunks == (n / row) / m, fine == 0,
    // dynamic LDS == 2 * (VMAX * 64 + 256 + 128) * 8 + the coarse point table
    float2* pr = chunk_lds + w * (VMAX * 64 + 256 + 128);
    float2* ab = pr + VMAX * 64;
    float* yt = (float*)(ab + 256);

    const int Bq = (int)(p.row >> 2);                  // float4 per bucket
    const int nf = m * Bq;                             // float4 per chunk
    const int nj = (nf + 63) >> 6;                     // rounds of 64 float4 (<= VMAX)
    const int mlanes = m < 64 ? m : 64;                // buckets reduced side by side
    const int G = 64 / mlanes;                         // lanes per bucket in the reduce step (power of two)
    const int bl = lane / G, sub = lane % G;
    const int step_q = 64 / Bq, step_r = 64 % Bq;      // bucket of float4 (lane + 64 j): advanced incrementally
    const int q0 = lane / Bq, r0 = lane % Bq;
    const Prep pp = make_prep(p.mean, p.me);
    const bool prescaled = (MODE == MODE_NEAREST && p.prescaled);
    const bool prep_on = p.mean != nullptr || p.me != INFINITY;
    const bool use_tab = MODE == MODE_QDQ && !p.stochastic && p.sm1 <= 15.0f;
    const float tab = (float)(lane & 15) / p.sm1;
    const int64_t wave = uniform_wave_index();
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;

    for (int64_t c = wave; c < nchunks; c += nwaves) {
        const int64_t b0 = c * m;                      // first bucket of the chunk
        const int64_t e0 = b0 * p.row;                 // first element
        const f4* src = (const f4*)(p.x + e0);
        f4 v[VMAX];
        // always VMAX loads, the address clamped to the chunk's last float4 (a broadcast re-load): a load behind
        // a branch -- even a wave-uniform one -- gets an s_waitcnt vmcnt(0) at the join and the chunk would be
        // fetched one memory round trip per float4.  The launcher picks VMAX in {8, 16, 32} to bound the waste.
#pragma unroll
        for (int j = 0; j < VMAX; ++j) {
            const int f = lane + 64 * j;
            v[j] = __builtin_nontemporal_load(src + (f < nf ? f : nf - 1));
        }
        __builtin_amdgcn_sched_barrier(0);             // all loads in flight before the first use
        bool div_ok = true;
        if (!prescaled) {
#pragma unroll
            for (int j = 0; j < VMAX; ++j) {
                const int f = lane + 64 * j;
                if (j < nj && f < nf) {
                    if (prep_on) v[j] = prep4(v[j], pp);
                    pr[f] = make_float2(pmin4(v[j]), pmax4(v[j]));     // NaN-propagating
                }
            }
            // LDS operations of one wave complete in order; the fence/barrier only stop compiler reordering
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int bb = bl; bb < m; bb += mlanes) {  // G > 1: m is a multiple of mlanes, so the trip count is uniform
                const float2* q = pr + bb * Bq;
                float mn = INFINITY, mx = -INFINITY;
                for (int t = sub; t < Bq; t += G) {
                    const float2 pm = q[t];
                    mn = pmin(mn, pm.x); mx = pmax(mx, pm.y);
                }
                for (int sft = 1; sft < G; sft <<= 1) {
                    mn = pmin(mn, __shfl_xor(mn, sft));
                    mx = pmax(mx, __shfl_xor(mx, sft));
                }
                float a, b;
                alpha_beta(mn, mx, a, b);
                div_ok &= fastdiv_ok(a);
                if (sub == 0) {
                    ab[bb] = make_float2(a, b);
                    yt[bb] = 1.0f / a;                  // RN(1/alpha), one IEEE division per bucket
                    if (p.alpha) p.alpha[b0 + bb] = a;
                    if (p.beta) p.beta[b0 + bb] = b;
                }
            }
        } else {
            for (int bb = lane; bb < m; bb += 64) ab[bb] = make_float2(p.alpha[b0 + bb], p.beta[b0 + bb]);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        f4* dst = (f4*)(p.out + e0);
        // only the level of u is consumed by quantize-dequantize: bucket-invariant division (qd_common.h) when every
        // bucket of the chunk is in its proven range
        const bool fast = MODE == MODE_QDQ && !prescaled && !__any(!div_ok);
        auto body = [&](auto fast_c) {
            constexpr bool FAST = decltype(fast_c)::value;
            int q = q0, r = r0;
#pragma unroll
            for (int j = 0; j < VMAX; ++j) {
                const int f = lane + 64 * j;
                if (j < nj) {                                  // whole wave: lanes past the chunk work on their duplicate
                    const int qi = q < m ? q : m - 1;
                    const float2 s = ab[qi];
                    const float y = FAST ? yt[qi] : 0.0f;
                    const int64_t e = e0 + ((int64_t)f << 2);
                    float side[4];
                    f4 o;
                    if (use_tab) {                             // <= 16 levels, deterministic: see k_bucket_vec
                        o.x = qdq_tab<FAST>(v[j].x, s.x, s.y, p.sm1, pp.mean, side[0], tab, y);
                        o.y = qdq_tab<FAST>(v[j].y, s.x, s.y, p.sm1, pp.mean, side[1], tab, y);
                        o.z = qdq_tab<FAST>(v[j].z, s.x, s.y, p.sm1, pp.mean, side[2], tab, y);
                        o.w = qdq_tab<FAST>(v[j].w, s.x, s.y, p.sm1, pp.mean, side[3], tab, y);
                    } else {
                        float rnd[4] = {0.f, 0.f, 0.f, 0.f};
                        if (MODE == MODE_QDQ && p.stochastic) philox_uniform4(p.seed, (uint64_t)e >> 2, rnd);
                        o = transform_f4<MODE, FAST>(p, T, v[j], s.x, s.y, pp.mean, rnd, side, y);
                    }
                    // (int64 indices: exchanged inside the DPP row -- 16 consecutive float4s, all in range -- so that each store
                    // instruction writes 256 contiguous bytes; the row that straddles the end of the chunk stores per lane)
                    const bool row_in = MODE == MODE_NEAREST && !group_any<16>(f >= nf);
                    if (MODE == MODE_NEAREST && row_in) {
                        __builtin_nontemporal_store(o, dst + f);
                        store_side4_row<MODE>(p, e, side);
                    } else if (f < nf) {
                        __builtin_nontemporal_store(o, dst + f);
                        store_side4<MODE>(p, e, side);
                    }
                }
                q += step_q; r += step_r;
                if (r >= Bq) { r -= Bq; ++q; }
            }
        };
        if (fast) body(std::true_type{}); else body(std::false_type{});
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the next chunk overwrites pr / ab
        __builtin_amdgcn_wave_barrier();
    }

    if (blockIdx.x == 0) {                             // buckets after the last whole chunk (incl. the ragged one); block 0 starts first
        if (p.row > 256) {
            tail_buckets<MODE>(p, T, nchunks * m, pp);
        } else {
            const int row_id = threadIdx.x >> 4;
            for (int64_t bkt = nchunks * m + row_id; bkt < p.nb; bkt += (blockDim.x >> 4)) {
                const int64_t lo = bkt * p.row;
                const int64_t hi = lo + p.row < p.n ? lo + p.row : p.n;
                if (hi - lo == p.row) bucket_lanes4<MODE, 16>(p, T, bkt, lo, threadIdx.x & 15, pp);   // full: float4 accesses
                else bucket_lanes<MODE, 16>(p, T, bkt, lo, hi, threadIdx.x & 15, pp);
            }
        }
    }
}

// Same for bucket sizes that are NOT a multiple of 4 (33, 50, 7, 3, 1, ...): m is a multiple of 4, so every chunk
// still starts 16-byte aligned and holds a whole number of float4, but a float4 may straddle two buckets.  So the
// registers only carry the chunk between HBM and LDS: the prepared values are staged in LDS (16 B per float4), the lane
// (group) that reduces a bucket goes straight on to TRANSFORM it in place in LDS -- alpha, beta and 1/alpha are then
// per-lane constants, no per-element choice between two buckets, and no register array stays live across the phases --
// and finally every lane streams its float4s from LDS to HBM, coalesced.  (The first version transformed the register
// copy and picked (alpha, beta) per element from the two candidate buckets: 48 VALU instructions per element against
// 32 in the vector kernel, VALU-bound at 107-138 us for 64 Mi elements.)
template <int MODE, int VMAX>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(1, 6)))
void k_bucket_chunk_any(KParams p, int m, int64_t nchunks, int lead) {
    PointStore Ts;
    PointTable Tc;
    const PointTable* T = &Tc;                             // (read only in the nearest-point mode)
    if (MODE == MODE_NEAREST) load_points(Tc, Ts, p.pts, p.k, p.fine);
    // dynamic LDS: [point table (nearest-point mode)] then per wave: vals[VMAX * 256] floats (+ side bytes)
    float2* chunk_lds = (float2*)(qd_dyn_lds + (MODE == MODE_NEAREST ? point_table_bytes(p.k) : 0));
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // Side outputs (level / point indices up to 255) are staged as ONE BYTE per element behind the values -- a quarter more
    // LDS, only when such an output is asked for -- and leave with the values: four per lane, coalesced.  Stored from the
    // transform loop they would leave element by element in LDS order (lanes a bucket apart): 216 us instead of 95 us for
    // quantize + levels at bucket 33, 405 us for int64 point indices (docs/history/profiles/r03_side_outputs.txt).  (Up to 32 points: with
    // the 10.3 KB table of a larger point set the extra bytes cost a resident block, which measured slower than the scattered
    // stores: k = 256 at bucket 33: 316 us against 281 us.)
    const bool stage8 = qd::stage8(MODE, p.lev8 != nullptr, p.idx != nullptr, p.k);
    const int wave_floats = VMAX * 256 + (stage8 ? VMAX * 64 : 0);             // (the plan sizes the LDS by the same function)
    float* vals = (float*)chunk_lds + w * wave_floats;
    uint8_t* sidev = (uint8_t*)(vals + VMAX * 256);

    const int B = (int)p.row;
    const int nf = (m * B) >> 2;                       // float4 per chunk (m % 4 == 0)
    const int mlanes = m < 64 ? m : 64;
    const int G = 64 / mlanes;                         // lanes per bucket (a power of two whenever it is > 1)
    const int bl = lane / G, sub = lane % G;
    const int steps = (B + G - 1) / G;                 // elements each lane of a group handles
    const int nrounds = (m + mlanes - 1) / mlanes;     // buckets each lane group handles
    const Prep pp = make_prep(p.mean, p.me);
    const bool prescaled = (MODE == MODE_NEAREST && p.prescaled);
    const bool prep_on = p.mean != nullptr || p.me != INFINITY;
    const bool use_tab = MODE == MODE_QDQ && !p.stochastic && p.sm1 <= 15.0f;
    const float tab = (float)(lane & 15) / p.sm1;
    const int64_t wave = uniform_wave_index();
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;

    for (int64_t c = wave; c < nchunks; c += nwaves) {
        const int64_t b0 = c * m;
        const int64_t e0 = b0 * p.row;
        const f4* src = (const f4*)(p.x + e0);
        // Lane i of round j holds float4 (i + 64 j - h) of the chunk, h = the chunk's distance from the 128-byte line below
        // it: every load and store instruction then covers eight whole lines instead of straddling nine (chunks start at
        // arbitrary multiples of 16 bytes; measured on the one-wave-per-bucket kernel: 107.7 -> 100.1 us at bucket 1000).
        // CONTRACT (plan_transform, held by tests/test_transform_plan.py for every bucket size): m % 4 == 0, m >= 4, room for the
        // lead-in: m * row / 4 + 7 <= VMAX * 64, the lane rule of k_bucket_chunk, fine == 0, dynamic LDS == 2 * wave_floats * 4 +
        // the coarse point table.  `lead` is always 1: the plan has no case without the lead-in (the host branch that passed 0,
        // for sizes 506 .. 511, was unreachable and is gone); the parameter stays because removing it changes device code -- a
        // later change, with an A/B measurement.
        const int h = lead ? (int)((e0 >> 2) & 7) : 0;
        {
            f4 v[VMAX];
#pragma unroll
            for (int j = 0; j < VMAX; ++j) {           // always-issued loads with a clamped address, as above
                const int f = lane + 64 * j - h;
                v[j] = __builtin_nontemporal_load(src + (f < 0 ? 0 : (f < nf ? f : nf - 1)));
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < VMAX; ++j) {
                const int f = lane + 64 * j - h;
                if (f >= 0 && f < nf) {
                    if (!prescaled && prep_on) v[j] = prep4(v[j], pp);
                    ((f4*)vals)[f] = v[j];
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();

        // every lane runs every round and every step (clamped indices, masked stores): the level table of qdq_tab is
        // fetched with ds_bpermute from the lanes of the own DPP row, which must all be active
        for (int rd = 0; rd < nrounds; ++rd) {
            const int bb_raw = bl + rd * mlanes;
            const bool live = bb_raw < m;
            const int bb = live ? bb_raw : m - 1;
            float* q = vals + bb * B;
            float a, b;
            if (prescaled) {
                a = p.alpha[b0 + bb]; b = p.beta[b0 + bb];
            } else {
                float mn = INFINITY, mx = -INFINITY;
                int t = sub;
                for (; t + G < B; t += 2 * G) {         // two elements per step: one min3 / max3 each (NaN-propagating)
                    const float x0 = q[t], x1 = q[t + G];
                    mn = pmin(mn, pmin(x0, x1)); mx = pmax(mx, pmax(x0, x1));
                }
                if (t < B) { const float x0 = q[t]; mn = pmin(mn, x0); mx = pmax(mx, x0); }
                for (int sft = 1; sft < G; sft <<= 1) {
                    mn = pmin(mn, __shfl_xor(mn, sft));
                    mx = pmax(mx, __shfl_xor(mx, sft));
                }
                alpha_beta(mn, mx, a, b);
                if (live && sub == 0) {
                    if (p.alpha) p.alpha[b0 + bb] = a;
                    if (p.beta) p.beta[b0 + bb] = b;
                }
            }
            // only the level of u is consumed by quantize-dequantize: bucket-invariant division (qd_common.h) when every
            // bucket of this round is in its proven range
            const bool fast = MODE == MODE_QDQ && !__any(!fastdiv_ok(a));
            const int64_t eb = e0 + (int64_t)bb * B;   // first element of the bucket
            auto body = [&](auto fast_c) {
                constexpr bool FAST = decltype(fast_c)::value;
                const float y = FAST ? 1.0f / a : 0.0f; // RN(1/alpha), one IEEE division per bucket
                // four steps at a time: the four LDS reads, and in the nearest-point mode the four point searches, are
                // independent of each other (one element per step left every lane with `steps` dependent LDS chains in a
                // row: 234 us for the pre-processed forward at bucket 33 against 95 us for the plain quantize)
                for (int i = 0; i < steps; i += 4) {
                    int tt[4];
                    bool ok[4];
                    float xv[4], o[4], side[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int t_raw = sub + (i + c) * G;
                        ok[c] = live && t_raw < B && i + c < steps;
                        tt[c] = t_raw < B ? t_raw : B - 1;
                    }
#pragma unroll
                    for (int c = 0; c < 4; ++c) xv[c] = q[tt[c]];
                    if (use_tab) {
#pragma unroll
                        for (int c = 0; c < 4; ++c) o[c] = qdq_tab<FAST>(xv[c], a, b, p.sm1, pp.mean, side[c], tab, y);
                    } else {
                        float rnd[4] = {0.f, 0.f, 0.f, 0.f};
                        if (MODE == MODE_QDQ && p.stochastic) {
#pragma unroll
                            for (int c = 0; c < 4; ++c) {
                                const int64_t e = eb + tt[c];
                                float r4[4];
                                philox_uniform4(p.seed, (uint64_t)e >> 2, r4);
                                rnd[c] = r4[e & 3];
                            }
                        }
                        transform_x4<MODE, FAST>(p, T, xv, a, b, pp.mean, rnd, side, o, y);
                    }
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        if (ok[c]) {
                            q[tt[c]] = o[c];
                            if (stage8) sidev[bb * B + tt[c]] = (uint8_t)(int)side[c];
                            else store_side1<MODE>(p, eb + tt[c], side[c]);
                        }
                    }
                }
            };
            if (fast) body(std::true_type{}); else body(std::false_type{});
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        f4* dst = (f4*)(p.out + e0);
#pragma unroll
        for (int j = 0; j < VMAX; ++j) {
            const int f = lane + 64 * j - h;
            const bool in = f >= 0 && f < nf;
            if (in) __builtin_nontemporal_store(((const f4*)vals)[f], dst + f);
            if (MODE != MODE_SCALE && stage8) {
                const uint32_t pk = in ? ((const uint32_t*)sidev)[f] : 0u;
                const int64_t e = e0 + ((int64_t)f << 2);
                if (MODE == MODE_QDQ) {
                    if (in) *(uint32_t*)(p.lev8 + e) = pk;
                } else if (p.idx_bytes == 1) {
                    if (in) *(uint32_t*)((uint8_t*)p.idx + e) = pk;
                } else {
                    // int64: through the DPP-row exchange where the row's 16 float4s are all inside the chunk
                    const float sd[4] = {(float)(pk & 255u), (float)((pk >> 8) & 255u), (float)((pk >> 16) & 255u), (float)(pk >> 24)};
                    if (!group_any<16>(!in)) store_side4_row<MODE>(p, e, sd);
                    else if (in) store_side4<MODE>(p, e, sd);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the next chunk overwrites vals
        __builtin_amdgcn_wave_barrier();
    }

    if (blockIdx.x == 0) tail_buckets<MODE>(p, T, nchunks * m, pp);
}

}  // namespace
