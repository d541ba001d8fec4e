// qd_element.h -- what every kernel of the bucket transform does to ONE element or ONE bucket: the kernel parameters
// (KParams), the per-element transform of each mode (transform, transform_x4, transform_f4), the side-output stores
// (store_side1, store_side4, store_side4_row) and the scalar / float4 two-pass routines that a lane group runs over one
// arbitrary bucket (bucket_lanes, bucket_lanes4, tail_buckets).  Device code only; no kernel.
#pragma once

#include "qd_points.h"         // PointTable and the point searches; through it qd_common.h: Prep, qdq*, philox_uniform4, ...

#include <math.h>

using namespace qd;

namespace {

struct KParams {
    const float* x;      // input [n]
    float* out;          // QDQ/NEAREST: [n]; SCALE: [padded]
    int64_t n;
    int64_t row;         // elements per bucket row (>= 1)
    int64_t nb;          // number of buckets
    float* alpha;        // [nb] outputs, or inputs when prescaled
    float* beta;
    const float* mean;   // device scalar or null
    float me;            // clamp limit, +inf when off
    float sm1;           // levels - 1
    uint8_t* lev8;       // optional [n] level index
    void* idx;           // NEAREST: optional index output
    int idx_bytes;       // 8 or 1
    const float* pts;    // NEAREST: [k] sorted points
    int k;
    int assign_mode;
    int prescaled;       // NEAREST: x is already u, alpha/beta are inputs
    int fine;            // NEAREST, midpoint rule, k > 32: the kernel builds and uses the fine cell table (see PointStore)
    int stochastic;
    uint64_t seed;
    int64_t nvec;        // number of leading full buckets handled by the vector path
};

// the pre-processing of a call: the mean to subtract (a device scalar, or none) and the clamp limit
__device__ __forceinline__ Prep make_prep(const float* mean, float me) {
    Prep pp;
    pp.mean = mean ? *mean : 0.0f;
    pp.me = me;
    return pp;
}

// ---- per-element transform shared by every bucket kernel -----------------------------------
// v: prepared value (mean subtracted, clamped) -- or u itself when prescaled.
// e: global element index (for the side outputs and the random stream).
template <int MODE, bool FAST = false>
__device__ __forceinline__ float transform(const KParams& p, const PointTable* T, float v, float a, float b,
                                           float mean, float rnd, float& side, float y = 0.0f) {
    if (MODE == MODE_QDQ) {
        return p.stochastic ? qdq_stochastic<FAST>(v, a, b, p.sm1, mean, rnd, side, y)
                            : qdq<FAST>(v, a, b, p.sm1, mean, side, y);
    } else if (MODE == MODE_SCALE) {
        float u = v - b;
        u = div_alpha<FAST>(u, a, y);                // FAST only where the caller has checked the bucket (scale_fast_ok)
        return u;
    } else {
        float u = v;
        if (!p.prescaled) { u = v - b; u = u / a; }
        const int i = T->fine ? midpoint_index_fine(*T->s, p.k, u) : assign_point(*T->s, p.k, p.assign_mode, u);
        const float pt = T->s->pts[i];
        side = (float)i;
        float y = pt * a;
        y = y + b;
        y = y + mean;
        return y;
    }
}

// transform<MODE>() of the four elements of a float4 that share (a, b): the same arithmetic per element; in the
// nearest-point mode the four point searches run together.
template <int MODE, bool FAST = false>
__device__ __forceinline__ void transform_x4(const KParams& p, const PointTable* T, const float (&v)[4], float a, float b,
                                             float mean, const float (&rnd)[4], float (&side)[4], float (&out)[4],
                                             float y = 0.0f) {
    if (MODE == MODE_NEAREST && p.k <= 32) {
        float u[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            u[c] = v[c];
            if (!p.prescaled) { u[c] = v[c] - b; u[c] = u[c] / a; }
        }
        int i[4];
        float pt[4];
        assign_point4(*T->s, p.k, p.assign_mode, u, i);
#pragma unroll
        for (int c = 0; c < 4; ++c) pt[c] = T->s->pts[i[c]];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            side[c] = (float)i[c];
            float o = pt[c] * a;
            o = o + b;
            o = o + mean;
            out[c] = o;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) out[c] = transform<MODE, FAST>(p, T, v[c], a, b, mean, rnd[c], side[c], y);
    }
}
template <int MODE, bool FAST = false>
__device__ __forceinline__ f4 transform_f4(const KParams& p, const PointTable* T, const f4& v, float a, float b, float mean,
                                           const float (&rnd)[4], float (&side)[4], float y = 0.0f) {
    const float xs[4] = {v.x, v.y, v.z, v.w};
    float o[4];
    transform_x4<MODE, FAST>(p, T, xs, a, b, mean, rnd, side, o, y);
    const f4 r = {o[0], o[1], o[2], o[3]};
    return r;
}

template <int MODE>
__device__ __forceinline__ void store_side1(const KParams& p, int64_t e, float side) {
    if (MODE == MODE_QDQ) {
        if (p.lev8) p.lev8[e] = (uint8_t)(int)side;
    } else if (MODE == MODE_NEAREST) {
        if (p.idx) {
            if (p.idx_bytes == 8) ((int64_t*)p.idx)[e] = (int64_t)side;
            else ((uint8_t*)p.idx)[e] = (uint8_t)(int)side;
        }
    }
}

template <int MODE>
__device__ __forceinline__ void store_side4(const KParams& p, int64_t e, const float (&s)[4]) {
    if (MODE == MODE_QDQ) {
        if (p.lev8) {
            const uint32_t pk = (uint32_t)(int)s[0] | ((uint32_t)(int)s[1] << 8) | ((uint32_t)(int)s[2] << 16) |
                                ((uint32_t)(int)s[3] << 24);
            *(uint32_t*)(p.lev8 + e) = pk;
        }
    } else if (MODE == MODE_NEAREST) {
        if (p.idx) {
            if (p.idx_bytes == 8) {
                l2* o = (l2*)((int64_t*)p.idx + e);
                l2 a = {(int64_t)s[0], (int64_t)s[1]}, b = {(int64_t)s[2], (int64_t)s[3]};
                o[0] = a;      // plain stores: the two 16-byte halves of a lane's 32 B merge in L2
                o[1] = b;
            } else {
                const uint32_t pk = (uint32_t)(int)s[0] | ((uint32_t)(int)s[1] << 8) |
                                    ((uint32_t)(int)s[2] << 16) | ((uint32_t)(int)s[3] << 24);
                *(uint32_t*)((uint8_t*)p.idx + e) = pk;
            }
        }
    }
}

// store_side4 for callers where the 16 lanes of a DPP row hold 16 CONSECUTIVE float4 and are all active
// (k_bucket_vec): int64 indices are exchanged inside the row first so that each of the two store
// instructions writes 16 x 16 B contiguous bytes (lane i: chunk i, then chunk 16 + i of the row's 512 B)
// instead of every lane writing two 16-B halves at a 32-B stride.  Indices fit 16 bits (k <= 1024).
template <int MODE>
__device__ __forceinline__ void store_side4_row(const KParams& p, int64_t e, const float (&s)[4]) {
    if (MODE == MODE_NEAREST && p.idx && p.idx_bytes == 8) {
        const int lane = threadIdx.x & 63, l16 = lane & 15, rowbase = lane & 48;
        const uint32_t lo = (uint32_t)(int)s[0] | ((uint32_t)(int)s[1] << 16);
        const uint32_t hi = (uint32_t)(int)s[2] | ((uint32_t)(int)s[3] << 16);
        const int src_a = rowbase + (l16 >> 1), src_b = src_a + 8;
        const uint32_t a_lo = __shfl(lo, src_a), a_hi = __shfl(hi, src_a);
        const uint32_t b_lo = __shfl(lo, src_b), b_hi = __shfl(hi, src_b);
        const bool odd = l16 & 1;
        const uint32_t ca = odd ? a_hi : a_lo, cb = odd ? b_hi : b_lo;
        const l2 va = {(int64_t)(ca & 0xFFFFu), (int64_t)(ca >> 16)}, vb = {(int64_t)(cb & 0xFFFFu), (int64_t)(cb >> 16)};
        l2* o = (l2*)((int64_t*)p.idx + (e - (int64_t)l16 * 4));          // the row's first element
        o[l16] = va;                  // plain stores: 175.8 us vs 180.0 us with the non-temporal hint (k = 4, round 3); round 4, index output
        o[16 + l16] = vb;             // kept alive by the caller: 201.0 vs 199.4 us, no difference either way (docs/history/profiles/r04_ab_idx_stores.txt)
    } else {
        store_side4<MODE>(p, e, s);
    }
}

// (Round 4 measured the whole-wave form of this exchange -- each store instruction one contiguous KiB instead of four 256-byte
// pieces at a 512-byte stride -- on the stream kernel: 189.7 us both ways.  The layout of the index stores is not what holds
// the int64 calls at 67-71 % of the HBM peak; torch's own fp32 -> int64 conversion, the same 1 : 2 read : write mix, is the
// yardstick: docs/history/profiles/r04_ab_idx_stores.txt.)
// ---- LANES lanes (16 = one DPP row, 64 = a wave) process one arbitrary bucket [lo, hi): scalar
// accesses, two passes (the second pass re-reads from L1/L2).  Used for the ragged last bucket,
// short buckets, odd bucket sizes and the multi-tensor kernel's unaligned cases.
// `l` = lane index inside the group (0..LANES-1).
template <int MODE, int LANES>
__device__ __forceinline__ void bucket_lanes(const KParams& p, const PointTable* T, int64_t bkt, int64_t lo,
                                             int64_t hi, int l, const Prep& pp) {
    float a, b;
    if (MODE == MODE_NEAREST && p.prescaled) {
        a = p.alpha[bkt]; b = p.beta[bkt];
    } else {
        float mn = INFINITY, mx = -INFINITY;
        bool nan = false;
        for (int64_t i = lo + l; i < hi; i += LANES) {
            const float v = prep(p.x[i], pp);
            mn = fminf(mn, v); mx = fmaxf(mx, v);
            nan |= (v != v);
        }
        if (LANES == 16) { mn = row16_min(mn); mx = row16_max(mx); }
        else { mn = wave_min(mn); mx = wave_max(mx); }
        if (group_any<LANES>(nan)) { mn = NAN; mx = NAN; }
        alpha_beta(mn, mx, a, b);
        if (l == 0) {
            if (p.alpha) p.alpha[bkt] = a;
            if (p.beta) p.beta[bkt] = b;
        }
    }
    float last = 0.0f;
    for (int64_t i = lo + l; i < hi; i += LANES) {
        float v = p.x[i];
        if (!(MODE == MODE_NEAREST && p.prescaled)) v = prep(v, pp);
        float rnd = 0.0f;
        if (MODE == MODE_QDQ && p.stochastic) {
            float r4[4];
            philox_uniform4(p.seed, (uint64_t)i >> 2, r4);
            rnd = r4[i & 3];
        }
        float side = 0.0f;
        const float y = transform<MODE>(p, T, v, a, b, pp.mean, rnd, side);
        p.out[i] = y;
        store_side1<MODE>(p, i, side);
        last = y;
    }
    if (MODE == MODE_SCALE) {
        // padding of the ragged last bucket: copies of x[n-1], scaled (help_functions.py:76-86)
        const int64_t end = lo + p.row;
        if (hi < end && hi == p.n && p.nb > 1) {
            const float u_last = transform<MODE>(p, T, prep(p.x[p.n - 1], pp), a, b, pp.mean, 0.0f, last);
            for (int64_t i = hi + l; i < end; i += LANES) p.out[i] = u_last;
        }
    }
}

// Same, for a FULL bucket whose length is a multiple of 4 and whose base is 16-byte aligned:
// float4 accesses (4x fewer memory instructions than the scalar routine).  Odd bucket sizes such
// as 100 take this path; the second pass re-reads the bucket from L1/L2.
template <int MODE, int LANES>
__device__ __forceinline__ void bucket_lanes4(const KParams& p, const PointTable* T, int64_t bkt, int64_t lo,
                                              int l, const Prep& pp) {
    const int nv = (int)(p.row >> 2);
    const f4* src = (const f4*)(p.x + lo);
    f4* dst = (f4*)(p.out + lo);
    const bool prescaled = (MODE == MODE_NEAREST && p.prescaled);
    float a, b;
    if (prescaled) {
        a = p.alpha[bkt]; b = p.beta[bkt];
    } else {
        float mn = INFINITY, mx = -INFINITY;
        bool nan = false;
        for (int i = l; i < nv; i += LANES) {
            const f4 v = prep4(src[i], pp);
            mn = fminf(mn, fminf(fminf(v.x, v.y), fminf(v.z, v.w)));
            mx = fmaxf(mx, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
            nan |= has_nan4(v);
        }
        if (LANES == 16) { mn = row16_min(mn); mx = row16_max(mx); }
        else { mn = wave_min(mn); mx = wave_max(mx); }
        if (group_any<LANES>(nan)) { mn = NAN; mx = NAN; }
        alpha_beta(mn, mx, a, b);
        if (l == 0) {
            if (p.alpha) p.alpha[bkt] = a;
            if (p.beta) p.beta[bkt] = b;
        }
    }
    for (int i = l; i < nv; i += LANES) {
        f4 v = src[i];
        if (!prescaled) v = prep4(v, pp);
        const int64_t e = lo + ((int64_t)i << 2);
        float rnd[4] = {0.f, 0.f, 0.f, 0.f};
        if (MODE == MODE_QDQ && p.stochastic) {
            // element index need not be a multiple of 4 here: draw per element from its own block
            for (int c = 0; c < 4; ++c) {
                float r4[4];
                philox_uniform4(p.seed, (uint64_t)(e + c) >> 2, r4);
                rnd[c] = r4[(e + c) & 3];
            }
        }
        float side[4];
        const f4 r = transform_f4<MODE>(p, T, v, a, b, pp.mean, rnd, side);
        __builtin_nontemporal_store(r, dst + i);
        for (int c = 0; c < 4; ++c) store_side1<MODE>(p, e + c, side[c]);
    }
}

// The buckets a kernel's main path leaves over (from `first` on: the ragged last bucket, the full ones after the last whole
// tile / chunk), done by ONE block: a DPP row each for buckets up to 256 elements, a whole wave each above that -- a
// 16-lane group needs 2 x 500 dependent iterations for an 8000-element bucket (measured: 60-130 us at the end of a
// 64 Mi-element launch when the LAST block did it; the caller is block 0, which starts first, so the tail overlaps the bulk).
template <int MODE>
__device__ __forceinline__ void tail_buckets(const KParams& p, const PointTable* T, int64_t first, const Prep& pp) {
    if (p.row > 256) {
        for (int64_t bkt = first + (threadIdx.x >> 6); bkt < p.nb; bkt += (blockDim.x >> 6)) {
            const int64_t lo = bkt * p.row;
            const int64_t hi = lo + p.row < p.n ? lo + p.row : p.n;
            bucket_lanes<MODE, 64>(p, T, bkt, lo, hi, threadIdx.x & 63, pp);
        }
    } else {
        for (int64_t bkt = first + (threadIdx.x >> 4); bkt < p.nb; bkt += (blockDim.x >> 4)) {
            const int64_t lo = bkt * p.row;
            const int64_t hi = lo + p.row < p.n ? lo + p.row : p.n;
            bucket_lanes<MODE, 16>(p, T, bkt, lo, hi, threadIdx.x & 15, pp);
        }
    }
}

}  // namespace
