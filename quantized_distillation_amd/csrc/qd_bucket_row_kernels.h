// qd_bucket_row_kernels.h -- the bucket kernels that give each bucket a unit of its own: k_bucket_wave_any (one, two or four
// waves per bucket, any size above 256, one pass over HBM), k_bucket_groups (a DPP row or a wave per bucket, two passes) and
// k_bucket_generic (a block per bucket, two passes).  The kernels in which a wave streams several buckets: qd_bucket_vec_kernels.h.
#pragma once

#include "qd_element.h"        // KParams, the transforms and side stores, make_prep, bucket_lanes*, tail_buckets

#include <type_traits>

using namespace qd;

namespace {

// ---- one wave per bucket, ANY bucket size above 256 (every mode): 513, 1000, 1001, 2000, 3000, ... ---------------
// The wave loads the 16-byte-aligned float4s that TOUCH its bucket [lo, hi) -- lane i holds float4 i, i + 64, ... counted
// from the aligned element at or below lo, so a bucket that does not start on a 16-byte boundary shares its first and last
// float4 with its neighbours (those two are fetched twice, the second time from L2) -- keeps them in registers, reduces
// min / max over the elements that belong to the bucket (rounds that lie wholly inside take the unmasked path: a
// wave-uniform test), and writes whole float4s with one 16-byte store, the up to 3 + 3 elements of the shared edge float4s
// one by one.  One pass over HBM at any size, the short last bucket included (the float4 that would reach past the end of
// the tensor is fetched as x[n-4 .. n-1] and rotated in registers: no byte outside the tensor is read, and nothing is
// ever stored outside the bucket) -- handing the last one or two buckets of a tensor to a 16-lane
// group, as the vector and chunk kernels do for their 256-element buckets, costs 60-130 us at bucket sizes of 3000-8000.  The chunk
// kernels (qd_bucket_vec_kernels.h) stay for small buckets, where a wave per bucket would leave most lanes idle.  The float4 grid is aligned in ELEMENT index (the base pointer is 16-byte aligned), so the
// stochastic draw of element e -- Philox block e >> 2, word e & 3 -- is the one every other kernel uses.
// G = waves per bucket (1, 2 or 4 of the block's four): above 2048 elements a single wave would need more than 8 rounds --
// 115-252 VGPRs, two to four waves per SIMD -- so the bucket is spread over 2 (up to 4096 elements) or 4 waves (up to
// 8192), which exchange their (min, max) through LDS across one block barrier; every wave then keeps at most 9 float4s.
template <int MODE, int V, int G>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))   // <= 256 VGPRs: the 32-float4 instance must keep two waves per SIMD
void k_bucket_wave_any(KParams p, int64_t nbk, int64_t amask) {
    PointStore Ts;
    PointTable Tc;
    __shared__ float red[2][4][2];                         // [iteration parity][wave of the block][min, max]
    const PointTable* T = &Tc;                             // (read only in the nearest-point mode)
    if (MODE == MODE_NEAREST) load_points(Tc, Ts, p.pts, p.k, p.fine);
    constexpr int GL = 64 * G;                             // lanes per bucket
    constexpr int GPB = 4 / G;                             // buckets per block and iteration
    const int lane = threadIdx.x & (GL - 1);               // lane inside the bucket's group
    const int wv = threadIdx.x >> 6;                       // wave of the block
    const Prep pp = make_prep(p.mean, p.me);
    const bool prescaled = (MODE == MODE_NEAREST && p.prescaled);
    const bool prep_on = !prescaled && (p.mean != nullptr || p.me != INFINITY);
    const bool use_tab = MODE == MODE_QDQ && !p.stochastic && p.sm1 <= 15.0f;
    const float tab = (float)(lane & 15) / p.sm1;
    const int64_t group = (int64_t)blockIdx.x * GPB + (threadIdx.x / GL);
    const int64_t ngroups = (int64_t)gridDim.x * GPB;
    const int64_t iters = (nbk + ngroups - 1) / ngroups;   // the same for every wave of the grid: the barriers below are uniform

    for (int64_t it = 0; it < iters; ++it) {
        const int64_t bkt = it * ngroups + group;
        const bool active = bkt < nbk;                     // uniform over the group's waves
        const int64_t lo = (active ? bkt : 0) * p.row;
        const int row = (int)(lo + p.row <= p.n ? p.row : p.n - lo);   // the last bucket may be short
        const int64_t a0 = lo & amask;                     // aligned element at or below lo (amask = ~31: a 128-byte line)
        const int off = (int)(a0 - lo);                    // -31 .. 0: position of a0 relative to the bucket
        const int nf = (int)(((lo + row + 3) >> 2) - (a0 >> 2));   // float4s from a0 to the bucket's last one
        const f4* src = (const f4*)(p.x + a0);
        // The bucket's last float4 may reach past the END OF THE TENSOR (n % 4 != 0; the last bucket, or the one before it
        // when the last one has fewer than 3 elements).  The lane that holds it fetches the 16 bytes x[n-4 .. n-1] instead
        // -- the same instruction with another address: 16-byte accesses need 4-byte alignment only -- and rotates the
        // t = n % 4 valid elements to the front; nothing outside the tensor is ever read.
        // (Instances with more than 16 float4 per lane -- buckets above 12288 elements -- sit at the 256-VGPR limit and have
        // no room for the rotation: the launcher keeps such buckets out of their range, block 0 does them with scalar
        // accesses below.)
        const bool tail_partial = V <= 16 && active && (((lo + row + 3) >> 2) << 2) > p.n;      // group-uniform
        // CONTRACT (plan_transform, held by tests/test_transform_plan.py for every bucket size): nf <= 64 * G * V, that is
        // row / 4 + (row % 4 ? 2 : 0) + (row % 32 ? 7 : 0) <= 64 * G * V; V <= 9 in the nearest-point mode (no scratch); nbk == nb
        // for V <= 16, and for V > 16 only the leading buckets whose last float4 ends inside the tensor
        f4 v[V];
        float a = 1.0f, b = 0.0f;
        float mn = INFINITY, mx = -INFINITY;
        if (active) {
#pragma unroll
            for (int j = 0; j < V; ++j) {                  // always issued, the index clamped (see k_bucket_chunk)
                const int f = lane + GL * j;
                const int fc = f < nf ? f : nf - 1;
                const float* ptr = (const float*)(src + fc);
                if (V <= 16 && tail_partial && fc == nf - 1) ptr = p.x + (p.n - 4);
                v[j] = __builtin_nontemporal_load((const f4*)ptr);
            }
            if (V <= 16 && tail_partial) {
                const int t = (int)(p.n & 3);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const int f = lane + GL * j;
                    if ((f < nf ? f : nf - 1) == nf - 1) {
                        const f4 w = v[j];
                        v[j].x = t == 1 ? w.w : (t == 2 ? w.z : w.y);
                        v[j].y = t == 2 ? w.w : w.z;
                        v[j].z = w.w;
                    }
                }
            }
            if (prescaled) {                               // x is u, alpha / beta are inputs
                a = p.alpha[bkt]; b = p.beta[bkt];
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    if (prep_on) v[j] = prep4(v[j], pp);
                    const int r0 = off + 4 * (lane + GL * j);      // position of this float4's first element in the bucket
                    if (off + 4 * GL * j >= 0 && off + 4 * GL * (j + 1) <= row) {   // group-uniform: the whole round is inside
                        mn = pmin(mn, pmin4(v[j])); mx = pmax(mx, pmax4(v[j]));
                    } else {
                        const float xs[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const bool in = (unsigned)(r0 + c) < (unsigned)row;
                            mn = pmin(mn, in ? xs[c] : INFINITY); mx = pmax(mx, in ? xs[c] : -INFINITY);
                        }
                    }
                }
                mn = wave_min(mn); mx = wave_max(mx);
            }
        }
        if (G > 1) {                                       // the bucket's waves exchange (min, max); parity: one barrier per iteration
            const int par = (int)(it & 1);
            if ((threadIdx.x & 63) == 0) { red[par][wv][0] = mn; red[par][wv][1] = mx; }
            __syncthreads();
            const int w0 = (wv / G) * G;
#pragma unroll
            for (int g = 0; g < G; ++g) { mn = pmin(mn, red[par][w0 + g][0]); mx = pmax(mx, red[par][w0 + g][1]); }
        }
        if (!active) continue;
        if (!prescaled) {
            alpha_beta(mn, mx, a, b);
            if (lane == 0) {
                if (p.alpha) p.alpha[bkt] = a;
                if (p.beta) p.beta[bkt] = b;
            }
        }
        const bool fast = MODE == MODE_QDQ && fastdiv_ok(a);   // a is uniform over the bucket's waves
        auto body = [&](auto fast_c) {
            constexpr bool FAST = decltype(fast_c)::value;
            const float y = FAST ? 1.0f / a : 0.0f;        // RN(1/alpha), one IEEE division per bucket
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const int f = lane + GL * j;
                const int r0 = off + 4 * f;
                const int64_t e = a0 + 4 * (int64_t)f;     // element index of this float4 (a multiple of 4)
                float side[4], o[4];
                const float xs[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
                if (use_tab) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) o[c] = qdq_tab<FAST>(xs[c], a, b, p.sm1, pp.mean, side[c], tab, y);
                } else {
                    float rnd[4] = {0.f, 0.f, 0.f, 0.f};
                    if (MODE == MODE_QDQ && p.stochastic) philox_uniform4(p.seed, (uint64_t)e >> 2, rnd);
#pragma unroll
                    for (int c = 0; c < 4; ++c) side[c] = 0.0f;
                    transform_x4<MODE, FAST>(p, T, xs, a, b, pp.mean, rnd, side, o, y);
                }
                if (off + 4 * GL * j >= 0 && off + 4 * GL * (j + 1) <= row) {   // group-uniform: the whole round is inside the bucket
                    const f4 r = {o[0], o[1], o[2], o[3]};
                    __builtin_nontemporal_store(r, (f4*)(p.out + e));
                    store_side4_row<MODE>(p, e, side);     // every DPP row holds 16 consecutive float4s, all lanes active
                } else if (r0 >= 0 && r0 + 4 <= row) {     // the float4 belongs to this bucket alone
                    const f4 r = {o[0], o[1], o[2], o[3]};
                    __builtin_nontemporal_store(r, (f4*)(p.out + e));
                    store_side4<MODE>(p, e, side);
                } else {                                   // shared with a neighbour (or outside the bucket): own elements only
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        if ((unsigned)(r0 + c) < (unsigned)row) {
                            p.out[e + c] = o[c];
                            store_side1<MODE>(p, e + c, side[c]);
                        }
                    }
                }
            }
        };
        if (fast) body(std::true_type{}); else body(std::false_type{});
        if (MODE == MODE_SCALE && row < (int)p.row) {
            // scale_down returns the padded layout: the short last bucket is filled up with copies of the scaled last
            // element (ref: help_functions.py:76-86)
            float ul = (prep_on ? prep(p.x[p.n - 1], pp) : p.x[p.n - 1]) - b;
            ul = ul / a;
            for (int64_t i = lo + row + lane; i < lo + p.row; i += GL) p.out[i] = ul;
        }
    }
    // nbk < p.nb only for the instances above 16 float4 per lane when the tensor's length is not a multiple of 4 (see the
    // launcher): the bucket(s) whose last float4 would reach past the end of the tensor, block 0, scalar accesses
    if (V > 16 && nbk < p.nb && blockIdx.x == 0) tail_buckets<MODE>(p, T, nbk, pp);
}

// ---- generic path, small/medium rows: one lane group (16 lanes or a wave) per bucket, 256-thread
// blocks, no LDS, no barrier.  Any row length / alignment.
template <int MODE, int LANES>
__global__ __launch_bounds__(256) void k_bucket_groups(KParams p) {
    PointStore Ts;
    PointTable Tc;
    const PointTable* T = &Tc;                             // (read only in the nearest-point mode)
    if (MODE == MODE_NEAREST) load_points(Tc, Ts, p.pts, p.k, p.fine);
    const Prep pp = make_prep(p.mean, p.me);
    const int64_t group = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / LANES;
    const int64_t ngroups = ((int64_t)gridDim.x * blockDim.x) / LANES;
    const int l = threadIdx.x % LANES;
    const bool vec4 = (p.row & 3) == 0 && (((((uintptr_t)p.x) | ((uintptr_t)p.out)) & kDataAlign) == 0);
    for (int64_t bkt = group; bkt < p.nb; bkt += ngroups) {
        const int64_t lo = bkt * p.row;
        const int64_t hi = lo + p.row < p.n ? lo + p.row : p.n;
        if (vec4 && hi - lo == p.row) bucket_lanes4<MODE, LANES>(p, T, bkt, lo, l, pp);
        else bucket_lanes<MODE, LANES>(p, T, bkt, lo, hi, l, pp);
    }
}

// ---- generic path, huge rows: one block per bucket, any row length / alignment ----------------
template <int MODE>
__global__ __launch_bounds__(1024) void k_bucket_generic(KParams p) {
    PointStore Ts;
    PointTable Tc;
    __shared__ float red[32];
    const PointTable* T = &Tc;                             // (read only in the nearest-point mode)
    if (MODE == MODE_NEAREST) load_points(Tc, Ts, p.pts, p.k, p.fine);
    const Prep pp = make_prep(p.mean, p.me);
    for (int64_t bkt = blockIdx.x; bkt < p.nb; bkt += gridDim.x) {
        const int64_t lo = bkt * p.row;
        const int64_t hi = lo + p.row < p.n ? lo + p.row : p.n;
        float a, b;
        if (MODE == MODE_NEAREST && p.prescaled) {
            a = p.alpha[bkt]; b = p.beta[bkt];
        } else {
            float mn = INFINITY, mx = -INFINITY;
            int nan = 0;
            for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
                const float v = prep(p.x[i], pp);
                mn = fminf(mn, v); mx = fmaxf(mx, v);
                nan |= (v != v);
            }
            block_minmax(mn, mx, red);
            if (__syncthreads_or(nan)) { mn = NAN; mx = NAN; }
            alpha_beta(mn, mx, a, b);
            if (threadIdx.x == 0) {
                if (p.alpha) p.alpha[bkt] = a;
                if (p.beta) p.beta[bkt] = b;
            }
        }
        for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
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
        }
        if (MODE == MODE_SCALE) {
            const int64_t end = lo + p.row;
            if (hi < end && hi == p.n && p.nb > 1) {
                float dummy;
                const float u_last = transform<MODE>(p, T, prep(p.x[p.n - 1], pp), a, b, pp.mean, 0.0f, dummy);
                for (int64_t i = hi + threadIdx.x; i < end; i += blockDim.x) p.out[i] = u_last;
            }
        }
    }
}

}  // namespace
