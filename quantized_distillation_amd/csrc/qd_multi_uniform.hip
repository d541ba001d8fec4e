// qd_multi_uniform.hip -- multi-tensor uniform quantization (K9): the per-parameter loop of the training steps
// (cnn_models/conv_forward_model.py:235-247) as one launch over a device table of QdTensorDesc.
//   bucketed    qd_multi_plan, qd_multi_uniform_f32                 k_multi_uniform: bit-identical to qd_uniform_f32 per tensor
//   no buckets  qd_multi_global_plan, qd_multi_uniform_global_f32   k_mg_*: bucket_size=None (e.g. cifar10_test.py:113), every
//               tensor one bucket with its own global min/max.  The loop costs three launches per tensor through
//               qd_uniform_f32 (reduce, fold, apply); here the whole model takes three launches in total.  Arithmetic
//               identical to qd_uniform_f32(bucket = 0).
//   options     qd_multi_uniform_opt_f32, qd_multi_uniform_global_opt_f32   k_multi_uniform_opt, k_mg_*_opt: the same two forms
//               with what the loops of translation_models/model.py:162,200-209 hand to every call: stochastic rounding and
//               maxElementAllowedForQuantization.  Siblings, not flags: the plain kernels above keep their code.  Tensor i of the
//               table draws with seed0 + i, seed0 a launch argument or one device word (a captured launch then draws anew
//               at every replay, once the cell has been advanced on the stream).
//   levels      qd_multi_uniform_levels_f32, qd_multi_uniform_global_levels_f32   k_multi_uniform_lv, k_mg_apply_lv: the forms with
//               options again, with a level count per tensor from a device array beside the table ("8 bits first and last").
//   buckets     qd_multi_buckets_plan, qd_multi_uniform_buckets_f32   k_multi_uniform_bk: the bucketed form with a level count
//               AND a bucket size per tensor, both from device arrays (per-channel scales: bucket_i = elements per channel).
//               The register body is chosen per tensor at run time; rows above 256 elements take a wave each.  A row of more
//               than 64 Ki elements runs on one wave: functional, not tuned (whole-tensor scaling: the no-buckets form).
#include "qd_transform.h"      // bucket_row16, KParams, Prep for k_multi_uniform; launch geometry
#include "qd_multi.h"

namespace {

// ---- bucketed: one launch for every parameter of a model ---------------------------------------
// A tile = 4 buckets of one tensor = one wave iteration; a DPP row owns a bucket.  Full, 16-byte
// aligned 256-element buckets take the register path, everything else the row16 scalar path.
template <int ROW>
__global__ __launch_bounds__(256) void k_multi_uniform(const QdTensorDesc* __restrict__ table, int ntensors, int64_t total_tiles,
                                                       int64_t bucket, float sm1) {
    const int lane = threadIdx.x & 63;
    const int sub = lane >> 4, l = lane & 15;
    const int64_t wave = uniform_wave_index();      // scalar: owner_of runs on s_load
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    Prep pp;
    pp.mean = 0.0f;
    pp.me = INFINITY;
    const bool use_tab = sm1 <= 15.0f;
    const float tab = (float)(lane & 15) / sm1;
    for (int64_t t = wave; t < total_tiles; t += nwaves) {
        const QdTensorDesc d = table[owner_of(table, ntensors, t)];
        KParams p;
        p.x = d.x; p.out = d.q; p.n = d.n;
        p.row = d.n < bucket ? d.n : bucket;
        p.nb = (d.n + p.row - 1) / p.row;
        p.alpha = nullptr; p.beta = nullptr; p.mean = nullptr; p.me = INFINITY; p.sm1 = sm1; p.lev8 = nullptr;
        p.idx = nullptr; p.idx_bytes = 0; p.pts = nullptr; p.k = 0; p.assign_mode = 0; p.prescaled = 0;
        p.stochastic = 0; p.seed = 0; p.nvec = 0;
        const int64_t bkt = (t - d.first_tile) * 4 + sub;
        if (bkt >= p.nb) continue;
        const int64_t lo = bkt * p.row;
        const int64_t hi = lo + p.row < p.n ? lo + p.row : p.n;
        const bool fast = ROW > 0 && (hi - lo) == ROW && p.row == ROW &&
                          (((((uintptr_t)d.x) | ((uintptr_t)d.q)) & 15) == 0);
        if (fast) {
            constexpr int V = ROW > 0 ? ROW / 64 : 1;
            const f4* src = (const f4*)(p.x + lo) + l;
            f4 v[V];
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = ldg_nt(src + j * 16);   // masters: read once
            float mn = pmin4(v[0]), mx = pmax4(v[0]);      // NaN-propagating
#pragma unroll
            for (int j = 1; j < V; ++j) { mn = pmin(mn, pmin4(v[j])); mx = pmax(mx, pmax4(v[j])); }
            mn = row16_min(mn); mx = row16_max(mx);
            float a, b, lev;
            alpha_beta(mn, mx, a, b);
            f4* dst = (f4*)(p.out + lo) + l;
            // rows of the wave that took this branch: all in the proven range -> bucket-invariant division (qd_common.h)
            const bool fdiv = !__any(!fastdiv_ok(a));
            auto body = [&](auto fast_c) {
                constexpr bool FAST = decltype(fast_c)::value;
                const float y = FAST ? 1.0f / a : 0.0f;
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    f4 r;
                    if (use_tab) {                         // <= 16 levels: see k_bucket_vec (a DPP row is active as a whole here)
                        r.x = qdq_tab<FAST>(v[j].x, a, b, sm1, 0.0f, lev, tab, y);
                        r.y = qdq_tab<FAST>(v[j].y, a, b, sm1, 0.0f, lev, tab, y);
                        r.z = qdq_tab<FAST>(v[j].z, a, b, sm1, 0.0f, lev, tab, y);
                        r.w = qdq_tab<FAST>(v[j].w, a, b, sm1, 0.0f, lev, tab, y);
                    } else {
                        r.x = qdq<FAST>(v[j].x, a, b, sm1, 0.0f, lev, y);
                        r.y = qdq<FAST>(v[j].y, a, b, sm1, 0.0f, lev, y);
                        r.z = qdq<FAST>(v[j].z, a, b, sm1, 0.0f, lev, y);
                        r.w = qdq<FAST>(v[j].w, a, b, sm1, 0.0f, lev, y);
                    }
                    stg_nt(r, dst + j * 16);
                }
            };
            if (fdiv) body(std::true_type{}); else body(std::false_type{});
        } else {
            bucket_row16<MODE_QDQ>(p, nullptr, bkt, lo, hi, l, pp);
        }
    }
}

// The first seed of a launch: the by-value argument, or the device word when there is one (a kernel argument, so the load
// is a scalar one; the kernel never writes the cell).
__device__ __forceinline__ uint64_t first_seed(uint64_t seed, const uint64_t* __restrict__ seed_cell) {
    return seed_cell ? *seed_cell : seed;
}

// ---- bucketed, with options: k_multi_uniform plus the clamp (Prep::me) and, STOCH, stochastic rounding --------------------
// Tensor ti draws with seed0 + ti (its position in the table, empty tensors included); element e of it takes word e & 3 of
// Philox block e >> 2 as in every other kernel.  On the register path e is a multiple of 4: one block per float4.
template <int ROW, int STOCH>
__global__ __launch_bounds__(256) void k_multi_uniform_opt(const QdTensorDesc* __restrict__ table, int ntensors, int64_t total_tiles,
                                                           int64_t bucket, float sm1, float me, uint64_t seed,
                                                           const uint64_t* __restrict__ seed_cell) {
    const int lane = threadIdx.x & 63;
    const int sub = lane >> 4, l = lane & 15;
    const int64_t wave = uniform_wave_index();      // scalar: owner_of runs on s_load
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t seed0 = STOCH ? first_seed(seed, seed_cell) : 0;
    Prep pp;
    pp.mean = 0.0f;
    pp.me = me;
    const bool use_tab = sm1 <= 15.0f;
    const float tab = (float)(lane & 15) / sm1;
    for (int64_t t = wave; t < total_tiles; t += nwaves) {
        const int ti = owner_of(table, ntensors, t);
        const QdTensorDesc d = table[ti];
        const uint64_t seed_t = seed0 + (uint64_t)ti;
        KParams p;
        p.x = d.x; p.out = d.q; p.n = d.n;
        p.row = d.n < bucket ? d.n : bucket;
        p.nb = (d.n + p.row - 1) / p.row;
        p.alpha = nullptr; p.beta = nullptr; p.mean = nullptr; p.me = me; p.sm1 = sm1; p.lev8 = nullptr;
        p.idx = nullptr; p.idx_bytes = 0; p.pts = nullptr; p.k = 0; p.assign_mode = 0; p.prescaled = 0;
        p.stochastic = STOCH; p.seed = seed_t; p.nvec = 0;
        const int64_t bkt = (t - d.first_tile) * 4 + sub;
        if (bkt >= p.nb) continue;
        const int64_t lo = bkt * p.row;
        const int64_t hi = lo + p.row < p.n ? lo + p.row : p.n;
        const bool fast = ROW > 0 && (hi - lo) == ROW && p.row == ROW &&
                          (((((uintptr_t)d.x) | ((uintptr_t)d.q)) & 15) == 0);
        if (fast) {
            constexpr int V = ROW > 0 ? ROW / 64 : 1;
            const f4* src = (const f4*)(p.x + lo) + l;
            f4 v[V];
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = ldg_nt(src + j * 16);   // masters: read once
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = prep4(v[j], pp);        // the clamp comes before the bucket's min / max
            float mn = pmin4(v[0]), mx = pmax4(v[0]);      // NaN-propagating
#pragma unroll
            for (int j = 1; j < V; ++j) { mn = pmin(mn, pmin4(v[j])); mx = pmax(mx, pmax4(v[j])); }
            mn = row16_min(mn); mx = row16_max(mx);
            float a, b, lev;
            alpha_beta(mn, mx, a, b);
            f4* dst = (f4*)(p.out + lo) + l;
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
                    f4 r;
                    if (STOCH && use_tab) {                // <= 16 levels: a DPP row is active as a whole here
                        r.x = qdq_stochastic_tab<FAST>(v[j].x, a, b, sm1, 0.0f, rnd[0], lev, tab, y);
                        r.y = qdq_stochastic_tab<FAST>(v[j].y, a, b, sm1, 0.0f, rnd[1], lev, tab, y);
                        r.z = qdq_stochastic_tab<FAST>(v[j].z, a, b, sm1, 0.0f, rnd[2], lev, tab, y);
                        r.w = qdq_stochastic_tab<FAST>(v[j].w, a, b, sm1, 0.0f, rnd[3], lev, tab, y);
                    } else if (STOCH) {
                        r.x = qdq_stochastic<FAST>(v[j].x, a, b, sm1, 0.0f, rnd[0], lev, y);
                        r.y = qdq_stochastic<FAST>(v[j].y, a, b, sm1, 0.0f, rnd[1], lev, y);
                        r.z = qdq_stochastic<FAST>(v[j].z, a, b, sm1, 0.0f, rnd[2], lev, y);
                        r.w = qdq_stochastic<FAST>(v[j].w, a, b, sm1, 0.0f, rnd[3], lev, y);
                    } else if (use_tab) {
                        r.x = qdq_tab<FAST>(v[j].x, a, b, sm1, 0.0f, lev, tab, y);
                        r.y = qdq_tab<FAST>(v[j].y, a, b, sm1, 0.0f, lev, tab, y);
                        r.z = qdq_tab<FAST>(v[j].z, a, b, sm1, 0.0f, lev, tab, y);
                        r.w = qdq_tab<FAST>(v[j].w, a, b, sm1, 0.0f, lev, tab, y);
                    } else {
                        r.x = qdq<FAST>(v[j].x, a, b, sm1, 0.0f, lev, y);
                        r.y = qdq<FAST>(v[j].y, a, b, sm1, 0.0f, lev, y);
                        r.z = qdq<FAST>(v[j].z, a, b, sm1, 0.0f, lev, y);
                        r.w = qdq<FAST>(v[j].w, a, b, sm1, 0.0f, lev, y);
                    }
                    stg_nt(r, dst + j * 16);
                }
            };
            if (fdiv) body(std::true_type{}); else body(std::false_type{});
        } else {
            bucket_row16<MODE_QDQ>(p, nullptr, bkt, lo, hi, l, pp);
        }
    }
}

// ---- no buckets (kTile, the elements of a wave tile: qd_multi.h) -----------------------------------

// phase 1: per-tile min/max -> part[2*tile], part[2*tile+1]
__global__ __launch_bounds__(256) void k_mg_minmax(const QdTensorDesc* __restrict__ table, int ntensors, int64_t total_tiles, float* part) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = uniform_wave_index();      // scalar: owner_of runs on s_load
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t t = wave; t < total_tiles; t += nwaves) {
        const QdTensorDesc d = table[owner_of(table, ntensors, t)];
        const int64_t lo = (t - d.first_tile) * kTile;
        const int64_t hi = lo + kTile < d.n ? lo + kTile : d.n;
        float mn = INFINITY, mx = -INFINITY;
        bool nan = false;
        if (hi - lo == kTile && ((((uintptr_t)d.x) & 15) == 0)) {
            const f4* src = (const f4*)(d.x + lo) + lane;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f4 v = ldg(src + j * 64);           // plain loads: phase 3 re-reads from L2 / MALL
                mn = fminf(mn, fminf(fminf(v.x, v.y), fminf(v.z, v.w)));
                mx = fmaxf(mx, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
                nan |= has_nan4(v);
            }
        } else {
            for (int64_t i = lo + lane; i < hi; i += 64) { const float v = d.x[i]; mn = fminf(mn, v); mx = fmaxf(mx, v); nan |= (v != v); }
        }
        mn = wave_min(mn); mx = wave_max(mx);
        if (group_any<64>(nan)) { mn = NAN; mx = NAN; }       // NaN poisons the tile and, in phase 2, the tensor
        if (lane == 0) { part[2 * t] = mn; part[2 * t + 1] = mx; }
    }
}

// phase 2: one block per tensor folds its tiles into (alpha, beta); the 1e-10 guard on the device
__global__ __launch_bounds__(256) void k_mg_fold(const QdTensorDesc* __restrict__ table, int ntensors, int64_t total_tiles,
                                                 const float* part, float* ab /* [ntensors][2] */) {
    __shared__ float red[32];
    const int ti = blockIdx.x;
    const int64_t t0 = table[ti].first_tile;
    const int64_t t1 = ti + 1 < ntensors ? table[ti + 1].first_tile : total_tiles;
    float mn = INFINITY, mx = -INFINITY;
    int nan = 0;
    for (int64_t t = t0 + threadIdx.x; t < t1; t += 256) {
        const float pm = part[2 * t];
        nan |= (pm != pm);
        mn = fminf(mn, pm); mx = fmaxf(mx, part[2 * t + 1]);
    }
    block_minmax(mn, mx, red);
    if (__syncthreads_or(nan)) { mn = NAN; mx = NAN; }
    if (threadIdx.x == 0) {
        float a, b;
        alpha_beta(mn, mx, a, b);
        ab[2 * ti] = a; ab[2 * ti + 1] = b;
    }
}

// phase 3: apply with the tensor's single (alpha, beta)
__global__ __launch_bounds__(256) void k_mg_apply(const QdTensorDesc* __restrict__ table, int ntensors, int64_t total_tiles,
                                                  const float* ab, float sm1) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = uniform_wave_index();      // scalar: owner_of runs on s_load
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t t = wave; t < total_tiles; t += nwaves) {
        const int ti = owner_of(table, ntensors, t);
        const QdTensorDesc d = table[ti];
        const float a = ab[2 * ti], b = ab[2 * ti + 1];
        const int64_t lo = (t - d.first_tile) * kTile;
        const int64_t hi = lo + kTile < d.n ? lo + kTile : d.n;
        float lev;
        if (hi - lo == kTile && (((((uintptr_t)d.x) | ((uintptr_t)d.q)) & 15) == 0)) {
            const f4* src = (const f4*)(d.x + lo) + lane;
            f4* dst = (f4*)(d.q + lo) + lane;
            f4 v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = ldg_nt(src + j * 64);
            __builtin_amdgcn_sched_barrier(0);          // all four loads in flight before the first use
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f4 r;
                r.x = qdq(v[j].x, a, b, sm1, 0.0f, lev); r.y = qdq(v[j].y, a, b, sm1, 0.0f, lev);
                r.z = qdq(v[j].z, a, b, sm1, 0.0f, lev); r.w = qdq(v[j].w, a, b, sm1, 0.0f, lev);
                stg_nt(r, dst + j * 64);
            }
        } else {
            for (int64_t i = lo + lane; i < hi; i += 64) d.q[i] = qdq(d.x[i], a, b, sm1, 0.0f, lev);
        }
    }
}

// phases 1 and 3 with options (phase 2, the fold, is k_mg_fold): min / max of the clamped values; apply with the clamp and,
// STOCH, the draws of tensor ti under seed0 + ti -- one Philox block per float4, block = element index in the tensor >> 2
__global__ __launch_bounds__(256) void k_mg_minmax_opt(const QdTensorDesc* __restrict__ table, int ntensors, int64_t total_tiles, float* part,
                                                       float me) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = uniform_wave_index();      // scalar: owner_of runs on s_load
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    Prep pp;
    pp.mean = 0.0f;
    pp.me = me;
    for (int64_t t = wave; t < total_tiles; t += nwaves) {
        const QdTensorDesc d = table[owner_of(table, ntensors, t)];
        const int64_t lo = (t - d.first_tile) * kTile;
        const int64_t hi = lo + kTile < d.n ? lo + kTile : d.n;
        float mn = INFINITY, mx = -INFINITY;
        bool nan = false;
        if (hi - lo == kTile && ((((uintptr_t)d.x) & 15) == 0)) {
            const f4* src = (const f4*)(d.x + lo) + lane;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f4 v = prep4(ldg(src + j * 64), pp);      // plain loads: phase 3 re-reads from L2 / MALL
                mn = fminf(mn, fminf(fminf(v.x, v.y), fminf(v.z, v.w)));
                mx = fmaxf(mx, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
                nan |= has_nan4(v);
            }
        } else {
            for (int64_t i = lo + lane; i < hi; i += 64) { const float v = prep(d.x[i], pp); mn = fminf(mn, v); mx = fmaxf(mx, v); nan |= (v != v); }
        }
        mn = wave_min(mn); mx = wave_max(mx);
        if (group_any<64>(nan)) { mn = NAN; mx = NAN; }       // NaN poisons the tile and, in phase 2, the tensor
        if (lane == 0) { part[2 * t] = mn; part[2 * t + 1] = mx; }
    }
}

template <int STOCH>
__global__ __launch_bounds__(256) void k_mg_apply_opt(const QdTensorDesc* __restrict__ table, int ntensors, int64_t total_tiles,
                                                      const float* ab, float sm1, float me, uint64_t seed,
                                                      const uint64_t* __restrict__ seed_cell) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = uniform_wave_index();      // scalar: owner_of runs on s_load
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t seed0 = STOCH ? first_seed(seed, seed_cell) : 0;
    Prep pp;
    pp.mean = 0.0f;
    pp.me = me;
    for (int64_t t = wave; t < total_tiles; t += nwaves) {
        const int ti = owner_of(table, ntensors, t);
        const QdTensorDesc d = table[ti];
        const uint64_t seed_t = seed0 + (uint64_t)ti;
        const float a = ab[2 * ti], b = ab[2 * ti + 1];
        const int64_t lo = (t - d.first_tile) * kTile;
        const int64_t hi = lo + kTile < d.n ? lo + kTile : d.n;
        float lev;
        if (hi - lo == kTile && (((((uintptr_t)d.x) | ((uintptr_t)d.q)) & 15) == 0)) {
            const f4* src = (const f4*)(d.x + lo) + lane;
            f4* dst = (f4*)(d.q + lo) + lane;
            const uint64_t blk0 = (uint64_t)(lo >> 2) + (uint64_t)lane;
            f4 v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = ldg_nt(src + j * 64);
            __builtin_amdgcn_sched_barrier(0);          // all four loads in flight before the first use
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f4 c = prep4(v[j], pp);
                f4 r;
                if (STOCH) {
                    float rnd[4];
                    philox_uniform4(seed_t, blk0 + (uint64_t)(j * 64), rnd);
                    r.x = qdq_stochastic(c.x, a, b, sm1, 0.0f, rnd[0], lev); r.y = qdq_stochastic(c.y, a, b, sm1, 0.0f, rnd[1], lev);
                    r.z = qdq_stochastic(c.z, a, b, sm1, 0.0f, rnd[2], lev); r.w = qdq_stochastic(c.w, a, b, sm1, 0.0f, rnd[3], lev);
                } else {
                    r.x = qdq(c.x, a, b, sm1, 0.0f, lev); r.y = qdq(c.y, a, b, sm1, 0.0f, lev);
                    r.z = qdq(c.z, a, b, sm1, 0.0f, lev); r.w = qdq(c.w, a, b, sm1, 0.0f, lev);
                }
                stg_nt(r, dst + j * 64);
            }
        } else {
            for (int64_t i = lo + lane; i < hi; i += 64) {
                const float c = prep(d.x[i], pp);
                if (STOCH) {
                    float r4[4];
                    philox_uniform4(seed_t, (uint64_t)i >> 2, r4);
                    d.q[i] = qdq_stochastic(c, a, b, sm1, 0.0f, r4[i & 3], lev);
                } else {
                    d.q[i] = qdq(c, a, b, sm1, 0.0f, lev);
                }
            }
        }
    }
}

// ---- a level count per tensor: k_multi_uniform_opt / k_mg_apply_opt with sm1 taken from the tensor's row of a device table ----
// levels[ti] is read with the descriptor, from the index owner_of returns: wave-uniform, a scalar load.  What the kernels above
// derive from sm1 once per wave -- use_tab and tab = (float)(lane & 15) / sm1, the same correctly rounded division -- is derived
// here whenever the wave moves on to another tensor (a scalar branch; the tiles of one tensor that a wave takes in a row share
// it).  An entry < 2 gives sm1 <= 0: wrong values in that tensor's output and nothing else (sm1 is never an address; the table
// lookup of qdq_tab is a cross-lane read).  Siblings again: the kernels above keep their code.
template <int ROW, int STOCH>
__global__ __launch_bounds__(256) void k_multi_uniform_lv(const QdTensorDesc* __restrict__ table, const int32_t* __restrict__ levels,
                                                          int ntensors, int64_t total_tiles, int64_t bucket, float me, uint64_t seed,
                                                          const uint64_t* __restrict__ seed_cell) {
    const int lane = threadIdx.x & 63;
    const int sub = lane >> 4, l = lane & 15;
    const int64_t wave = uniform_wave_index();      // scalar: owner_of runs on s_load
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t seed0 = STOCH ? first_seed(seed, seed_cell) : 0;
    Prep pp;
    pp.mean = 0.0f;
    pp.me = me;
    int cur = -1;                                   // the tensor sm1 / use_tab / tab below belong to
    float sm1 = 1.0f, tab = 0.0f;
    bool use_tab = false;
    for (int64_t t = wave; t < total_tiles; t += nwaves) {
        const int ti = owner_of(table, ntensors, t);
        const QdTensorDesc d = table[ti];
        if (ti != cur) {
            cur = ti;
            sm1 = (float)(levels[ti] - 1);
            use_tab = sm1 <= 15.0f;
            tab = (float)(lane & 15) / sm1;
        }
        const uint64_t seed_t = seed0 + (uint64_t)ti;
        KParams p;
        p.x = d.x; p.out = d.q; p.n = d.n;
        p.row = d.n < bucket ? d.n : bucket;
        p.nb = (d.n + p.row - 1) / p.row;
        p.alpha = nullptr; p.beta = nullptr; p.mean = nullptr; p.me = me; p.sm1 = sm1; p.lev8 = nullptr;
        p.idx = nullptr; p.idx_bytes = 0; p.pts = nullptr; p.k = 0; p.assign_mode = 0; p.prescaled = 0;
        p.stochastic = STOCH; p.seed = seed_t; p.nvec = 0;
        const int64_t bkt = (t - d.first_tile) * 4 + sub;
        if (bkt >= p.nb) continue;
        const int64_t lo = bkt * p.row;
        const int64_t hi = lo + p.row < p.n ? lo + p.row : p.n;
        const bool fast = ROW > 0 && (hi - lo) == ROW && p.row == ROW &&
                          (((((uintptr_t)d.x) | ((uintptr_t)d.q)) & 15) == 0);
        if (fast) {
            constexpr int V = ROW > 0 ? ROW / 64 : 1;
            const f4* src = (const f4*)(p.x + lo) + l;
            f4 v[V];
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = ldg_nt(src + j * 16);   // masters: read once
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = prep4(v[j], pp);        // the clamp comes before the bucket's min / max
            float mn = pmin4(v[0]), mx = pmax4(v[0]);      // NaN-propagating
#pragma unroll
            for (int j = 1; j < V; ++j) { mn = pmin(mn, pmin4(v[j])); mx = pmax(mx, pmax4(v[j])); }
            mn = row16_min(mn); mx = row16_max(mx);
            float a, b, lev;
            alpha_beta(mn, mx, a, b);
            f4* dst = (f4*)(p.out + lo) + l;
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
                    f4 r;
                    if (STOCH && use_tab) {                // <= 16 levels: a DPP row is active as a whole here
                        r.x = qdq_stochastic_tab<FAST>(v[j].x, a, b, sm1, 0.0f, rnd[0], lev, tab, y);
                        r.y = qdq_stochastic_tab<FAST>(v[j].y, a, b, sm1, 0.0f, rnd[1], lev, tab, y);
                        r.z = qdq_stochastic_tab<FAST>(v[j].z, a, b, sm1, 0.0f, rnd[2], lev, tab, y);
                        r.w = qdq_stochastic_tab<FAST>(v[j].w, a, b, sm1, 0.0f, rnd[3], lev, tab, y);
                    } else if (STOCH) {
                        r.x = qdq_stochastic<FAST>(v[j].x, a, b, sm1, 0.0f, rnd[0], lev, y);
                        r.y = qdq_stochastic<FAST>(v[j].y, a, b, sm1, 0.0f, rnd[1], lev, y);
                        r.z = qdq_stochastic<FAST>(v[j].z, a, b, sm1, 0.0f, rnd[2], lev, y);
                        r.w = qdq_stochastic<FAST>(v[j].w, a, b, sm1, 0.0f, rnd[3], lev, y);
                    } else if (use_tab) {
                        r.x = qdq_tab<FAST>(v[j].x, a, b, sm1, 0.0f, lev, tab, y);
                        r.y = qdq_tab<FAST>(v[j].y, a, b, sm1, 0.0f, lev, tab, y);
                        r.z = qdq_tab<FAST>(v[j].z, a, b, sm1, 0.0f, lev, tab, y);
                        r.w = qdq_tab<FAST>(v[j].w, a, b, sm1, 0.0f, lev, tab, y);
                    } else {
                        r.x = qdq<FAST>(v[j].x, a, b, sm1, 0.0f, lev, y);
                        r.y = qdq<FAST>(v[j].y, a, b, sm1, 0.0f, lev, y);
                        r.z = qdq<FAST>(v[j].z, a, b, sm1, 0.0f, lev, y);
                        r.w = qdq<FAST>(v[j].w, a, b, sm1, 0.0f, lev, y);
                    }
                    stg_nt(r, dst + j * 16);
                }
            };
            if (fdiv) body(std::true_type{}); else body(std::false_type{});
        } else {
            bucket_row16<MODE_QDQ>(p, nullptr, bkt, lo, hi, l, pp);
        }
    }
}

// no buckets: phases 1 and 2 do not depend on the level count (k_mg_minmax_opt, k_mg_fold); phase 3 with the tensor's own sm1
template <int STOCH>
__global__ __launch_bounds__(256) void k_mg_apply_lv(const QdTensorDesc* __restrict__ table, const int32_t* __restrict__ levels,
                                                     int ntensors, int64_t total_tiles, const float* ab, float me, uint64_t seed,
                                                     const uint64_t* __restrict__ seed_cell) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = uniform_wave_index();      // scalar: owner_of runs on s_load
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t seed0 = STOCH ? first_seed(seed, seed_cell) : 0;
    Prep pp;
    pp.mean = 0.0f;
    pp.me = me;
    for (int64_t t = wave; t < total_tiles; t += nwaves) {
        const int ti = owner_of(table, ntensors, t);
        const QdTensorDesc d = table[ti];
        const float sm1 = (float)(levels[ti] - 1);
        const uint64_t seed_t = seed0 + (uint64_t)ti;
        const float a = ab[2 * ti], b = ab[2 * ti + 1];
        const int64_t lo = (t - d.first_tile) * kTile;
        const int64_t hi = lo + kTile < d.n ? lo + kTile : d.n;
        float lev;
        if (hi - lo == kTile && (((((uintptr_t)d.x) | ((uintptr_t)d.q)) & 15) == 0)) {
            const f4* src = (const f4*)(d.x + lo) + lane;
            f4* dst = (f4*)(d.q + lo) + lane;
            const uint64_t blk0 = (uint64_t)(lo >> 2) + (uint64_t)lane;
            f4 v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = ldg_nt(src + j * 64);
            __builtin_amdgcn_sched_barrier(0);          // all four loads in flight before the first use
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f4 c = prep4(v[j], pp);
                f4 r;
                if (STOCH) {
                    float rnd[4];
                    philox_uniform4(seed_t, blk0 + (uint64_t)(j * 64), rnd);
                    r.x = qdq_stochastic(c.x, a, b, sm1, 0.0f, rnd[0], lev); r.y = qdq_stochastic(c.y, a, b, sm1, 0.0f, rnd[1], lev);
                    r.z = qdq_stochastic(c.z, a, b, sm1, 0.0f, rnd[2], lev); r.w = qdq_stochastic(c.w, a, b, sm1, 0.0f, rnd[3], lev);
                } else {
                    r.x = qdq(c.x, a, b, sm1, 0.0f, lev); r.y = qdq(c.y, a, b, sm1, 0.0f, lev);
                    r.z = qdq(c.z, a, b, sm1, 0.0f, lev); r.w = qdq(c.w, a, b, sm1, 0.0f, lev);
                }
                stg_nt(r, dst + j * 64);
            }
        } else {
            for (int64_t i = lo + lane; i < hi; i += 64) {
                const float c = prep(d.x[i], pp);
                if (STOCH) {
                    float r4[4];
                    philox_uniform4(seed_t, (uint64_t)i >> 2, r4);
                    d.q[i] = qdq_stochastic(c, a, b, sm1, 0.0f, r4[i & 3], lev);
                } else {
                    d.q[i] = qdq(c, a, b, sm1, 0.0f, lev);
                }
            }
        }
    }
}

// ---- a level count AND a bucket size per tensor (per-channel scales: bucket_i = elements per output channel) ----------------
// One full, 16-byte aligned bucket row of 64 V elements held by the 16 lanes of a DPP row: the register body of
// k_multi_uniform_lv, V a constant here and the row a run-time fact of the tensor.
template <int V, int STOCH>
__device__ __forceinline__ void bk_reg_row(const float* x, float* out, int64_t lo, int l, const Prep& pp, float sm1, bool use_tab,
                                           float tab, uint64_t seed_t) {
    const f4* src = (const f4*)(x + lo) + l;
    f4 v[V];
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = ldg_nt(src + j * 16);   // masters: read once
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = prep4(v[j], pp);        // the clamp comes before the bucket's min / max
    float mn = pmin4(v[0]), mx = pmax4(v[0]);      // NaN-propagating
#pragma unroll
    for (int j = 1; j < V; ++j) { mn = pmin(mn, pmin4(v[j])); mx = pmax(mx, pmax4(v[j])); }
    mn = row16_min(mn); mx = row16_max(mx);
    float a, b, lev;
    alpha_beta(mn, mx, a, b);
    f4* dst = (f4*)(out + lo) + l;
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
            f4 r;
            if (STOCH && use_tab) {                // <= 16 levels: a DPP row is active as a whole here
                r.x = qdq_stochastic_tab<FAST>(v[j].x, a, b, sm1, 0.0f, rnd[0], lev, tab, y);
                r.y = qdq_stochastic_tab<FAST>(v[j].y, a, b, sm1, 0.0f, rnd[1], lev, tab, y);
                r.z = qdq_stochastic_tab<FAST>(v[j].z, a, b, sm1, 0.0f, rnd[2], lev, tab, y);
                r.w = qdq_stochastic_tab<FAST>(v[j].w, a, b, sm1, 0.0f, rnd[3], lev, tab, y);
            } else if (STOCH) {
                r.x = qdq_stochastic<FAST>(v[j].x, a, b, sm1, 0.0f, rnd[0], lev, y);
                r.y = qdq_stochastic<FAST>(v[j].y, a, b, sm1, 0.0f, rnd[1], lev, y);
                r.z = qdq_stochastic<FAST>(v[j].z, a, b, sm1, 0.0f, rnd[2], lev, y);
                r.w = qdq_stochastic<FAST>(v[j].w, a, b, sm1, 0.0f, rnd[3], lev, y);
            } else if (use_tab) {
                r.x = qdq_tab<FAST>(v[j].x, a, b, sm1, 0.0f, lev, tab, y);
                r.y = qdq_tab<FAST>(v[j].y, a, b, sm1, 0.0f, lev, tab, y);
                r.z = qdq_tab<FAST>(v[j].z, a, b, sm1, 0.0f, lev, tab, y);
                r.w = qdq_tab<FAST>(v[j].w, a, b, sm1, 0.0f, lev, tab, y);
            } else {
                r.x = qdq<FAST>(v[j].x, a, b, sm1, 0.0f, lev, y);
                r.y = qdq<FAST>(v[j].y, a, b, sm1, 0.0f, lev, y);
                r.z = qdq<FAST>(v[j].z, a, b, sm1, 0.0f, lev, y);
                r.w = qdq<FAST>(v[j].w, a, b, sm1, 0.0f, lev, y);
            }
            stg_nt(r, dst + j * 16);
        }
    };
    if (fdiv) body(std::true_type{}); else body(std::false_type{});
}

// levels[ti] and buckets[ti] are read with the descriptor (wave-uniform: scalar loads); sm1, use_tab, tab and the tensor's
// geometry (bucket_tiles, qd_multi.h: the rule qd_multi_buckets_plan counted with) are re-derived whenever the wave moves on to
// another tensor.  Which body a bucket takes:
//   row <= 256, a DPP row per bucket: a full row of a 16-byte aligned tensor takes the register body at row 64 / 128 / 256
//     (a scalar branch on the row, the wave is uniform in it), bucket_lanes4<16> at any other multiple of 4; a ragged last row,
//     a row that is no multiple of 4 and an unaligned tensor take bucket_row16;
//   row > 256, the wave per bucket: bucket_lanes4<64> for a full row that is a multiple of 4 in an aligned tensor, else
//     bucket_lanes<64>.  Two passes, the second served by L2.  A row of more than 64 Ki elements (a bucket size beyond the
//     tensor included) still runs on that one wave: correct, not tuned -- whole-tensor scaling has the bucket_size=None launch.
// Min / max do not depend on the order, the draws are indexed by element and the division is the bucket-invariant one only
// where it is exact, so every body gives the bits of qd_uniform_f32 at (buckets[ti], levels[ti]).  A buckets entry < 1 (the
// plan refuses one; the device array is the caller's) leaves its tensor unwritten and touches nothing else.
template <int STOCH>
__global__ __launch_bounds__(256) void k_multi_uniform_bk(const QdTensorDesc* __restrict__ table, const int32_t* __restrict__ levels,
                                                          const int64_t* __restrict__ buckets, int ntensors, int64_t total_tiles,
                                                          float me, uint64_t seed, const uint64_t* __restrict__ seed_cell) {
    const int lane = threadIdx.x & 63;
    const int sub = lane >> 4, l = lane & 15;
    const int64_t wave = uniform_wave_index();      // scalar: owner_of runs on s_load
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t seed0 = STOCH ? first_seed(seed, seed_cell) : 0;
    Prep pp;
    pp.mean = 0.0f;
    pp.me = me;
    int cur = -1;                                   // the tensor everything below belongs to
    float sm1 = 1.0f, tab = 0.0f;
    bool use_tab = false;
    BucketTiles geo;
    geo.row = 1; geo.nb = 0; geo.tiles = 0; geo.wave = false;
    for (int64_t t = wave; t < total_tiles; t += nwaves) {
        const int ti = owner_of(table, ntensors, t);
        const QdTensorDesc d = table[ti];
        if (d.n <= 0) continue;                     // (an empty tensor owns no tile)
        if (ti != cur) {
            cur = ti;
            sm1 = (float)(levels[ti] - 1);
            use_tab = sm1 <= 15.0f;
            tab = (float)(lane & 15) / sm1;
            const int64_t bucket = buckets[ti];
            geo = bucket_tiles(d.n, bucket > 0 ? bucket : 1);
            if (bucket <= 0) geo.nb = 0;            // no bucket of this tensor is reached
        }
        const uint64_t seed_t = seed0 + (uint64_t)ti;
        KParams p;
        p.x = d.x; p.out = d.q; p.n = d.n;
        p.row = geo.row;
        p.nb = geo.nb;
        p.alpha = nullptr; p.beta = nullptr; p.mean = nullptr; p.me = me; p.sm1 = sm1; p.lev8 = nullptr;
        p.idx = nullptr; p.idx_bytes = 0; p.pts = nullptr; p.k = 0; p.assign_mode = 0; p.prescaled = 0;
        p.stochastic = STOCH; p.seed = seed_t; p.nvec = 0;
        const int64_t local = t - d.first_tile;
        const bool aligned = ((((uintptr_t)d.x) | ((uintptr_t)d.q)) & 15) == 0;     // rows that are a multiple of 4 then start aligned
        const bool row4 = aligned && (p.row & 3) == 0;
        if (geo.wave) {
            const int64_t bkt = local;
            if (bkt >= p.nb) continue;              // (a tile count that does not belong to this table reaches no bucket)
            const int64_t lo = bkt * p.row;
            const int64_t hi = lo + p.row < p.n ? lo + p.row : p.n;
            if (row4 && hi - lo == p.row) bucket_lanes4<MODE_QDQ, 64>(p, nullptr, bkt, lo, lane, pp);
            else bucket_lanes<MODE_QDQ, 64>(p, nullptr, bkt, lo, hi, lane, pp);
        } else {
            const int64_t bkt = local * 4 + sub;
            if (bkt >= p.nb) continue;
            const int64_t lo = bkt * p.row;
            const int64_t hi = lo + p.row < p.n ? lo + p.row : p.n;
            if (row4 && hi - lo == p.row) {
                if (p.row == 256) bk_reg_row<4, STOCH>(p.x, p.out, lo, l, pp, sm1, use_tab, tab, seed_t);
                else if (p.row == 128) bk_reg_row<2, STOCH>(p.x, p.out, lo, l, pp, sm1, use_tab, tab, seed_t);
                else if (p.row == 64) bk_reg_row<1, STOCH>(p.x, p.out, lo, l, pp, sm1, use_tab, tab, seed_t);
                else bucket_lanes4<MODE_QDQ, 16>(p, nullptr, bkt, lo, l, pp);
            } else {
                bucket_row16<MODE_QDQ>(p, nullptr, bkt, lo, hi, l, pp);
            }
        }
    }
}

// clamp != 0 needs a positive limit (not NaN); the limit the kernels see, +inf when the clamp is off
inline bool clamp_limit(int clamp, float max_element, float& me) {
    me = clamp ? max_element : INFINITY;
    return !clamp || max_element > 0.0f;
}

}  // namespace

// phases 1 and 2 for qd_multi_uniform_out16.hip (qd_multi.h): the launches of qd_multi_uniform_global_levels_f32 below
void qd::launch_mg_minmax_fold(const QdTensorDesc* table, int ntensors, int64_t total_tiles, float* part, float me,
                               float* alpha_beta, int blocks, hipStream_t st) {
    hipLaunchKernelGGL(k_mg_minmax_opt, dim3(blocks), dim3(256), 0, st, table, ntensors, total_tiles, part, me);
    hipLaunchKernelGGL(k_mg_fold, dim3(ntensors), dim3(256), 0, st, table, ntensors, total_tiles, part, alpha_beta);
}

extern "C" {

int64_t qd_multi_plan(QdTensorDesc* host_table, int ntensors, int64_t bucket) {
    if (!host_table || ntensors < 0 || bucket <= 0) return -1;
    return fill_prefix(host_table, ntensors, [bucket](const QdTensorDesc& d) -> int64_t {
        if (d.n <= 0) return 0;
        int64_t nb, row;
        geometry(d.n, bucket, nb, row);
        return (nb + 3) / 4;                             // a tile: 4 buckets
    });
}

int qd_multi_uniform_f32(const QdTensorDesc* table, int ntensors, int64_t total_tiles, int64_t bucket, int levels,
                         void* stream) {
    if (!table || ntensors <= 0 || total_tiles < 0 || bucket <= 0 || levels < 2) return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = blocks_for(total_tiles, 4);
    const float sm1 = (float)(levels - 1);
    if (bucket == 256)
        hipLaunchKernelGGL((k_multi_uniform<256>), dim3(blocks), dim3(256), 0, st, table, ntensors, total_tiles, bucket, sm1);
    else if (bucket == 128)
        hipLaunchKernelGGL((k_multi_uniform<128>), dim3(blocks), dim3(256), 0, st, table, ntensors, total_tiles, bucket, sm1);
    else if (bucket == 64)
        hipLaunchKernelGGL((k_multi_uniform<64>), dim3(blocks), dim3(256), 0, st, table, ntensors, total_tiles, bucket, sm1);
    else
        hipLaunchKernelGGL((k_multi_uniform<0>), dim3(blocks), dim3(256), 0, st, table, ntensors, total_tiles, bucket, sm1);
    return check_launch();
}

int qd_multi_uniform_opt_f32(const QdTensorDesc* table, int ntensors, int64_t total_tiles, int64_t bucket, int levels,
                             int clamp, float max_element, int stochastic, uint64_t seed, const uint64_t* seed_cell,
                             void* stream) {
    float me;
    if (!table || ntensors <= 0 || total_tiles < 0 || bucket <= 0 || levels < 2 || !clamp_limit(clamp, max_element, me))
        return QD_ERR_INVALID_ARGUMENT;
    if (seed_cell && (((uintptr_t)seed_cell) & 7)) return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = blocks_for(total_tiles, 4);
    const float sm1 = (float)(levels - 1);
#define QD_MULTI_OPT(ROW)                                                                                                \
    {                                                                                                                    \
        if (stochastic)                                                                                                  \
            hipLaunchKernelGGL((k_multi_uniform_opt<ROW, 1>), dim3(blocks), dim3(256), 0, st, table, ntensors, total_tiles, \
                               bucket, sm1, me, seed, seed_cell);                                                        \
        else                                                                                                             \
            hipLaunchKernelGGL((k_multi_uniform_opt<ROW, 0>), dim3(blocks), dim3(256), 0, st, table, ntensors, total_tiles, \
                               bucket, sm1, me, seed, seed_cell);                                                        \
    }
    if (bucket == 256) QD_MULTI_OPT(256)
    else if (bucket == 128) QD_MULTI_OPT(128)
    else if (bucket == 64) QD_MULTI_OPT(64)
    else QD_MULTI_OPT(0)
#undef QD_MULTI_OPT
    return check_launch();
}

int64_t qd_multi_global_plan(QdTensorDesc* host_table, int ntensors) {
    if (!host_table || ntensors < 0) return -1;
    return fill_prefix(host_table, ntensors, [](const QdTensorDesc& d) { return (d.n + kTile - 1) / kTile; });
}

int qd_multi_uniform_global_f32(const QdTensorDesc* table, int ntensors, int64_t total_tiles, int levels,
                                float* alpha_beta, void* workspace, size_t workspace_bytes, void* stream) {
    if (!table || ntensors <= 0 || total_tiles < 0 || levels < 2 || !alpha_beta) return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    if (!workspace || (((uintptr_t)workspace) & 15) || workspace_bytes < (size_t)total_tiles * 2 * sizeof(float))
        return QD_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)workspace;
    const int blocks = blocks_for(total_tiles, 4);
    hipLaunchKernelGGL(k_mg_minmax, dim3(blocks), dim3(256), 0, st, table, ntensors, total_tiles, part);
    hipLaunchKernelGGL(k_mg_fold, dim3(ntensors), dim3(256), 0, st, table, ntensors, total_tiles, part, alpha_beta);
    hipLaunchKernelGGL(k_mg_apply, dim3(blocks), dim3(256), 0, st, table, ntensors, total_tiles, alpha_beta,
                       (float)(levels - 1));
    return (int)hipGetLastError();
}

int qd_multi_uniform_global_opt_f32(const QdTensorDesc* table, int ntensors, int64_t total_tiles, int levels,
                                    int clamp, float max_element, int stochastic, uint64_t seed, const uint64_t* seed_cell,
                                    float* alpha_beta, void* workspace, size_t workspace_bytes, void* stream) {
    float me;
    if (!table || ntensors <= 0 || total_tiles < 0 || levels < 2 || !alpha_beta || !clamp_limit(clamp, max_element, me))
        return QD_ERR_INVALID_ARGUMENT;
    if (seed_cell && (((uintptr_t)seed_cell) & 7)) return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    if (!workspace || (((uintptr_t)workspace) & 15) || workspace_bytes < (size_t)total_tiles * 2 * sizeof(float))
        return QD_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)workspace;
    const int blocks = blocks_for(total_tiles, 4);
    const float sm1 = (float)(levels - 1);
    hipLaunchKernelGGL(k_mg_minmax_opt, dim3(blocks), dim3(256), 0, st, table, ntensors, total_tiles, part, me);
    hipLaunchKernelGGL(k_mg_fold, dim3(ntensors), dim3(256), 0, st, table, ntensors, total_tiles, part, alpha_beta);
    if (stochastic)
        hipLaunchKernelGGL(k_mg_apply_opt<1>, dim3(blocks), dim3(256), 0, st, table, ntensors, total_tiles, alpha_beta, sm1, me,
                           seed, seed_cell);
    else
        hipLaunchKernelGGL(k_mg_apply_opt<0>, dim3(blocks), dim3(256), 0, st, table, ntensors, total_tiles, alpha_beta, sm1, me,
                           seed, seed_cell);
    return (int)hipGetLastError();
}

int qd_multi_uniform_levels_f32(const QdTensorDesc* table, const int32_t* levels, int ntensors, int64_t total_tiles,
                                int64_t bucket, int clamp, float max_element, int stochastic, uint64_t seed,
                                const uint64_t* seed_cell, void* stream) {
    float me;
    if (!table || !levels || (((uintptr_t)levels) & 3) || ntensors <= 0 || total_tiles < 0 || bucket <= 0 ||
        !clamp_limit(clamp, max_element, me))
        return QD_ERR_INVALID_ARGUMENT;
    if (seed_cell && (((uintptr_t)seed_cell) & 7)) return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = blocks_for(total_tiles, 4);
#define QD_MULTI_LV(ROW)                                                                                                 \
    {                                                                                                                    \
        if (stochastic)                                                                                                  \
            hipLaunchKernelGGL((k_multi_uniform_lv<ROW, 1>), dim3(blocks), dim3(256), 0, st, table, levels, ntensors,    \
                               total_tiles, bucket, me, seed, seed_cell);                                                \
        else                                                                                                             \
            hipLaunchKernelGGL((k_multi_uniform_lv<ROW, 0>), dim3(blocks), dim3(256), 0, st, table, levels, ntensors,    \
                               total_tiles, bucket, me, seed, seed_cell);                                                \
    }
    if (bucket == 256) QD_MULTI_LV(256)
    else if (bucket == 128) QD_MULTI_LV(128)
    else if (bucket == 64) QD_MULTI_LV(64)
    else QD_MULTI_LV(0)
#undef QD_MULTI_LV
    return check_launch();
}

int qd_multi_buckets_plan(QdTensorDesc* host_table, const int64_t* buckets, int ntensors, int64_t* total_tiles_out) {
    if (!host_table || !buckets || ntensors <= 0 || !total_tiles_out) return QD_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < ntensors; ++i) {
        const QdTensorDesc& d = host_table[i];
        if (buckets[i] <= 0 || d.n < 0 || (d.n > 0 && (!d.x || !d.q))) return QD_ERR_INVALID_ARGUMENT;
    }
    *total_tiles_out = fill_prefix(host_table, ntensors, [host_table, buckets](const QdTensorDesc& d) -> int64_t {
        return d.n > 0 ? bucket_tiles(d.n, buckets[&d - host_table]).tiles : 0;      // (the descriptor's position)
    });
    return 0;
}

int qd_multi_uniform_buckets_f32(const QdTensorDesc* table, const int32_t* levels, const int64_t* buckets, int ntensors,
                                 int64_t total_tiles, int clamp, float max_element, int stochastic, uint64_t seed,
                                 const uint64_t* seed_cell, void* stream) {
    float me;
    if (!table || !levels || (((uintptr_t)levels) & 3) || !buckets || (((uintptr_t)buckets) & 7) || ntensors <= 0 ||
        total_tiles < 0 || !clamp_limit(clamp, max_element, me))
        return QD_ERR_INVALID_ARGUMENT;
    if (seed_cell && (((uintptr_t)seed_cell) & 7)) return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = blocks_for(total_tiles, 4);
    if (stochastic)
        hipLaunchKernelGGL((k_multi_uniform_bk<1>), dim3(blocks), dim3(256), 0, st, table, levels, buckets, ntensors, total_tiles,
                           me, seed, seed_cell);
    else
        hipLaunchKernelGGL((k_multi_uniform_bk<0>), dim3(blocks), dim3(256), 0, st, table, levels, buckets, ntensors, total_tiles,
                           me, seed, seed_cell);
    return check_launch();
}

int qd_multi_uniform_global_levels_f32(const QdTensorDesc* table, const int32_t* levels, int ntensors, int64_t total_tiles,
                                       int clamp, float max_element, int stochastic, uint64_t seed, const uint64_t* seed_cell,
                                       float* alpha_beta, void* workspace, size_t workspace_bytes, void* stream) {
    float me;
    if (!table || !levels || (((uintptr_t)levels) & 3) || ntensors <= 0 || total_tiles < 0 || !alpha_beta ||
        !clamp_limit(clamp, max_element, me))
        return QD_ERR_INVALID_ARGUMENT;
    if (seed_cell && (((uintptr_t)seed_cell) & 7)) return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    if (!workspace || (((uintptr_t)workspace) & 15) || workspace_bytes < (size_t)total_tiles * 2 * sizeof(float))
        return QD_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)workspace;
    const int blocks = blocks_for(total_tiles, 4);
    hipLaunchKernelGGL(k_mg_minmax_opt, dim3(blocks), dim3(256), 0, st, table, ntensors, total_tiles, part, me);
    hipLaunchKernelGGL(k_mg_fold, dim3(ntensors), dim3(256), 0, st, table, ntensors, total_tiles, part, alpha_beta);
    if (stochastic)
        hipLaunchKernelGGL(k_mg_apply_lv<1>, dim3(blocks), dim3(256), 0, st, table, levels, ntensors, total_tiles, alpha_beta, me,
                           seed, seed_cell);
    else
        hipLaunchKernelGGL(k_mg_apply_lv<0>, dim3(blocks), dim3(256), 0, st, table, levels, ntensors, total_tiles, alpha_beta, me,
                           seed, seed_cell);
    return (int)hipGetLastError();
}

}  // extern "C"
