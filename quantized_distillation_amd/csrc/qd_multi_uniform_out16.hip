// qd_multi_uniform_out16.hip -- the one-launch model quantizer writing fp16 / bf16 outputs (fp32 masters, a 16-bit student):
//   bucketed    qd_multi_uniform_out16_f32          k_multi_uniform_o16<ROW, STOCH, OUT>
//   no buckets  qd_multi_uniform_global_out16_f32   k_mg_minmax_opt, k_mg_fold (qd_multi_uniform.hip, as they are: neither
//               touches q), then k_mg_apply_o16<STOCH, OUT>
// Siblings of k_multi_uniform_lv / k_mg_apply_lv (qd_multi_uniform.hip), the superset forms: a level count per tensor from a
// device array, the clamp, optional stochastic rounding.  Every fp32 operation -- min / max, alpha / beta, the bucket-invariant
// division, the level table up to 16 levels, the Philox draws, the clamp -- is the sibling's, line for line; the fp32 result is
// then converted by the compiler's own fp32 -> fp16 / bf16 conversion (IEEE round to nearest even: v_cvt_f16_f32,
// v_cvt_pk_bf16_f32 on gfx950; NaN stays NaN, +-inf stays, finite values beyond the format become +-inf, fp16 subnormals are
// produced, the sign of zero is kept) and stored as 16 bits.  Element e of tensor i is therefore that conversion of element e
// of what qd_multi_uniform_levels_f32 / qd_multi_uniform_global_levels_f32 writes, bit for bit.
// OUT is the out_kind of the C ABI (QD_OUT_F16 = 1, QD_OUT_BF16 = 2): an int, so that the kernel names read the same in every
// demangler.
#include "qd_transform.h"      // KParams, Prep, transform<MODE_QDQ>; launch geometry
#include "qd_multi.h"

namespace {

// Out16<OUT>::type and store4_nt (four results, one 8-byte non-temporal store): qd_multi.h

// bucket_lanes<MODE_QDQ, 16> (qd_transform.h) with a 16-bit store: a DPP row processes one arbitrary bucket [lo, hi) with scalar
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

__device__ __forceinline__ uint64_t first_seed(uint64_t seed, const uint64_t* __restrict__ seed_cell) {
    return seed_cell ? *seed_cell : seed;
}

// ---- bucketed: k_multi_uniform_lv with 16-bit stores ---------------------------------------------------------------------
// The register path wants x 16-byte aligned (float4 loads) and q 8-byte aligned (a lane stores its four results as 8 bytes; a
// full bucket starts a multiple of 128 bytes into q); everything else goes through the row path.  Both give the same bits.
template <int ROW, int STOCH, int OUT>
__global__ __launch_bounds__(256) void k_multi_uniform_o16(const QdTensorDesc* __restrict__ table, const int32_t* __restrict__ levels,
                                                           int ntensors, int64_t total_tiles, int64_t bucket, float me, uint64_t seed,
                                                           const uint64_t* __restrict__ seed_cell) {
    typedef typename Out16<OUT>::type O;
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
        O* const q = (O*)d.q;                       // n 16-bit elements (include/qd_hip.h)
        KParams p;
        p.x = d.x; p.out = nullptr; p.n = d.n;
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
                          ((((uintptr_t)d.x) & 15) | (((uintptr_t)d.q) & 7)) == 0;
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
            O* dst = q + lo + l * 4;                       // this lane's first four elements; the next four are 64 further on
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
                    store4_nt(r, dst + j * 64);
                }
            };
            if (fdiv) body(std::true_type{}); else body(std::false_type{});
        } else {
            bucket_row16_o16<O>(p, q, lo, hi, l, pp);
        }
    }
}

// ---- no buckets: k_mg_apply_lv with 16-bit stores (phase 3; phases 1 and 2 are the fp32 launch's own kernels) -------------
template <int STOCH, int OUT>
__global__ __launch_bounds__(256) void k_mg_apply_o16(const QdTensorDesc* __restrict__ table, const int32_t* __restrict__ levels,
                                                      int ntensors, int64_t total_tiles, const float* ab, float me, uint64_t seed,
                                                      const uint64_t* __restrict__ seed_cell) {
    typedef typename Out16<OUT>::type O;
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
        O* const q = (O*)d.q;                       // n 16-bit elements
        float lev;
        if (hi - lo == kTile && ((((uintptr_t)d.x) & 15) | (((uintptr_t)d.q) & 7)) == 0) {
            const f4* src = (const f4*)(d.x + lo) + lane;
            O* dst = q + lo + lane * 4;
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
                store4_nt(r, dst + j * 256);
            }
        } else {
            for (int64_t i = lo + lane; i < hi; i += 64) {
                const float c = prep(ldg(d.x + i), pp);
                if (STOCH) {
                    float r4[4];
                    philox_uniform4(seed_t, (uint64_t)i >> 2, r4);
                    stg((O)qdq_stochastic(c, a, b, sm1, 0.0f, r4[i & 3], lev), q + i);
                } else {
                    stg((O)qdq(c, a, b, sm1, 0.0f, lev), q + i);
                }
            }
        }
    }
}

// what both entry points refuse before anything else (the refusals of the _levels entry points, and the output kind)
inline bool args_ok(const QdTensorDesc* table, const int32_t* levels, int ntensors, int64_t total_tiles, int out_kind, int clamp,
                    float max_element, const uint64_t* seed_cell, float& me) {
    me = clamp ? max_element : INFINITY;
    if (!table || !levels || (((uintptr_t)levels) & 3) || ntensors <= 0 || total_tiles < 0) return false;
    if (out_kind != QD_OUT_F16 && out_kind != QD_OUT_BF16) return false;
    if (clamp && !(max_element > 0.0f)) return false;           // a positive limit, not NaN
    if (seed_cell && (((uintptr_t)seed_cell) & 7)) return false;
    return true;
}

}  // namespace

extern "C" {

int qd_multi_uniform_out16_f32(const QdTensorDesc* table, const int32_t* levels, int ntensors, int64_t total_tiles,
                               int64_t bucket, int out_kind, int clamp, float max_element, int stochastic, uint64_t seed,
                               const uint64_t* seed_cell, void* stream) {
    float me;
    if (bucket <= 0 || !args_ok(table, levels, ntensors, total_tiles, out_kind, clamp, max_element, seed_cell, me))
        return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = blocks_for(total_tiles, 4);
#define QD_MULTI_O16(ROW, STOCH, OUT)                                                                                      \
    hipLaunchKernelGGL((k_multi_uniform_o16<ROW, STOCH, OUT>), dim3(blocks), dim3(256), 0, st, table, levels, ntensors,    \
                       total_tiles, bucket, me, seed, seed_cell)
#define QD_MULTI_O16_ROW(ROW)                                                                                              \
    {                                                                                                                      \
        if (out_kind == QD_OUT_F16) { if (stochastic) QD_MULTI_O16(ROW, 1, QD_OUT_F16); else QD_MULTI_O16(ROW, 0, QD_OUT_F16); }    \
        else { if (stochastic) QD_MULTI_O16(ROW, 1, QD_OUT_BF16); else QD_MULTI_O16(ROW, 0, QD_OUT_BF16); }                         \
    }
    if (bucket == 256) QD_MULTI_O16_ROW(256)
    else if (bucket == 128) QD_MULTI_O16_ROW(128)
    else if (bucket == 64) QD_MULTI_O16_ROW(64)
    else QD_MULTI_O16_ROW(0)
#undef QD_MULTI_O16_ROW
#undef QD_MULTI_O16
    return check_launch();
}

int qd_multi_uniform_global_out16_f32(const QdTensorDesc* table, const int32_t* levels, int ntensors, int64_t total_tiles,
                                      int out_kind, int clamp, float max_element, int stochastic, uint64_t seed,
                                      const uint64_t* seed_cell, float* alpha_beta, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    float me;
    if (!alpha_beta || !args_ok(table, levels, ntensors, total_tiles, out_kind, clamp, max_element, seed_cell, me))
        return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    if (!workspace || (((uintptr_t)workspace) & 15) || workspace_bytes < (size_t)total_tiles * 2 * sizeof(float))
        return QD_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = blocks_for(total_tiles, 4);
    launch_mg_minmax_fold(table, ntensors, total_tiles, (float*)workspace, me, alpha_beta, blocks, st);
#define QD_MG_O16(STOCH, OUT)                                                                                              \
    hipLaunchKernelGGL((k_mg_apply_o16<STOCH, OUT>), dim3(blocks), dim3(256), 0, st, table, levels, ntensors, total_tiles, \
                       alpha_beta, me, seed, seed_cell)
    if (out_kind == QD_OUT_F16) { if (stochastic) QD_MG_O16(1, QD_OUT_F16); else QD_MG_O16(0, QD_OUT_F16); }
    else { if (stochastic) QD_MG_O16(1, QD_OUT_BF16); else QD_MG_O16(0, QD_OUT_BF16); }
#undef QD_MG_O16
    return (int)hipGetLastError();
}

}  // extern "C"
