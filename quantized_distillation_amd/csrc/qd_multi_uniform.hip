// qd_multi_uniform.hip -- multi-tensor uniform quantization (K9): the per-parameter loop of the training steps
// (cnn_models/conv_forward_model.py:235-247) as one launch over a device table of QdTensorDesc.
//   bucketed    qd_multi_plan, qd_multi_uniform_f32                 k_multi_uniform: bit-identical to qd_uniform_f32 per tensor
//   no buckets  qd_multi_global_plan, qd_multi_uniform_global_f32   k_mg_*: bucket_size=None (e.g. cifar10_test.py:113), every
//               tensor one bucket with its own global min/max.  The loop costs three launches per tensor through
//               qd_uniform_f32 (reduce, fold, apply); here the whole model takes three launches in total.  Arithmetic
//               identical to qd_uniform_f32(bucket = 0).
//   options     qd_multi_uniform_opt_f32, qd_multi_uniform_global_opt_f32   k_multi_uniform_opt, k_mg_*_opt: the same two forms
//               with what the loops of translation_models/model.py:162,200-209 hand to every call: stochastic rounding and
//               maxElementAllowedForQuantization.  Tensor i of the table draws with seed0 + i, seed0 a launch argument or one
//               device word (a captured launch then draws anew at every replay, once the cell has been advanced on the stream).
//   levels      qd_multi_uniform_levels_f32, qd_multi_uniform_global_levels_f32   k_multi_uniform_lv, k_mg_apply_lv: the forms with
//               options again, with a level count per tensor from a device array beside the table ("8 bits first and last").
//   buckets     qd_multi_buckets_plan, qd_multi_uniform_buckets_f32   k_multi_uniform_bk: the bucketed form with a level count
//               AND a bucket size per tensor, both from device arrays (per-channel scales: bucket_i = elements per channel).
//               The register body is chosen per tensor at run time; rows above 256 elements take a wave each.  A row of more
//               than 64 Ki elements runs on one wave: functional, not tuned (whole-tensor scaling: the no-buckets form).
// Every kernel here is an instantiation of a body of qd_multi_uniform.h; the kernels stay separate symbols, so a launch without
// options runs code that has never heard of them:
//   k_multi_uniform, _opt, _lv   bucketed_tile<ROW, CLAMP, STOCH, float>, the level count an argument (the first two) or levels[ti]
//   k_multi_uniform_bk           its own tile rule (bucket_tiles, qd_multi.h) around reg_row and the row paths of qd_element.h
//   k_mg_minmax, _opt            mg_minmax_tile<CLAMP>
//   k_mg_apply, _opt, _lv        mg_apply_tile<CLAMP, STOCH, float>
#include "qd_multi_uniform.h"
// Nothing of this header is used here.  It stays because of k_mg_fold: the compiler assigns two scalar registers of its
// block_minmax loop the other way round (same instructions, same size) unless an earlier kernel of the unit has inlined
// block_minmax already, and until now k_minmax_partial / k_minmax_final of this header were those kernels.  The unit
// therefore still emits the two (4 KB, never launched from here); dropping them changes k_mg_fold's bytes -- a later
// change, with an A/B measurement.  (qd_multi_uniform_out16.hip has no such kernel and does without.)
#include "qd_single_kernels.h"

namespace {

// Every kernel below: a wave takes the tiles wave, wave + nwaves, ... ; uniform_wave_index() is scalar, so the tile -> tensor
// search (owner_of) and the descriptor load run on s_load.
template <int ROW>
__global__ __launch_bounds__(256) void k_multi_uniform(const QdTensorDesc* __restrict__ table, int ntensors, int64_t total_tiles,
                                                       int64_t bucket, float sm1) {
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const Levels lv = levels_of(sm1, threadIdx.x & 63);
    for (int64_t t = uniform_wave_index(); t < total_tiles; t += nwaves)
        bucketed_tile<ROW, false, 0, float>(table[owner_of(table, ntensors, t)], t, bucket, lv, INFINITY, 0);
}

template <int ROW, int STOCH>
__global__ __launch_bounds__(256) void k_multi_uniform_opt(const QdTensorDesc* __restrict__ table, int ntensors, int64_t total_tiles,
                                                           int64_t bucket, float sm1, float me, uint64_t seed,
                                                           const uint64_t* __restrict__ seed_cell) {
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t seed0 = STOCH ? first_seed(seed, seed_cell) : 0;
    const Levels lv = levels_of(sm1, threadIdx.x & 63);
    for (int64_t t = uniform_wave_index(); t < total_tiles; t += nwaves) {
        const int ti = owner_of(table, ntensors, t);
        bucketed_tile<ROW, true, STOCH, float>(table[ti], t, bucket, lv, me, seed0 + (uint64_t)ti);
    }
}

template <int ROW, int STOCH>
__global__ __launch_bounds__(256) void k_multi_uniform_lv(const QdTensorDesc* __restrict__ table, const int32_t* __restrict__ levels,
                                                          int ntensors, int64_t total_tiles, int64_t bucket, float me, uint64_t seed,
                                                          const uint64_t* __restrict__ seed_cell) {
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t seed0 = STOCH ? first_seed(seed, seed_cell) : 0;
    int cur = -1;                                   // the tensor lv belongs to
    Levels lv = {1.0f, 0.0f, false};
    for (int64_t t = uniform_wave_index(); t < total_tiles; t += nwaves) {
        const int ti = owner_of(table, ntensors, t);
        if (ti != cur) {
            cur = ti;
            lv = levels_of((float)(levels[ti] - 1), threadIdx.x & 63);
        }
        bucketed_tile<ROW, true, STOCH, float>(table[ti], t, bucket, lv, me, seed0 + (uint64_t)ti);
    }
}

// ---- no buckets: phase 1, phase 2 (one kernel for every form: it does not depend on the options), phase 3 ----
__global__ __launch_bounds__(256) void k_mg_minmax(const QdTensorDesc* __restrict__ table, int ntensors, int64_t total_tiles, float* part) {
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t t = uniform_wave_index(); t < total_tiles; t += nwaves)
        mg_minmax_tile<false>(table[owner_of(table, ntensors, t)], t, part, INFINITY);
}

__global__ __launch_bounds__(256) void k_mg_minmax_opt(const QdTensorDesc* __restrict__ table, int ntensors, int64_t total_tiles, float* part,
                                                       float me) {
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t t = uniform_wave_index(); t < total_tiles; t += nwaves)
        mg_minmax_tile<true>(table[owner_of(table, ntensors, t)], t, part, me);
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

__global__ __launch_bounds__(256) void k_mg_apply(const QdTensorDesc* __restrict__ table, int ntensors, int64_t total_tiles,
                                                  const float* ab, float sm1) {
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t t = uniform_wave_index(); t < total_tiles; t += nwaves) {
        const int ti = owner_of(table, ntensors, t);
        mg_apply_tile<false, 0, float>(table[ti], ti, t, ab, sm1, INFINITY, 0);
    }
}

template <int STOCH>
__global__ __launch_bounds__(256) void k_mg_apply_opt(const QdTensorDesc* __restrict__ table, int ntensors, int64_t total_tiles,
                                                      const float* ab, float sm1, float me, uint64_t seed,
                                                      const uint64_t* __restrict__ seed_cell) {
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t seed0 = STOCH ? first_seed(seed, seed_cell) : 0;
    for (int64_t t = uniform_wave_index(); t < total_tiles; t += nwaves) {
        const int ti = owner_of(table, ntensors, t);
        mg_apply_tile<true, STOCH, float>(table[ti], ti, t, ab, sm1, me, seed0 + (uint64_t)ti);
    }
}

// phases 1 and 2 do not depend on the level count (k_mg_minmax_opt, k_mg_fold); phase 3 with the tensor's own sm1
template <int STOCH>
__global__ __launch_bounds__(256) void k_mg_apply_lv(const QdTensorDesc* __restrict__ table, const int32_t* __restrict__ levels,
                                                     int ntensors, int64_t total_tiles, const float* ab, float me, uint64_t seed,
                                                     const uint64_t* __restrict__ seed_cell) {
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t seed0 = STOCH ? first_seed(seed, seed_cell) : 0;
    for (int64_t t = uniform_wave_index(); t < total_tiles; t += nwaves) {
        const int ti = owner_of(table, ntensors, t);
        mg_apply_tile<true, STOCH, float>(table[ti], ti, t, ab, (float)(levels[ti] - 1), me, seed0 + (uint64_t)ti);
    }
}

// ---- a level count AND a bucket size per tensor (per-channel scales: bucket_i = elements per output channel) ----------------
// levels[ti] and buckets[ti] are read with the descriptor (wave-uniform: scalar loads); sm1, use_tab, tab and the tensor's
// geometry (bucket_tiles, qd_multi.h: the rule qd_multi_buckets_plan counted with) are re-derived whenever the wave moves on to
// another tensor.  Which body a bucket takes:
//   row <= 256, a DPP row per bucket: a full row of a 16-byte aligned tensor takes reg_row at row 64 / 128 / 256 (a scalar
//     branch on the row, the wave is uniform in it), bucket_lanes4<16> at any other multiple of 4; a ragged last row, a row that
//     is no multiple of 4 and an unaligned tensor take bucket_lanes<16>;
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
    const int64_t wave = uniform_wave_index();
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t seed0 = STOCH ? first_seed(seed, seed_cell) : 0;
    Prep pp;
    pp.mean = 0.0f;
    pp.me = me;
    int cur = -1;                                   // the tensor lv and geo belong to
    Levels lv = {1.0f, 0.0f, false};
    BucketTiles geo;
    geo.row = 1; geo.nb = 0; geo.tiles = 0; geo.wave = false;
    for (int64_t t = wave; t < total_tiles; t += nwaves) {
        const int ti = owner_of(table, ntensors, t);
        const QdTensorDesc d = table[ti];
        if (d.n <= 0) continue;                     // (an empty tensor owns no tile)
        if (ti != cur) {
            cur = ti;
            lv = levels_of((float)(levels[ti] - 1), lane);
            const int64_t bucket = buckets[ti];
            geo = bucket_tiles(d.n, bucket > 0 ? bucket : 1);
            if (bucket <= 0) geo.nb = 0;            // no bucket of this tensor is reached
        }
        const uint64_t seed_t = seed0 + (uint64_t)ti;
        const KParams p = row_params<float>(d, geo.row, geo.nb, me, lv.sm1, STOCH, seed_t);
        const int64_t local = t - d.first_tile;
        const bool row4 = vector_aligned<float>(d) && (p.row & 3) == 0;     // rows that are a multiple of 4 then start aligned
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
                if (p.row == 256) reg_row<4, true, STOCH>(p.x, p.out, lo, l, pp, lv.sm1, lv.use_tab, lv.tab, seed_t);
                else if (p.row == 128) reg_row<2, true, STOCH>(p.x, p.out, lo, l, pp, lv.sm1, lv.use_tab, lv.tab, seed_t);
                else if (p.row == 64) reg_row<1, true, STOCH>(p.x, p.out, lo, l, pp, lv.sm1, lv.use_tab, lv.tab, seed_t);
                else bucket_lanes4<MODE_QDQ, 16>(p, nullptr, bkt, lo, l, pp);
            } else {
                bucket_lanes<MODE_QDQ, 16>(p, nullptr, bkt, lo, hi, l, pp);
            }
        }
    }
}

}  // namespace

// Phases 1 and 2 of every launch without buckets that has options (qd_multi.h; qd_multi_uniform_out16.hip calls it too).
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
    float me;
    if (!multi_args_ok(table, ntensors, total_tiles, bucket, levels, {}, 0, 0.0f, nullptr, me)) return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    dispatch(bucket, 0, QD_OUT_F16, [&](auto row, auto, auto) {
        hipLaunchKernelGGL((k_multi_uniform<decltype(row)::value>), dim3(blocks_for(total_tiles, 4)), dim3(256), 0,
                           (hipStream_t)stream, table, ntensors, total_tiles, bucket, (float)(levels - 1));
    });
    return check_launch();
}

int qd_multi_uniform_opt_f32(const QdTensorDesc* table, int ntensors, int64_t total_tiles, int64_t bucket, int levels,
                             int clamp, float max_element, int stochastic, uint64_t seed, const uint64_t* seed_cell,
                             void* stream) {
    float me;
    if (!multi_args_ok(table, ntensors, total_tiles, bucket, levels, {}, clamp, max_element, seed_cell, me))
        return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    dispatch(bucket, stochastic, QD_OUT_F16, [&](auto row, auto stoch, auto) {
        hipLaunchKernelGGL((k_multi_uniform_opt<decltype(row)::value, decltype(stoch)::value>), dim3(blocks_for(total_tiles, 4)),
                           dim3(256), 0, (hipStream_t)stream, table, ntensors, total_tiles, bucket, (float)(levels - 1), me, seed,
                           seed_cell);
    });
    return check_launch();
}

int64_t qd_multi_global_plan(QdTensorDesc* host_table, int ntensors) {
    if (!host_table || ntensors < 0) return -1;
    return fill_prefix(host_table, ntensors, [](const QdTensorDesc& d) { return (d.n + kTile - 1) / kTile; });
}

int qd_multi_uniform_global_f32(const QdTensorDesc* table, int ntensors, int64_t total_tiles, int levels,
                                float* alpha_beta, void* workspace, size_t workspace_bytes, void* stream) {
    float me;
    if (!multi_args_ok(table, ntensors, total_tiles, 1, levels, {{alpha_beta, 0}}, 0, 0.0f, nullptr, me))
        return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    if (!workspace_ok(workspace, workspace_bytes, total_tiles)) return QD_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)workspace;
    const int blocks = blocks_for(total_tiles, 4);
    // the plain phase 1 (no clamp in its text), then the fold and the plain phase 3
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
    if (!multi_args_ok(table, ntensors, total_tiles, 1, levels, {{alpha_beta, 0}}, clamp, max_element, seed_cell, me))
        return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    if (!workspace_ok(workspace, workspace_bytes, total_tiles)) return QD_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = blocks_for(total_tiles, 4);
    launch_mg_minmax_fold(table, ntensors, total_tiles, (float*)workspace, me, alpha_beta, blocks, st);
    dispatch(0, stochastic, QD_OUT_F16, [&](auto, auto stoch, auto) {
        hipLaunchKernelGGL(k_mg_apply_opt<decltype(stoch)::value>, dim3(blocks), dim3(256), 0, st, table, ntensors, total_tiles,
                           alpha_beta, (float)(levels - 1), me, seed, seed_cell);
    });
    return (int)hipGetLastError();
}

int qd_multi_uniform_levels_f32(const QdTensorDesc* table, const int32_t* levels, int ntensors, int64_t total_tiles,
                                int64_t bucket, int clamp, float max_element, int stochastic, uint64_t seed,
                                const uint64_t* seed_cell, void* stream) {
    float me;
    if (!multi_args_ok(table, ntensors, total_tiles, bucket, 2, {{levels, 3}}, clamp, max_element, seed_cell, me))
        return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    dispatch(bucket, stochastic, QD_OUT_F16, [&](auto row, auto stoch, auto) {
        hipLaunchKernelGGL((k_multi_uniform_lv<decltype(row)::value, decltype(stoch)::value>), dim3(blocks_for(total_tiles, 4)),
                           dim3(256), 0, (hipStream_t)stream, table, levels, ntensors, total_tiles, bucket, me, seed, seed_cell);
    });
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
    if (!multi_args_ok(table, ntensors, total_tiles, 1, 2, {{levels, 3}, {buckets, 7}}, clamp, max_element, seed_cell, me))
        return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    dispatch(0, stochastic, QD_OUT_F16, [&](auto, auto stoch, auto) {
        hipLaunchKernelGGL((k_multi_uniform_bk<decltype(stoch)::value>), dim3(blocks_for(total_tiles, 4)), dim3(256), 0,
                           (hipStream_t)stream, table, levels, buckets, ntensors, total_tiles, me, seed, seed_cell);
    });
    return check_launch();
}

int qd_multi_uniform_global_levels_f32(const QdTensorDesc* table, const int32_t* levels, int ntensors, int64_t total_tiles,
                                       int clamp, float max_element, int stochastic, uint64_t seed, const uint64_t* seed_cell,
                                       float* alpha_beta, void* workspace, size_t workspace_bytes, void* stream) {
    float me;
    if (!multi_args_ok(table, ntensors, total_tiles, 1, 2, {{levels, 3}, {alpha_beta, 0}}, clamp, max_element, seed_cell, me))
        return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    if (!workspace_ok(workspace, workspace_bytes, total_tiles)) return QD_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = blocks_for(total_tiles, 4);
    launch_mg_minmax_fold(table, ntensors, total_tiles, (float*)workspace, me, alpha_beta, blocks, st);
    dispatch(0, stochastic, QD_OUT_F16, [&](auto, auto stoch, auto) {
        hipLaunchKernelGGL(k_mg_apply_lv<decltype(stoch)::value>, dim3(blocks), dim3(256), 0, st, table, levels, ntensors,
                           total_tiles, alpha_beta, me, seed, seed_cell);
    });
    return (int)hipGetLastError();
}

}  // extern "C"
