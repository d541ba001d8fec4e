// qd_multi_uniform_out16.hip -- the one-launch model quantizer writing fp16 / bf16 outputs (fp32 masters, a 16-bit student):
//   bucketed    qd_multi_uniform_out16_f32          k_multi_uniform_o16<ROW, STOCH, OUT>
//   no buckets  qd_multi_uniform_global_out16_f32   k_mg_minmax_opt, k_mg_fold (qd_multi_uniform.hip, as they are: neither
//               touches q), then k_mg_apply_o16<STOCH, OUT>
// The superset forms -- a level count per tensor from a device array, the clamp, optional stochastic rounding -- as the bodies
// k_multi_uniform_lv and k_mg_apply_lv are instantiated from (qd_multi_uniform.h: bucketed_tile, mg_apply_tile), with a 16-bit
// output element.  Every fp32 operation -- min / max, alpha / beta, the bucket-invariant division, the level table up to 16
// levels, the Philox draws, the clamp -- is therefore the fp32 launch's own text; the fp32 result is then converted by the
// compiler's own fp32 -> fp16 / bf16 conversion (IEEE round to nearest even: v_cvt_f16_f32, v_cvt_pk_bf16_f32 on gfx950; NaN
// stays NaN, +-inf stays, finite values beyond the format become +-inf, fp16 subnormals are produced, the sign of zero is kept)
// and stored as 16 bits.  Element e of tensor i is that conversion of element e of what qd_multi_uniform_levels_f32 /
// qd_multi_uniform_global_levels_f32 writes, bit for bit.
// OUT is the out_kind of the C ABI (QD_OUT_F16 = 1, QD_OUT_BF16 = 2): an int, so that the kernel names read the same in every
// demangler.
#include "qd_multi_uniform.h"

namespace {

template <int ROW, int STOCH, int OUT>
__global__ __launch_bounds__(256) void k_multi_uniform_o16(const QdTensorDesc* __restrict__ table, const int32_t* __restrict__ levels,
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
        bucketed_tile<ROW, true, STOCH, typename Out16<OUT>::type>(table[ti], t, bucket, lv, me, seed0 + (uint64_t)ti);
    }
}

template <int STOCH, int OUT>
__global__ __launch_bounds__(256) void k_mg_apply_o16(const QdTensorDesc* __restrict__ table, const int32_t* __restrict__ levels,
                                                      int ntensors, int64_t total_tiles, const float* ab, float me, uint64_t seed,
                                                      const uint64_t* __restrict__ seed_cell) {
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t seed0 = STOCH ? first_seed(seed, seed_cell) : 0;
    for (int64_t t = uniform_wave_index(); t < total_tiles; t += nwaves) {
        const int ti = owner_of(table, ntensors, t);
        mg_apply_tile<true, STOCH, typename Out16<OUT>::type>(table[ti], ti, t, ab, (float)(levels[ti] - 1), me,
                                                              seed0 + (uint64_t)ti);
    }
}

}  // namespace

extern "C" {

int qd_multi_uniform_out16_f32(const QdTensorDesc* table, const int32_t* levels, int ntensors, int64_t total_tiles,
                               int64_t bucket, int out_kind, int clamp, float max_element, int stochastic, uint64_t seed,
                               const uint64_t* seed_cell, void* stream) {
    float me;
    if (!multi_args_ok(table, ntensors, total_tiles, bucket, 2, {{levels, 3}}, clamp, max_element, seed_cell, me, out_kind))
        return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    dispatch(bucket, stochastic, out_kind, [&](auto row, auto stoch, auto out) {
        hipLaunchKernelGGL((k_multi_uniform_o16<decltype(row)::value, decltype(stoch)::value, decltype(out)::value>),
                           dim3(blocks_for(total_tiles, 4)), dim3(256), 0, (hipStream_t)stream, table, levels, ntensors,
                           total_tiles, bucket, me, seed, seed_cell);
    });
    return check_launch();
}

int qd_multi_uniform_global_out16_f32(const QdTensorDesc* table, const int32_t* levels, int ntensors, int64_t total_tiles,
                                      int out_kind, int clamp, float max_element, int stochastic, uint64_t seed,
                                      const uint64_t* seed_cell, float* alpha_beta, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    float me;
    if (!multi_args_ok(table, ntensors, total_tiles, 1, 2, {{levels, 3}, {alpha_beta, 0}}, clamp, max_element, seed_cell, me,
                       out_kind))
        return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    if (!workspace_ok(workspace, workspace_bytes, total_tiles)) return QD_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = blocks_for(total_tiles, 4);
    launch_mg_minmax_fold(table, ntensors, total_tiles, (float*)workspace, me, alpha_beta, blocks, st);
    dispatch(0, stochastic, out_kind, [&](auto, auto stoch, auto out) {
        hipLaunchKernelGGL((k_mg_apply_o16<decltype(stoch)::value, decltype(out)::value>), dim3(blocks), dim3(256), 0, st, table,
                           levels, ntensors, total_tiles, alpha_beta, me, seed, seed_cell);
    });
    return (int)hipGetLastError();
}

}  // extern "C"
