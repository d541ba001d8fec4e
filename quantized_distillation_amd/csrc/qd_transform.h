// qd_transform.h -- the launcher of the MODE-templated half of the gfx950 fake-quantization kernels, run_transform<MODE>(): it
// derives the inputs of plan_transform() (qd_plan.h: which kernel, which grid, which LDS -- one pure function), and launches
// what the plan says.  The kernels it instantiates live in the headers it includes, one per family:
//     qd_points.h               the LDS point table and the point searches of the nearest-point mode
//     qd_element.h              KParams, the per-element transforms, the side-output stores, the row routines
//     qd_bucket_vec_kernels.h   k_bucket_vec, k_bucket_chunk, k_bucket_chunk_any   (a wave streams several buckets)
//     qd_bucket_row_kernels.h   k_bucket_wave_any, k_bucket_groups, k_bucket_generic   (a lane group, wave or block per bucket)
//     qd_single_kernels.h       one bucket: three launches, or one with its grid-wide barrier
//     qd_launch.h               host only: workspace carving, grid cap, launch check (all qd_reductions.hip and qd_ste.hip take)
//
// Included by THREE translation units, one per mode, so that hipcc builds them in parallel (as one file the kernels took
// 55 s to compile):
//     qd_kernels.hip   MODE_QDQ      qd_uniform_f32, the multi-tensor launch, and every non-templated kernel (K3, K6, K7, K8, ...)
//     qd_scale.hip     MODE_SCALE    qd_scale_down_f32
//     qd_nearest.hip   MODE_NEAREST  qd_nearest_point_f32
// Everything here sits in an anonymous namespace: each unit gets its own copy of the few non-templated helpers (min/max
// partials, launch helpers) and its own barrier slots and epoch counter for the one-launch kernel -- no device symbol
// crosses a translation unit (no -fgpu-rdc).  The only shared state is the host-side switch qd_fused_mode_state.
//
// Reference being replaced (paths relative to the reference root):
//   quantization/quant_functions.py:56-152   ScalingFunction.scale_down / inv_scale_down
//   quantization/quant_functions.py:155-194  uniformQuantization
//   quantization/quant_functions.py:196-290  nonUniformQuantization (+ SearchSorted :509-573)
//   quantization/help_functions.py:67-94     create_bucket_tensor (semantics folded in)
//
// No CUDA compatibility layer, no dual code paths: gfx950 only.
#pragma once

#include "qd_bucket_vec_kernels.h"
#include "qd_bucket_row_kernels.h"
#include "qd_single_kernels.h"
#include "qd_launch.h"
#include "qd_plan.h"       // the launch plan, and the constants the kernels share with it
#include "../../include/qd_hip.h"

using namespace qd;

// qd_set_single_fused_mode(): 0 = always the three-launch path, 1 = default, 2 / 3 / 4 = test hooks (see qd_hip.h).  Defined in
// qd_kernels.hip; hidden: not part of the ABI.
extern "C" __attribute__((visibility("hidden"))) int qd_fused_mode_state;

namespace {

// ---- the single-tensor transform: derive the plan's inputs, plan (qd_plan.h), launch what the plan says ------------------
// The plan is a function of numbers: what needs a pointer or the runtime is turned into one here -- the alignment facts, the
// compute-unit count (asked only in the nearest-point mode: nothing else caps a grid by it), and "the one-launch single-bucket
// kernel may be tried" (not switched off by qd_set_single_fused_mode(0), not in place: a block that gives up re-reads x).
// The plan's nb / row / nvec / fine enter the kernels' parameters here and nowhere else.
template <int MODE>
TransformPlan plan_call(KParams& p, int64_t bucket) {
    PlanInput in = {};
    in.mode = MODE;
    in.n = p.n;
    in.bucket = bucket;
    in.data_misalign = (int)((((uintptr_t)p.x) | ((uintptr_t)p.out)) & 15);
    const void* side = MODE == MODE_QDQ ? (const void*)p.lev8 : MODE == MODE_NEAREST ? (const void*)p.idx : nullptr;
    in.side_bytes = !side ? 0 : MODE == MODE_QDQ ? 1 : p.idx_bytes;
    in.side_misalign = (int)(((uintptr_t)side) & 15);
    in.k = p.k;
    in.assign_mode = p.assign_mode;
    in.prescaled = MODE == MODE_NEAREST && p.prescaled;
    in.q_null = MODE == MODE_NEAREST && p.out == nullptr;
    in.fused_ok = qd_fused_mode_state != 0 && (const void*)p.x != (const void*)p.out;
    in.cus = MODE == MODE_NEAREST ? device_cus() : 0;
    in.grid_cap = grid_cap();
    const TransformPlan pl = plan_transform(in);
    p.nb = pl.nb;
    p.row = pl.row;
    p.nvec = pl.nvec;
    p.fine = pl.fine;
    return pl;
}

// (defined in qd_nearest.hip: planned and launched in the nearest-point mode only.  The launch bounds must stand on this first
// declaration: the definition's alone are ignored -- tools/device_code_diff.py showed the kernel compiled for 1024 threads)
template <bool TWO>
__global__ __launch_bounds__(256) void k_nearest_prescaled_stream(KParams p);

// One launch of a plan: the kernel its family and arguments name, instantiated from the same lists the plan selected from
// (qd_plan.h), with the grid, block and dynamic LDS the plan computed.
template <int MODE>
void launch_planned(const Launch& L, const TransformPlan& pl, const KParams& p, const Workspace& w, hipStream_t st) {
    const dim3 grid((unsigned)L.blocks), block((unsigned)L.threads);
    const float* ab = pl.ab_ready ? w.ab : nullptr;             // k_single_apply: (alpha, beta) in the scratch slot, or nparts partials to fold
    switch (L.family) {
        case FAM_VEC:
#define QD_LAUNCH_VEC(ROW, LPB, V, U) \
            if (L.a == LPB && L.b == V) hipLaunchKernelGGL((k_bucket_vec<MODE, LPB, V, U>), grid, block, L.lds, st, p);
            QD_VEC_SHAPES(QD_LAUNCH_VEC)
#undef QD_LAUNCH_VEC
            break;
        case FAM_WAVE_ANY:
#define QD_LAUNCH_WAVE(V, G) \
            if (L.a == V && L.b == G) hipLaunchKernelGGL((k_bucket_wave_any<MODE, V, G>), grid, block, L.lds, st, p, pl.nbk, pl.amask);
            if constexpr (MODE == MODE_QDQ) { QD_WAVE_SHAPES_QDQ(QD_LAUNCH_WAVE) }
            else if constexpr (MODE == MODE_SCALE) { QD_WAVE_SHAPES_SCALE(QD_LAUNCH_WAVE) }
            else { QD_WAVE_SHAPES_NEAREST(QD_LAUNCH_WAVE) }
#undef QD_LAUNCH_WAVE
            break;
        case FAM_CHUNK:
            hipLaunchKernelGGL((k_bucket_chunk<MODE, kChunkV>), grid, block, L.lds, st, p, pl.m, pl.nchunks);
            break;
        case FAM_CHUNK_ANY:                                     // lead = 1: the plan has no case without the lead-in
            hipLaunchKernelGGL((k_bucket_chunk_any<MODE, kChunkV>), grid, block, L.lds, st, p, pl.m, pl.nchunks, 1);
            break;
        case FAM_GROUPS:
            if (L.a == 16) hipLaunchKernelGGL((k_bucket_groups<MODE, 16>), grid, block, L.lds, st, p);
            else hipLaunchKernelGGL((k_bucket_groups<MODE, 64>), grid, block, L.lds, st, p);
            break;
        case FAM_GENERIC:
            hipLaunchKernelGGL((k_bucket_generic<MODE>), grid, block, L.lds, st, p);
            break;
        case FAM_MINMAX_PARTIAL:
            hipLaunchKernelGGL(k_minmax_partial, grid, block, 0, st, p.x, p.n, p.mean, p.me, w.minmax_part);
            break;
        case FAM_MINMAX_FINAL:
            hipLaunchKernelGGL(k_minmax_final, grid, block, 0, st, w.minmax_part, pl.nparts, w.ab, p.alpha, p.beta);
            break;
        case FAM_SINGLE_APPLY:
            hipLaunchKernelGGL((k_single_apply<MODE>), grid, block, L.lds, st, p, ab, w.minmax_part, pl.nparts);
            break;
        case FAM_PRESCALED_STREAM:
            if constexpr (MODE == MODE_NEAREST) {
                if (L.a) hipLaunchKernelGGL(k_nearest_prescaled_stream<true>, grid, block, L.lds, st, p);
                else hipLaunchKernelGGL(k_nearest_prescaled_stream<false>, grid, block, L.lds, st, p);
            }
            break;
        default: break;                                        // (FAM_FUSED needs the occupancy: apply_plan)
    }
}

template <int MODE>
int apply_plan(const TransformPlan& pl, const KParams& p, void* ws, size_t ws_bytes, hipStream_t st) {
    if (pl.nlaunch == 0) return QD_ERR_INVALID_ARGUMENT;        // indices only, and the pre-scaled stream cannot take the call
    Workspace w = {};
    if (pl.needs_workspace && !carve(ws, ws_bytes, w)) return QD_ERR_WORKSPACE_TOO_SMALL;
    if (pl.fused_blocks[0] > 0 && !stream_capturing(st)) {      // one launch, if that many blocks are resident at once
        const int fmode = qd_fused_mode_state;
        bool fused = false;
#define QD_TRY_FUSED(I, V, W)                                                                                         \
        if (!fused) {                                                                                                 \
            const int cap = fused_capacity<MODE, V, W>();                                                             \
            fused = cap > 0 && pl.fused_blocks[I] <= cap;                                                             \
            if (fused) launch_fused<MODE, V, W>(p, pl.fused_blocks[I], pl.fused_lds, fmode, st);                      \
        }
        QD_FUSED_SHAPES(QD_TRY_FUSED)
#undef QD_TRY_FUSED
        if (fused) return check_launch();
    }
    if (pl.copies_ab) {            // alpha/beta are inputs: copy the pair into the scratch slot the apply kernel reads
        (void)hipMemcpyAsync(w.ab, p.alpha, sizeof(float), hipMemcpyDeviceToDevice, st);
        (void)hipMemcpyAsync(w.ab + 1, p.beta, sizeof(float), hipMemcpyDeviceToDevice, st);
    }
    for (int i = 0; i < pl.nlaunch; ++i) launch_planned<MODE>(pl.launch[i], pl, p, w, st);
    return check_launch();
}

template <int MODE>
int run_transform(KParams& p, int64_t bucket, void* ws, size_t ws_bytes, hipStream_t st) {
    if (p.n == 0) return 0;
    const TransformPlan pl = plan_call<MODE>(p, bucket);
    return apply_plan<MODE>(pl, p, ws, ws_bytes, st);
}

}  // namespace
