// qd_launch.h -- what a launcher needs on the HOST and nothing else: the carve-up of the caller's workspace, the grid cap and
// the block count under it, the launch check, "is this stream capturing".  No kernel and no __device__ function: a translation
// unit that includes only this header (qd_reductions.hip, qd_ste.hip) parses and emits none of the bucket-transform kernels.
#pragma once

#include "qd_common.h"         // device_cus, hook_grid_cap; through it qd_plan.h: capped_blocks, kPartialBlocks, kMaxPoints

#include <stddef.h>
#include <stdlib.h>            // getenv, atoi (QD_TUNING builds only)

using namespace qd;

namespace {

struct Workspace {           // fixed carve-up of the caller's scratch buffer
    float* minmax_part;      // [2*kPartialBlocks]
    float* ab;               // [2]
    double* sum_part;        // [kPartialBlocks]
    float* arg_pv;           // [2*kPartialBlocks]
    int64_t* arg_pi;         // [2*kPartialBlocks]
    float* pg_part;          // [kPartialBlocks * kMaxPoints]
};
constexpr size_t kWsBytes = 64 * 1024 + (size_t)kPartialBlocks * kMaxPoints * sizeof(float);

bool carve(void* ws, size_t bytes, Workspace& w) {
    if (!ws || bytes < kWsBytes || (((uintptr_t)ws) & 15)) return false;
    char* p = (char*)ws;
    w.minmax_part = (float*)p;               p += 2 * kPartialBlocks * sizeof(float);     // 8 KiB
    w.ab = (float*)p;                        p += 64;
    w.sum_part = (double*)p;                 p += kPartialBlocks * sizeof(double);        // 8 KiB
    w.arg_pv = (float*)p;                    p += 2 * kPartialBlocks * sizeof(float);     // 8 KiB
    w.arg_pi = (int64_t*)p;                  p += 2 * kPartialBlocks * sizeof(int64_t);   // 16 KiB
    p = (char*)ws + 64 * 1024;
    w.pg_part = (float*)p;
    return true;
}

inline int grid_cap() {
    // Measured on MI355X (tools/tune_k1.py, docs/history/profiles/r01_tune.txt): one wave-tile per wave (no grid-stride
    // reuse) streams fastest -- 85.9 us vs 97 us at 2048 persistent blocks for the 64 Mi-element
    // headline tensor -- so the cap only bounds the grid dimension.
#ifdef QD_TUNING        // launch-geometry experiments only (build with -DQD_TUNING): QD_GRID_CAP=<blocks>
    const char* e = getenv("QD_GRID_CAP");
    const int v = e ? atoi(e) : 0;
    if (v > 0) return v;
#endif
    return hook_grid_cap();                                    // kDefaultGridCap unless qd_set_grid_cap() lowered it (qd_common.h)
}
inline int blocks_for(int64_t items, int per_block) { return capped_blocks(items, per_block, kNoOwnCap, grid_cap()); }

inline int check_launch() {
    const hipError_t e = hipGetLastError();
    return (int)e;
}

// a captured launch would bake its barrier slot and epoch into the graph, and two replays in flight would share them
inline bool stream_capturing(hipStream_t st) {
    hipStreamCaptureStatus cap_status = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap_status) == hipSuccess && cap_status == hipStreamCaptureStatusNone) return false;
    (void)hipGetLastError();
    return true;
}

}  // namespace
