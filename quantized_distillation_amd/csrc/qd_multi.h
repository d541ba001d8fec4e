// qd_multi.h -- what the multi-tensor launches share (qd_multi_uniform.hip, qd_multi_dq.hip, k_multi_ste in qd_reductions.hip).
//
// Each of them runs over a device table of per-tensor descriptors (QdTensorDesc, QdDiffQuantDesc, QdSteDesc; include/qd_hip.h)
// that the host plan has cut into work items ("tiles"): a descriptor's prefix field holds the number of items of the tensors
// before it, and a wave finds the tensor of item t by a binary search over that field.  A new descriptor type needs a prefix
// field and nothing else from here.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qd_hip.h"          // QdTensorDesc

namespace qd {

// The last tensor whose prefix field is <= item (a tensor without items is never the answer for an item that exists).
// Call it with a wave-uniform `item` that derives from uniform_wave_index(): the whole search then runs on scalar loads.
template <typename Desc, int64_t Desc::*First = &Desc::first_tile>
__device__ __forceinline__ int owner_of(const Desc* table, int ntensors, int64_t item) {
    int lo = 0, hi = ntensors - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].*First <= item) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Host plan: write the running sum of items_of(descriptor) into each descriptor's first_tile; returns the total.
template <typename Desc, typename Count>
inline int64_t fill_prefix(Desc* host_table, int ntensors, Count items_of) {
    int64_t total = 0;
    for (int i = 0; i < ntensors; ++i) {
        host_table[i].first_tile = total;
        total += items_of(host_table[i]);
    }
    return total;
}

// ---- the un-bucketed uniform launches (qd_multi_uniform.hip, qd_multi_uniform_out16.hip) ----
constexpr int kTile = 1024;     // elements per wave tile: 64 lanes x 4 float4

// Phases 1 and 2 with the clamp limit `me` (+inf: off): k_mg_minmax_opt into part[2 * total_tiles], k_mg_fold into
// alpha_beta[ntensors][2], on `st`.  Defined next to the kernels in qd_multi_uniform.hip, for the translation unit whose phase 3
// stores another type: the kernels exist once.  Not part of the C ABI.
__attribute__((visibility("hidden"))) void launch_mg_minmax_fold(const QdTensorDesc* table, int ntensors, int64_t total_tiles,
                                                                 float* part, float me, float* alpha_beta, int blocks,
                                                                 hipStream_t st);

}  // namespace qd
