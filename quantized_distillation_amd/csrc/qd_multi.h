// qd_multi.h -- what the multi-tensor launches share (qd_multi_uniform.hip, qd_multi_dq.hip, qd_ste.hip).
//
// Each of them runs over a device table of per-tensor descriptors (QdTensorDesc, QdDiffQuantDesc, QdSteDesc; include/qd_hip.h)
// that the host plan has cut into work items ("tiles"): a descriptor's prefix field holds the number of items of the tensors
// before it, and a wave finds the tensor of item t by a binary search over that field.  A new descriptor type needs a prefix
// field and nothing else from here.  The 16-bit forms of those launches (fp16 / bf16 outputs, fp16 / bf16 gradients) share the
// element types, the exact widening and the converting store further down.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qd_common.h"       // f4, stg_nt
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

// ---- a bucket size per tensor (qd_multi_buckets_plan, k_multi_uniform_bk): the ONE statement of the tile rule ----
// A tensor of n > 0 elements under its own bucket size has rows of row = min(n, bucket) elements, nb = ceil(n / row) of them.
//   row <= 256: a tile is four buckets, a DPP row of the wave each -- ceil(nb / 4) tiles;
//   row >  256: a tile is one bucket, the whole wave owns it      -- nb tiles.
// The host plan counts with it and the kernel maps tile -> bucket with it, from the same two numbers.
struct BucketTiles {
    int64_t row, nb;     // elements per bucket row, number of buckets
    int64_t tiles;       // wave iterations the tensor owns
    bool wave;           // row > 256: one bucket per tile
};
__host__ __device__ __forceinline__ BucketTiles bucket_tiles(int64_t n, int64_t bucket) {
    BucketTiles g;
    g.row = n < bucket ? n : bucket;
    g.nb = (n + g.row - 1) / g.row;
    g.wave = g.row > 256;
    g.tiles = g.wave ? g.nb : (g.nb + 3) / 4;
    return g;
}

// ---- 16-bit elements of the launches that write fp16 / bf16 outputs or read fp16 / bf16 gradients ----
// The kernels are instantiated on the out_kind / grad_kind of the C ABI (QD_OUT_F16 = QD_GRAD_F16 = 1, QD_OUT_BF16 =
// QD_GRAD_BF16 = 2): an int, so that the kernel names read the same in every demangler.
template <int OUT> struct Out16;
template <> struct Out16<QD_OUT_F16> { typedef _Float16 type; };
template <> struct Out16<QD_OUT_BF16> { typedef __bf16 type; };
template <int KIND> struct Grad16;
template <> struct Grad16<QD_GRAD_F16> { typedef _Float16 type; };
template <> struct Grad16<QD_GRAD_BF16> { typedef __bf16 type; };

// Widening is exact: bf16 is the upper half of the fp32 pattern (an integer shift), fp16 goes through v_cvt_f32_f16
// (subnormals kept, not flushed; the sign of zero and +-inf kept; a NaN stays a NaN).
__device__ __forceinline__ float widen(float g) { return g; }
__device__ __forceinline__ float widen(_Float16 g) { return (float)g; }
__device__ __forceinline__ float widen(__bf16 g) {
    return __uint_as_float((unsigned)__builtin_bit_cast(unsigned short, g) << 16);
}

// four consecutive 16-bit elements from p, widened.  g8: p is 8-byte aligned -- one 8-byte load; otherwise element by element,
// the same four elements.  (gfx950 under HSA runs with unaligned access allowed, and the compiler knows: it may fuse the four
// 2-byte loads again.)  Read once: non-temporal.
template <typename G>
__device__ __forceinline__ f4 load16x4_nt(const G* p, bool g8) {
    typedef unsigned short us4 __attribute__((ext_vector_type(4)));
    us4 h;
    if (g8) {
        h = ldg_nt((const us4*)p);
    } else {
        const unsigned short* e = (const unsigned short*)p;
        h.x = ldg_nt(e); h.y = ldg_nt(e + 1); h.z = ldg_nt(e + 2); h.w = ldg_nt(e + 3);
    }
    f4 r;
    r.x = widen(__builtin_bit_cast(G, (unsigned short)h.x)); r.y = widen(__builtin_bit_cast(G, (unsigned short)h.y));
    r.z = widen(__builtin_bit_cast(G, (unsigned short)h.z)); r.w = widen(__builtin_bit_cast(G, (unsigned short)h.w));
    return r;
}

// four fp32 results as four 16-bit values (the compiler's own conversion: IEEE round to nearest even, v_cvt_f16_f32 /
// v_cvt_pk_bf16_f32 on gfx950): one 8-byte non-temporal store (the output is written once)
template <typename O>
__device__ __forceinline__ void store4_nt(const f4& r, O* dst) {
    typedef O o4 __attribute__((ext_vector_type(4)));
    o4 h;
    h.x = (O)r.x; h.y = (O)r.y; h.z = (O)r.z; h.w = (O)r.w;
    stg_nt(h, (o4*)dst);
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
