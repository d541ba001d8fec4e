// qd_points.h -- the LDS-resident table of quantization points of the nearest-point kernels and the searches in it: the
// coarse and the fine cell tables (load_points), #{ midpoints <= u } (midpoint_index, midpoint_index_fine) and the nearest
// point under either rule (assign_point, assign_point4).  Device code only.
#pragma once

#include "qd_common.h"         // count_before, count_before4; through it qd_plan.h: kCells, kFineCells, kSmallTable, kMaxPoints
#include "../../include/qd_hip.h"      // QD_ASSIGN_MIDPOINT

using namespace qd;

namespace {

// LDS-resident point table (+ midpoints, quant_functions.py:533; kCells, kFineCells, point_table_bytes: qd_plan.h)
// The table lives at the START of the kernel's dynamic LDS (every nearest-point launch asks for point_table_bytes(k) more),
// sized by the number of points: 256 bytes up to 32 points -- every configuration of the reference's scripts -- instead of
// a static 10.3 KB for the 1024 points the ABI allows.  (The static table left the chunk kernels 6 / 5 blocks per CU, bound
// by LDS; the point search is a chain of dependent LDS reads, so resident waves are what hides it.)
// (pointers in the LDS address space: 32-bit addresses and ds_read straight away, instead of 64-bit generic pointers that
// the compiler first has to prove to be LDS -- the k = 256 search is VALU- and bank-conflict-bound, every instruction counts)
typedef __attribute__((address_space(3))) float lds_f32;
typedef __attribute__((address_space(3))) int lds_i32;
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));      // (a native vector: HIP's uint2 class has no LDS-qualified operators)
typedef __attribute__((address_space(3))) u32x2 lds_u2;
struct PointStore {
    lds_f32* pts;                       // [cap]
    lds_f32* mid;                       // [cap]
    lds_i32* start;                     // [kCells + 4], k > 32 only: start[c] = #{ j : cell(mid_j) < c }, c = 0..kCells
    lds_i32* startp;                    // same for the points themselves (distance rule)
    lds_u2* cell;                       // [kFineCells], `fine` only: {start | count << 16, first midpoint of the cell}
};
extern __shared__ __attribute__((aligned(16))) unsigned char qd_dyn_lds[];     // every kernel's dynamic LDS starts here
// Many points, midpoint rule (the per-step call): a FINE grid of 2048 cells over [0, 1] whose entry answers an element by
// itself when its cell holds at most one midpoint -- index = start + (first midpoint <= u) -- with ONE 8-byte LDS read, no
// loop; only cells with two or more midpoints fall back to the binary search inside the cell.  With k = 256 points spread
// like uniform samples 0.7 % of the elements need the fallback (a wave executes it for an element slot in which any of its
// 64 lanes does: about once per three float4 instead of for every element).  Why: at k = 256 the kernel is bound by VALU
// issue and LDS bank conflicts, not by latency -- 61 M VALU wave-instructions per 64 Mi-element launch (25 M at k = 4), half
// of its 35.7 M LDS-active cycles lost to conflicts of five to six random table reads per element
// (docs/history/profiles/r03_sq_counters.txt).  Points crowded into few cells (percentile-initialised, bell-shaped weights) keep taking the
// fallback: never slower than the narrowed search it replaces, only no faster.  16 KB more LDS, so only the kernels without
// LDS staging of their own use it (`fine` is cleared for the chunk kernels), on a capped grid (kFineBlocksPerCu) so that
// the table is built a few thousand times, not once per 16 KB of data.
// (kFineCells = 2048; the cap kFineBlocksPerCu and its measurements: qd_plan.h)

// What the kernels pass around: a handle on the LDS table.  (Tried in round 3 and dropped: for small point sets the points
// and midpoints themselves in registers, the assignment as k - 1 compares and selects without any LDS access.  With k <= 8
// and the values forced into scalar registers, 23 more live SGPRs put the kernels 88-179 SGPR spills over the limit and the
// pre-processed forward got slower at every bucket size -- k = 4, bucket 256 / 100 / 1000: 107 / 192 / 130 us against
// 93 / 114 / 97 us with the joint LDS search of count_before4.  With k <= 4 in vector registers (+26 VGPRs in the chunk
// kernel) it tied or lost on the per-step call (bucket 100: 119 us against 105 us) and gained 5-10 % on the one-off
// nonUniformQuantization call only.  docs/history/profiles/r03_side_outputs.txt.)
struct PointTable {
    const PointStore* s;
    bool fine;
};

// cell of a scaled value: monotone non-decreasing in u (x256 is exact in fp32, then truncation and a
// clamp), which is all the narrowing below relies on; NaN lands in cell 0
__device__ __forceinline__ int cell_of(float u) {
    const float t = u * (float)kCells;
    int c = t > 0.0f ? (int)t : 0;
    return c < kCells - 1 ? c : kCells - 1;
}

__device__ __forceinline__ int fine_cell_of(float u) {           // as cell_of: exact scaling by a power of two, monotone, NaN -> 0
    const float t = u * (float)kFineCells;
    int c = t > 0.0f ? (int)t : 0;
    return c < kFineCells - 1 ? c : kFineCells - 1;
}

__device__ __forceinline__ void load_points(PointTable& C, PointStore& T, const float* pts, int k, int fine = 0) {
    const int cap = k <= kSmallTable ? kSmallTable : kMaxPoints;
    // midpoints FIRST and the cell tables at a constant distance: the searches of the per-step call (midpoint rule) then
    // address LDS with compile-time offsets again, whatever the table size; only the points sit at a k-dependent offset
    // (with both arrays behind a run-time offset the k = 256 search, which is VALU-bound, issued 5 % more instructions)
    T.mid = (lds_f32*)qd_dyn_lds;
    T.pts = T.mid + cap;
    T.start = (lds_i32*)(T.mid + 2 * kMaxPoints);            // (k > 32 only, where cap == kMaxPoints)
    T.startp = T.start + (kCells + 4);
    T.cell = (lds_u2*)(qd_dyn_lds + kCoarseTableBytes);      // (`fine` only)
    for (int j = threadIdx.x; j < k; j += blockDim.x) T.pts[j] = pts[j];
    __syncthreads();
    for (int j = threadIdx.x; j + 1 < k; j += blockDim.x) {
        float d = T.pts[j + 1] - T.pts[j];   // np.diff(k)
        d = d / 2.0f;                        //  / 2
        T.mid[j] = T.pts[j] + d;             // k[:-1] + ...
    }
    __syncthreads();
    if (k > 32 && !fine) {                                   // (the fine table below replaces both coarse ones: `fine` is midpoint-rule only)
        // start[c] by binary search on the monotone predicate cell(mid_j) < c
        for (int c = threadIdx.x; c <= kCells; c += blockDim.x) {
            int lo = 0, n = k - 1;
            while (n > 0) {
                const int half = n >> 1;
                if (cell_of(T.mid[lo + half]) < c) { lo += half + 1; n -= half + 1; } else n = half;
            }
            T.start[c] = lo;
            lo = 0; n = k;
            while (n > 0) {
                const int half = n >> 1;
                if (cell_of(T.pts[lo + half]) < c) { lo += half + 1; n -= half + 1; } else n = half;
            }
            T.startp[c] = lo;
        }
        __syncthreads();
    }
    if (k > 32 && fine) {
        // count the midpoints per fine cell (integer LDS atomics), exclusive scan over the cells, then the entries
        lds_i32* cnt = (lds_i32*)T.cell;                     // the first kFineCells dwords of the entry array, for now
        lds_i32* wsum = cnt + kFineCells;                    // wave totals of the scan (<= 16)
        for (int c = threadIdx.x; c < kFineCells; c += blockDim.x) cnt[c] = 0;
        __syncthreads();
        for (int j = threadIdx.x; j + 1 < k; j += blockDim.x)
            __hip_atomic_fetch_add(&cnt[fine_cell_of(T.mid[j])], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
        // thread t owns cells [t * per, (t + 1) * per); blockDim is 128, 256 or 1024: per = 16, 8, 2
        const int per = kFineCells / (int)blockDim.x;
        int mine[16];
        int local = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) { mine[q] = q < per ? cnt[threadIdx.x * per + q] : 0; local += mine[q]; }
        int incl = local;                                    // inclusive scan over the lanes of the wave
#pragma unroll
        for (int sft = 1; sft < 64; sft <<= 1) {
            const int o = __shfl_up(incl, sft);
            incl += (int)(threadIdx.x & 63) >= sft ? o : 0;
        }
        if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
        __syncthreads();                                     // every thread has read its counters: the array may be overwritten
        int base = incl - local;
        for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) base += wsum[w];
        __syncthreads();                                     // (wsum sits inside the entry array)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            if (q < per) {
                const int n_here = mine[q];
                u32x2 e;
                e.x = (uint32_t)base | ((uint32_t)n_here << 16);
                e.y = n_here > 0 ? __float_as_uint(T.mid[base]) : 0x7FC00000u;      // NaN: no midpoint, the compare is false
                T.cell[threadIdx.x * per + q] = e;
                base += n_here;
            }
        }
        __syncthreads();
    }
    C.s = &T;
    C.fine = k > 32 && fine;
}

// #{ midpoints <= u }.  For many points the search is narrowed to the midpoints that fall in u's
// grid cell: every midpoint in an earlier cell is < u and every one in a later cell is > u (cell_of
// is monotone), so the count is exact whatever the point distribution; with roughly uniform points
// the remaining range holds 0-2 midpoints instead of k-1 (LDS reads per element: ~4 instead of ~9
// at k = 256, and fewer bank conflicts).
// A NaN u fails every comparison, which would count no midpoint (index 0); numpy's searchsorted, which the reference and
// libqd_host.so follow, orders a NaN after every point: index k - 1.  One select per element says so on every path below.
__device__ __forceinline__ int nan_last(float u, int k, int i) { return u != u ? k - 1 : i; }
__device__ __forceinline__ int midpoint_index_fine(const PointStore& T, int k, float u) {
    const u32x2 e = T.cell[fine_cell_of(u)];
    const int s0 = (int)(e.x & 0xFFFFu), n_here = (int)(e.x >> 16);
    int i = s0 + ((__uint_as_float(e.y) <= u) ? 1 : 0);                   // right for a cell with 0 or 1 midpoints
    if (n_here > 1) i = s0 + count_before<true>(T.mid + s0, n_here, u);   // crowded cell: search inside it
    return nan_last(u, k, i);
}
__device__ __forceinline__ int midpoint_index(const PointStore& T, int k, float u) {
    if (k <= 32) return nan_last(u, k, count_before<true>(T.mid, k - 1, u));
    const int c = cell_of(u);
    const int s0 = T.start[c];
    return nan_last(u, k, s0 + count_before<true>(T.mid + s0, T.start[c + 1] - s0, u));
}

// nearest point of u (quant_functions.py:267-273 or :531-573)
__device__ __forceinline__ int assign_point(const PointStore& T, int k, int mode, float u) {
    if (mode == QD_ASSIGN_MIDPOINT) return midpoint_index(T, k, u);
    int i;                                           // searchsorted(side='left'): #{ points < u }
    if (k <= 32) {
        i = count_before<false>(T.pts, k, u);
    } else {                                         // narrowed to u's grid cell, exact for the same reason
        const int c = cell_of(u);
        const int s0 = T.startp[c];
        i = s0 + count_before<false>(T.pts + s0, T.startp[c + 1] - s0, u);
    }
    i = i > k - 1 ? k - 1 : i;                       // .clip(max=k-1)
    if (i > 0) {
        const float dl = fabsf(u - T.pts[i - 1]);
        const float dh = fabsf(u - T.pts[i]);
        i -= (dl < dh) ? 1 : 0;                      // strictly closer to the lower point
    }
    return nan_last(u, k, i);
}

// nearest points of the four elements of a float4, up to 32 points (every configuration of the reference's scripts:
// 2^bits points, bits <= 4 in the differentiable-quantization runs): the four searches advance together (count_before4).
// Above 32 points transform_x4 keeps the element-by-element form of assign_point: there the kernel is bound by VALU issue
// and LDS bank conflicts, not by latency (at k = 256: 64 M VALU wave-instructions per 64 Mi-element launch ~ 105 us of
// issue time, half of the 35.7 M LDS-active cycles lost to conflicts of random reads in 256-entry tables), and both a
// joint narrowed search with always-issued reads (134 us against 115 us) and merely routing the four per-element searches
// through this function (125 us) measured slower.  docs/history/profiles/r03_sq_counters.txt.
__device__ __forceinline__ void assign_point4(const PointStore& T, int k, int mode, const float (&u)[4], int (&i)[4]) {
    if (mode == QD_ASSIGN_MIDPOINT) {
        count_before4<true>(T.mid, k - 1, u, i);
#pragma unroll
        for (int c = 0; c < 4; ++c) i[c] = nan_last(u[c], k, i[c]);
        return;
    }
    count_before4<false>(T.pts, k, u, i);                // searchsorted(side='left'): #{ points < u }
#pragma unroll
    for (int c = 0; c < 4; ++c) i[c] = i[c] > k - 1 ? k - 1 : i[c];                 // .clip(max=k-1)
    float pl[4], ph[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) { pl[c] = T.pts[i[c] > 0 ? i[c] - 1 : 0]; ph[c] = T.pts[i[c]]; }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float dl = fabsf(u[c] - pl[c]);
        const float dh = fabsf(u[c] - ph[c]);
        i[c] -= (i[c] > 0 && dl < dh) ? 1 : 0;           // strictly closer to the lower point
        i[c] = nan_last(u[c], k, i[c]);
    }
}

}  // namespace
