// qd_single_kernels.h -- the single-bucket (bucket_size=None) path of a large tensor: three launches (k_minmax_partial,
// k_minmax_final, k_single_apply), or ONE (k_single_fused: the tensor in registers across a grid-wide barrier) with the host
// side of that barrier (fused_capacity, launch_fused).  For the three mode units (through qd_transform.h): the two non-templated
// kernels are emitted once per includer, and so are the barrier slots g_fused_ctl wherever k_single_fused is instantiated.
#pragma once

#include "qd_element.h"        // KParams, the transforms and side stores, make_prep

#include <atomic>

using namespace qd;

namespace {

// ---- single-bucket (bucket_size=None) path for large tensors: reduce, finalize, apply --------
// stage 1: per-block partial min/max of prep(x)
__global__ __launch_bounds__(256) void k_minmax_partial(const float* x, int64_t n, const float* mean, float me,
                                                        float* part /* [2*kPartialBlocks] */) {
    __shared__ float red[32];
    const Prep pp = make_prep(mean, me);
    float mn = INFINITY, mx = -INFINITY;
    int nan = 0;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nth = (int64_t)gridDim.x * blockDim.x;
    if ((((uintptr_t)x) & kDataAlign) == 0) {
        const int64_t n4 = n >> 2;
        const f4* x4 = (const f4*)x;
        for (int64_t i = tid; i < n4; i += nth) {
            const f4 v = prep4(x4[i], pp);          // plain load: keep the lines in L2/MALL for stage 3
            mn = fminf(mn, fminf(fminf(v.x, v.y), fminf(v.z, v.w)));
            mx = fmaxf(mx, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
            nan |= has_nan4(v);
        }
        for (int64_t i = (n4 << 2) + tid; i < n; i += nth) {
            const float v = prep(x[i], pp);
            mn = fminf(mn, v); mx = fmaxf(mx, v);
            nan |= (v != v);
        }
    } else {
        for (int64_t i = tid; i < n; i += nth) {
            const float v = prep(x[i], pp);
            mn = fminf(mn, v); mx = fmaxf(mx, v);
            nan |= (v != v);
        }
    }
    block_minmax(mn, mx, red);
    if (__syncthreads_or(nan)) { mn = NAN; mx = NAN; }      // NaN poisons the partial (and, in stage 2, the tensor)
    if (threadIdx.x == 0) { part[blockIdx.x] = mn; part[kPartialBlocks + blockIdx.x] = mx; }
}

// stage 2: one block folds the partials into alpha/beta (device scalars; no host sync, unlike
// the reference's `alpha[0] < tol` at quant_functions.py:96)
__global__ __launch_bounds__(256) void k_minmax_final(const float* part, int nparts, float* ab /* [2] */,
                                                      float* alpha_out, float* beta_out) {
    __shared__ float red[32];
    float mn = INFINITY, mx = -INFINITY;
    int nan = 0;
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
        const float pm = part[i];
        nan |= (pm != pm);
        mn = fminf(mn, pm);
        mx = fmaxf(mx, part[kPartialBlocks + i]);
    }
    block_minmax(mn, mx, red);
    if (__syncthreads_or(nan)) { mn = NAN; mx = NAN; }
    if (threadIdx.x == 0) {
        float a, b;
        alpha_beta(mn, mx, a, b);
        ab[0] = a; ab[1] = b;
        if (alpha_out) alpha_out[0] = a;
        if (beta_out) beta_out[0] = b;
    }
}

// stage 3: elementwise apply with the single (alpha, beta)
// ab != null: the pair was finalised by k_minmax_final (huge tensors: many apply blocks).
// ab == null: every block folds the `nparts` stage-1 partials itself (a few KB from L2) -- one
// launch fewer for the model-sized tensors, where the call is launch-bound, not bandwidth-bound.
template <int MODE>
__global__ __launch_bounds__(256) void k_single_apply(KParams p, const float* ab, const float* part, int nparts) {
    PointStore Ts;
    PointTable Tc;
    __shared__ float red[32];
    const PointTable* T = &Tc;                             // (read only in the nearest-point mode)
    if (MODE == MODE_NEAREST) load_points(Tc, Ts, p.pts, p.k, p.fine);
    const Prep pp = make_prep(p.mean, p.me);
    float a, b;
    if (ab) {
        a = ab[0]; b = ab[1];
    } else {
        float mn = INFINITY, mx = -INFINITY;
        int nan = 0;
        for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
            const float pm = part[i];
            nan |= (pm != pm);
            mn = fminf(mn, pm);
            mx = fmaxf(mx, part[kPartialBlocks + i]);
        }
        block_minmax(mn, mx, red);
        if (__syncthreads_or(nan)) { mn = NAN; mx = NAN; }
        alpha_beta(mn, mx, a, b);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            if (p.alpha) p.alpha[0] = a;
            if (p.beta) p.beta[0] = b;
        }
    }
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nth = (int64_t)gridDim.x * blockDim.x;
    const bool prescaled = (MODE == MODE_NEAREST && p.prescaled);
    int64_t done = 0;
    if (((((uintptr_t)p.x) | ((uintptr_t)p.out)) & kDataAlign) == 0) {
        const int64_t n4 = p.n >> 2;
        const f4* x4 = (const f4*)p.x;
        f4* o4 = (f4*)p.out;
        for (int64_t i = tid; i < n4; i += nth) {
            f4 v = __builtin_nontemporal_load(x4 + i);
            if (!prescaled) v = prep4(v, pp);
            float rnd[4] = {0.f, 0.f, 0.f, 0.f};
            if (MODE == MODE_QDQ && p.stochastic) philox_uniform4(p.seed, (uint64_t)i, rnd);
            float side[4];
            const f4 r = transform_f4<MODE>(p, T, v, a, b, pp.mean, rnd, side);
            __builtin_nontemporal_store(r, o4 + i);
            store_side4<MODE>(p, i << 2, side);
        }
        done = n4 << 2;
    }
    for (int64_t i = done + tid; i < p.n; i += nth) {
        float v = p.x[i];
        if (!prescaled) v = prep(v, pp);
        float rnd = 0.0f;
        if (MODE == MODE_QDQ && p.stochastic) {
            float r4[4];
            philox_uniform4(p.seed, (uint64_t)i >> 2, r4);
            rnd = r4[i & 3];
        }
        float side = 0.0f;
        p.out[i] = transform<MODE>(p, T, v, a, b, pp.mean, rnd, side);
        store_side1<MODE>(p, i, side);
    }
}

// ---- single-bucket path in ONE launch for tensors that fit the register files ------------------
// k_single_fused: every lane loads its share of the tensor ONCE into registers (V float4 per lane), the blocks
// publish their min/max, meet at a grid-wide barrier, and transform their registers with the folded (alpha, beta):
// the tensor is read from HBM once and written once (8 B/element instead of 12) in one launch instead of three
// (ref: quant_functions.py:85-87,95-97 with bucket_size=None).
//
// The barrier has NO counter.  Device-scope round trips cost 1-2 us on this chip (the coherence point is behind
// the XCDs' private L2s) and same-address atomics serialise (~40 ns each): a counter that 780 blocks increment
// and poll measured +35 us, a 32-way fan-out of it +22 us.  Instead every block writes its (min, max) into its
// own slot, tagged with the launch's epoch (two 8-byte atomic stores, nothing to wait for), and then polls ALL G
// slots -- each lane checks G/256 of them, one round trip per sweep -- until every slot carries this epoch; the
// last sweep IS the fold.  No read-modify-write, no fence, no serialisation.
//
// The barrier is also OPTIMISTIC, and a block that gives up depends on NOBODY.  A grid barrier needs all blocks
// resident at the same time; the launch is sized for that (<= one block per CU), but another stream or process may
// hold part of the GPU, and two such kernels could starve each other forever.  So a block that still misses a slot
// after 2 ms of the 100 MHz wall clock stops waiting and folds the min/max of the WHOLE tensor itself, from memory
// (at most 1 Mi elements = 4 MiB, served by L2 / the Infinity Cache; x is never written: in-place calls take the
// three-launch path), then transforms its own registers like everybody else.  min / max do not depend on the fold order,
// so it arrives at the same (alpha, beta) bit for bit as the blocks that did meet.  There is no departure count, no
// "last block", no flag that one block sets and another must see: every block's output depends only on x and on slot
// values it has itself observed with this launch's tag (round 2's protocol -- a relaxed gave_up counter read by the last
// block out -- could miss a departure and leave a slice unwritten).
// A slot is two 8-byte words {min bits | tag_min << 32}, {max bits | tag_max << 32}; each word is written and read with
// one atomic access, so a value can never be seen with another launch's tag.  BOTH tags are unique to the launch among
// all launches that can have touched the slot: the host draws a 64-bit epoch that never repeats and sets
// tag_min = its low half, tag_max = low half ^ (high half * odd constant), both non-zero (a never-written slot is 0 | 0).
// A slot left over from another launch matches tag_min only if its epoch has the same low half, i.e. lies 2^32 launches
// back, and then its tag_max differs because the high half does.  (Tagging the two words with the two HALVES of the epoch
// does not work: the high half is the same for 2^32 launches in a row, so a sweep could pair this launch's min with the max
// a previous launch left in the slot.  A 31-bit epoch alone wrapped after 2^31 launches, and slots that only large grids
// touch could still carry the old tag.)  Should two launches ever share a slot set while both are running (more than
// kFusedSlots of these kernels in flight), they overwrite each other's tags, their sweeps fail, and both take the give-up
// path: slow, still correct.  The slots live in a __device__ array (zero-initialised when the module is loaded, per device
// and per process), not in the caller's workspace, whose contents are undefined by contract.
constexpr int kFusedSlots = 64;
constexpr int kFusedMaxBlocks = 256;                   // <= one block per CU: every block sweeps all G slots
constexpr long long kBarrierTimeout = 200000;          // 2 ms of the 100 MHz wall clock
struct FusedCtl {
    unsigned long long slot[kFusedMaxBlocks][2];
};
__device__ FusedCtl g_fused_ctl[kFusedSlots];

// test hooks of qd_set_single_fused_mode(): which blocks skip the barrier and take the give-up path at once
enum { FUSED_GIVE_UP_NONE = 0, FUSED_GIVE_UP_ALL = 1, FUSED_GIVE_UP_EVERY_7TH = 2, FUSED_GIVE_UP_ONE = 3 };

__device__ __forceinline__ unsigned long long ld_agent(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(unsigned long long* p, unsigned long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int MODE>
__device__ __forceinline__ f4 transform4(const KParams& p, const PointTable* T, f4 v, float a, float b, float mean,
                                         int64_t i4, float (&side)[4]) {
    float rnd[4] = {0.f, 0.f, 0.f, 0.f};
    if (MODE == MODE_QDQ && p.stochastic) philox_uniform4(p.seed, (uint64_t)i4, rnd);
    return transform_f4<MODE>(p, T, v, a, b, mean, rnd, side);
}

// One sweep over the G slots (all threads of the block): true when every slot carries this launch's epoch; then
// (mn, mx) is the fold of all partials (NaN in any of them poisons both, as torch's min/max do).
__device__ __forceinline__ bool sweep_slots(const FusedCtl* ctl, unsigned G, unsigned tag_min, unsigned tag_max, float* red,
                                            float& mn, float& mx) {
    float fmn = INFINITY, fmx = -INFINITY;
    int fnan = 0, missing = 0;
    for (unsigned i = threadIdx.x; i < G; i += blockDim.x) {
        const unsigned long long a = ld_agent(&ctl->slot[i][0]);
        const unsigned long long b = ld_agent(&ctl->slot[i][1]);
        missing |= ((unsigned)(a >> 32) != tag_min) | ((unsigned)(b >> 32) != tag_max);
        const float pm = __uint_as_float((unsigned)a), px = __uint_as_float((unsigned)b);
        fnan |= (pm != pm);
        fmn = fminf(fmn, pm);
        fmx = fmaxf(fmx, px);
    }
    if (__syncthreads_or(missing)) return false;
    block_minmax(fmn, fmx, red);
    if (__syncthreads_or(fnan)) { fmn = NAN; fmx = NAN; }
    mn = fmn; mx = fmx;
    return true;
}

// V float4 per lane at W waves per SIMD (W = 4: 128 VGPRs).  The launcher uses it up to 1 Mi elements (V <= 4).
template <int MODE, int V, int W>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(W, W)))
void k_single_fused(KParams p, int slot_set, unsigned tag_min, unsigned tag_max, int give_up_mode) {
    PointStore Ts;
    PointTable Tc;
    __shared__ float red[32];
    __shared__ int s_timed_out;
    const PointTable* T = &Tc;                             // (read only in the nearest-point mode)
    if (MODE == MODE_NEAREST) load_points(Tc, Ts, p.pts, p.k, p.fine);
    const Prep pp = make_prep(p.mean, p.me);
    const unsigned G = gridDim.x;
    FusedCtl* ctl = &g_fused_ctl[slot_set];
    const int64_t n4 = p.n >> 2;
    const f4* x4 = (const f4*)p.x;
    f4* o4 = (f4*)p.out;
    const bool forced = give_up_mode == FUSED_GIVE_UP_ALL ||
                        (give_up_mode == FUSED_GIVE_UP_EVERY_7TH && blockIdx.x % 7 == 3) ||
                        (give_up_mode == FUSED_GIVE_UP_ONE && blockIdx.x == G / 2);

    // ---- load once, reduce ----
    f4 v[V];
    float mn = INFINITY, mx = -INFINITY;
    int nan = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int64_t i = ((int64_t)j * G + blockIdx.x) * 256 + threadIdx.x;
        if (i < n4) {
            v[j] = prep4(ldg_nt(x4 + i), pp);
            mn = fminf(mn, fminf(fminf(v[j].x, v[j].y), fminf(v[j].z, v[j].w)));
            mx = fmaxf(mx, fmaxf(fmaxf(v[j].x, v[j].y), fmaxf(v[j].z, v[j].w)));
            nan |= has_nan4(v[j]);
        }
    }
    float tail[3] = {0.f, 0.f, 0.f};
    const int ntail = (int)(p.n & 3);
    const bool owns_tail = blockIdx.x == 0 && threadIdx.x == 0;
    if (owns_tail)
        for (int t = 0; t < ntail; ++t) {
            tail[t] = prep(p.x[(n4 << 2) + t], pp);
            mn = fminf(mn, tail[t]); mx = fmaxf(mx, tail[t]);
            nan |= (tail[t] != tail[t]);
        }
    block_minmax(mn, mx, red);
    if (__syncthreads_or(nan)) { mn = NAN; mx = NAN; }      // NaN poisons the partial, hence the tensor

    // ---- publish (also by a block that is about to give up: the others must not wait for it) ----
    if (threadIdx.x == 0) {
        st_agent(&ctl->slot[blockIdx.x][0], (unsigned long long)__float_as_uint(mn) | ((unsigned long long)tag_min << 32));
        st_agent(&ctl->slot[blockIdx.x][1], (unsigned long long)__float_as_uint(mx) | ((unsigned long long)tag_max << 32));
        s_timed_out = forced ? 1 : 0;
    }
    __syncthreads();

    // ---- meet: sweep the slots until all carry this epoch (the successful sweep is the fold) ----
    bool met = false;
    if (!forced) {
        const long long t0 = wall_clock64();
        for (;;) {
            if (sweep_slots(ctl, G, tag_min, tag_max, red, mn, mx)) { met = true; break; }
            if (threadIdx.x == 0 && wall_clock64() - t0 > kBarrierTimeout) s_timed_out = 1;
            __syncthreads();
            if (s_timed_out) break;
            __builtin_amdgcn_s_sleep(4);
        }
    }
    if (!met) {
        // ---- gave up: this block folds the whole tensor alone (same min / max, whatever the order) ----
        float gmn = INFINITY, gmx = -INFINITY;
        int gnan = 0;
        for (int64_t i = threadIdx.x; i < n4; i += 256) {
            const f4 t = prep4(x4[i], pp);
            gmn = fminf(gmn, fminf(fminf(t.x, t.y), fminf(t.z, t.w)));
            gmx = fmaxf(gmx, fmaxf(fmaxf(t.x, t.y), fmaxf(t.z, t.w)));
            gnan |= has_nan4(t);
        }
        if (threadIdx.x == 0)
            for (int t = 0; t < ntail; ++t) {
                const float e = prep(p.x[(n4 << 2) + t], pp);
                gmn = fminf(gmn, e); gmx = fmaxf(gmx, e);
                gnan |= (e != e);
            }
        block_minmax(gmn, gmx, red);
        if (__syncthreads_or(gnan)) { gmn = NAN; gmx = NAN; }
        mn = gmn; mx = gmx;
    }

    float a, b;
    alpha_beta(mn, mx, a, b);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (p.alpha) p.alpha[0] = a;
        if (p.beta) p.beta[0] = b;
    }
    // ---- transform the registers ----
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int64_t i = ((int64_t)j * G + blockIdx.x) * 256 + threadIdx.x;
        if (i < n4) {
            float side[4];
            const f4 r = transform4<MODE>(p, T, v[j], a, b, pp.mean, i, side);
            stg_nt(r, o4 + i);
            store_side4<MODE>(p, i << 2, side);
        }
    }
    if (owns_tail)
        for (int t = 0; t < ntail; ++t) {
            const int64_t e = (n4 << 2) + t;
            float rnd = 0.0f;
            if (MODE == MODE_QDQ && p.stochastic) {
                float r4[4];
                philox_uniform4(p.seed, (uint64_t)e >> 2, r4);
                rnd = r4[e & 3];
            }
            float side = 0.0f;
            p.out[e] = transform<MODE>(p, T, tail[t], a, b, pp.mean, rnd, side);
            store_side1<MODE>(p, e, side);
        }
}

// ---- host side of the one-launch kernel ----
// one-launch single bucket (k_single_fused) when the tensor fits the register files of a resident grid
// qd_set_single_fused_mode(): 0 = always the three-launch path, 1 = default, 2 / 3 / 4 = every block / every block with
// blockIdx % 7 == 3 / exactly one block skips the barrier and takes the give-up path, so that the tests reach the
// contention fallback deterministically on an idle GPU.  A plain int: set it before launching, not concurrently.
// (the switch itself lives in qd_kernels.hip -- one variable for the three translation units that include this header)
template <int MODE, int V, int W>
int fused_capacity() {                                         // blocks of k_single_fused<MODE, V> resident at once, 0 if unusable
    static int caps[64];                                       // per device, stored + 1 (0 = not asked yet)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 0; }
    const bool cached = dev >= 0 && dev < 64;                  // a device index beyond the table is asked every time, never aliased
    int& slot = caps[cached ? dev : 0];
    int cap = cached ? __atomic_load_n(&slot, __ATOMIC_RELAXED) - 1 : -1;
    if (cap < 0) {
        int per_cu = 0;
        hipFuncAttributes fa;
        const void* fn = (const void*)k_single_fused<MODE, V, W>;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, MODE == MODE_NEAREST ? point_table_bytes(kMaxPoints, 1) : 0) != hipSuccess ||
            hipFuncGetAttributes(&fa, fn) != hipSuccess || fa.localSizeBytes != 0 /* spills: not worth it */)
            per_cu = 0;
        (void)hipGetLastError();
        int c = per_cu * device_cus();
        cap = c > kFusedMaxBlocks ? kFusedMaxBlocks : c;
        if (cached) __atomic_store_n(&slot, cap + 1, __ATOMIC_RELAXED);
    }
    return cap;
}
// one epoch sequence for ALL instantiations, 64 bits: a tag never repeats on a slot set (epoch 0 = a never-written slot)
std::atomic<uint64_t> next_launch{1};
template <int MODE, int V, int W>
void launch_fused(const KParams& p, int64_t blocks, size_t lds, int fmode, hipStream_t st) {
    uint64_t epoch;
    unsigned tag_min, tag_max;
    do {                                                       // both tags non-zero: 0 | 0 is a never-written slot
        epoch = next_launch.fetch_add(1, std::memory_order_relaxed);
        tag_min = (unsigned)epoch;
        tag_max = tag_min ^ ((unsigned)(epoch >> 32) * 0x9E3779B9u);
    } while (tag_min == 0u || tag_max == 0u);
    const int slot = (int)(epoch % kFusedSlots);
    hipLaunchKernelGGL((k_single_fused<MODE, V, W>), dim3((unsigned)blocks), dim3(256), lds, st, p, slot, tag_min, tag_max,
                       fmode >= 2 ? fmode - 1 : 0);
}

}  // namespace
