// qd_multi_dq.hip -- multi-tensor kernels for the differentiable-quantization step (gfx950).
//
// The reference's optimize_quantization_points loop (cnn_models/conv_forward_model.py:524-545)
// calls, for EVERY parameter tensor EVERY step,
//     p_quantized.data = quantizationFunctions[i].forward(None, points[i].data)      (:532)
//     points[i].grad.data = quantizationFunctions[i].backward(p.grad.data)[1]        (:545)
// With 60 tensors that is 120+ kernel launches per step from Python; the two entry points here
// do each sweep in ONE launch over a device table of per-tensor descriptors.  Arithmetic is
// identical to qd_nearest_point_f32(prescaled, QD_ASSIGN_MIDPOINT) / qd_point_grad_f32.
//   qd_multi_nearest_f32, qd_multi_point_grad_f32             fp32 outputs / gradients
//   qd_multi_nearest_out16_f32, qd_multi_point_grad_in16_f32  fp16 / bf16 outputs / gradients (a 16-bit student over fp32 masters):
//                                                             the same bodies instantiated on the element type
#include "qd_common.h"
#include "qd_multi.h"
#include "../../include/qd_hip.h"

using namespace qd;

namespace {

constexpr int kMaxK = 256;                             // the index is a uint8

// this tensor's points and fp32 midpoints (quant_functions.py:533) into the wave's LDS slot;
// LDS operations of one wave complete in order, the barriers only stop compiler reordering
__device__ __forceinline__ void load_point_tables(float* pts, float* mid, const float* points, int k, int lane) {
    __builtin_amdgcn_wave_barrier();
#pragma unroll 1
    for (int j = lane; j < k; j += 64) pts[j] = points[j];             // one pass while k <= 64
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll 1
    for (int j = lane; j + 1 < k; j += 64) {
        float df = pts[j + 1] - pts[j];
        df = df / 2.0f;
        mid[j] = pts[j] + df;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// one element: the count over the midpoints (a NaN orders last, as in qd_nearest_point_f32), then p alpha, + beta, + 0.0f
// as three separately rounded operations
__device__ __forceinline__ int nearest1(const float* pts, const float* mid, int k, float u, float a, float b, float& q) {
    int id = count_before<true>(mid, k - 1, u);
    id = u != u ? k - 1 : id;
    float y = pts[id] * a;
    y = y + b;
    q = y + 0.0f;
    return id;
}

// a float4 of one bucket: the quantized values and the four indices packed for one 4-byte store
__device__ __forceinline__ uint32_t nearest4(const float* pts, const float* mid, int k, const f4& v, float a, float b, f4& r) {
    float q0, q1, q2, q3;
    const uint32_t i0 = (uint32_t)nearest1(pts, mid, k, v.x, a, b, q0);
    const uint32_t i1 = (uint32_t)nearest1(pts, mid, k, v.y, a, b, q1);
    const uint32_t i2 = (uint32_t)nearest1(pts, mid, k, v.z, a, b, q2);
    const uint32_t i3 = (uint32_t)nearest1(pts, mid, k, v.w, a, b, q3);
    r.x = q0; r.y = q1; r.z = q2; r.w = q3;
    return i0 | (i1 << 8) | (i2 << 16) | (i3 << 24);
}

// The store type Q of the forward sweep: float (qd_multi_nearest_f32; the code is then what it always was) or _Float16 / __bf16
// (qd_multi_nearest_out16_f32: d.q addresses n 16-bit elements).  Every fp32 operation is the same; the fp32 result is converted
// by the compiler's own conversion (IEEE round to nearest even) in the store.  The register path wants u 16-byte aligned, idx
// 4-byte aligned, and q aligned for one store of four results per lane: 16 bytes for fp32, 8 bytes for 16-bit.
template <typename Q> constexpr uintptr_t q_fast_mask() { return sizeof(Q) == 4 ? 15 : 7; }
template <typename Q> struct Vec4 { typedef Q type __attribute__((ext_vector_type(4))); };      // a lane's four consecutive elements
template <typename Q>
__device__ __forceinline__ void store_q4(const f4& r, typename Vec4<Q>::type* dst) {
    if constexpr (std::is_same<Q, float>::value) stg_nt(r, dst);
    else store4_nt(r, (Q*)dst);
}

// block_dim: blockDim.x, read by the kernel (a device function reads it the slow way, through the partial-work-group check)
__device__ __forceinline__ int64_t uniform_wave_index(unsigned block_dim) {
    return (int64_t)blockIdx.x * (block_dim >> 6) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

// forward: a tile = 4 buckets of one tensor = one wave iteration; a DPP row owns a bucket
template <int ROW, typename Q>
__device__ __forceinline__ void multi_nearest(const QdDiffQuantDesc* table, int ntensors, int64_t total_tiles,
                                              int64_t bucket, const float* points, int k, unsigned block_dim) {
    __shared__ float s_pts[4][kMaxK];
    __shared__ float s_mid[4][kMaxK];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int sub = lane >> 4, l = lane & 15;
    const int64_t wave = uniform_wave_index(block_dim);      // scalar: owner_of runs on s_load
    const int64_t nwaves = ((int64_t)gridDim.x * block_dim) >> 6;
    for (int64_t t = wave; t < total_tiles; t += nwaves) {
        const int ti = owner_of(table, ntensors, t);                   // wave-uniform
        const QdDiffQuantDesc d = table[ti];
        load_point_tables(s_pts[w], s_mid[w], points + (int64_t)ti * k, k, lane);
        const int64_t row = d.n < bucket ? d.n : bucket;
        const int64_t nb = (d.n + row - 1) / row;
        const int64_t bkt = (t - d.first_tile) * 4 + sub;
        if (bkt >= nb) continue;
        const int64_t lo = bkt * row;
        const int64_t hi = lo + row < d.n ? lo + row : d.n;
        const float a = ldg(d.alpha + bkt), b = ldg(d.beta + bkt);
        Q* const qo = (Q*)d.q;                                          // n elements of the store type (include/qd_hip.h)
        const bool fast = ROW > 0 && (hi - lo) == ROW && ((((uintptr_t)d.u) & 15) | (((uintptr_t)d.q) & q_fast_mask<Q>())) == 0 &&
                          ((((uintptr_t)d.idx) & 3) == 0);
        if (fast) {
            constexpr int V = ROW > 0 ? ROW / 64 : 1;
            const f4* src = (const f4*)(d.u + lo) + l;
            typename Vec4<Q>::type* dst = (typename Vec4<Q>::type*)(qo + lo) + l;
            f4 v[V];
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = ldg_nt(src + j * 16);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                f4 r;
                const uint32_t pk = nearest4(s_pts[w], s_mid[w], k, v[j], a, b, r);
                store_q4<Q>(r, dst + j * 16);
                stg(pk, (uint32_t*)(d.idx + lo + ((int64_t)(j * 16 + l) << 2)));
            }
        } else {
            for (int64_t i = lo + l; i < hi; i += 16) {
                float q;
                const int id = nearest1(s_pts[w], s_mid[w], k, d.u[i], a, b, q);
                qo[i] = (Q)q;
                d.idx[i] = (uint8_t)id;
            }
        }
    }
}

template <int ROW>
__global__ __launch_bounds__(256) void k_multi_nearest(const QdDiffQuantDesc* __restrict__ table, int ntensors, int64_t total_tiles,
                                                       int64_t bucket, const float* points, int k) {
    multi_nearest<ROW, float>(table, ntensors, total_tiles, bucket, points, k, blockDim.x);
}

// OUT: the out_kind of the C ABI
template <int ROW, int OUT>
__global__ __launch_bounds__(256) void k_multi_nearest_o16(const QdDiffQuantDesc* __restrict__ table, int ntensors,
                                                           int64_t total_tiles, int64_t bucket, const float* points, int k) {
    multi_nearest<ROW, typename Out16<OUT>::type>(table, ntensors, total_tiles, bucket, points, k, blockDim.x);
}

// forward without buckets (bucket == 0): a tile = kFlatTile consecutive elements of one tensor = one wave iteration, all under
// the tensor's one (alpha[0], beta[0]).  A full tile of aligned pointers: four float4 loads of u per lane up front, per float4
// one float4 store of q and one packed store of the four indices; a tensor's last partial tile, and tensors whose u / q are
// not 16-byte or whose idx is not 4-byte aligned, go element by element.
constexpr int kFlatTile = 1024;

template <typename Q>
__device__ __forceinline__ void multi_nearest_flat(const QdDiffQuantDesc* table, int ntensors, int64_t total_tiles,
                                                   const float* points, int k, unsigned block_dim) {
    __shared__ float s_pts[4][kMaxK];
    __shared__ float s_mid[4][kMaxK];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t wave = uniform_wave_index(block_dim);
    const int64_t nwaves = ((int64_t)gridDim.x * block_dim) >> 6;
    for (int64_t t = wave; t < total_tiles; t += nwaves) {
        const int ti = owner_of(table, ntensors, t);                   // wave-uniform
        const QdDiffQuantDesc d = table[ti];
        load_point_tables(s_pts[w], s_mid[w], points + (int64_t)ti * k, k, lane);
        const int64_t lo = (t - d.first_tile) * kFlatTile;
        const int64_t hi = lo + kFlatTile < d.n ? lo + kFlatTile : d.n;
        const float a = ldg(d.alpha), b = ldg(d.beta);
        Q* const qo = (Q*)d.q;
        const bool fast = (hi - lo) == kFlatTile && ((((uintptr_t)d.u) & 15) | (((uintptr_t)d.q) & q_fast_mask<Q>())) == 0 &&
                          ((((uintptr_t)d.idx) & 3) == 0);
        if (fast) {
            const f4* src = (const f4*)(d.u + lo) + lane;
            typename Vec4<Q>::type* dst = (typename Vec4<Q>::type*)(qo + lo) + lane;
            uint32_t* ix = (uint32_t*)(d.idx + lo) + lane;
            f4 v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = ldg_nt(src + j * 64);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f4 r;
                const uint32_t pk = nearest4(s_pts[w], s_mid[w], k, v[j], a, b, r);
                store_q4<Q>(r, dst + j * 64);
                stg(pk, ix + j * 64);
            }
        } else {
            for (int64_t i = lo + lane; i < hi; i += 64) {
                float q;
                const int id = nearest1(s_pts[w], s_mid[w], k, d.u[i], a, b, q);
                qo[i] = (Q)q;
                d.idx[i] = (uint8_t)id;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_multi_nearest_flat(const QdDiffQuantDesc* __restrict__ table, int ntensors,
                                                            int64_t total_tiles, const float* points, int k) {
    multi_nearest_flat<float>(table, ntensors, total_tiles, points, k, blockDim.x);
}

template <int OUT>
__global__ __launch_bounds__(256) void k_multi_nearest_flat_o16(const QdDiffQuantDesc* __restrict__ table, int ntensors,
                                                                int64_t total_tiles, const float* points, int k) {
    multi_nearest_flat<typename Out16<OUT>::type>(table, ntensors, total_tiles, points, k, blockDim.x);
}

// ---- backward: grad of the points of every tensor, one launch + one fold --------------------------------------------
// Work unit: a GRADIENT TILE = 1024 consecutive elements of one tensor (a wave iteration: four 1 KiB rows of gradient, four
// 256 B rows of uint8 indices).  QdDiffQuantDesc.first_block is the prefix of FULL gradient tiles over the tensors; the
// tensors' full tiles form ONE sequence 0 ... T - 1, and the main grid strides over it as qd_point_grad_f32's does over its
// one tensor: wave g of the W = 4 B waves takes tiles g, g + W, g + 2 W, ... -- every wave streams the same number of bytes
// whatever the tensor sizes are, and the whole grid moves through memory front to back together.  What is left of a tensor
// after its full tiles (n mod 1024 elements: every bias and batch-norm vector is only that) goes to EXTRA blocks behind the
// main grid, one wave per tensor: short-lived waves that run beside the sweep instead of inside one of its waves.
//   round 4: every tensor its own ceil(n / 128 Ki) blocks -- 631 blocks of 65 Ki ... 128 Ki elements on the WRN-16-22 shape
//            list, 60 tensors swept concurrently: 71.8 us = 72.1 % of the HBM peak; 47.7 us on the 1 M-parameter CIFAR student
//   round 5 (profiles/r05_ab_k6m.txt): 512 equal blocks, each its own CONTIGUOUS piece of the sequence: 73.5 us -- 512 separate
//            streaming windows are worse than 60; the wave-strided sequence WITH the partial tiles in it: 74.2 us (on ONE 64 Mi
//            tensor 54.7 us, the single-tensor kernel's time, against 65.2 us for round 4's) -- 47 of the 60 WRN tensors end
//            in a partial tile, 43 are nothing else, and each cost one of the 40-tile waves a slow masked tile + two flushes
// Partial sums: a wave keeps its bins while its tiles stay in one tensor and writes them out -- one row of k floats -- when they
// move on to the next one.  Tensor ti with c full tiles from f0 on is visited by the waves (f0 + i) mod W, i < min(c, W), each
// once: wave g writes row first_row[ti] + ((g - f0) mod W) and the extra wave of the tensor row first_row[ti] + min(c, W), so a
// tensor owns min(c, W) + 1 rows (round 6: it owned W + 1 whatever its size -- 105 MB of scratch for 200 small tensors at
// k = 64) and the fold reads them front to back.  Which rows exist is a function of the table alone, so nothing needs zeroing.
// Fixed tile -> wave assignment, fixed fold order: deterministic.
constexpr int kGradTile = 1024;
constexpr int64_t kGradWaves = 2048;                   // the main grid: 2048 waves x 4 independent 1 KiB streams, the shape that
                                                       // measured best for qd_point_grad_f32; waves beyond the last tile return at once

// T is not an argument of the entry point (the host holds no copy of the device table): the last tensor's prefix + its tiles
__device__ __forceinline__ int64_t total_grad_tiles(const QdDiffQuantDesc* table, int ntensors) {
    return table[ntensors - 1].first_block + table[ntensors - 1].n / kGradTile;
}

// last tensor whose tile prefix is <= t, for a whole wave at once: every lane looks at one tensor's prefix, a ballot counts
// (one memory round trip per 64 tensors instead of log2(ntensors) dependent scalar loads before the wave's first tile)
__device__ __forceinline__ int owner_of_tile(const QdDiffQuantDesc* table, int ntensors, int64_t t, int lane) {
    int cnt = 0;
    for (int base = 0; base < ntensors; base += 64) {
        const int i = base + lane;
        const bool le = i < ntensors && table[i].first_block <= t;
        cnt += __popcll(__ballot(le));
    }
    return __builtin_amdgcn_readfirstlane(cnt - 1);
}

// KR > 0: k <= KR bins in registers (compare-select-add); KR == 0: lane-private LDS columns [k][64 WPB].
// WPB: waves per block -- 4 while the columns of k <= 64 bins fit 64 KB of LDS, 1 above that ([256][64] floats = 64 KB); the
// tile -> wave -> row assignment is that of the 2048 waves whatever a block holds of them, so the fold does not change.
// DIV: the bucket is not a power of two -- the alpha of element e is alpha[e / bucket], looked up per element (a float4 can
// straddle a bucket end); otherwise alpha[e >> row_shift], one per float4.  Functional, not tuned.
// G: the gradient's element type -- float (qd_multi_point_grad_f32; the code is then what it always was) or _Float16 / __bf16
// (qd_multi_point_grad_in16_f32: d.grad addresses n 16-bit elements, widened exactly on load).  Only the load differs: the one
// fp32 multiply g alpha, the bins, the flush order and the rows are the same.  With 16-bit gradients the alignment of grad has no
// say in the summation order: a lane owns four consecutive elements whenever idx is 4-byte aligned (grad is read with 8-byte
// loads where it is 8-byte aligned -- a tile starts a multiple of 2 KiB into the tensor, a lane's four a multiple of 8 bytes into
// the tile -- and element by element otherwise), so the sums are those of the fp32 launch on a 16-byte-aligned widened copy.
template <int KR, int WPB, bool DIV, typename G>
__device__ __forceinline__ void multi_point_grad(const QdDiffQuantDesc* table, int ntensors, int64_t bucket,
                                                 int row_shift, int k, float* part /* [rows][k] */) {
    extern __shared__ __attribute__((aligned(16))) float lds[];        // KR == 0: [k][64 WPB]
    constexpr bool G32 = std::is_same<G, float>::value;
    typedef G G4 __attribute__((ext_vector_type(4)));                  // a lane's four consecutive gradients: 16 or 8 bytes
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    constexpr int C = 64 * WPB;                                        // columns = lanes of a block
    constexpr int64_t W = kGradWaves;
    constexpr int B = (int)(W / WPB);                                  // blocks of the main grid
    float acc[KR > 0 ? KR : 1];
    float* col = lds + threadIdx.x;                                    // this lane's column; a wave owns columns 64 w ... 64 w + 63
    auto clear = [&]() {
        if (KR > 0) {
#pragma unroll
            for (int j = 0; j < (KR > 0 ? KR : 1); ++j) acc[j] = 0.0f;
        } else {
            for (int j = 0; j < k; ++j) col[j * C] = 0.0f;
        }
    };
    auto add = [&](int id, float m) {
        if (KR > 0) {
#pragma unroll
            for (int j = 0; j < (KR > 0 ? KR : 1); ++j) acc[j] += (id == j) ? m : 0.0f;
        } else {
            col[id * C] += m;                                          // private column: plain LDS read-add-write
        }
    };
    auto flush = [&](const QdDiffQuantDesc& dd, int64_t r) {           // this wave's sums for tensor dd -> its row for wave r (W: the extra wave), bins cleared
        const int64_t full = dd.n / kGradTile;
        int64_t c = r - dd.first_block % W;                            // (r - f0) mod W for a wave of the main grid
        c = c < 0 ? c + W : c;
        c = r == W ? (full < W ? full : W) : c;
        float* row = part + (dd.first_row + c) * k;
        if (KR > 0) {
#pragma unroll
            for (int j = 0; j < (KR > 0 ? KR : 1); ++j) {
                // wave_sum() as lane 0 sees it -- (row 0 + row 1) + (row 2 + row 3) -- with the four row sums read as scalars
                const float rs = row16_sum(acc[j]);
                const float s0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rs), 0));
                const float s1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rs), 16));
                const float s2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rs), 32));
                const float s3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rs), 48));
                const float sum = (s0 + s1) + (s2 + s3);
                if (lane == 0 && j < k) row[j] = sum;
            }
        } else {
            // LDS operations of one wave complete in order; the barriers only pin the compiler.  Lane j folds bin j's 64 columns
            // of this wave (rotated start: bank-conflict free) in a fixed order.
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            auto fold_bin = [&](int j) {
                const float* base = lds + j * C + 64 * w;
                float s0 = 0.0f, s1 = 0.0f;
                for (int c = 0; c < 64; c += 2) { s0 += base[(c + lane) & 63]; s1 += base[(c + 1 + lane) & 63]; }
                row[j] = s0 + s1;
            };
            if (WPB == 4) {                                             // k <= 64: one pass, as one statement (as a loop it costs 25 VGPRs)
                if (lane < k) fold_bin(lane);
            } else {
#pragma unroll 1
                for (int j = lane; j < k; j += 64) fold_bin(j);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        clear();
    };
    auto bucket_of = [&](int64_t e) { return DIV ? e / bucket : e >> row_shift; };
    // the alphas of the `cnt` (<= 4) elements from e on.  DIV: a bucket that is no power of two holds at least 3 elements, so
    // at most one bucket end lies inside e ... e + 3
    auto alpha4 = [&](const QdDiffQuantDesc& d, bool single, int64_t e, int64_t cnt, float (&a)[4]) {
        if (!DIV) {
            a[0] = a[1] = a[2] = a[3] = cnt > 0 ? ldg(d.alpha + (single ? 0 : bucket_of(e))) : 0.0f;
        } else {
            const int64_t b0 = single ? 0 : e / bucket;
            const int64_t r = e - b0 * bucket;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int step = r + j >= bucket ? 1 : 0;              // r + j < bucket + 3 <= 2 bucket
                a[j] = cnt > j ? ldg(d.alpha + (single ? 0 : b0 + step)) : 0.0f;
            }
        }
    };
    auto scalar_span = [&](const QdDiffQuantDesc& d, int64_t lo, int64_t hi) {        // element by element (a view at an odd offset)
        const bool single = d.n <= bucket;
        for (int64_t e = lo + lane; e < hi; e += 64)
            add((int)d.idx[e], widen(((const G*)d.grad)[e]) * d.alpha[single ? 0 : bucket_of(e)]);
    };
    // a lane's four consecutive gradients (all four exist).  g8: the tensor's grad is 8-byte aligned (16-bit gradients only)
    auto load4 = [&](const G4* p, bool g8) -> f4 {
        if constexpr (G32) return ldg_nt(p);
        else return load16x4_nt((const G*)p, g8);
    };

    if ((int)blockIdx.x >= B) {
        // ---- the extra waves: what is left of tensor ti after its full tiles
        const int ti = ((int)blockIdx.x - B) * WPB + w;
        if (ti >= ntensors) return;
        const QdDiffQuantDesc d = table[ti];
        const int64_t rem = d.n % kGradTile;
        if (rem == 0) return;
        clear();
        const int64_t e0 = d.n - rem;
        const bool single = d.n <= bucket;
        const bool aligned = (!G32 || ((((uintptr_t)d.grad) & 15) == 0)) && ((((uintptr_t)d.idx) & 3) == 0);
        const bool g8 = (((uintptr_t)d.grad) & 7) == 0;
        if (aligned) {
            // every lane issues its loads up front; the float4 that straddles the end is assembled from scalar loads; elements past
            // the end add an exact +0 to bin 0 (not 0 x alpha, which is NaN for the alpha = inf of a bucket that holds an infinity)
            const G4* g4 = (const G4*)((const G*)d.grad + e0) + lane;
            const uint32_t* i4 = (const uint32_t*)(d.idx + e0) + lane;
            const int64_t left = rem - 4 * lane;                        // elements from this lane's first float4 to the end
            f4 gv[4]; uint32_t pk[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t lu = left - 256 * u;
                const G* gs = (const G*)(g4 + 64 * u);
                const uint8_t* is = (const uint8_t*)(i4 + 64 * u);
                float al[4];
                alpha4(d, single, e0 + 256 * u + 4 * lane, lu, al);
                f4 gq = {0.0f, 0.0f, 0.0f, 0.0f};
                uint32_t pq = 0;
                if (lu >= 4) {
                    gq = load4(g4 + 64 * u, g8);
                    pq = ldg_nt(i4 + 64 * u);
                } else {
                    if (lu > 0) { gq.x = widen(gs[0]); pq |= (uint32_t)is[0]; }
                    if (lu > 1) { gq.y = widen(gs[1]); pq |= (uint32_t)is[1] << 8; }
                    if (lu > 2) { gq.z = widen(gs[2]); pq |= (uint32_t)is[2] << 16; }
                }
                gv[u].x = lu > 0 ? gq.x * al[0] : 0.0f; gv[u].y = lu > 1 ? gq.y * al[1] : 0.0f;     // one fp32 multiply each, quant_functions.py:495
                gv[u].z = lu > 2 ? gq.z * al[2] : 0.0f; gv[u].w = lu > 3 ? gq.w * al[3] : 0.0f;
                pk[u] = pq;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                add(pk[u] & 255, gv[u].x);
                add((pk[u] >> 8) & 255, gv[u].y);
                add((pk[u] >> 16) & 255, gv[u].z);
                add(pk[u] >> 24, gv[u].w);
            }
        } else {
            scalar_span(d, e0, d.n);
        }
        flush(d, W);
        return;
    }

    // ---- the main grid: full tiles only
    const int64_t T = total_grad_tiles(table, ntensors);
    const int64_t g = (int64_t)blockIdx.x * WPB + w;                   // a block's waves take adjacent tiles
    if (g >= T) return;
    int ti = owner_of_tile(table, ntensors, g, lane);                  // once per wave
    clear();
    QdDiffQuantDesc d = table[ti];
    int64_t next_first = ti + 1 < ntensors ? table[ti + 1].first_block : T;
    for (int64_t t = g; t < T; t += W) {
        if (t >= next_first) {                                          // this wave's tiles have moved on to a later tensor
            flush(d, g);
            do {
                ++ti;
                next_first = ti + 1 < ntensors ? table[ti + 1].first_block : T;
            } while (t >= next_first);
            d = table[ti];
        }
        const int64_t e0 = (t - d.first_block) * kGradTile;
        const bool aligned = (!G32 || ((((uintptr_t)d.grad) & 15) == 0)) && ((((uintptr_t)d.idx) & 3) == 0);
        const bool g8 = (((uintptr_t)d.grad) & 7) == 0;
        if (aligned) {                                                  // four (gradient float4, four indices, alpha) loads up front
            const G4* g4 = (const G4*)((const G*)d.grad + e0) + lane;
            const uint32_t* i4 = (const uint32_t*)(d.idx + e0) + lane;
            f4 gv[4]; uint32_t pk[4]; float a[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                gv[u] = load4(g4 + 64 * u, g8);
                pk[u] = ldg_nt(i4 + 64 * u);
                alpha4(d, d.n <= bucket, e0 + 256 * u + 4 * lane, 4, a[u]);                                 // n <= bucket: one alpha
            }
            __builtin_amdgcn_sched_barrier(0);                          // keep the loads together (not sunk to their uses)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                add(pk[u] & 255, gv[u].x * a[u][0]);                    // one fp32 multiply each, quant_functions.py:495
                add((pk[u] >> 8) & 255, gv[u].y * a[u][1]);
                add((pk[u] >> 16) & 255, gv[u].z * a[u][2]);
                add(pk[u] >> 24, gv[u].w * a[u][3]);
            }
        } else {
            scalar_span(d, e0, e0 + kGradTile);
        }
    }
    flush(d, g);
}

template <int KR, int WPB, bool DIV>
__global__ __launch_bounds__(64 * WPB) void k_multi_point_grad(const QdDiffQuantDesc* __restrict__ table, int ntensors,
                                                               int64_t bucket, int row_shift, int k, float* part /* [rows][k] */) {
    multi_point_grad<KR, WPB, DIV, float>(table, ntensors, bucket, row_shift, k, part);
}

// KIND: the grad_kind of the C ABI
template <int KR, int WPB, bool DIV, int KIND>
__global__ __launch_bounds__(64 * WPB) void k_multi_point_grad_in16(const QdDiffQuantDesc* __restrict__ table, int ntensors,
                                                                    int64_t bucket, int row_shift, int k, float* part) {
    multi_point_grad<KR, WPB, DIV, typename Grad16<KIND>::type>(table, ntensors, bucket, row_shift, k, part);
}

// backward stage 2: block (tensor, bin) folds the rows that tensor's waves wrote, front to back.  Up to 2048 + 1 rows per
// tensor: 256 threads, eight independent loads in flight each (one dependent load per row and thread was 32 round trips =
// ~12 us on the WRN shape list, more than the sweep gained).
__global__ __launch_bounds__(256) void k_multi_point_grad_final(const QdDiffQuantDesc* __restrict__ table, int ntensors,
                                                                int k, const float* part,
                                                                float* grad_points /* [ntensors][k] */) {
    __shared__ double s_w[4];
    constexpr int64_t W = kGradWaves;
    const int ti = blockIdx.x / k, j = blockIdx.x % k;
    const int64_t full = table[ti].n / kGradTile;
    const int64_t rows = full < W ? full : W;                           // row i: wave (f0 + i) mod W, the i-th of the waves that had a tile of this tensor
    const float* base = part + table[ti].first_row * k + j;
    auto row = [&](int64_t i) { return base[i * k]; };
    double acc = 0.0;
    int64_t i = threadIdx.x;
    for (; i + 7 * 256 < rows; i += 8 * 256) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = row(i + u * 256);
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += (double)v[u];
    }
    for (; i < rows; i += 256) acc += (double)row(i);
    if (threadIdx.x == 0 && (table[ti].n % kGradTile) != 0) acc += (double)base[rows * k];   // the extra wave's row
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) grad_points[(int64_t)ti * k + j] = (float)((s_w[0] + s_w[1]) + (s_w[2] + s_w[3]));
}

// gradient sweep + fold of both backward entry points.  grad_kind 0: fp32 gradients
int point_grad_launch(const QdDiffQuantDesc* table, int ntensors, int64_t total_blocks, int64_t bucket, int k, int grad_kind,
                      float* grad_points, void* workspace, size_t workspace_bytes, void* stream) {
    if (!table || ntensors <= 0 || total_blocks <= 0 || bucket < 0 || k < 1 || k > kMaxK || !grad_points)
        return QD_ERR_INVALID_ARGUMENT;
    // total_blocks is what qd_multi_dq_plan wrote: between 1 and 2048 + 1 partial rows per tensor
    if (total_blocks < ntensors || total_blocks > (kGradWaves + 1) * (int64_t)ntensors) return QD_ERR_INVALID_ARGUMENT;
    if (!workspace || (((uintptr_t)workspace) & 15) || workspace_bytes < (size_t)total_blocks * k * sizeof(float))
        return QD_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    const bool div = (bucket & (bucket - 1)) != 0;                     // alpha[e / bucket] per element instead of alpha[e >> row_shift]
    const int64_t kb = bucket == 0 ? INT64_MAX : bucket;               // no buckets: every tensor is "n <= bucket", one alpha
    int row_shift = 0;
    while (row_shift < 62 && ((int64_t)1 << row_shift) < kb) ++row_shift;
    float* part = (float*)workspace;
    // grid: the blocks of the sweep over the full tiles, 2048 waves in all (a wave beyond the last tile returns at once) + one
    // wave per tensor for what is left after them
    auto launch = [&](auto kernel, int wpb, size_t lds) {
        const unsigned grid = (unsigned)(kGradWaves / wpb + (ntensors + wpb - 1) / wpb);
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * wpb), lds, st, table, ntensors, kb, row_shift, k, part);
    };
    // KR, WPB: k <= 4 in registers; k <= 64 four waves per block; above, [k][64] columns: 64 KB at k = 256
    const size_t lds4 = (size_t)k * 256 * sizeof(float), lds1 = (size_t)k * 64 * sizeof(float);
#define QD_DQ_GRAD(KERNEL, ...)                                                                                            \
    {                                                                                                                      \
        if (k <= 4) {                                                                                                      \
            if (div) launch(KERNEL<4, 4, true __VA_ARGS__>, 4, 0); else launch(KERNEL<4, 4, false __VA_ARGS__>, 4, 0);     \
        } else if (k <= 64) {                                                                                              \
            if (div) launch(KERNEL<0, 4, true __VA_ARGS__>, 4, lds4); else launch(KERNEL<0, 4, false __VA_ARGS__>, 4, lds4); \
        } else {                                                                                                           \
            if (div) launch(KERNEL<0, 1, true __VA_ARGS__>, 1, lds1); else launch(KERNEL<0, 1, false __VA_ARGS__>, 1, lds1); \
        }                                                                                                                  \
    }
#define QD_COMMA ,
    if (grad_kind == 0) QD_DQ_GRAD(k_multi_point_grad)
    else if (grad_kind == QD_GRAD_F16) QD_DQ_GRAD(k_multi_point_grad_in16, QD_COMMA QD_GRAD_F16)
    else QD_DQ_GRAD(k_multi_point_grad_in16, QD_COMMA QD_GRAD_BF16)
#undef QD_COMMA
#undef QD_DQ_GRAD
    hipLaunchKernelGGL(k_multi_point_grad_final, dim3((unsigned)(ntensors * k)), dim3(256), 0, st, table, ntensors, k, part,
                       grad_points);
    return (int)hipGetLastError();
}

// what both forward entry points refuse
inline bool nearest_args_ok(const QdDiffQuantDesc* table, int ntensors, int64_t total_tiles, int64_t bucket, const float* points,
                            int k) {
    return table && ntensors > 0 && total_tiles >= 0 && bucket >= 0 && points && k >= 1 && k <= kMaxK;
}

}  // namespace

extern "C" {

int64_t qd_multi_dq_plan(QdDiffQuantDesc* host_table, int ntensors, int64_t bucket, int64_t* total_blocks_out) {
    if (!host_table || ntensors <= 0 || bucket < 0 || !total_blocks_out) return -1;
    // the only place that sees the pointers (the launches take a device table): an odd q or grad is wrong for every element
    // type, the 16-bit ones of the _out16 / _in16 entry points included
    for (int i = 0; i < ntensors; ++i)
        if (host_table[i].n > 0 && ((((uintptr_t)host_table[i].q) | ((uintptr_t)host_table[i].grad)) & 1)) return -1;
    int64_t tiles = 0, gtiles = 0, rows = 0;
    for (int i = 0; i < ntensors; ++i) {
        const int64_t n = host_table[i].n;
        const int64_t row = bucket == 0 || n < bucket ? (n > 0 ? n : 1) : bucket;
        const int64_t nb = n > 0 ? (n + row - 1) / row : 0;
        host_table[i].first_tile = tiles;
        host_table[i].first_block = gtiles;              // prefix of FULL 1024-element gradient tiles (k_multi_point_grad)
        host_table[i].first_row = rows;                  // prefix of partial rows: min(full tiles, 2048) + 1 per tensor
        const int64_t full = n > 0 ? n / kGradTile : 0;
        tiles += bucket == 0 ? (n > 0 ? (n + kFlatTile - 1) / kFlatTile : 0) : (nb + 3) / 4;     // k_multi_nearest_flat / k_multi_nearest
        gtiles += full;
        rows += (full < kGradWaves ? full : kGradWaves) + 1;
    }
    *total_blocks_out = rows;                            // partial rows of the gradient sweep, see k_multi_point_grad
    return tiles;
}

int qd_multi_nearest_f32(const QdDiffQuantDesc* table, int ntensors, int64_t total_tiles, int64_t bucket,
                         const float* points, int k, void* stream) {
    if (!nearest_args_ok(table, ntensors, total_tiles, bucket, points, k)) return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = grid_blocks(total_tiles, 4, kNoOwnCap);
    if (bucket == 0) hipLaunchKernelGGL(k_multi_nearest_flat, dim3(blocks), dim3(256), 0, st, table, ntensors, total_tiles, points, k);
    else if (bucket == 256) hipLaunchKernelGGL((k_multi_nearest<256>), dim3(blocks), dim3(256), 0, st, table, ntensors, total_tiles, bucket, points, k);
    else if (bucket == 128) hipLaunchKernelGGL((k_multi_nearest<128>), dim3(blocks), dim3(256), 0, st, table, ntensors, total_tiles, bucket, points, k);
    else if (bucket == 64) hipLaunchKernelGGL((k_multi_nearest<64>), dim3(blocks), dim3(256), 0, st, table, ntensors, total_tiles, bucket, points, k);
    else hipLaunchKernelGGL((k_multi_nearest<0>), dim3(blocks), dim3(256), 0, st, table, ntensors, total_tiles, bucket, points, k);
    return (int)hipGetLastError();
}

int qd_multi_nearest_out16_f32(const QdDiffQuantDesc* table, int ntensors, int64_t total_tiles, int64_t bucket,
                               const float* points, int k, int out_kind, void* stream) {
    if (!nearest_args_ok(table, ntensors, total_tiles, bucket, points, k)) return QD_ERR_INVALID_ARGUMENT;
    if (out_kind != QD_OUT_F16 && out_kind != QD_OUT_BF16) return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = grid_blocks(total_tiles, 4, kNoOwnCap);
#define QD_DQ_O16(OUT)                                                                                                      \
    {                                                                                                                       \
        if (bucket == 0) hipLaunchKernelGGL((k_multi_nearest_flat_o16<OUT>), dim3(blocks), dim3(256), 0, st, table, ntensors, total_tiles, points, k); \
        else if (bucket == 256) hipLaunchKernelGGL((k_multi_nearest_o16<256, OUT>), dim3(blocks), dim3(256), 0, st, table, ntensors, total_tiles, bucket, points, k); \
        else if (bucket == 128) hipLaunchKernelGGL((k_multi_nearest_o16<128, OUT>), dim3(blocks), dim3(256), 0, st, table, ntensors, total_tiles, bucket, points, k); \
        else if (bucket == 64) hipLaunchKernelGGL((k_multi_nearest_o16<64, OUT>), dim3(blocks), dim3(256), 0, st, table, ntensors, total_tiles, bucket, points, k); \
        else hipLaunchKernelGGL((k_multi_nearest_o16<0, OUT>), dim3(blocks), dim3(256), 0, st, table, ntensors, total_tiles, bucket, points, k); \
    }
    if (out_kind == QD_OUT_F16) QD_DQ_O16(QD_OUT_F16)
    else QD_DQ_O16(QD_OUT_BF16)
#undef QD_DQ_O16
    return (int)hipGetLastError();
}

int qd_multi_point_grad_f32(const QdDiffQuantDesc* table, int ntensors, int64_t total_blocks, int64_t bucket, int k,
                            float* grad_points, void* workspace, size_t workspace_bytes, void* stream) {
    return point_grad_launch(table, ntensors, total_blocks, bucket, k, 0, grad_points, workspace, workspace_bytes, stream);
}

int qd_multi_point_grad_in16_f32(const QdDiffQuantDesc* table, int ntensors, int64_t total_blocks, int64_t bucket, int k,
                                 int grad_kind, float* grad_points, void* workspace, size_t workspace_bytes, void* stream) {
    if (grad_kind != QD_GRAD_F16 && grad_kind != QD_GRAD_BF16) return QD_ERR_INVALID_ARGUMENT;
    return point_grad_launch(table, ntensors, total_blocks, bucket, k, grad_kind, grad_points, workspace, workspace_bytes, stream);
}

}  // extern "C"
