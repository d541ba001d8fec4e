// qdm_linear.hip -- libqd_infer_mm.so: the Linear layer of include/qd_infer.h for MANY rows of x (include/qd_infer_mm.h),
// gfx950.  The one kernel of this project that uses matrix instructions: a weight decoded once from its bits / 8 bytes
// feeds up to 64 rows of x through v_mfma_f32_16x16x4_f32 -- fp32 in, fp32 accumulate, so every weight is bit for bit the
// value of the header and neither x nor y is rounded to a narrower type.  Nothing of libqd_hip.so or libqd_infer.so is
// linked in; the decode is the shared one of qdi_packed.h.
//
// k_linear_mm, one block of 256 threads (4 waves) per tile of 16 weight rows (N) x up to 64 rows of x (an "m-chunk"):
//   split     tiles = N-tiles x m-chunks, m-chunk fastest (the blocks that decode the same 16 weight rows run next to each
//             other and find the stream in L2), strided over the grid.  Wave w owns the rows [16 w, 16 w + 16) of x of the chunk
//             and all 16 weight rows: ONE 16 x 16 accumulator (4 AGPRs); a wave whose rows lie at or past m skips the MFMAs.
//             No split-K, no atomics.  The first version had tiles of 64 weight rows (wave w: weight rows [16 w, + 16), four
//             accumulators over the rows of x).  It lost to the row-wise kernel on [4096, 4096] at m = 64 (564 us against
//             195 us): 64 tiles on 256 CUs, one wave per SIMD, and each thread decoding 16 weights per slab through about 1500
//             instructions with nothing to overlap them with -- the slab took 6 us whatever m was, also after its loads had
//             been freed of their waits.  Tiles of 16 rows give 4 x the blocks, a quarter of the decode per thread and slab
//             (ONE group of four), and registers for four and more blocks per CU; the price is that the x slab is staged once per 16
//             weight rows instead of once per 64 (from L2: x is m K 4 bytes).
//   K slabs   64 columns at a time through LDS: ws[16][68] (weights, decoded ONCE per tile and slab: thread t decodes the group
//             of four [4 (t % 16), + 4) of row t / 16: one bucket search per thread and tile, steps of 64 elements from there)
//             and xs[64][68] (thread t: the 16 columns [16 (t % 4), + 16) of row t / 4, 16-byte global loads at any 4-byte phase,
//             64 contiguous bytes of a row per thread; the 16 lanes of a b128 LDS write cover all 64 banks).  The second
//             buffer is REGISTERS, not LDS: slab s + 1's loads (two stream words, alpha, beta, x: 20 VGPRs) are issued before
//             slab s's MFMAs and become LDS contents after them (fetch4 / finish4), with two barriers per slab.  fetch() holds
//             loads ONLY -- no instruction that consumes a loaded value -- so none of them is waited for before the MFMAs.
//   operands  A = x (a lane gives x[i0 + 16 w + l % 16][k]), B = W^T (w[r0 + l % 16][k]), so D[i][j] has j = l % 16 along N: the
//             16 lanes of a row group store 64 contiguous bytes of one row of y.
//   LDS reads a row stride of 68 floats; lane l reads the FOUR floats [l % 16][16 q + 4 (l / 16), + 4) of a 16-column
//             group as one ds_read_b128 and feeds them to four MFMAs: MFMA jj of group q multiplies the columns
//             16 q + jj + {0, 4, 8, 12}.  68 r mod 64 = 4 r: the 16 lanes a b128 read serves per cycle cover all 64 banks.
//   order     of an output element: slabs front to back, inside a slab the 16-column groups front to back, inside a group
//             jj = 0 .. 3, each MFMA adding its four products to the running accumulator; a last slab of fewer than 64
//             columns runs only the groups that hold a column.  A function of cols alone.
#include "qdi_packed.h"       // Packed, describe, stream_bits, divmod, build_quotients, fetch4 / finish4: shared with qdi_layers.hip

#include "../../../include/qd_infer_mm.h"

using namespace qd;

namespace {

constexpr int kTile = 64;              // rows of x of a chunk and columns of a slab
constexpr int kRows = 16;              // weight rows of a tile: one MFMA block
constexpr int kStride = 68;            // floats per LDS row: 16-byte aligned rows, conflict-free operand reads (above)

int g_grid_cap = 0;                    // qdm_set_grid_cap: 0 = none

int capped(int64_t blocks, int64_t own_cap) {
    if (blocks > own_cap) blocks = own_cap;
    if (g_grid_cap >= 1 && blocks > g_grid_cap) blocks = g_grid_cap;
    return blocks < 1 ? 1 : (int)blocks;
}

__global__ __launch_bounds__(256) void k_linear_mm(Packed P, const float* x, int64_t m, const float* bias, float* y, int64_t m_chunks,
                                                   int64_t tiles, int64_t step_q, int64_t step_r /* 64 = step_q bucket + step_r */) {
    __shared__ float qtab[256];
    __shared__ __attribute__((aligned(16))) float ws[kRows * kStride];
    __shared__ __attribute__((aligned(16))) float xs[kTile * kStride];
    build_quotients(qtab, P.levels);
    const int tid = threadIdx.x;
    const int wr = tid >> 4, wc = (tid & 15) << 2;                      // staging of W: the group of four [wc, wc + 4) of row wr of the slab
    const int srow = tid >> 2, scol = (tid & 3) << 4;                   // staging of x: row srow, the four groups [scol + 4 j, + 4)
    const int lane = tid & 63, fr = lane & 15, fk = (lane >> 4) << 2;    // fragments: row fr of a 16-row block, columns fk .. fk + 3 of a group
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t N = P.rows, K = P.cols;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t nt = tile / m_chunks;
        const int64_t r0 = nt * kRows, i0 = (tile - nt * m_chunks) * kTile;
        const int mrows = m - i0 < kTile ? (int)(m - i0) : kTile;        // rows of x in this chunk, >= 1
        const bool wrow = r0 + wr < N, xrow = srow < mrows;              // this thread's weight row / row of x exists
        const bool mine = 16 * wave < mrows;                             // this wave's 16 rows of x hold one (wave-uniform)
        // A thread without a weight row (!wrow), without a row of x (!xrow) or whose columns lie past K still carries e, xp, bkt and
        // rem along (past the arrays, or 0 stepped on): every USE below is under the same wrow / xrow / column test, in fetch and
        // in commit alike, so none of them is ever turned into an address that is read.
        int64_t e = (r0 + wr) * K + wc;                                  // its group's first element in the current slab ...
        const float* xp = x + (i0 + srow) * K + scol;
        int64_t bkt = 0, rem = 0;                                        // ... and that element's bucket, as k_embedding finds it
        if (wrow && wc < K) divmod(e, P.bucket, P.small, bkt, rem);
        f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t lo, hi;                                                 // the next slab between its loads and its LDS writes
        float a0, b0;
        f4 xn[4];

        // The loads of a slab of kl <= 64 columns, and nothing but loads: no instruction here consumes a loaded value, so all of
        // them (8 per thread) are in flight at once while the MFMAs of the slab before run.  Whole groups of four of x only; the
        // one ragged group of a row (its last, in the last slab) and the last words of the stream are read in commit().
        auto fetch = [&](int kl) {
            if (wrow && kl - wc > 0) fetch4(P, e, bkt, lo, hi, a0, b0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (xrow && kl - scol - 4 * j >= 4) {
                    const f4u u = *(const f4u*)(xp + 4 * j);
                    xn[j] = (f4){u.x, u.y, u.z, u.w};
                }
            }
        };
        // the same slab from the registers into LDS: zeros wherever nothing is to be read
        auto commit = [&](int kl) {
            const int nw = kl - wc;                                      // columns from this group's first to the end of the row
            float w[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (wrow && nw > 0) finish4(P, qtab, lo, hi, a0, b0, e, bkt, rem, nw < 4 ? nw : 4, w);
            *(f4*)&ws[wr * kStride + wc] = (f4){w[0], w[1], w[2], w[3]};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int nv = kl - scol - 4 * j;
                f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
                if (xrow && nv >= 4) v = xn[j];
                if (xrow && nv > 0 && nv < 4) {                          // the ragged group: nothing past x[i][K)
                    v.x = xp[4 * j];
                    if (nv > 1) v.y = xp[4 * j + 1];
                    if (nv > 2) v.z = xp[4 * j + 2];
                }
                *(f4*)&xs[srow * kStride + scol + 4 * j] = v;
            }
        };

        int64_t kleft = K;                                               // columns from the current slab's first to the end of the row
        if (kleft > 0) fetch(kleft < kTile ? (int)kleft : kTile);
        while (kleft > 0) {
            const int kl = kleft < kTile ? (int)kleft : kTile;
            commit(kl);
            __syncthreads();
            kleft -= kTile;
            if (kleft > 0) {
                bkt += step_q; rem += step_r;                            // 64 columns on: the bucket of the next slab's group
                if (rem >= P.bucket) { rem -= P.bucket; ++bkt; }
                e += kTile; xp += kTile;
                fetch(kleft < kTile ? (int)kleft : kTile);               // in flight during the MFMAs below
            }
            if (mine) {
                const int groups = (kl + 15) >> 4;
                for (int q = 0; q < groups; ++q) {
                    const f4 b = *(const f4*)&ws[fr * kStride + 16 * q + fk];
                    const f4 a = *(const f4*)&xs[(16 * wave + fr) * kStride + 16 * q + fk];
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[jj], b[jj], acc, 0, 0, 0);
                }
            }
            __syncthreads();                                             // every wave is done with this slab before the next commit
        }

        // D[i][j]: j = lane % 16 (weight row), i = 4 (lane / 16) + v (row of x inside the wave's 16-row block)
        const int64_t r = r0 + fr;
        if (mine && r < N) {
            const float bv = bias ? bias[r] : 0.0f;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int64_t i = i0 + 16 * wave + fk + v;
                if (i < m) y[i * N + r] = bias ? acc[v] + bv : acc[v];
            }
        }
    }
}

}  // namespace

extern "C" {

int qdm_abi_version(void) { return QDM_ABI_VERSION; }
const char* qdm_target_arch(void) { return "gfx950"; }

const char* qdm_error_string(int code) {
    if (code == 0) return "success";
    if (code == QDM_ERR_INVALID_ARGUMENT) return "invalid argument";
    if (code > 0) return hipGetErrorString((hipError_t)code);
    return "unknown error";
}

int qdm_set_grid_cap(int blocks) {
    const int prev = g_grid_cap;
    g_grid_cap = blocks >= 1 ? blocks : 0;
    return prev;
}

int qdm_linear_packed_f32(const uint8_t* packed, const float* alpha, const float* beta, int64_t rows, int64_t cols, int64_t bucket,
                          int levels, int bits, const float* x, int64_t m, const float* bias, float* y, void* stream) {
    Packed P;
    if (!describe(P, packed, alpha, beta, rows, cols, bucket, levels, bits) || m < 0) return QDM_ERR_INVALID_ARGUMENT;
    if ((((uintptr_t)x) & 3) || (((uintptr_t)bias) & 3) || (((uintptr_t)y) & 3)) return QDM_ERR_INVALID_ARGUMENT;
    int64_t t = 0;
    if (__builtin_mul_overflow(m, rows, &t) || __builtin_mul_overflow(m, cols, &t)) return QDM_ERR_INVALID_ARGUMENT;
    if (m == 0 || rows == 0) return 0;
    if (!y || (cols > 0 && (!packed || !alpha || !beta || !x))) return QDM_ERR_INVALID_ARGUMENT;
    const int64_t m_chunks = (m - 1) / kTile + 1;
    const int64_t tiles = ((rows - 1) / kRows + 1) * m_chunks;          // <= m rows: fits
    const int blocks = capped(tiles, (int64_t)device_cus() * 8);
    hipLaunchKernelGGL(k_linear_mm, dim3(blocks), dim3(256), 0, (hipStream_t)stream, P, x, m, bias, y, m_chunks, tiles,
                       kTile / P.bucket, kTile % P.bucket);
    return (int)hipGetLastError();
}

}  // extern "C"
