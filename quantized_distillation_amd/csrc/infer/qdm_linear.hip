// qdm_linear.hip -- libqd_infer_mm.so: the Linear layer of include/qd_infer.h for MANY rows of x (include/qd_infer_mm.h),
// gfx950.  A weight decoded once from its bits / 8 bytes feeds up to 64 rows of x through v_mfma_f32_16x16x4_f32 -- fp32 in,
// fp32 accumulate, so every weight is bit for bit the value of the header and neither x nor y is rounded to a narrower type.
// Nothing of libqd_hip.so or libqd_infer.so is linked in; the decode is the shared one of qdi_packed.h; the slabs, the LDS
// layout, the register double buffer and the order of an output element are described in qdi_mm.h, which holds the pieces of the K
// walk this kernel shares with k_lstm_cell_mm and k_conv2d_mm.  The staging of x and the slab loop are written out here (and, the
// same text, in k_lstm_cell_mm): qdi_mm.h says why.
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
//   operands  A = x (a lane gives x[i0 + 16 w + l % 16][k]), B = W^T (w[r0 + l % 16][k]), so D[i][j] has j = l % 16 along N: the
//             16 lanes of a row group store 64 contiguous bytes of one row of y.
#include "qdi_mm.h"           // the shared pieces of the K walk; through it qdi_packed.h: Packed, describe, the decode, the host helpers

#include "../../../include/qd_infer_mm.h"

using namespace qd;

namespace {

constexpr int kTile = 64;              // rows of x of a chunk

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
        int64_t bkt, rem;                                                // ... and that element's bucket
        weight_bucket(P, e, wrow && wc < K, bkt, rem);
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
            weight_commit(P, qtab, ws, wrow, kl, wr, wc, lo, hi, a0, b0, e, bkt, rem);
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
                weight_step(P, step_q, step_r, e, bkt, rem);
                xp += kTile;
                fetch(kleft < kTile ? (int)kleft : kTile);               // in flight during the MFMAs below
            }
            if (mine) rows_mfma<false>(ws, xs, kl, fr, fk, wave, acc);
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
const char* qdm_error_string(int code) { return error_string(code, QDM_ERR_INVALID_ARGUMENT); }
int qdm_set_grid_cap(int blocks) { return set_grid_cap(blocks); }

int qdm_linear_packed_f32(const uint8_t* packed, const float* alpha, const float* beta, int64_t rows, int64_t cols, int64_t bucket,
                          int levels, int bits, const float* x, int64_t m, const float* bias, float* y, void* stream) {
    Packed P;
    if (!describe(P, packed, alpha, beta, rows, cols, bucket, levels, bits) || m < 0) return QDM_ERR_INVALID_ARGUMENT;
    if (misaligned(x) || misaligned(bias) || misaligned(y)) return QDM_ERR_INVALID_ARGUMENT;
    int64_t t = 0;
    if (__builtin_mul_overflow(m, rows, &t) || __builtin_mul_overflow(m, cols, &t)) return QDM_ERR_INVALID_ARGUMENT;
    if (m == 0 || rows == 0) return 0;
    if (!y || (cols > 0 && (!packed || !alpha || !beta || !x))) return QDM_ERR_INVALID_ARGUMENT;
    const int64_t m_chunks = (m - 1) / kTile + 1;
    const int64_t tiles = ((rows - 1) / kRows + 1) * m_chunks;          // <= m rows: fits
    const int blocks = capped(tiles, (int64_t)device_cus() * 8);
    hipLaunchKernelGGL(k_linear_mm, dim3(blocks), dim3(256), 0, (hipStream_t)stream, P, x, m, bias, y, m_chunks, tiles,
                       kSlab / P.bucket, kSlab % P.bucket);
    return (int)hipGetLastError();
}

}  // extern "C"
