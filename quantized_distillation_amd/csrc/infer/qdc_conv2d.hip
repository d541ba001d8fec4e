// qdc_conv2d.hip -- libqd_infer_conv.so: nn.Conv2d from the packed low-bit weights (include/qd_infer_conv.h), gfx950.  An
// implicit GEMM on v_mfma_f32_16x16x4_f32 -- fp32 in, fp32 accumulate -- with N = cout, M = batch oh ow output pixels and
// K = cin kh kw: the weights are decoded from their bits / 8 bytes (the shared decode of qdi_packed.h, bit for bit the value
// of the header) and the input windows are gathered from x; neither the fp32 weight nor an im2col matrix exists in memory.
// Nothing of the other libraries is linked in.
//
// k_conv2d_mm, one block of 256 threads (4 waves) per tile of 16 output channels x 256 output pixels:
//   split     tiles = N-tiles x pixel chunks, chunk fastest (the blocks that decode the same 16 weight rows run next to each
//             other and find the stream in L2), strided over the grid.  The flat pixel index is n oh ow + p ow + q.  Wave v
//             owns the pixels [64 v, 64 v + 64) of the chunk and all 16 channels: FOUR 16 x 16 accumulators (16 AGPRs / VGPRs);
//             a wave whose pixels all lie at or past M skips its gather and its MFMAs.  A slab of weights is decoded once per
//             256 pixels (k_linear_mm: once per 64 rows of x -- DESIGN.md 11.1 found decode and staging, not the MFMAs, to set
//             that kernel's time, and a convolution has 10^4 .. 10^5 pixels per call).  No split-K, no atomics.
//   operands  swapped against k_linear_mm: A = W (a lane gives w[r0 + l % 16][k]), B = the gathered input (column l % 16 is a
//             pixel), so D[i][j] has j = l % 16 along PIXELS, the contiguous axis of an NCHW output: the 16 lanes of a row
//             group store 64 contiguous bytes of y[n][co] wherever their 16 pixels lie in one image.
//   weights   ws[16][68], the staging of qdi_mm.h (weight_bucket, weight_step): thread t decodes the group of four [4 (t % 16), + 4) of row t / 16, one
//             bucket search per thread and tile, steps of 64 elements from there; fetch4 (loads only) before the MFMAs of the
//             slab before, finish4 after them.
//   gather    xs[64][260], K-MAJOR: row = column of the slab, 256 pixels + 4 floats of padding.  Each wave stages ITS OWN 64
//             pixels, lane = pixel, for the 64 columns of the slab: a load is 64 lanes x 4 bytes (at stride 1: 256 contiguous
//             bytes of an image row, up to row breaks), an LDS write 64 consecutive floats.  The split of a column into
//             (ci, a, b) is the same for all lanes and is carried on the scalar unit, one step per column (no division at all:
//             a tile starts at column 0); the split of a pixel into (n, p, q) is done once per lane and tile.  The second
//             buffer is REGISTERS: the 64 loads of slab s + 1 are issued -- each under its window test, so a padded position
//             is never loaded -- before the MFMAs of slab s, and become LDS contents after them, with zeros wherever the test
//             fails; the test is recomputed at the commit, not kept (64 bits of predicate per lane would be two more VGPRs
//             and as many v_cmp to extract them).
//   LDS reads 260 = 4 mod 64: lane l reads xs[16 q + 4 (l / 16) + jj][64 wave + 16 blk + l % 16], one ds_read_b32 -- the four
//             k-rows of a read fall on banks 16 apart and the 16 pixels on consecutive ones: conflict-free.  The weights are
//             one ds_read_b128 per group, as in k_linear_mm.
//   order     of an output element: slabs front to back, inside a slab the 16-column groups front to back, inside a group
//             jj = 0 .. 3, each MFMA adding its four products to the running accumulator; a last slab of fewer than 64
//             columns runs only the groups that hold a column.  A function of K alone.
//   offsets   of x and y are unsigned and wrap (a window that starts left of or above the image has a "negative" first
//             offset; the offsets that are LOADED are the true ones): 32 bits wide where x and y hold fewer than 2^31 elements
//             each, 64 bits otherwise -- one kernel, the width a by-value argument.
#include "qdi_mm.h"           // the weight pieces of the K walk; through it qdi_packed.h: Packed, describe, the decode, the host helpers

#include "../../../include/qd_infer_conv.h"

using namespace qd;

namespace {

constexpr int kPix = 256;              // output pixels of a tile: 64 per wave
constexpr int kXS = 260;               // floats per row of xs: 256 pixels + 4, so that k-rows 4 apart lie 16 banks apart

// By-value geometry of a call.
struct Conv {
    int64_t h, w, ow, ohow;  // of the image and of the output; oh ow
    int64_t chw;             // cin h w: elements of one image of x
    int64_t M;               // batch oh ow: output pixels
    int64_t m_chunks, tiles;
    int step_q, step_r;      // 64 = step_q bucket + step_r
    uint32_t kh, kw, sh, sw, ph, pw;     // none negative: unsigned, so that widening one to 64 bits costs no register
    int small;               // x and y below 2^31 elements (and every extent below 2^31): 32-bit offsets
};

// The tiles of one block.  U: the unsigned type of the offsets into x and y, S: its signed twin (window coordinates).
template <typename U, typename S>
__device__ __forceinline__ void conv_tiles(const Packed& P, const Conv& C, const float* x, const float* bias, float* y, const float* qtab,
                                           float* ws, float* xs, const int64_t* geo) {
    const int tid = threadIdx.x;
    const int wr = tid >> 4, wc = (tid & 15) << 2;                      // staging of W: the group of four [wc, wc + 4) of row wr of the slab
    const int lane = tid & 63, fr = lane & 15, fk = (lane >> 4) << 2;    // fragments: channel / pixel fr of a 16-block, columns fk .. fk + 3 of a group
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t N = P.rows, K = P.cols;
    const U M = (U)C.M, m_chunks = (U)C.m_chunks, tiles = (U)C.tiles;        // tiles <= cout M, the element count of y; + 511 fits U
    const uint32_t kh = C.kh, kw = C.kw;
    const U row_skip = (U)C.w - (U)kw;                                       // offset from (a, kw) to (a + 1, 0), less the step itself
    const U chan_skip = ((U)C.h - (U)kh) * (U)C.w;                                // and from (ci, kh, 0) to (ci + 1, 0, 0)
    float* const xw = xs + 64 * wave + lane;                             // staging: this lane's pixel, column j of the slab at xw[j kXS]
    const float* const xf = xs + fk * kXS + 64 * wave + fr;              // fragments: pixel fr of block blk, column 16 q + fk + jj at xf[(16 q + jj) kXS + 16 blk]

    for (U tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const U nt = tile / m_chunks;
        const U m0 = (tile - nt * m_chunks) * kPix;
        const int64_t r0 = (int64_t)nt * kRows;
        // What only per-lane arithmetic needs, once per tile, comes from LDS into VGPRs (see k_conv2d_mm) and is not held in SGPRs.
        const U ohow = (U)geo[0], ow = (U)geo[1], h = (U)geo[3], w = (U)geo[4];
        const bool wrow = r0 + wr < N;                                   // this thread's weight row exists
        const bool mine = m0 + 64 * wave < M;                            // this wave's 64 pixels hold one (wave-uniform)
        // As in k_linear_mm: a thread without a weight row or whose columns lie past K carries e, bkt and rem along; every USE is
        // under the same test in fetch and in commit.  Likewise a lane without a pixel (!valid) or a window position outside the
        // image carries an offset that is never turned into an address that is read.
        int64_t e = (r0 + wr) * K + wc;
        int64_t bkt, rem;
        weight_bucket(P, e, wrow && wc < K, bkt, rem);
        const U pix = m0 + 64 * wave + lane;
        const bool valid = pix < M;
        U img = 0, r = 0, xb = 0;                                        // image, pixel inside it, offset of the window's first element in x
        S ih0 = 0, iw0 = 0;                                              // the window's first row and column in the image
        if (valid) {
            img = pix / ohow;
            r = pix - img * ohow;
            const U p = r / ow, q = r - p * ow;
            ih0 = (S)(p * (U)geo[5] - (U)geo[7]);
            iw0 = (S)(q * (U)geo[6] - (U)geo[8]);
            xb = img * (U)geo[2] + (U)ih0 * w + (U)iw0;
        }
        f4 acc[4];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) acc[blk] = (f4){0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t ca = 0, cb = 0;                                             // (a, b) of the current slab's first column: wave-uniform ...
        U coff = 0;                                                      // ... and its offset (ci h + a) w + b inside an image
        uint32_t lo, hi;                                                 // the next slab between its loads and its LDS writes
        float a0, b0;
        float xn[kSlab];

        // One column on.  rowok: the window row of column (ci, a, .) lies inside the image, per lane, renewed when a changes.
        auto next_column = [&](uint32_t& a_, uint32_t& b_, U& c_, bool& rowok) {
            ++b_; ++c_;
            if (b_ == kw) {
                b_ = 0; c_ += row_skip;
                if (++a_ == kh) { a_ = 0; c_ += chan_skip; }
                rowok = valid && (U)ih0 + (U)a_ < h;
            }
        };

        // The loads of a slab of kl <= 64 columns, and nothing but loads (fetch4's words): all of them are in flight while the
        // MFMAs of the slab before run.  A position outside the image, a column past K and a lane without a pixel load nothing.
        auto fetch = [&](int kl) {
            if (wrow && kl - wc > 0) fetch4(P, e, bkt, lo, hi, a0, b0);
            if (!mine) return;
            uint32_t a_ = ca, b_ = cb;
            U c_ = coff;
            bool rowok = valid && (U)ih0 + (U)a_ < h;
#pragma unroll
            for (int j = 0; j < kSlab; ++j) {
                if (rowok && j < kl && (U)iw0 + (U)b_ < w) xn[j] = x[(U)(xb + c_)];
                next_column(a_, b_, c_, rowok);
            }
        };
        // The same slab from the registers into LDS, zeros wherever nothing was loaded; then (ca, cb, coff) are 64 columns on.
        auto commit = [&](int kl) {
            // weight_commit of qdi_mm.h, left written out: called from here the compiler schedules this kernel's prologue differently
            // (profiles/infer_mm_dedup_device_code.txt), and the device code is to stay what it was.
            const int nw = kl - wc;                                      // columns from this group's first to the end of the row
            float wv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (wrow && nw > 0) finish4(P, qtab, lo, hi, a0, b0, e, bkt, rem, nw < 4 ? nw : 4, wv);
            *(f4*)&ws[wr * kStride + wc] = (f4){wv[0], wv[1], wv[2], wv[3]};
            if (!mine) return;
            uint32_t a_ = ca, b_ = cb;
            U c_ = coff;
            bool rowok = valid && (U)ih0 + (U)a_ < h;
#pragma unroll
            for (int j = 0; j < kSlab; ++j) {
                const bool in = rowok && j < kl && (U)iw0 + (U)b_ < w;
                xw[j * kXS] = in ? xn[j] : 0.0f;
                next_column(a_, b_, c_, rowok);
            }
            ca = a_; cb = b_; coff = c_;
        };

        int64_t kleft = K;                                               // columns from the first of the slab to fetch to the end of the row
        int klp = 0;                                                     // columns of the slab that is in LDS
        for (;;) {
            const int kl = kleft < kSlab ? (int)kleft : kSlab;           // 0: no further slab
            if (kl > 0) fetch(kl);                                       // in flight during the MFMAs below
            if (klp > 0) {
                if (mine) {
                    const int groups = (klp + 15) >> 4;
                    for (int q = 0; q < groups; ++q) {
                        const f4 a = *(const f4*)&ws[fr * kStride + 16 * q + fk];
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj) {
#pragma unroll
                            for (int blk = 0; blk < 4; ++blk)
                                acc[blk] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[jj], xf[(16 * q + jj) * kXS + 16 * blk], acc[blk], 0, 0, 0);
                        }
                    }
                }
                __syncthreads();                                         // every wave is done with this slab before the next commit
            }
            if (kl <= 0) break;
            commit(kl);
            __syncthreads();
            weight_step(P, C.step_q, C.step_r, e, bkt, rem);
            klp = kl;
            kleft -= kSlab;
        }

        // D[i][j] of block blk: i = 4 (lane / 16) + v (channel inside the tile), j = lane % 16 (pixel 16 blk + j of the wave's 64,
        // whose image and position the lane that staged it knows).
        const U yb = img * (U)N * ohow + r;                              // y offset of (image, channel 0, pixel)
        float bv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int v = 0; v < 4; ++v)
            if (bias && mine && r0 + fk + v < N) bv[v] = bias[r0 + fk + v];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) {
            const U ybb = (U)__shfl((unsigned long long)yb, 16 * blk + fr);
            const int pv = __shfl((int)valid, 16 * blk + fr);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int64_t co = r0 + fk + v;
                if (mine && pv && co < N) y[(U)(ybb + (U)co * ohow)] = bias ? acc[blk][v] + bv[v] : acc[blk][v];
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_conv2d_mm(Packed P, Conv C, const float* x, const float* bias, float* y) {
    __shared__ float qtab[256];
    __shared__ __attribute__((aligned(16))) float ws[kRows * kStride];
    __shared__ __attribute__((aligned(16))) float xs[kSlab * kXS];
    // The geometry that enters per-lane arithmetic only (the split of a pixel, the window tests): nine numbers that would
    // otherwise sit in up to 14 SGPRs through the whole kernel, which has none to spare.
    __shared__ int64_t geo[9];
    if (threadIdx.x == 0) {
        geo[0] = C.ohow; geo[1] = C.ow; geo[2] = C.chw; geo[3] = C.h; geo[4] = C.w;
        geo[5] = C.sh; geo[6] = C.sw; geo[7] = C.ph; geo[8] = C.pw;
    }
    build_quotients(qtab, P.levels);                                     // ends with the barrier that publishes geo as well
    if (C.small) conv_tiles<uint32_t, int32_t>(P, C, x, bias, y, qtab, ws, xs, geo);
    else conv_tiles<uint64_t, int64_t>(P, C, x, bias, y, qtab, ws, xs, geo);
}

}  // namespace

extern "C" {

int qdc_abi_version(void) { return QDC_ABI_VERSION; }
const char* qdc_target_arch(void) { return "gfx950"; }

const char* qdc_error_string(int code) { return error_string(code, QDC_ERR_INVALID_ARGUMENT); }
int qdc_set_grid_cap(int blocks) { return set_grid_cap(blocks); }

int qdc_conv2d_packed_f32(const uint8_t* packed, const float* alpha, const float* beta, int64_t cout, int64_t cin, int kh, int kw,
                          int64_t bucket, int levels, int bits, const float* x, int64_t batch, int64_t h, int64_t w, int stride_h,
                          int stride_w, int pad_h, int pad_w, const float* bias, float* y, void* stream) {
    const int64_t lim = (int64_t)1 << 31;
    if (cin < 0 || batch < 0 || h < 0 || w < 0 || kh < 1 || kw < 1 || stride_h < 1 || stride_w < 1 || pad_h < 0 || pad_w < 0)
        return QDC_ERR_INVALID_ARGUMENT;
    int64_t K = 0, hp = 0, wp = 0, chw = 0, xn = 0, M = 0, yn = 0;
    if (__builtin_mul_overflow(cin, (int64_t)kh * kw, &K)) return QDC_ERR_INVALID_ARGUMENT;
    Packed P;
    if (!describe(P, packed, alpha, beta, cout, K, bucket, levels, bits)) return QDC_ERR_INVALID_ARGUMENT;
    if (misaligned(x) || misaligned(bias) || misaligned(y)) return QDC_ERR_INVALID_ARGUMENT;
    if (__builtin_add_overflow(h, 2 * (int64_t)pad_h, &hp) || __builtin_add_overflow(w, 2 * (int64_t)pad_w, &wp) || hp < kh || wp < kw)
        return QDC_ERR_INVALID_ARGUMENT;
    const int64_t oh = (hp - kh) / stride_h + 1, ow = (wp - kw) / stride_w + 1;
    // the element counts of x and y: a count with a factor 0 is 0 whatever the other factors are
    if (batch > 0 && cin > 0 &&
        (__builtin_mul_overflow(h, w, &chw) || __builtin_mul_overflow(chw, cin, &chw) || __builtin_mul_overflow(chw, batch, &xn)))
        return QDC_ERR_INVALID_ARGUMENT;
    if (batch == 0 || cout == 0) return 0;
    if (__builtin_mul_overflow(oh, ow, &M) || __builtin_mul_overflow(M, batch, &M) || __builtin_mul_overflow(M, cout, &yn))
        return QDC_ERR_INVALID_ARGUMENT;
    if (!y || (K > 0 && (!packed || !alpha || !beta)) || (xn > 0 && !x)) return QDC_ERR_INVALID_ARGUMENT;
    Conv C;
    C.h = h; C.w = w; C.ow = ow; C.ohow = M / batch; C.chw = chw; C.M = M;
    C.m_chunks = (M - 1) / kPix + 1;
    C.tiles = ((cout - 1) / kRows + 1) * C.m_chunks;                     // <= M cout: fits
    C.step_q = (int)(kSlab / P.bucket); C.step_r = (int)(kSlab % P.bucket);
    C.kh = kh; C.kw = kw; C.sh = stride_h; C.sw = stride_w; C.ph = pad_h; C.pw = pad_w;
    C.small = xn < lim && yn < lim && hp < lim && wp < lim;              // then M, oh ow, cin h w, p stride, q stride < 2^31 as well
    const int blocks = capped(C.tiles, (int64_t)device_cus() * 2);       // 71 KiB of LDS: two blocks per CU
    hipLaunchKernelGGL(k_conv2d_mm, dim3(blocks), dim3(256), 0, (hipStream_t)stream, P, C, x, bias, y);
    return (int)hipGetLastError();
}

}  // extern "C"
