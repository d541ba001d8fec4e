// qdi_mm.h -- what the packed-weight MFMA kernels share of their K walk, written down once: k_linear_mm (qdm_linear.hip),
// k_lstm_cell_mm (qdr_lstm.hip, once per part) and the weight half of k_conv2d_mm (qdc_conv2d.hip).  All three multiply a tile
// of 16 weight rows, decoded from the packed stream, by activations through v_mfma_f32_16x16x4_f32, 64 columns of K (a "slab")
// at a time.
//
//   ws        ws[16][68], the weights of a slab, decoded ONCE per tile and slab: thread t of 256 decodes the group of four
//             [4 (t % 16), + 4) of tile row t / 16.  One bucket search per thread and walk (weight_bucket), steps of 64 elements
//             from there (weight_step).
//   xs        xs[64][68], the row-major activations of a slab (Linear's x, the LSTM's x or h; the convolution gathers its own,
//             K-major): thread t stages the 16 columns [16 (t % 4), + 16) of row t / 4, 16-byte global loads at any 4-byte
//             phase, 64 contiguous bytes of a row per thread; the 16 lanes of a b128 LDS write cover all 64 banks.
//   registers the second buffer is REGISTERS, not LDS: slab s + 1's loads (two stream words, alpha, beta, 16 activations: 20
//             VGPRs) are issued before slab s's MFMAs and become LDS contents after them, with two barriers per slab.  A
//             kernel's fetch() holds loads ONLY -- fetch4 of qdi_packed.h and its activations, no instruction that consumes a
//             loaded value -- so none of them is waited for before the MFMAs; its commit() writes zeros wherever nothing is
//             to be read (weight_commit for the weights).
//   LDS reads a row stride of 68 floats; lane l reads the FOUR floats [l % 16][16 q + 4 (l / 16), + 4) of a 16-column group as
//             one ds_read_b128 and feeds them to four MFMAs: MFMA jj of group q multiplies the columns 16 q + jj +
//             {0, 4, 8, 12}.  68 r mod 64 = 4 r: the 16 lanes a b128 read serves per cycle cover all 64 banks (rows_mfma).
//   order     of an output element: slabs front to back, inside a slab the 16-column groups front to back, inside a group
//             jj = 0 .. 3, each MFMA adding its four products to the running accumulator; a last slab of fewer than 64
//             columns runs only the groups that hold a column.  A function of K alone.
//
// Free functions over the caller's own locals, not a struct with methods: with the walk's state (lo, hi, a0, b0, e, bkt, rem) in
// a struct the compiler gave k_linear_mm the same instructions with two VGPRs exchanged.  What is here is what could be shared
// with the device code of every kernel byte for byte what it was (profiles/infer_mm_dedup_device_code.txt).  What is NOT
// here, and stays written out in k_linear_mm and k_lstm_cell_mm: the staging of the 16 activation columns (both halves) and
// the slab loop around it.  As functions of this header they compile to other instructions in k_linear_mm -- the column
// tests kl - scol - 4 j come out associated differently -- and a change of a kernel's code needs a measurement, which this
// header's introduction did not take.  Whoever writes the next kernel of the family: copy those two from k_linear_mm, guards
// (xrow, nv) included.
// Unnamed namespace for the reason qdi_packed.h gives.
#pragma once

#include "qdi_packed.h"

namespace {

constexpr int kSlab = 64;              // columns of a slab
constexpr int kRows = 16;              // weight rows of a tile: one MFMA block
constexpr int kStride = 68;            // floats per LDS row of ws and xs: 16-byte aligned rows, conflict-free operand reads (above)

// The bucket of e, the first element of this thread's group in the first slab, as k_embedding finds it -- under the caller's
// liveness test (its weight row exists and wc < K); 0, 0 otherwise, stepped on and never used.
__device__ __forceinline__ void weight_bucket(const Packed& P, int64_t e, bool live, int64_t& bkt, int64_t& rem) {
    bkt = 0; rem = 0;
    if (live) divmod(e, P.bucket, P.small, bkt, rem);
}

// The same group from the registers into ws: one f4 store, zeros where the row or the columns do not exist.
__device__ __forceinline__ void weight_commit(const Packed& P, const float* qtab, float* ws, bool wrow, int kl, int wr, int wc, uint32_t lo, uint32_t hi,
                                              float a0, float b0, int64_t e, int64_t bkt, int64_t rem) {
    const int nw = kl - wc;                                              // columns from this group's first to the end of the row
    float w[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (wrow && nw > 0) finish4(P, qtab, lo, hi, a0, b0, e, bkt, rem, nw < 4 ? nw : 4, w);
    *(f4*)&ws[wr * kStride + wc] = (f4){w[0], w[1], w[2], w[3]};
}

// 64 columns on: the bucket of the next slab's group.  64 = step_q bucket + step_r.
__device__ __forceinline__ void weight_step(const Packed& P, int64_t step_q, int64_t step_r, int64_t& e, int64_t& bkt, int64_t& rem) {
    bkt += step_q; rem += step_r;
    if (rem >= P.bucket) { rem -= P.bucket; ++bkt; }
    e += kSlab;
}

// The MFMAs of one wave over a committed slab of kl columns: its 16 rows of xs against the 16 rows of ws.  kWeightIsA: A = W,
// so D[i][j] has i along the weight rows (the LSTM: the four gates of a unit in one lane); otherwise A = the activations and j
// runs along the weight rows (Linear: 16 lanes store 64 contiguous bytes of a row of y).
template <bool kWeightIsA>
__device__ __forceinline__ void rows_mfma(const float* ws, const float* xs, int kl, int fr, int fk, int wave, f4& acc) {
    const int groups = (kl + 15) >> 4;
    for (int q = 0; q < groups; ++q) {
        const f4 w = *(const f4*)&ws[fr * kStride + 16 * q + fk];
        const f4 x = *(const f4*)&xs[(16 * wave + fr) * kStride + 16 * q + fk];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
            acc = kWeightIsA ? __builtin_amdgcn_mfma_f32_16x16x4f32(w[jj], x[jj], acc, 0, 0, 0)
                             : __builtin_amdgcn_mfma_f32_16x16x4f32(x[jj], w[jj], acc, 0, 0, 0);
    }
}

}  // namespace
