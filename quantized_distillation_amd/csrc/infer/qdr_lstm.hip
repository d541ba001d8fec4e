// qdr_lstm.hip -- libqd_infer_rnn.so: one LSTM step from the packed recurrent weights (include/qd_infer_rnn.h), gfx950.  Both
// products of the step go through v_mfma_f32_16x16x4_f32 into one accumulator and the gate arithmetic is finished in the lane
// that holds the accumulator: one launch per step, nothing of the [batch, 4 hidden] pre-activations goes to memory unless the
// caller asks for it.  Nothing of the other libraries is linked in; the decode is the shared one of qdi_packed.h, unchanged,
// the weight pieces of the K walk and the MFMA loop those of qdi_mm.h.
//
// k_lstm_cell_mm, one block of 256 threads (4 waves) per tile of 4 hidden units x 4 gates (16 weight rows) x up to 64 batch rows:
//   split     tiles = unit-tiles x batch-chunks, chunk fastest (the blocks that decode the same 16 weight rows run next to each
//             other), strided over the grid.  Tile row 4 u + g is weight row g hidden + j0 + u: a GATHERED set of rows, `hidden` rows
//             apart, so every thread finds its group's bucket by one division per tile and part, as k_linear_mm does.  Wave w
//             owns the batch rows [16 w, 16 w + 16) of the chunk; a wave whose rows lie at or past the batch skips the MFMAs.
//             No split-K, no atomics, no block waits for another.
//   roles     A = W (a lane gives w[tile row l % 16][k]), B = the activations (x or h [i0 + 16 w + l % 16][k]), so D[i][j] has
//             i = 4 (l / 16) + v along the tile rows and j = l % 16 along the batch: the FOUR accumulator registers of a lane are
//             the gates i, f, g, o of unit j0 + l / 16 for batch row l % 16.  The epilogue is in-lane: no cross-lane exchange, no
//             LDS; a lane loads one c and stores one c', one h' and, if asked, four gates.
//   K walk    two parts, W_ih against x and then W_hh against h (pre mode: W_hh alone), each walked as k_linear_mm walks a weight:
//             slabs of 64 columns through LDS -- ws[16][68], decoded once per tile and slab, thread t the group [4 (t % 16), + 4) of
//             tile row t / 16; acts[64][68], thread t the 16 columns [16 (t % 4), + 16) of batch row t / 4 -- the next slab held in
//             registers (fetch4 before the MFMAs, finish4 after them), two barriers per slab.  Each part has its own ragged last
//             slab; a slab never straddles the parts.  The description, the quotient table, the bucket state and the activation
//             pointer switch once per tile, between the parts; the accumulator runs through.
//   LDS reads rows_mfma of qdi_mm.h (there: the slab layout, the bucket search and step, the weight commit), A = W.
//   order     of a pre-activation: the parts in turn, slabs front to back, groups front to back, jj = 0 .. 3: a function of
//             input and hidden alone.
#include "qdi_mm.h"           // the pieces of the K walk; through it qdi_packed.h: Packed, describe, the decode, the host helpers

#include "../../../include/qd_infer_rnn.h"

using namespace qd;

namespace {

constexpr int kTile = 64;              // batch rows of a chunk
constexpr int kUnits = 4;              // hidden units of a tile: 4 units x 4 gates = kRows weight rows, one MFMA block

// One of the two products of a step: the weight, the activations it multiplies ([batch][P.cols]) and 64 = step_q bucket + step_r.
struct Part {
    Packed P;
    const float* act;
    int64_t step_q, step_r;
};
struct Parts { Part part[2]; };        // [0]: W_ih against x (cell mode only), [1]: W_hh against h

__device__ __forceinline__ float sigmoidf(float a) { return 1.0f / (1.0f + expf(-a)); }

__global__ __launch_bounds__(256) void k_lstm_cell_mm(Parts parts, int64_t hidden, int64_t batch, const float* pre, const float* c,
                                                      const float* bias_ih, const float* bias_hh, float* h_out, float* c_out, float* gates,
                                                      int64_t chunks, int64_t tiles) {
    __shared__ float qtabs[2][256];
    __shared__ __attribute__((aligned(16))) float ws[kRows * kStride];
    __shared__ __attribute__((aligned(16))) float acts[kTile * kStride];
    const bool cell = pre == nullptr;                                   // cell mode: both parts; pre mode: W_hh alone
    if (cell) build_quotients(qtabs[0], parts.part[0].P.levels);
    build_quotients(qtabs[1], parts.part[1].P.levels);
    const int tid = threadIdx.x;
    const int wr = tid >> 4, wc = (tid & 15) << 2;                      // staging of W: the group of four [wc, wc + 4) of tile row wr of the slab
    const int srow = tid >> 2, scol = (tid & 3) << 4;                   // staging of x / h: batch row srow, the four groups [scol + 4 j, + 4)
    const int lane = tid & 63, fr = lane & 15, fk = (lane >> 4) << 2;    // fragments: row fr of a 16-row block, columns fk .. fk + 3 of a group
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t ut = tile / chunks;
        const int64_t j0 = ut * kUnits, i0 = (tile - ut * chunks) * kTile;
        const int brows = batch - i0 < kTile ? (int)(batch - i0) : kTile;   // batch rows of this chunk, >= 1
        const bool wrow = j0 + (wr >> 2) < hidden, arow = srow < brows;  // this thread's unit / batch row exists
        const bool mine = 16 * wave < brows;                             // this wave's 16 batch rows hold one (wave-uniform)
        const int64_t wrow_index = (int64_t)(wr & 3) * hidden + j0 + (wr >> 2);   // tile row 4 u + g is weight row g hidden + j0 + u
        f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};

        // One part, as k_linear_mm walks a weight of pt.P.cols columns; acc runs through.  A thread without a unit (!wrow), without
        // a batch row (!arow) or whose columns lie past K still carries e, ap, bkt and rem along: every USE below is under the same
        // wrow / arow / column test, in fetch and in commit alike, so none of them is ever turned into an address that is read.
        for (int part = cell ? 0 : 1; part < 2; ++part) {
            const Part& pt = parts.part[part];                            // kernel arguments: read again per tile and part, not kept
            const float* qtab = qtabs[part];
            const Packed& P = pt.P;
            const int64_t K = P.cols;
            int64_t e = wrow_index * K + wc;                              // its group's first element in the current slab ...
            const float* ap = pt.act + (i0 + srow) * K + scol;
            int64_t bkt, rem;                                             // ... and that element's bucket
            weight_bucket(P, e, wrow && wc < K, bkt, rem);
            uint32_t lo, hi;                                              // the next slab between its loads and its LDS writes
            float a0, b0;
            f4 an[4];

            // the loads of a slab of kl <= 64 columns, and nothing but loads: all in flight during the MFMAs of the slab before
            auto fetch = [&](int kl) {
                if (wrow && kl - wc > 0) fetch4(P, e, bkt, lo, hi, a0, b0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (arow && kl - scol - 4 * j >= 4) {
                        const f4u u = *(const f4u*)(ap + 4 * j);
                        an[j] = (f4){u.x, u.y, u.z, u.w};
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
                    if (arow && nv >= 4) v = an[j];
                    if (arow && nv > 0 && nv < 4) {                       // the ragged group: nothing past act[i][K)
                        v.x = ap[4 * j];
                        if (nv > 1) v.y = ap[4 * j + 1];
                        if (nv > 2) v.z = ap[4 * j + 2];
                    }
                    *(f4*)&acts[srow * kStride + scol + 4 * j] = v;
                }
            };

            int64_t kleft = K;                                            // columns from the current slab's first to the end of the row
            if (kleft > 0) fetch(kleft < kSlab ? (int)kleft : kSlab);
            while (kleft > 0) {
                const int kl = kleft < kSlab ? (int)kleft : kSlab;
                commit(kl);
                __syncthreads();
                kleft -= kSlab;
                if (kleft > 0) {
                    weight_step(P, pt.step_q, pt.step_r, e, bkt, rem);
                    ap += kSlab;
                    fetch(kleft < kSlab ? (int)kleft : kSlab);            // in flight during the MFMAs below
                }
                if (mine) rows_mfma<true>(ws, acts, kl, fr, fk, wave, acc);
                __syncthreads();                                          // every wave is done with this slab before the next commit (of either part)
            }
        }

        // D[i][j]: i = 4 (lane / 16) + v = tile row: unit lane / 16, gate v; j = lane % 16: batch row inside the wave's 16-row block
        const int64_t j = j0 + (lane >> 4), i = i0 + 16 * wave + fr;
        if (mine && j < hidden && i < batch) {
            float a[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int64_t r = v * hidden + j;
                float t = acc[v];
                if (cell) {
                    if (bias_ih) t = t + bias_ih[r];
                } else {
                    t = t + pre[i * 4 * hidden + r];
                }
                if (bias_hh) t = t + bias_hh[r];
                a[v] = t;
                if (gates) gates[i * 4 * hidden + r] = t;
            }
            const float gi = sigmoidf(a[0]), gf = sigmoidf(a[1]), gg = tanhf(a[2]), go = sigmoidf(a[3]);
            const float cn = gf * c[i * hidden + j] + gi * gg;
            c_out[i * hidden + j] = cn;
            h_out[i * hidden + j] = go * tanhf(cn);
        }
    }
}

}  // namespace

extern "C" {

int qdr_abi_version(void) { return QDR_ABI_VERSION; }
const char* qdr_target_arch(void) { return "gfx950"; }

const char* qdr_error_string(int code) { return error_string(code, QDR_ERR_INVALID_ARGUMENT); }
int qdr_set_grid_cap(int blocks) { return set_grid_cap(blocks); }

int qdr_lstm_cell_packed_f32(const uint8_t* packed_ih, const float* alpha_ih, const float* beta_ih, int64_t bucket_ih, int levels_ih, int bits_ih,
                             const uint8_t* packed_hh, const float* alpha_hh, const float* beta_hh, int64_t bucket_hh, int levels_hh, int bits_hh,
                             int64_t hidden, int64_t input, const float* x, const float* pre, const float* h, const float* c, int64_t batch,
                             const float* bias_ih, const float* bias_hh, float* h_out, float* c_out, float* gates, void* stream) {
    const bool cell = pre == nullptr;
    int64_t rows = 0, t = 0;
    if (hidden < 0 || batch < 0 || (cell && input < 0) || __builtin_mul_overflow(hidden, (int64_t)4, &rows)) return QDR_ERR_INVALID_ARGUMENT;
    if (__builtin_mul_overflow(batch, rows, &t) || (cell && __builtin_mul_overflow(batch, input, &t))) return QDR_ERR_INVALID_ARGUMENT;
    if (misaligned(x) || misaligned(pre) || misaligned(h) || misaligned(c) || misaligned(bias_ih) || misaligned(bias_hh) || misaligned(h_out) ||
        misaligned(c_out) || misaligned(gates))
        return QDR_ERR_INVALID_ARGUMENT;
    if ((x && pre) || (pre && bias_ih)) return QDR_ERR_INVALID_ARGUMENT;
    Parts parts = {};
    Part &ih = parts.part[0], &hh = parts.part[1];
    if (!describe(hh.P, packed_hh, alpha_hh, beta_hh, rows, hidden, bucket_hh, levels_hh, bits_hh)) return QDR_ERR_INVALID_ARGUMENT;
    if (cell && !describe(ih.P, packed_ih, alpha_ih, beta_ih, rows, input, bucket_ih, levels_ih, bits_ih)) return QDR_ERR_INVALID_ARGUMENT;
    if (batch == 0 || hidden == 0) return 0;
    if (!x && !pre) return QDR_ERR_INVALID_ARGUMENT;
    if (!h || !c || !h_out || !c_out || h_out == h || !packed_hh || !alpha_hh || !beta_hh) return QDR_ERR_INVALID_ARGUMENT;
    if (cell && input > 0 && (!packed_ih || !alpha_ih || !beta_ih)) return QDR_ERR_INVALID_ARGUMENT;
    hh.act = h; hh.step_q = kSlab / hh.P.bucket; hh.step_r = kSlab % hh.P.bucket;
    if (cell) { ih.act = x; ih.step_q = kSlab / ih.P.bucket; ih.step_r = kSlab % ih.P.bucket; }
    const int64_t chunks = (batch - 1) / kTile + 1;
    const int64_t tiles = ((hidden - 1) / kUnits + 1) * chunks;         // <= batch hidden: fits
    const int blocks = capped(tiles, (int64_t)device_cus() * 8);
    hipLaunchKernelGGL(k_lstm_cell_mm, dim3(blocks), dim3(256), 0, (hipStream_t)stream, parts, hidden, batch, pre, c, bias_ih, bias_hh, h_out, c_out,
                       gates, chunks, tiles);
    return (int)hipGetLastError();
}

}  // extern "C"
