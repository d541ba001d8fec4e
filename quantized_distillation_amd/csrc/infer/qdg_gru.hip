// qdg_gru.hip -- libqd_infer_gru.so: one GRU step from the packed recurrent weights (include/qd_infer_gru.h), gfx950.  Both
// products of the step go through v_mfma_f32_16x16x4_f32, each into a sum of its OWN -- the reset gate multiplies the recurrent
// half of the candidate, n = tanh(gi_n + r gh_n), so W_ih x and W_hh h may not meet in one accumulator as they do in
// k_lstm_cell_mm -- and the gate arithmetic is finished in the lane that holds both sums: one launch per step, nothing of the
// [batch, 3 hidden] products goes to memory unless the caller asks for it.  Nothing of the other libraries is linked in; the decode
// is the shared one of qdi_packed.h, unchanged, the weight pieces of the K walk and the MFMA loop those of qdi_mm.h.
//
// k_gru_cell_mm, one block of 256 threads (4 waves) per tile of 4 hidden units x 4 tile rows x up to 64 batch rows:
//   split     tiles = unit-tiles x batch-chunks, chunk fastest (the blocks that decode the same weight rows run next to each
//             other), strided over the grid.  Wave w owns the batch rows [16 w, 16 w + 16) of the chunk; a wave whose rows lie at
//             or past the batch skips the MFMAs.  No split-K, no atomics, no block waits for another.
//   row map   tile row 4 u + g, g < 3, is weight row g hidden + j0 + u (gate g: 0 = r, 1 = z, 2 = n): a GATHERED set of rows, `hidden`
//             rows apart, so every thread finds its group's bucket by one division per tile and part (weight_bucket).  Tile row
//             4 u + 3 is IDLE: its 16 decode threads issue no load and commit zeros, and its accumulator register is never read.
//   why idle  A = W (rows_mfma<true>), B = the activations: D[i][j] has i = 4 (l / 16) + v along the tile rows and j = l % 16 along
//             the batch, so the FOUR accumulator registers of a lane are the four tile rows of unit j0 + l / 16 for batch row
//             l % 16.  With a unit on four tile rows its r, z and n meet in ONE lane and the whole epilogue needs no cross-lane
//             exchange and no LDS, as in the LSTM.  5 units x 3 rows would fill 15 of the 16 MFMA rows, but a unit's gates would lie
//             in different lanes (rows 3 u .. 3 u + 2 straddle the groups of four).  The price is a quarter of the MFMA rows; it
//             costs no loads and no decodes.  The LSTM's times move with the number of slabs, not with the MFMA work (DESIGN.md
//             11.3); that the same holds here is supposed, not measured.
//   never     read the idle row: a zero weight row times an inf / NaN activation is NaN in that register.  gi and gh are sums over
//             real weight rows only, so no artifact of the tiling reaches an output.
//   K walk    two parts, W_ih against x and then W_hh against h (pre mode: W_hh alone, gi is loaded from `pre`), each walked as
//             k_linear_mm walks a weight: slabs of 64 columns through LDS -- ws[16][68], decoded once per tile and slab, thread t the
//             group [4 (t % 16), + 4) of tile row t / 16; acts[64][68], thread t the 16 columns [16 (t % 4), + 16) of batch row t / 4
//             -- the next slab held in registers (fetch4 before the MFMAs, finish4 after them), two barriers per slab.  Each part has
//             its own ragged last slab.  Between the parts the ONE running accumulator is copied out as gi and restarted at +0.0f
//             for gh (an acc[part] array indexed by the loop variable would be a dynamically indexed register array: scratch).  The
//             parts are an array of two in one kernel argument, read again per tile and part (two by-value descriptions spilled
//             SGPRs in k_lstm_cell_mm).
//   LDS reads rows_mfma of qdi_mm.h (there: the slab layout, the bucket search and step, the weight commit), A = W.
//   order     of a gi / gh element: slabs front to back, groups front to back, jj = 0 .. 3: a function of input / hidden alone.
#include "qdi_mm.h"           // the pieces of the K walk; through it qdi_packed.h: Packed, describe, the decode, the host helpers

#include "../../../include/qd_infer_gru.h"

using namespace qd;

namespace {

constexpr int kTile = 64;              // batch rows of a chunk
constexpr int kUnits = 4;              // hidden units of a tile: 4 units x (3 gates + 1 idle row) = kRows tile rows, one MFMA block
constexpr int kGates = 3;              // r, z, n

// One of the two products of a step: the weight, the activations it multiplies ([batch][P.cols]) and 64 = step_q bucket + step_r.
struct Part {
    Packed P;
    const float* act;
    int64_t step_q, step_r;
};
struct Parts { Part part[2]; };        // [0]: W_ih against x (cell mode only), [1]: W_hh against h

__device__ __forceinline__ float sigmoidf(float a) { return 1.0f / (1.0f + expf(-a)); }

__global__ __launch_bounds__(256) void k_gru_cell_mm(Parts parts, int64_t hidden, int64_t batch, const float* pre, const float* bias_ih,
                                                     const float* bias_hh, float* h_out, float* gates, int64_t chunks, int64_t tiles) {
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
    const float* h = parts.part[1].act;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t ut = tile / chunks;
        const int64_t j0 = ut * kUnits, i0 = (tile - ut * chunks) * kTile;
        const int brows = batch - i0 < kTile ? (int)(batch - i0) : kTile;   // batch rows of this chunk, >= 1
        const bool wrow = (wr & 3) < kGates && j0 + (wr >> 2) < hidden;   // this thread's tile row is a gate's (not the idle one) of a unit that exists
        const bool arow = srow < brows;                                  // this thread's batch row exists
        const bool mine = 16 * wave < brows;                             // this wave's 16 batch rows hold one (wave-uniform)
        const int64_t wrow_index = (int64_t)(wr & 3) * hidden + j0 + (wr >> 2);   // tile row 4 u + g is weight row g hidden + j0 + u
        f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};                                // the running sum of the current part ...
        f4 gi = {0.0f, 0.0f, 0.0f, 0.0f};                                 // ... and part 0's, copied out when it is complete

        // One part, as k_linear_mm walks a weight of pt.P.cols columns.  A thread without a weight row (!wrow: the idle row, or a
        // unit past `hidden`), without a batch row (!arow) or whose columns lie past K still carries e, ap, bkt and rem along: every
        // USE below is under the same wrow / arow / column test, in fetch and in commit alike, so none of them is ever turned
        // into an address that is read.
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
            // the same slab from the registers into LDS: zeros wherever nothing is to be read (the idle row among them)
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
            if (part == 0) {                                              // W_ih x is complete: it is gi, and gh starts at +0.0f
                gi = acc;
                acc = (f4){0.0f, 0.0f, 0.0f, 0.0f};
            }
        }

        // D[i][j]: i = 4 (lane / 16) + v = tile row: unit lane / 16, gate v < 3 (v = 3: the idle row, never read); j = lane % 16: batch
        // row inside the wave's 16-row block.  acc is gh now.
        const int64_t j = j0 + (lane >> 4), i = i0 + 16 * wave + fr;
        if (mine && j < hidden && i < batch) {
            float a[kGates], b[kGates];
#pragma unroll
            for (int v = 0; v < kGates; ++v) {
                const int64_t r = v * hidden + j;
                float t = gi[v];
                if (cell) {
                    if (bias_ih) t = t + bias_ih[r];
                } else {
                    t = pre[i * kGates * hidden + r];
                }
                float s = acc[v];
                if (bias_hh) s = s + bias_hh[r];
                a[v] = t;
                b[v] = s;
                if (gates) {
                    gates[(2 * i) * kGates * hidden + r] = t;
                    gates[(2 * i + 1) * kGates * hidden + r] = s;
                }
            }
            const float gr = sigmoidf(a[0] + b[0]), gz = sigmoidf(a[1] + b[1]);
            const float gn = tanhf(a[2] + gr * b[2]);
            h_out[i * hidden + j] = (1.0f - gz) * gn + gz * h[i * hidden + j];
        }
    }
}

}  // namespace

extern "C" {

int qdg_abi_version(void) { return QDG_ABI_VERSION; }
const char* qdg_target_arch(void) { return "gfx950"; }

const char* qdg_error_string(int code) { return error_string(code, QDG_ERR_INVALID_ARGUMENT); }
int qdg_set_grid_cap(int blocks) { return set_grid_cap(blocks); }

int qdg_gru_cell_packed_f32(const uint8_t* packed_ih, const float* alpha_ih, const float* beta_ih, int64_t bucket_ih, int levels_ih, int bits_ih,
                            const uint8_t* packed_hh, const float* alpha_hh, const float* beta_hh, int64_t bucket_hh, int levels_hh, int bits_hh,
                            int64_t hidden, int64_t input, const float* x, const float* pre, const float* h, int64_t batch, const float* bias_ih,
                            const float* bias_hh, float* h_out, float* gates, void* stream) {
    const bool cell = pre == nullptr;
    int64_t rows = 0, t = 0;
    if (hidden < 0 || batch < 0 || (cell && input < 0) || __builtin_mul_overflow(hidden, (int64_t)kGates, &rows)) return QDG_ERR_INVALID_ARGUMENT;
    if (__builtin_mul_overflow(batch, rows, &t) || __builtin_mul_overflow(t, (int64_t)2, &t) || (cell && __builtin_mul_overflow(batch, input, &t)))
        return QDG_ERR_INVALID_ARGUMENT;
    if (misaligned(x) || misaligned(pre) || misaligned(h) || misaligned(bias_ih) || misaligned(bias_hh) || misaligned(h_out) || misaligned(gates))
        return QDG_ERR_INVALID_ARGUMENT;
    if ((x && pre) || (pre && bias_ih)) return QDG_ERR_INVALID_ARGUMENT;
    Parts parts = {};
    Part &ih = parts.part[0], &hh = parts.part[1];
    if (!describe(hh.P, packed_hh, alpha_hh, beta_hh, rows, hidden, bucket_hh, levels_hh, bits_hh)) return QDG_ERR_INVALID_ARGUMENT;
    if (cell && !describe(ih.P, packed_ih, alpha_ih, beta_ih, rows, input, bucket_ih, levels_ih, bits_ih)) return QDG_ERR_INVALID_ARGUMENT;
    if (batch == 0 || hidden == 0) return 0;
    if (!x && !pre) return QDG_ERR_INVALID_ARGUMENT;
    if (!h || !h_out || h_out == h || !packed_hh || !alpha_hh || !beta_hh) return QDG_ERR_INVALID_ARGUMENT;
    if (cell && input > 0 && (!packed_ih || !alpha_ih || !beta_ih)) return QDG_ERR_INVALID_ARGUMENT;
    hh.act = h; hh.step_q = kSlab / hh.P.bucket; hh.step_r = kSlab % hh.P.bucket;
    if (cell) { ih.act = x; ih.step_q = kSlab / ih.P.bucket; ih.step_r = kSlab % ih.P.bucket; }
    const int64_t chunks = (batch - 1) / kTile + 1;
    const int64_t tiles = ((hidden - 1) / kUnits + 1) * chunks;         // <= batch hidden: fits
    const int blocks = capped(tiles, (int64_t)device_cus() * 8);
    hipLaunchKernelGGL(k_gru_cell_mm, dim3(blocks), dim3(256), 0, (hipStream_t)stream, parts, hidden, batch, pre, bias_ih, bias_hh, h_out, gates, chunks,
                       tiles);
    return (int)hipGetLastError();
}

}  // extern "C"
