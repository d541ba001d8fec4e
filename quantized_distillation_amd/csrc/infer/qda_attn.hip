// qda_attn.hip -- libqd_infer_attn.so: one Luong global-attention step of a decoder whose output projection is a packed weight
// (include/qd_infer_attn.h), gfx950.  Two kernels, one launch each: k_attn_context (scores, masked softmax and context of a
// batch row, the scores never leaving LDS) and k_attn_out_mm (tanh(W_out [ctx ; x] + bias) with the packed [dim][2 dim] weight
// walked in two parts, so [ctx ; x] is never made).  Nothing of the other libraries is linked in; the decode is the shared one of
// qdi_packed.h, unchanged, the weight pieces of the K walk and the MFMA loop those of qdi_mm.h.
//
// k_attn_context, one block of 256 threads (4 waves) per batch row.  Per row this is a GEMV (S x dim by dim) and a weighted sum
// of S rows: there is no second operand dimension to fill a matrix instruction with, so none is used.
//   split     batch rows strided over the grid; a block does everything of its row, so no atomics and no block waits for another.
//   LDS       dynamic: red[16] (the two cross-wave reductions), qs[ceil4(dim)] (the query, staged once per row, zeros past
//             dim), sc[ceil4(S)] (score, then p, then align of position s) and, on the resident path, rows[S][ceil4(dim)].
//   scores    wave w takes the positions w, w + 4, ...; lane l the column groups [4 (l + 64 t), + 4): one 16-byte load at 4-byte
//             alignment per group (a wave reads 1 KiB of a row per instruction), q from LDS as one b128 read, four fmaf into
//             the lane's partial sum; the row's ragged last group is read float by float and never past dim.  One xor tree
//             over the wave; lane 0 writes sc[s].
//   softmax   thread t the positions t, t + 256, ...: max (xor tree per wave, the four through red), p = expf(score - m) and
//             their sum (the same tree, ((w0 + w1) + w2) + w3), align = p / l back into sc and out to memory, +0.0f from len on.
//   context   thread t owns the column groups t, t + 256, ... and walks s = 0 .. len - 1 in order: align_s from LDS (a
//             broadcast read), the group of row s as one 16-byte load -- 256 threads read 4 KiB contiguous of a row --, four fmaf.
//   resident  values == keys and S ceil4(dim) floats fit next to qs and sc (QDA_CONTEXT_LDS_LIMIT: the 160 KiB of a gfx950
//             workgroup): the score pass writes every group it loads to rows[s] and the context pass reads it from there, so the
//             source is read from memory once.  The same floats in the same order: the same bits.  Chosen on the host.
//   order     functions of dim and len alone (the header words them); nothing depends on batch, the grid or the path.
//   padding   no address at or past position len of a row is formed into a load.
//   considered, not built: at dim = 500 the context pass keeps 125 of 256 threads busy; splitting s over the two thread halves
//             with a fixed combine would use them all at the price of a second order of summation to describe.
//
// k_attn_out_mm, one block of 256 threads per tile of 16 weight rows x up to 64 batch rows: k_linear_mm (qdm_linear.hip) with a
// K walk of TWO parts over ONE weight.
//   split     tiles = row-tiles x batch-chunks, chunk fastest, strided over the grid.  Wave w owns the batch rows [16 w, + 16) of
//             the chunk; a wave whose rows lie at or past the batch skips the MFMAs.  No split-K, no atomics.
//   operands  A = the activations, B = W^T (rows_mfma<false>): D[i][j] has j = l % 16 along the weight rows, so 16 lanes store 64
//             contiguous bytes of a row of attn_h.
//   K walk    part 0: the columns [0, dim) of the 16 rows against ctx; part 1: the columns [dim, 2 dim) against x.  Each part is
//             walked as k_linear_mm walks a weight of dim columns -- ws[16][68], xs[64][68], the next slab held in registers
//             (fetch4 before the MFMAs, finish4 after them), two barriers per slab -- with a ragged last slab of its OWN: a slab
//             never straddles the two sources.  A thread's first element in part p is r 2 dim + p dim + wc: one weight_bucket
//             division per thread, tile and part, steps of 64 from there.  The accumulator runs through both parts.  The
//             activations of a part are read from the kernel argument `acts` per tile and part (two by-value descriptions
//             spilled SGPRs in k_lstm_cell_mm).
//   epilogue  in the lane that holds the sum: + bias, the optional store of pre, tanhf, store.
//   order     of a sum: part 0 then part 1, slabs, groups, jj = 0 .. 3: a function of dim alone.
#include "qdi_mm.h"           // the pieces of the K walk; through it qdi_packed.h: Packed, describe, the decode, the host helpers

#include "../../../include/qd_infer_attn.h"

using namespace qd;

namespace {

constexpr int kTile = 64;              // batch rows of a chunk (k_attn_out_mm)
constexpr int kRed = 16;               // floats at the front of k_attn_context's LDS: [0, 4) the waves' maxima, [4, 8) their sums

// The group of four [c, c + 4) of a row of `dim` floats: one 16-byte load where all four exist, float by float (zeros past the
// end) for the row's ragged last group.  c < dim.
__device__ __forceinline__ f4 load_group(const float* row, int c, int dim) {
    const int nv = dim - c;
    if (nv >= 4) {
        const f4u u = *(const f4u*)(row + c);
        return (f4){u.x, u.y, u.z, u.w};
    }
    f4 v = {row[c], 0.0f, 0.0f, 0.0f};
    if (nv > 1) v.y = row[c + 1];
    if (nv > 2) v.z = row[c + 2];
    return v;
}

__device__ __forceinline__ void store_group(float* row, int c, int dim, f4 v) {
    const int nv = dim - c;
    if (nv >= 4) {
        *(f4u*)(row + c) = (f4u){v.x, v.y, v.z, v.w};
        return;
    }
    row[c] = v.x;
    if (nv > 1) row[c + 1] = v.y;
    if (nv > 2) row[c + 2] = v.z;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d);
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d));
    return v;
}

__global__ __launch_bounds__(256) void k_attn_context(const float* q, const float* keys, const float* values, const int64_t* lengths, int64_t batch,
                                                      int S, int dim, int resident, float* align, float* ctx) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int ldim = (dim + 3) & ~3, groups = ldim >> 2;
    float* red = lds;
    float* qs = lds + kRed;
    float* sc = qs + ldim;
    float* rows = sc + ((S + 3) & ~3);                                   // resident path only: [S][ldim]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int64_t b = blockIdx.x; b < batch; b += gridDim.x) {
        const int64_t want = lengths ? lengths[b] : (int64_t)S;
        const int len = want < 0 ? 0 : want > S ? S : (int)want;         // the same for every thread of the block
        float* arow = align + b * S;
        float* crow = ctx + b * dim;
        if (len == 0) {                                                  // a row masked everywhere: NaN, and nothing of it is read
            const float nan = __builtin_nanf("");
            for (int s = tid; s < S; s += 256) arow[s] = nan;
            for (int k = tid; k < dim; k += 256) crow[k] = nan;
            continue;
        }
        for (int g = tid; g < groups; g += 256) *(f4*)&qs[4 * g] = load_group(q + b * dim, 4 * g, dim);
        __syncthreads();

        // scores: a wave per position, a lane per column group
        const float* kb = keys + b * S * dim;
        for (int s = wave; s < len; s += 4) {
            const float* kr = kb + (int64_t)s * dim;
            float part = 0.0f;
            for (int g = lane; g < groups; g += 64) {
                const f4 k = load_group(kr, 4 * g, dim);
                const f4 qq = *(const f4*)&qs[4 * g];
                if (resident) *(f4*)&rows[s * ldim + 4 * g] = k;
                part = fmaf(qq.x, k.x, part);
                part = fmaf(qq.y, k.y, part);
                part = fmaf(qq.z, k.z, part);
                part = fmaf(qq.w, k.w, part);
            }
            part = wave_sum(part);
            if (lane == 0) sc[s] = part;
        }
        __syncthreads();

        // softmax over sc[0 .. len): a thread only ever touches its own positions t, t + 256, ... of sc
        float m = -__builtin_inff();
        for (int s = tid; s < len; s += 256) m = fmaxf(m, sc[s]);
        m = wave_max(m);
        if (lane == 0) red[wave] = m;
        __syncthreads();
        m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        float l = 0.0f;
        for (int s = tid; s < len; s += 256) {
            const float p = expf(sc[s] - m);
            sc[s] = p;
            l = l + p;
        }
        l = wave_sum(l);
        if (lane == 0) red[4 + wave] = l;
        __syncthreads();
        l = ((red[4] + red[5]) + red[6]) + red[7];
        for (int s = tid; s < S; s += 256) {
            float a = 0.0f;
            if (s < len) {
                a = sc[s] / l;
                sc[s] = a;
            }
            arow[s] = a;
        }
        __syncthreads();

        // context: a thread per column group, the positions in order
        const float* vb = values + b * S * dim;
        for (int g = tid; g < groups; g += 256) {
            const f4 v0 = resident ? *(const f4*)&rows[4 * g] : load_group(vb, 4 * g, dim);
            const float a0 = sc[0];
            f4 acc = {a0 * v0.x, a0 * v0.y, a0 * v0.z, a0 * v0.w};
#pragma unroll 4
            for (int s = 1; s < len; ++s) {
                const f4 v = resident ? *(const f4*)&rows[s * ldim + 4 * g] : load_group(vb + (int64_t)s * dim, 4 * g, dim);
                const float a = sc[s];
                acc.x = fmaf(a, v.x, acc.x);
                acc.y = fmaf(a, v.y, acc.y);
                acc.z = fmaf(a, v.z, acc.z);
                acc.w = fmaf(a, v.w, acc.w);
            }
            store_group(crow, 4 * g, dim, acc);
        }
        // the next row's first write to sc or rows lies behind the barrier after its qs staging, which every thread reaches only
        // after this context pass; qs and red[0 .. 4) are not read here
    }
}

struct Acts { const float* act[2]; };  // what part p of the weight's columns multiplies: [0] ctx, [1] x, each [batch][dim]

__global__ __launch_bounds__(256) void k_attn_out_mm(Packed P, Acts acts, int64_t batch, const float* bias, float* attn_h, float* pre, int64_t chunks,
                                                     int64_t tiles, int64_t step_q, int64_t step_r /* 64 = step_q bucket + step_r */) {
    __shared__ float qtab[256];
    __shared__ __attribute__((aligned(16))) float ws[kRows * kStride];
    __shared__ __attribute__((aligned(16))) float xs[kTile * kStride];
    build_quotients(qtab, P.levels);
    const int tid = threadIdx.x;
    const int wr = tid >> 4, wc = (tid & 15) << 2;                      // staging of W: the group of four [wc, wc + 4) of row wr of the slab
    const int srow = tid >> 2, scol = (tid & 3) << 4;                   // staging of ctx / x: batch row srow, the four groups [scol + 4 j, + 4)
    const int lane = tid & 63, fr = lane & 15, fk = (lane >> 4) << 2;    // fragments: row fr of a 16-row block, columns fk .. fk + 3 of a group
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t N = P.rows, K = N;                                     // W_out[dim][2 dim]: dim rows, dim columns per part
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t nt = tile / chunks;
        const int64_t r0 = nt * kRows, i0 = (tile - nt * chunks) * kTile;
        const int brows = batch - i0 < kTile ? (int)(batch - i0) : kTile;   // batch rows of this chunk, >= 1
        const bool wrow = r0 + wr < N, xrow = srow < brows;              // this thread's weight row / batch row exists
        const bool mine = 16 * wave < brows;                             // this wave's 16 batch rows hold one (wave-uniform)
        f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};                                // one sum through both parts

        // One part, as k_linear_mm walks a weight of K columns.  A thread without a weight row (!wrow), without a batch row (!xrow)
        // or whose columns lie past K still carries e, xp, bkt and rem along: every USE below is under the same wrow / xrow /
        // column test, in fetch and in commit alike, so none of them is ever turned into an address that is read.
        for (int part = 0; part < 2; ++part) {
            int64_t e = (r0 + wr) * P.cols + part * K + wc;               // its group's first element in the part's first slab ...
            const float* xp = acts.act[part] + (i0 + srow) * K + scol;    // the kernel argument: read again per tile and part
            int64_t bkt, rem;                                             // ... and that element's bucket
            weight_bucket(P, e, wrow && wc < K, bkt, rem);
            uint32_t lo, hi;                                              // the next slab between its loads and its LDS writes
            float a0, b0;
            f4 xn[4];

            // the loads of a slab of kl <= 64 columns, and nothing but loads: all in flight during the MFMAs of the slab before
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
                    if (xrow && nv > 0 && nv < 4) {                       // the ragged group: nothing past act[i][K)
                        v.x = xp[4 * j];
                        if (nv > 1) v.y = xp[4 * j + 1];
                        if (nv > 2) v.z = xp[4 * j + 2];
                    }
                    *(f4*)&xs[srow * kStride + scol + 4 * j] = v;
                }
            };

            int64_t kleft = K;                                            // columns from the current slab's first to the end of the part
            fetch(kleft < kSlab ? (int)kleft : kSlab);                    // K >= 1: the launcher returns before an empty dim
            while (kleft > 0) {
                const int kl = kleft < kSlab ? (int)kleft : kSlab;
                commit(kl);
                __syncthreads();
                kleft -= kSlab;
                if (kleft > 0) {
                    weight_step(P, step_q, step_r, e, bkt, rem);
                    xp += kSlab;
                    fetch(kleft < kSlab ? (int)kleft : kSlab);            // in flight during the MFMAs below
                }
                if (mine) rows_mfma<false>(ws, xs, kl, fr, fk, wave, acc);
                __syncthreads();                                          // every wave is done with this slab before the next commit (of either part)
            }
        }

        // D[i][j]: j = lane % 16 (weight row), i = 4 (lane / 16) + v (batch row inside the wave's 16-row block)
        const int64_t r = r0 + fr;
        if (mine && r < N) {
            const float bv = bias ? bias[r] : 0.0f;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int64_t i = i0 + 16 * wave + fk + v;
                if (i < batch) {
                    const float t = bias ? acc[v] + bv : acc[v];
                    if (pre) pre[i * N + r] = t;
                    attn_h[i * N + r] = tanhf(t);
                }
            }
        }
    }
}

inline int64_t ceil4(int64_t v) { return (v + 3) & ~(int64_t)3; }

}  // namespace

extern "C" {

int qda_abi_version(void) { return QDA_ABI_VERSION; }
const char* qda_target_arch(void) { return "gfx950"; }
const char* qda_error_string(int code) { return error_string(code, QDA_ERR_INVALID_ARGUMENT); }
int qda_set_grid_cap(int blocks) { return set_grid_cap(blocks); }

int qda_attn_context_f32(const float* q, const float* keys, const float* values, const int64_t* lengths, int64_t batch, int64_t S, int64_t dim,
                         float* align, float* ctx, void* stream) {
    int64_t t = 0;
    if (batch < 0 || S < 0 || dim < 0 || __builtin_mul_overflow(batch, S, &t) || __builtin_mul_overflow(t, dim, &t) ||
        __builtin_mul_overflow(batch, dim, &t))
        return QDA_ERR_INVALID_ARGUMENT;
    if (misaligned(q) || misaligned(keys) || misaligned(values) || misaligned(align) || misaligned(ctx) || (((uintptr_t)lengths) & 7) != 0)
        return QDA_ERR_INVALID_ARGUMENT;
    constexpr int64_t limit = QDA_CONTEXT_LDS_LIMIT / 4;                // in floats
    if (dim > limit || S > limit || kRed + ceil4(dim) + ceil4(S) > limit) return QDA_ERR_INVALID_ARGUMENT;
    if (batch == 0 || S == 0 || dim == 0) return 0;
    if (!q || !keys || !values || !align || !ctx) return QDA_ERR_INVALID_ARGUMENT;
    if (align == ctx || align == q || align == keys || align == values || ctx == q || ctx == keys || ctx == values) return QDA_ERR_INVALID_ARGUMENT;
    const int64_t base = kRed + ceil4(dim) + ceil4(S);
    const int resident = values == keys && base + S * ceil4(dim) <= limit;   // S, ceil4(dim) <= 40960: the product fits
    const size_t lds_bytes = 4 * (size_t)(resident ? base + S * ceil4(dim) : base);
    if (lds_bytes > 64 * 1024) {                                         // beyond the default: the kernel is told so, once per process and device
        static bool raised[64] = {false};
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return (int)hipGetLastError();
        if (dev < 0 || dev >= 64 || !__atomic_load_n(&raised[dev], __ATOMIC_RELAXED)) {
            const hipError_t rc = hipFuncSetAttribute((const void*)k_attn_context, hipFuncAttributeMaxDynamicSharedMemorySize, QDA_CONTEXT_LDS_LIMIT);
            if (rc != hipSuccess) { (void)hipGetLastError(); return (int)rc; }
            if (dev >= 0 && dev < 64) __atomic_store_n(&raised[dev], true, __ATOMIC_RELAXED);
        }
    }
    const int blocks = capped(batch, (int64_t)device_cus() * 8);
    hipLaunchKernelGGL(k_attn_context, dim3(blocks), dim3(256), lds_bytes, (hipStream_t)stream, q, keys, values, lengths, batch, (int)S, (int)dim,
                       resident, align, ctx);
    return (int)hipGetLastError();
}

int qda_attn_out_packed_f32(const uint8_t* packed, const float* alpha, const float* beta, int64_t bucket, int levels, int bits, int64_t dim,
                            const float* ctx, const float* x, int64_t batch, const float* bias, float* attn_h, float* pre, void* stream) {
    int64_t cols = 0, t = 0;
    if (dim < 0 || batch < 0 || __builtin_mul_overflow(dim, (int64_t)2, &cols) || __builtin_mul_overflow(batch, dim, &t)) return QDA_ERR_INVALID_ARGUMENT;
    Packed P;
    if (!describe(P, packed, alpha, beta, dim, cols, bucket, levels, bits)) return QDA_ERR_INVALID_ARGUMENT;
    if (misaligned(ctx) || misaligned(x) || misaligned(bias) || misaligned(attn_h) || misaligned(pre)) return QDA_ERR_INVALID_ARGUMENT;
    if (batch == 0 || dim == 0) return 0;
    if (!packed || !alpha || !beta || !ctx || !x || !attn_h) return QDA_ERR_INVALID_ARGUMENT;
    if (attn_h == ctx || attn_h == x || attn_h == bias || attn_h == pre || (pre && (pre == ctx || pre == x || pre == bias))) return QDA_ERR_INVALID_ARGUMENT;
    Acts acts = {{ctx, x}};
    const int64_t chunks = (batch - 1) / kTile + 1;
    const int64_t tiles = ((dim - 1) / kRows + 1) * chunks;             // <= batch dim: fits
    const int blocks = capped(tiles, (int64_t)device_cus() * 8);
    hipLaunchKernelGGL(k_attn_out_mm, dim3(blocks), dim3(256), 0, (hipStream_t)stream, P, acts, batch, bias, attn_h, pre, chunks, tiles,
                       kSlab / P.bucket, kSlab % P.bucket);
    return (int)hipGetLastError();
}

}  // extern "C"
