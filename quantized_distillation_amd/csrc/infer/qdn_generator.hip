// qdn_generator.hip -- libqd_infer_gen.so: the end of a decoder step -- vocabulary projection, log-softmax and top-k -- from the
// packed generator weight W[V][dim] (include/qd_infer_gen.h), gfx950.  Two kernels, one launch each: k_gen_panel_mm (the logits of
// a panel of 64 words x up to 64 rows of x on fp32 MFMA, reduced to (max, sum of exp, top-k) in the lanes that hold them) and
// k_gen_finish (the panels of a row combined).  Nothing of the other libraries is linked in; the decode is the shared one of
// qdi_packed.h, unchanged, the weight pieces of the K walk and the MFMA loop those of qdi_mm.h.
//
// k_gen_panel_mm, one block of 256 threads (4 waves) per panel of QDN_PANEL = 64 vocabulary rows x up to 64 rows of x:
//   split     work items = panels x m-chunks, m-chunk fastest, strided over the grid.  Wave w owns the rows [16 w, + 16) of x of the
//             chunk; a wave whose rows lie at or past m skips the MFMAs and the epilogue.  No split-K, no atomics.
//   K walk    the panel is FOUR consecutive tiles of 16 weight rows, each walked exactly as k_linear_mm (qdm_linear.hip) walks
//             its tile -- ws[16][68], xs[64][68], the next slab held in registers (fetch4 before the MFMAs, weight_commit after
//             them), two barriers per slab, rows_mfma<false> (A = x, B = W^T), ONE 16 x 16 accumulator per wave -- the staging of x
//             and the slab loop copied from there with their guards, as qdi_mm.h instructs.  Not one tile of 64 rows with four
//             accumulators: DESIGN.md 11.1 has that version measured.  The x slab is staged again per tile (from L2).  A tile that
//             starts at or past V (the ragged last panel) is not walked.
//   registers after tile t lane l holds the logits of word 64 p + 16 t + l % 16 for the four rows 16 w + 4 (l / 16) + v of x.  They
//             are kept: lg[4], 16 VGPRs.  The tile loop is NOT unrolled (it would be the K walk four times over); the four f4
//             are a shift register instead -- lg[0] = lg[1], ..., lg[3] = the new tile -- so every index is a constant and after
//             the fourth tile lg[t] is tile t.
//   epilogue  the 64 logits of a row of x then sit in a 16-lane group x 4 tiles.  Every reduction is a 4-way step inside the lane
//             and an xor tree over the group (distance 8, 4, 2, 1, all inside l / 16): no LDS, no memory.  Per row: max(k, 1) rounds
//             of argmax under the header's total order, each taking the first candidate strictly AFTER the round before's winner
//             (nothing is mutated, nothing is sorted); round 0's winner is the row maximum; sum of expf(logit - max), tiles 0 .. 3
//             inside the lane, the tree across.  Lane l % 16 == 0 writes (max, sum, k x (value, int32 word)) to work[i][p]; with
//             logp the 16 lanes of a group store 64 contiguous bytes of raw logits per tile.
// k_gen_finish, one block of 256 threads per row of x, rows strided over the grid: M, S and lse as the header words them; k rounds
//   of a block-wide argmax over the panels k candidates, streamed from work (L2-resident: it was written a launch ago) -- per
//   thread its candidates t, t + 256, ..., an xor tree per wave, the four waves through LDS (two sets of slots, used in turn: one
//   barrier per round); then logp -= lse in place, 16 bytes per thread and access.
#include "qdi_mm.h"           // the pieces of the K walk; through it qdi_packed.h: Packed, describe, the decode, the host helpers

#include "../../../include/qd_infer_gen.h"

#include <cstddef>
#include <type_traits>

using namespace qd;

namespace {

constexpr int kTile = 64;              // rows of x of a chunk
constexpr int kPanelTiles = QDN_PANEL / kRows;
static_assert(QDN_PANEL == 64 && kPanelTiles == 4, "a panel is four tiles: one f4 of logits per tile, a 16-lane group per row of x");

// The header's total order as ONE unsigned comparison: a comes before b exactly where ticket(a) > ticket(b).  High word: the
// logit on a scale that rises with it -- z + 0.0f (so -0.0f and +0.0f are one value), sign bit flipped for the positive, all bits
// for the negative, NaN above every number (0xfffffffe; +inf is 0xff800000); low word: ~word, so the lower index wins a tie.  0
// is no ticket at all (an empty place): the smallest high word of a logit is -inf's, 0x007fffff.  ~0 is no ticket either -- the
// high word 0xffffffff is left unused for it -- and is what the rounds start from: "strictly after nothing".  (With NaN at
// 0xffffffff a NaN at word 0 WAS ~0 and was never selected.)  Written with float compares the same selection kept a dozen
// lane masks alive per candidate and k_gen_panel_mm spilled SGPRs; this is one v_cmp_gt_u64 and two v_cndmask.
__device__ __forceinline__ uint64_t ticket(float z, int word) {
    z = z + 0.0f;
    uint32_t u = __float_as_uint(z);
    u ^= (uint32_t)((int32_t)u >> 31) | 0x80000000u;
    if (z != z) u = 0xfffffffeu;
    return ((uint64_t)u << 32) | (uint32_t)~word;
}

// the logit of a ticket (z + 0.0f; of a NaN a quiet NaN), -inf for none; its word, -1 for none
__device__ __forceinline__ float ticket_value(uint64_t t) {
    const uint32_t u = (uint32_t)(t >> 32);
    return t ? __uint_as_float(u ^ ((uint32_t)((int32_t)~u >> 31) | 0x80000000u)) : -__builtin_inff();
}
__device__ __forceinline__ int ticket_word(uint64_t t) { return t ? (int)~(uint32_t)t : -1; }

__device__ __forceinline__ uint64_t first_of(uint64_t a, uint64_t b) { return a > b ? a : b; }

__device__ __forceinline__ uint64_t first_across(uint64_t a, int d) {
    const uint32_t lo = __shfl_xor((uint32_t)a, d), hi = __shfl_xor((uint32_t)(a >> 32), d);
    return first_of(a, ((uint64_t)hi << 32) | lo);
}

// A value the compiler is to compute from where it is used: what it cannot see through, it does not turn into lane masks and
// addresses that are made once per kernel and then live, in SGPRs, across the K walk -- which takes 97 of them in k_linear_mm.
template <class T> __device__ __forceinline__ T opaque_s(T v) { asm volatile("" : "+s"(v)); return v; }
__device__ __forceinline__ int opaque_v(int v) { asm volatile("" : "+v"(v)); return v; }

// the first of two maxima in the total order, by value alone: NaN, else the larger
__device__ __forceinline__ float first_value(float a, float b) { return a != a ? a : b != b ? b : fmaxf(a, b); }

// The arguments of k_gen_panel_mm, ONE by-value struct so that it is the kernel-argument segment from its first byte on.  What only
// the epilogue of a tile or of a panel needs (`late`) is never named through the parameter: it is read from the segment where it
// is used, a scalar load behind an opaque pointer, and so holds no SGPR during the K walk.  As plain parameters these seven values
// and what the compiler derives from them once per kernel were live across the walk, and the kernel spilled SGPRs.
struct GenArgs {
    Packed P;
    const float* x;
    int64_t m, m_chunks, items;
    int step_q, step_r;                // 64 = step_q bucket + step_r
    struct Late {                      // (x, m, m_chunks and items are read the same way, at the item's and the tile's start)
        const float* bias;
        float* logp;
        float* work;
        int64_t panels;
        int k;
    } late;
};
typedef const __attribute__((address_space(4))) GenArgs* KernArgs;
// The assumption: the explicit arguments of a kernel start at byte 0 of its kernel-argument segment (the AMDGPU HSA ABI: hidden
// arguments follow them), so the one by-value GenArgs IS the segment's head and late_args()->f is a.f.  The layout the reads rest on:
static_assert(offsetof(GenArgs, x) == 72 && offsetof(GenArgs, late) == 112 && sizeof(GenArgs) == 152 && std::is_trivially_copyable<GenArgs>::value,
              "GenArgs is read from the kernel-argument segment by offset: keep it one trivially copyable struct, the kernel's only parameter");
// What guards the reason for it: tests/test_infer_gen_abi.py holds the kernel to no spills.  A compiler that keeps these values out of
// the walk's SGPRs by itself makes late_args() unnecessary, never wrong.

__device__ __forceinline__ KernArgs late_args() { return opaque_s((KernArgs)__builtin_amdgcn_kernarg_segment_ptr()); }

__global__ __launch_bounds__(256) void k_gen_panel_mm(GenArgs a) {
    const Packed& P = a.P;
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
    for (int64_t item = blockIdx.x; item < late_args()->items; item += gridDim.x) {
        const int64_t m_chunks = late_args()->m_chunks;
        int64_t m = late_args()->m;
        const int p = (int)(item / m_chunks);                            // < 2^25: V < 2^31
        const int64_t i0 = (item - p * m_chunks) * kTile;
        const int mrows = m - i0 < kTile ? (int)(m - i0) : kTile;        // rows of x in this chunk, >= 1
        const bool xrow = srow < mrows;                                  // this thread's row of x exists
        const bool mine = 16 * wave < mrows;                             // this wave's 16 rows of x hold one (wave-uniform)
        f4 lg[kPanelTiles];                                              // the shift register of the panel's logits
#pragma unroll
        for (int t = 0; t < kPanelTiles; ++t) lg[t] = (f4){0.0f, 0.0f, 0.0f, 0.0f};

#pragma unroll 1
        for (int t = 0; t < kPanelTiles; ++t) {
            const int64_t r0 = (int64_t)p * QDN_PANEL + t * kRows;
            f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
            if (r0 < N) {                                                // block-uniform: a tile past V holds no word and is not walked
                const bool wrow = r0 + wr < N;                           // this thread's weight row exists
                // k_linear_mm's walk of the tile.  A thread without a weight row (!wrow), without a row of x (!xrow) or whose columns lie
                // past K still carries e, xp, bkt and rem along (past the arrays, or 0 stepped on): every USE below is under the same
                // wrow / xrow / column test, in fetch and in commit alike, so none of them is ever turned into an address that is read.
                int64_t e = (r0 + wr) * K + wc;                          // its group's first element in the current slab ...
                const float* xp = late_args()->x + (i0 + srow) * K + scol;
                int64_t bkt, rem;                                        // ... and that element's bucket
                weight_bucket(P, e, wrow && wc < K, bkt, rem);
                uint32_t lo, hi;                                         // the next slab between its loads and its LDS writes
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
                        if (xrow && nv > 0 && nv < 4) {                  // the ragged group: nothing past x[i][K)
                            v.x = xp[4 * j];
                            if (nv > 1) v.y = xp[4 * j + 1];
                            if (nv > 2) v.z = xp[4 * j + 2];
                        }
                        *(f4*)&xs[srow * kStride + scol + 4 * j] = v;
                    }
                };

                int64_t kleft = K;                                       // columns from the current slab's first to the end of the row
                if (kleft > 0) fetch(kleft < kSlab ? (int)kleft : kSlab);
                while (kleft > 0) {
                    const int kl = kleft < kSlab ? (int)kleft : kSlab;
                    commit(kl);
                    __syncthreads();
                    kleft -= kSlab;
                    if (kleft > 0) {
                        weight_step(P, a.step_q, a.step_r, e, bkt, rem);
                        xp += kSlab;
                        fetch(kleft < kSlab ? (int)kleft : kSlab);       // in flight during the MFMAs below
                    }
                    if (mine) rows_mfma<false>(ws, xs, kl, fr, fk, wave, acc);
                    __syncthreads();                                     // every wave is done with this slab before the next commit (of this tile or the next)
                }
                // D[i][j]: j = lane % 16 (weight row), i = 4 (lane / 16) + v (row of x inside the wave's 16-row block)
                const int64_t r = r0 + fr;
                const KernArgs late = late_args();
                m = late->m;
                const float* bias_t = late->late.bias;
                float* logp_t = late->late.logp;
                if (bias_t && r < N) {
                    const float bv = bias_t[r];
#pragma unroll
                    for (int v = 0; v < 4; ++v) acc[v] = acc[v] + bv;
                }
                if (logp_t && mine && r < N) {                             // the raw logits; k_gen_finish subtracts lse in place
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int64_t i = i0 + 16 * wave + fk + v;
                        if (i < m) logp_t[i * N + r] = acc[v];
                    }
                }
            }
#pragma unroll
            for (int s = 0; s + 1 < kPanelTiles; ++s) lg[s] = lg[s + 1];
            lg[kPanelTiles - 1] = acc;
        }

        if (!mine) continue;                                             // wave-uniform: the shuffles below are taken by whole waves
        const KernArgs late = late_args();
        m = late->m;
        const int k_e = late->late.k, fr_e = opaque_v(fr);
        float* work = late->late.work;
        const int64_t panels = late->late.panels;
        const int stride = 2 + 2 * k_e;                                  // words of work per row and panel
        const int w0 = p * QDN_PANEL + fr_e;                        // this lane's word of tile 0; tile t: + 16 t.  V < 2^31 - 64 (launcher)
        const int nwords = (int)(N - (int64_t)p * QDN_PANEL < QDN_PANEL ? N - (int64_t)p * QDN_PANEL : QDN_PANEL) - fr_e;   // word w0 + 16 t exists where 16 t < nwords
        const float ninf = -__builtin_inff();
#pragma unroll 1
        for (int v = 0; v < 4; ++v) {                                    // not unrolled: the row in turn is component 0, the f4 rotate (below)
            const int64_t i = i0 + 16 * wave + fk + v;                   // the same for the 16 lanes of a group
            float* out = work + (i * panels + p) * stride;               // formed, not used, for i >= m
            const bool writer = fr_e == 0 && i < m;
            uint64_t cand[kPanelTiles];                                  // this lane's four words of the row; 0 past V
#pragma unroll
            for (int t = 0; t < kPanelTiles; ++t) cand[t] = 16 * t < nwords ? ticket(lg[t].x, w0 + 16 * t) : 0;
            uint64_t prev = ~(uint64_t)0;                                // the round before's winner; after an empty round nothing is open
            const int rounds = k_e > 1 ? k_e : 1;
            for (int round = 0; round < rounds; ++round) {
                uint64_t best = 0;
#pragma unroll
                for (int t = 0; t < kPanelTiles; ++t) best = first_of(best, cand[t] < prev ? cand[t] : 0);
#pragma unroll
                for (int d = 8; d >= 1; d >>= 1) best = first_across(best, d);
                prev = best;
                const float bv = ticket_value(best);
                const int bi = ticket_word(best);
                if (round == 0) {                                        // the panel holds a word: round 0 has a winner, the row maximum
                    const float mx = bv;
                    float s = 0.0f;
#pragma unroll
                    for (int t = 0; t < kPanelTiles; ++t)
                        if (16 * t < nwords) s = s + expf(lg[t].x - mx);
#pragma unroll
                    for (int d = 8; d >= 1; d >>= 1) s = s + __shfl_xor(s, d);
                    if (mx == ninf) s = 0.0f;
                    if (writer) { out[0] = mx; out[1] = s; }
                }
                if (writer && round < k_e) {
                    out[2 + 2 * round] = bi >= 0 ? bv : ninf;
                    ((int*)out)[3 + 2 * round] = bi;
                }
            }
#pragma unroll
            for (int t = 0; t < kPanelTiles; ++t) lg[t] = (f4){lg[t].y, lg[t].z, lg[t].w, lg[t].x};
        }
    }
}

__global__ __launch_bounds__(256) void k_gen_finish(const float* work, int64_t m, int64_t V, int64_t panels, int k, float* lse, float* logp,
                                                    float* top_val, int64_t* top_idx) {
    __shared__ float redv[2][4];
    __shared__ uint64_t redt[2][4];                                      // slots of their own: a write of redv or redt is always two barriers behind the last read of the same slot
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int stride = 2 + 2 * k;
    const float ninf = -__builtin_inff();
    for (int64_t i = blockIdx.x; i < m; i += gridDim.x) {
        const float* row = work + i * panels * stride;
        // M: the first of the panel maxima
        float M = ninf;
        for (int64_t p = tid; p < panels; p += 256) M = first_value(M, row[p * stride]);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) M = first_value(M, __shfl_xor(M, d));
        if (lane == 0) redv[0][wave] = M;
        __syncthreads();
        M = first_value(first_value(redv[0][0], redv[0][1]), first_value(redv[0][2], redv[0][3]));
        // S
        float S = 0.0f;
        for (int64_t p = tid; p < panels; p += 256) {
            const float mp = row[p * stride];
            S = S + (mp == ninf ? 0.0f : row[p * stride + 1] * expf(mp - M));
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) S = S + __shfl_xor(S, d);
        if (lane == 0) redv[1][wave] = S;
        __syncthreads();
        S = ((redv[1][0] + redv[1][1]) + redv[1][2]) + redv[1][3];
        const float l = (M == ninf || M == -ninf) ? M : M + logf(S);
        if (tid == 0) lse[i] = l;

        // top-k: k rounds, each the first candidate strictly after the round before's winner
        uint64_t prev = ~(uint64_t)0;                                    // after an empty round nothing is open
        const int64_t cands = panels * k;
        for (int round = 0; round < k; ++round) {
            uint64_t best = 0;
            for (int64_t c = tid; c < cands; c += 256) {
                const int64_t p = c / k;
                const float* cand = row + p * stride + 2 + 2 * (c - p * k);
                const int word = ((const int*)cand)[1];
                const uint64_t tk = word >= 0 ? ticket(cand[0], word) : 0;
                best = first_of(best, tk < prev ? tk : 0);
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) best = first_across(best, d);
            const int slot = round & 1;                                  // written two rounds apart: one barrier per round
            if (lane == 0) redt[slot][wave] = best;
            __syncthreads();
            best = first_of(first_of(redt[slot][0], redt[slot][1]), first_of(redt[slot][2], redt[slot][3]));
            prev = best;
            if (tid == 0) {
                top_val[i * k + round] = best ? ticket_value(best) - l : ninf;
                top_idx[i * k + round] = ticket_word(best);
            }
        }

        if (logp) {                                                      // log-probs in place: 16 bytes per access at the row's own 4-byte phase
            float* z = logp + i * V;
            const int64_t groups = V >> 2;
            for (int64_t g = tid; g < groups; g += 256) {
                f4u u = *(const f4u*)(z + 4 * g);
                u.x = u.x - l; u.y = u.y - l; u.z = u.z - l; u.w = u.w - l;
                *(f4u*)(z + 4 * g) = u;
            }
            for (int64_t r = 4 * groups + tid; r < V; r += 256) z[r] = z[r] - l;
        }
    }
}

// words of work per row and panel, and the panels; false: the sizes are refused
inline bool work_size(int64_t V, int64_t m, int k, int64_t& panels, int64_t& bytes) {
    if (V < 0 || m < 0 || k < 0 || k > QDN_MAX_TOPK || V > (int64_t)INT32_MAX - QDN_PANEL) return false;
    panels = (V + QDN_PANEL - 1) / QDN_PANEL;
    return !__builtin_mul_overflow(m, panels, &bytes) && !__builtin_mul_overflow(bytes, (int64_t)(4 * (2 + 2 * k)), &bytes);
}

}  // namespace

extern "C" {

int qdn_abi_version(void) { return QDN_ABI_VERSION; }
const char* qdn_target_arch(void) { return "gfx950"; }
const char* qdn_error_string(int code) { return error_string(code, QDN_ERR_INVALID_ARGUMENT); }
int qdn_set_grid_cap(int blocks) { return set_grid_cap(blocks); }

int64_t qdn_generator_work_bytes(int64_t V, int64_t m, int k) {
    int64_t panels = 0, bytes = 0;
    return work_size(V, m, k, panels, bytes) ? bytes : -1;
}

int qdn_generator_packed_f32(const uint8_t* packed, const float* alpha, const float* beta, int64_t V, int64_t dim, int64_t bucket, int levels,
                             int bits, const float* x, int64_t m, const float* bias, float* lse, float* logp, int k, float* top_val,
                             int64_t* top_idx, void* work, void* stream) {
    Packed P;
    int64_t panels = 0, bytes = 0, t = 0;
    if (!describe(P, packed, alpha, beta, V, dim, bucket, levels, bits) || !work_size(V, m, k, panels, bytes)) return QDN_ERR_INVALID_ARGUMENT;
    if (misaligned(x) || misaligned(bias) || misaligned(lse) || misaligned(logp) || misaligned(work)) return QDN_ERR_INVALID_ARGUMENT;
    if (k > 0 && (misaligned(top_val) || (((uintptr_t)top_idx) & 7) != 0)) return QDN_ERR_INVALID_ARGUMENT;
    if (__builtin_mul_overflow(m, V, &t) || __builtin_mul_overflow(m, dim, &t)) return QDN_ERR_INVALID_ARGUMENT;
    if (m == 0 || V == 0) return 0;
    if (!lse || !work || (dim > 0 && (!packed || !alpha || !beta || !x)) || (k > 0 && (!top_val || !top_idx))) return QDN_ERR_INVALID_ARGUMENT;
    const void* ins[5] = {packed, alpha, beta, x, bias};
    const void* outs[5] = {lse, logp, k > 0 ? top_val : nullptr, k > 0 ? top_idx : nullptr, work};
    for (int a = 0; a < 5; ++a) {
        if (!outs[a]) continue;
        for (int b = 0; b < 5; ++b)
            if (outs[a] == ins[b] || (b > a && outs[a] == outs[b])) return QDN_ERR_INVALID_ARGUMENT;
    }
    const int64_t m_chunks = (m - 1) / kTile + 1;
    const int64_t items = panels * m_chunks;                             // <= m panels: fits
    const int64_t own_cap = (int64_t)device_cus() * 8;
    const GenArgs args = {P, x, m, m_chunks, items, (int)(kSlab / P.bucket), (int)(kSlab % P.bucket), {bias, logp, (float*)work, panels, k}};
    hipLaunchKernelGGL(k_gen_panel_mm, dim3(capped(items, own_cap)), dim3(256), 0, (hipStream_t)stream, args);
    const int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(k_gen_finish, dim3(capped(m, own_cap)), dim3(256), 0, (hipStream_t)stream, (const float*)work, m, V, panels, k, lse, logp,
                       top_val, top_idx);
    return (int)hipGetLastError();
}

}  // extern "C"
