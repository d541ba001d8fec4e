// qdl_kd.hip -- libqd_loss.so (include/qd_loss.h): the distillation loss and its gradient with respect to the student's logits
// in one pass over the logits.  One translation unit; DESIGN.md section 12 has the reasoning.
//
//   k_kd_rows<STAGING, T1>   per row: the softmax statistics of student and teacher, row_kl, row_nll and the row of grad.
//                            STAGING says where the row waits between the pass that finds (max, sum of exp) and the pass that
//                            needs them for every element: in registers (one wave per row), in LDS (one workgroup per row) or
//                            nowhere (one workgroup per row, read again).  T1: temperature == 1, softmax(z / T) IS softmax(z).
//   k_kd_finish              loss = sum over the rows, one block, an order that depends on `rows` alone.
//
// Compile with -ffp-contract=off (build.HIPCC_FLAGS): the header words every fp32 operation as one rounded operation.
#include "../qd_common.h"
#include "qd_loss.h"

#include <math.h>

namespace {

using namespace qd;

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));     // a 16-byte access at the 4-byte alignment of fp32 data

constexpr int kWave = 0, kLds = 1, kStream = 2;                         // the stagings
constexpr int kWaveBlock = 256;                                         // wave staging: four rows per block
constexpr int kWaveRegs = QDL_WAVE_COLS / 64;                           // columns per lane there
constexpr int kRowBlock = 1024;                                         // the other two: sixteen waves on one row
constexpr int kRowWaves = kRowBlock / 64;
static_assert(QDL_WAVE_COLS % 64 == 0 && QDL_LDS_COLS % 4 == 0, "whole lanes, whole 16-byte groups");
static_assert(8 * QDL_LDS_COLS + 4 * 3 * kRowWaves <= 160 * 1024, "the row of z, the row of t and the scratch are one workgroup's LDS");

struct KdArgs {
    const float* z;
    const float* t;
    const int64_t* y;
    int64_t rows, cols;
    float T, ks /* kl_scale / T */, ns /* nll_scale */;
    int64_t ignore;
    float* grad;
    float* row_kl;
    float* row_nll;
};

__device__ __forceinline__ f4 load4(const float* p) { const f4u u = *(const QD_AS_GLOBAL f4u*)p; return (f4){u.x, u.y, u.z, u.w}; }
__device__ __forceinline__ void store4(float* p, const f4& v) { *(QD_AS_GLOBAL f4u*)p = (f4u){v.x, v.y, v.z, v.w}; }

template <bool T1> __device__ __forceinline__ float over_t(float d, float T) { return T1 ? d : d / T; }

// The running (max, sum of exp((x - max) / T)) of one lane, and with BOTH the sum of exp(x - max) next to it (the student at
// T != 1: softmax(z / T) and softmax(z) have the same max).  A lane that has seen nothing holds (-inf, 0) and adds exactly 0
// to the row's sum.
template <bool T1, bool BOTH>
struct Online {
    float m = -INFINITY, s = 0.0f, s1 = 0.0f;
    __device__ __forceinline__ void add4(const f4& v, float T) {
        const float mn = pmax(m, pmax4(v));
        const float d = m - mn;
        s = s * expf(over_t<T1>(d, T)) + (((expf(over_t<T1>(v.x - mn, T)) + expf(over_t<T1>(v.y - mn, T))) + expf(over_t<T1>(v.z - mn, T))) + expf(over_t<T1>(v.w - mn, T)));
        if (BOTH) s1 = s1 * expf(d) + (((expf(v.x - mn) + expf(v.y - mn)) + expf(v.z - mn)) + expf(v.w - mn));
        m = mn;
    }
    __device__ __forceinline__ void add1(float x, float T) {
        const float mn = pmax(m, x);
        const float d = m - mn;
        s = s * expf(over_t<T1>(d, T)) + expf(over_t<T1>(x - mn, T));
        if (BOTH) s1 = s1 * expf(d) + expf(x - mn);
        m = mn;
    }
    // this lane's share of the row's sums once the row's max M is known
    __device__ __forceinline__ float share(float M, float T) const { return s * expf(over_t<T1>(m - M, T)); }
    __device__ __forceinline__ float share1(float M) const { return s1 * expf(m - M); }
};

// all-reduce of three values over NW waves (NW == 1: the wave alone, no LDS and no barrier); the waves front to back
struct OpSum { static __device__ __forceinline__ float wave(float v) { return wave_sum(v); } static __device__ __forceinline__ float two(float a, float b) { return a + b; } };
struct OpMax { static __device__ __forceinline__ float wave(float v) { return wave_max(v); } static __device__ __forceinline__ float two(float a, float b) { return pmax(a, b); } };
struct OpMin { static __device__ __forceinline__ float wave(float v) { return wave_min(v); } static __device__ __forceinline__ float two(float a, float b) { return pmin(a, b); } };

template <int NW, typename A, typename B, typename C>
__device__ __forceinline__ void all3(float& a, float& b, float& c, float* red) {
    a = A::wave(a); b = B::wave(b); c = C::wave(c);
    if (NW == 1) return;
    const int w = threadIdx.x >> 6;
    __syncthreads();                                                     // `red` may still be read from its last use
    if ((threadIdx.x & 63) == 0) { red[w] = a; red[NW + w] = b; red[2 * NW + w] = c; }
    __syncthreads();
    a = red[0]; b = red[NW]; c = red[2 * NW];
    for (int i = 1; i < NW; ++i) { a = A::two(a, red[i]); b = B::two(b, red[NW + i]); c = C::two(c, red[2 * NW + i]); }
}

// What the second pass needs of a row.
struct RowStats {
    float Mz, Mt;            // the maxima, NaN where the row holds a non-finite value or its target is out of range
    float Sz, St, S1;        // sums of exp
    float rz, rt, r1;        // their reciprocals, for the exact quotient (qd_common.h: div_alpha)
    float lz, lt;            // logf(Sz), logf(St)
    int64_t y;
};

template <bool T1>
__device__ __forceinline__ void finish_stats(RowStats& r, float Sz, float St, float S1) {
    r.Sz = Sz; r.St = St; r.S1 = T1 ? Sz : S1;
    r.rz = 1.0f / r.Sz; r.rt = 1.0f / r.St; r.r1 = 1.0f / r.S1;
    r.lz = logf(r.Sz); r.lt = logf(r.St);
}

// grad of one element; its KL term is added to `kl`.  e / S is the correctly rounded quotient: S is in [1, cols], far inside
// div_alpha's range; an e below 2^-100 may lose its last bit, which is nothing against the 2^-24 of a probability near 1.
template <bool T1>
__device__ __forceinline__ float element(float z, float t, int64_t c, const RowStats& r, const KdArgs& a, float& kl) {
    const float dz = z - r.Mz;
    const float az = over_t<T1>(dz, a.T), at = over_t<T1>(t - r.Mt, a.T);
    const float ps = div_alpha<true>(expf(az), r.Sz, r.rz);
    const float pt = div_alpha<true>(expf(at), r.St, r.rt);
    const float p1 = T1 ? ps : div_alpha<true>(expf(dz), r.S1, r.r1);
    const float term = pt * ((at - r.lt) - (az - r.lz));
    kl = kl + (pt == 0.0f ? 0.0f : term);                               // an underflowed pt adds 0, never 0 x inf
    return a.ks * (ps - pt) + a.ns * (p1 - (c == r.y ? 1.0f : 0.0f));
}

// NaN where the target is neither a column nor ignore_index, else +0.0f: added to both maxima, it makes the row loud
__device__ __forceinline__ float target_poison(int64_t y, int64_t cols) { return (y < 0 || y >= cols) ? __builtin_nanf("") : 0.0f; }

// ---- wave staging: one wave per row, the row in registers --------------------------------------------------------------
// Lane l holds the columns l, l + 64, ...: every load and store of the wave is one contiguous run of the row.  No LDS, no
// barrier: the four waves of a block are on four rows and never meet.
template <bool T1>
__device__ __forceinline__ void rows_by_wave(const KdArgs& a) {
    const int lane = threadIdx.x & 63;
    const int64_t first = (int64_t)blockIdx.x * (kWaveBlock / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t step = (int64_t)gridDim.x * (kWaveBlock / 64);
    for (int64_t row = first; row < a.rows; row += step) {
        const int64_t y = ldg(a.y + row);
        float* g = a.grad + row * a.cols;
        if (y == a.ignore) {
#pragma unroll
            for (int j = 0; j < kWaveRegs; ++j)
                if (lane + 64 * j < a.cols) stg(0.0f, g + lane + 64 * j);
            if (lane == 0) { stg(0.0f, a.row_kl + row); stg(0.0f, a.row_nll + row); }
            continue;
        }
        const float* zp = a.z + row * a.cols;
        const float* tp = a.t + row * a.cols;
        float z[kWaveRegs], t[kWaveRegs];
        float mz = -INFINITY, mt = -INFINITY, lo = INFINITY;
#pragma unroll
        for (int j = 0; j < kWaveRegs; ++j) {
            const bool in = lane + 64 * j < a.cols;
            z[j] = in ? ldg(zp + lane + 64 * j) : 0.0f;
            t[j] = in ? ldg(tp + lane + 64 * j) : 0.0f;
            if (in) { mz = pmax(mz, z[j]); mt = pmax(mt, t[j]); lo = pmin(lo, pmin(z[j], t[j])); }
        }
        all3<1, OpMax, OpMax, OpMin>(mz, mt, lo, nullptr);
        const float poison = (lo - lo) + target_poison(y, a.cols);       // lo - lo: NaN for -inf, +inf and NaN, else 0
        RowStats r;
        r.Mz = mz + poison; r.Mt = mt + poison; r.y = y;
        float sz = 0.0f, st = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int j = 0; j < kWaveRegs; ++j) {
            if (lane + 64 * j < a.cols) {
                sz = sz + expf(over_t<T1>(z[j] - r.Mz, a.T));
                st = st + expf(over_t<T1>(t[j] - r.Mt, a.T));
                if (!T1) s1 = s1 + expf(z[j] - r.Mz);
            }
        }
        all3<1, OpSum, OpSum, OpSum>(sz, st, s1, nullptr);
        finish_stats<T1>(r, sz, st, s1);
        float kl = 0.0f, unused0 = 0.0f, unused1 = 0.0f;
#pragma unroll
        for (int j = 0; j < kWaveRegs; ++j)
            if (lane + 64 * j < a.cols) stg(element<T1>(z[j], t[j], lane + 64 * j, r, a, kl), g + lane + 64 * j);
        all3<1, OpSum, OpSum, OpSum>(kl, unused0, unused1, nullptr);
        if (lane == 0) {
            const float zy = (y >= 0 && y < a.cols) ? ldg(zp + y) : 0.0f;
            stg(kl, a.row_kl + row);
            stg(logf(r.S1) - (zy - r.Mz), a.row_nll + row);
        }
    }
}

// ---- LDS and streamed staging: one workgroup of 1024 lanes per row --------------------------------------------------------
// Pass 1 streams z and t in 16-byte groups at the row's own 4-byte phase -- a lane asks for its next group of each before it
// consumes the one it holds, four loads before the first wait -- leaves them in LDS (kLds) and keeps the lane's running (max, sum of exp).  Pass 2 takes every element from LDS (kLds) or from
// memory again (kStream), and stores grad in the same 16-byte groups.
template <int STAGING, bool T1>
__device__ __forceinline__ void rows_by_block(const KdArgs& a, float* zs, float* ts, float* red) {
    const int tid = threadIdx.x;
    const int64_t groups = a.cols >> 2;
    const int64_t tail = 4 * groups + tid;                               // the lanes 0 .. cols % 4 - 1 take one last column each
    for (int64_t row = blockIdx.x; row < a.rows; row += gridDim.x) {
        const int64_t y = ldg(a.y + row);
        float* g = a.grad + row * a.cols;
        if (y == a.ignore) {
            const f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int64_t k = tid; k < groups; k += kRowBlock) store4(g + 4 * k, zero);
            if (tail < a.cols) stg(0.0f, g + tail);
            if (tid == 0) { stg(0.0f, a.row_kl + row); stg(0.0f, a.row_nll + row); }
            continue;
        }
        const float* zp = a.z + row * a.cols;
        const float* tp = a.t + row * a.cols;
        Online<T1, !T1> oz;
        Online<T1, false> ot;
        float lo = INFINITY;
        int64_t k = tid;
        bool have = k < groups;
        f4 z0 = {0.0f, 0.0f, 0.0f, 0.0f}, t0 = z0;
        if (have) { z0 = load4(zp + 4 * k); t0 = load4(tp + 4 * k); }
        while (have) {                                                   // the loads of the lane's next group fly while this one is consumed
            const int64_t k1 = k + kRowBlock;
            const bool more = k1 < groups;
            f4 z1 = z0, t1 = t0;
            if (more) { z1 = load4(zp + 4 * k1); t1 = load4(tp + 4 * k1); }
            if (STAGING == kLds) { *(f4*)(zs + 4 * k) = z0; *(f4*)(ts + 4 * k) = t0; }
            oz.add4(z0, a.T);
            ot.add4(t0, a.T);
            lo = pmin(lo, pmin(pmin4(z0), pmin4(t0)));
            z0 = z1; t0 = t1; k = k1; have = more;
        }
        if (tail < a.cols) {
            const float z0 = ldg(zp + tail), t0 = ldg(tp + tail);
            if (STAGING == kLds) { zs[tail] = z0; ts[tail] = t0; }
            oz.add1(z0, a.T);
            ot.add1(t0, a.T);
            lo = pmin(lo, pmin(z0, t0));
        }
        float mz = oz.m, mt = ot.m;
        all3<kRowWaves, OpMax, OpMax, OpMin>(mz, mt, lo, red);
        const float poison = (lo - lo) + target_poison(y, a.cols);       // lo - lo: NaN for -inf, +inf and NaN, else 0
        RowStats r;
        r.Mz = mz + poison; r.Mt = mt + poison; r.y = y;
        float sz = oz.share(r.Mz, a.T), st = ot.share(r.Mt, a.T), s1 = T1 ? 0.0f : oz.share1(r.Mz);
        all3<kRowWaves, OpSum, OpSum, OpSum>(sz, st, s1, red);            // its second barrier also publishes zs / ts to every lane
        finish_stats<T1>(r, sz, st, s1);

        float kl = 0.0f, unused0 = 0.0f, unused1 = 0.0f;
        for (int64_t q = tid; q < groups; q += kRowBlock) {
            const f4 zv = STAGING == kLds ? *(const f4*)(zs + 4 * q) : load4(zp + 4 * q);
            const f4 tv = STAGING == kLds ? *(const f4*)(ts + 4 * q) : load4(tp + 4 * q);
            f4 o;
            o.x = element<T1>(zv.x, tv.x, 4 * q, r, a, kl);
            o.y = element<T1>(zv.y, tv.y, 4 * q + 1, r, a, kl);
            o.z = element<T1>(zv.z, tv.z, 4 * q + 2, r, a, kl);
            o.w = element<T1>(zv.w, tv.w, 4 * q + 3, r, a, kl);
            store4(g + 4 * q, o);
        }
        if (tail < a.cols) {
            const float zv = STAGING == kLds ? zs[tail] : ldg(zp + tail), tv = STAGING == kLds ? ts[tail] : ldg(tp + tail);
            stg(element<T1>(zv, tv, tail, r, a, kl), g + tail);
        }
        all3<kRowWaves, OpSum, OpSum, OpSum>(kl, unused0, unused1, red);  // its first barrier: every lane is done with zs / ts
        if (tid == 0) {
            const float zy = (y >= 0 && y < a.cols) ? ldg(zp + y) : 0.0f;
            stg(kl, a.row_kl + row);
            stg(logf(r.S1) - (zy - r.Mz), a.row_nll + row);
        }
    }
}

template <int STAGING, bool T1>
__global__ void __launch_bounds__(STAGING == kWave ? kWaveBlock : kRowBlock) k_kd_rows(const KdArgs a) {
    if (STAGING == kWave) {
        rows_by_wave<T1>(a);
    } else {
        __shared__ __attribute__((aligned(16))) float rowbuf[STAGING == kLds ? 2 * QDL_LDS_COLS : 4];
        __shared__ float red[3 * kRowWaves];
        rows_by_block<STAGING, T1>(a, rowbuf, rowbuf + (STAGING == kLds ? QDL_LDS_COLS : 0), red);
    }
}

// loss[0] = sum_n (kl_scale row_kl[n] + nll_scale row_nll[n]): lane l adds the rows l, l + 1024, ... front to back to +0.0f,
// the xor tree over each wave, the sixteen waves front to back.
__global__ void __launch_bounds__(kRowBlock) k_kd_finish(const float* row_kl, const float* row_nll, int64_t rows, float kl_scale, float nll_scale,
                                                         float* loss) {
    __shared__ float red[3 * kRowWaves];
    float s = 0.0f, unused0 = 0.0f, unused1 = 0.0f;
    for (int64_t n = threadIdx.x; n < rows; n += kRowBlock) s = s + (kl_scale * ldg(row_kl + n) + nll_scale * ldg(row_nll + n));
    all3<kRowWaves, OpSum, OpSum, OpSum>(s, unused0, unused1, red);
    if (threadIdx.x == 0) stg(s, loss);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
int g_grid_cap = 0;                                                      // qdl_set_grid_cap: blocks per launch, 0 = none

inline int capped(int64_t blocks, int64_t own_cap) {
    if (blocks > own_cap) blocks = own_cap;
    if (g_grid_cap >= 1 && blocks > g_grid_cap) blocks = g_grid_cap;
    return blocks < 1 ? 1 : (int)blocks;
}

inline bool misaligned(const void* p, uintptr_t mask) { return (((uintptr_t)p) & mask) != 0; }

template <int STAGING>
inline void launch_rows(const KdArgs& a, int blocks, hipStream_t stream) {
    const dim3 block(STAGING == kWave ? kWaveBlock : kRowBlock);
    if (a.T == 1.0f) hipLaunchKernelGGL((k_kd_rows<STAGING, true>), dim3(blocks), block, 0, stream, a);
    else hipLaunchKernelGGL((k_kd_rows<STAGING, false>), dim3(blocks), block, 0, stream, a);
}

}  // namespace

extern "C" {

int qdl_abi_version(void) { return QDL_ABI_VERSION; }
const char* qdl_target_arch(void) { return "gfx950"; }
const char* qdl_error_string(int code) {
    if (code == 0) return "success";
    if (code == QDL_ERR_INVALID_ARGUMENT) return "invalid argument";
    if (code > 0) return hipGetErrorString((hipError_t)code);
    return "unknown error";
}
int qdl_set_grid_cap(int blocks) {
    const int prev = g_grid_cap;
    g_grid_cap = blocks >= 1 ? blocks : 0;
    return prev;
}
int64_t qdl_wave_cols(void) { return QDL_WAVE_COLS; }
int64_t qdl_lds_cols(void) { return QDL_LDS_COLS; }

int qdl_kd_loss_f32(const float* student, const float* teacher, const int64_t* target, int64_t rows, int64_t cols, float temperature,
                    float kl_scale, float nll_scale, int64_t ignore_index, float* grad, float* row_kl, float* row_nll, float* loss,
                    void* stream) {
    int64_t n = 0;
    if (rows < 0 || cols <= 0 || __builtin_mul_overflow(rows, cols, &n) || __builtin_mul_overflow(n, (int64_t)4, &n)) return QDL_ERR_INVALID_ARGUMENT;
    if (!(temperature > 0.0f) || isinf(temperature)) return QDL_ERR_INVALID_ARGUMENT;               // NaN fails the comparison
    if (misaligned(student, 3) || misaligned(teacher, 3) || misaligned(target, 7) || misaligned(grad, 3) || misaligned(row_kl, 3) ||
        misaligned(row_nll, 3) || misaligned(loss, 3) || !loss)
        return QDL_ERR_INVALID_ARGUMENT;
    if (rows > 0 && (!student || !teacher || !target || !grad || !row_kl || !row_nll)) return QDL_ERR_INVALID_ARGUMENT;
    const void* arrays[7] = {grad, row_kl, row_nll, loss, student, teacher, target};                 // the four outputs first
    for (int o = 0; o < 4; ++o)
        for (int b = o + 1; b < 7; ++b)
            if (arrays[o] && arrays[o] == arrays[b]) return QDL_ERR_INVALID_ARGUMENT;
    if (rows > 0) {
        const KdArgs a = {student, teacher, target, rows, cols, temperature, kl_scale / temperature, nll_scale, ignore_index, grad, row_kl, row_nll};
        const int64_t cus = device_cus();
        if (cols <= QDL_WAVE_COLS) launch_rows<kWave>(a, capped((rows + 3) / 4, cus * 16), (hipStream_t)stream);
        else if (cols <= QDL_LDS_COLS) launch_rows<kLds>(a, capped(rows, cus * 16), (hipStream_t)stream);
        else launch_rows<kStream>(a, capped(rows, cus * 16), (hipStream_t)stream);
        const int rc = (int)hipGetLastError();
        if (rc != 0) return rc;
    }
    hipLaunchKernelGGL(k_kd_finish, dim3(1), dim3(kRowBlock), 0, (hipStream_t)stream, (const float*)row_kl, (const float*)row_nll, rows, kl_scale,
                       nll_scale, loss);
    return (int)hipGetLastError();
}

}  // extern "C"
