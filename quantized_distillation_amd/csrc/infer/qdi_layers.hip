// qdi_layers.hip -- libqd_infer.so: Embedding and Linear computed from the packed level indices of a quantized weight
// (include/qd_infer.h), gfx950.  Nothing here is linked into libqd_hip.so, and nothing of that library is needed to run it.
//
// Both kernels are sweeps over the packed stream -- bits / 8 bytes per weight -- without MFMA:
//   k_embedding       an element-wise gather bound by the 4 B per element it writes: a lane decodes four consecutive weights
//                     of one row and stores them (16 bytes at once where the address allows it);
//   k_linear<MT>      a GEMV-like sweep for a handful of rows of x (decode time: batch x beam): one wave per output row,
//                     a lane decodes four consecutive weights per trip and feeds MT accumulators, one per row of x; one
//                     cross-lane tree at the end.  m > 8 re-decodes the weights per tile of 8 rows (functional, not tuned).
// The level index -> c / (levels - 1) quotient comes from a table in LDS that each block builds with the correctly rounded
// division the codec uses (qd_codec.hip: k_unpack_any), so a weight is bit for bit what qd_unpack_uniform_f32 writes and
// no lane divides per element.  The bucket of an element is found with one division per lane and row (linear) or per
// group of four (embedding); inside a group an element that leaves the group's first bucket steps on (three buckets at the most).
#include "../qd_common.h"

#include "../../../include/qd_infer.h"

using namespace qd;

namespace {

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));     // a 16-byte access at the 4-byte alignment of fp32 data

int g_grid_cap = 0;                                                    // qdi_set_grid_cap: 0 = none

int capped(int64_t blocks, int64_t own_cap) {
    if (blocks > own_cap) blocks = own_cap;
    if (g_grid_cap >= 1 && blocks > g_grid_cap) blocks = g_grid_cap;
    return blocks < 1 ? 1 : (int)blocks;
}

// By-value description of the packed weight, shared by both kernels.
struct Packed {
    const uint8_t* packed;
    const float* alpha;
    const float* beta;
    int64_t rows, cols;
    int64_t nbytes;          // of the stream: ceil(rows cols bits / 8)
    int64_t bucket;          // EFFECTIVE bucket: rows cols where the tensor is one bucket, so e / bucket is the bucket of e
    int levels, bits;
    int small;               // rows cols < 2^32: 32-bit divisions
};

// The 32 stream bits from bit p on (a group of four level indices is 4 bits <= 32 bits of them): two aligned 32-bit words
// and a shift where both lie wholly inside the stream, byte by byte (five at the most) at its end -- group_bits of
// qd_codec.hip for every width.
__device__ __forceinline__ uint32_t stream_bits(const uint8_t* packed, int64_t p, int64_t nbytes) {
    const int64_t w = p >> 5;
    if ((w + 2) * 4 <= nbytes) {
        const uint32_t lo = ((const uint32_t*)packed)[w], hi = ((const uint32_t*)packed)[w + 1];
        return (uint32_t)((((uint64_t)hi << 32) | lo) >> (p & 31));
    }
    uint64_t acc = 0;
    const int64_t b0 = p >> 3;
    for (int c = 0; c < 5 && b0 + c < nbytes; ++c) acc |= (uint64_t)packed[b0 + c] << (8 * c);
    return (uint32_t)(acc >> (p & 7));
}

__device__ __forceinline__ void divmod(int64_t a, int64_t b, int small, int64_t& q, int64_t& r) {
    if (small) { q = (uint32_t)a / (uint32_t)b; } else { q = a / b; }
    r = a - q * b;
}

// The `levels` quotients c / (levels - 1), each the correctly rounded fp32 division of k_unpack_any.
__device__ __forceinline__ void build_quotients(float* qtab, int levels) {
    const float sm1 = (float)(levels - 1);
    for (int c = threadIdx.x; c < levels; c += blockDim.x) qtab[c] = (float)c / sm1;
    __syncthreads();
}

// The nv <= 4 weights of the group whose first element is e (bucket bkt, rem elements into it): w[c] for c < nv.
__device__ __forceinline__ void decode4(const Packed& P, const float* qtab, int64_t e, int64_t bkt, int64_t rem, int nv, float (&w)[4]) {
    const uint32_t code = stream_bits(P.packed, e * P.bits, P.nbytes);
    const uint32_t mask = (1u << P.bits) - 1u;
    const float a0 = P.alpha[bkt], b0 = P.beta[bkt];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        w[c] = 0.0f;
        if (c < nv) {
            float a = a0, b = b0;
            if (rem + c >= P.bucket) {                                   // the group leaves its first bucket (bucket < 4: more than once)
                int64_t bc = bkt, rr = rem + c;
                do { rr -= P.bucket; ++bc; } while (rr >= P.bucket);     // rem < bucket and c <= 3: three steps at the most
                a = P.alpha[bc]; b = P.beta[bc];
            }
            float v = qtab[(code >> (c * P.bits)) & mask] * a;          // the three operations after the division, each rounded
            v = v + b;
            w[c] = v + 0.0f;
        }
    }
}

__global__ __launch_bounds__(256) void k_embedding(Packed P, const int64_t* idx, int64_t count, float* out) {
    __shared__ float qtab[256];
    build_quotients(qtab, P.levels);
    const int64_t gpr = (P.cols + 3) >> 2;                               // groups of four per row
    const int64_t total = count * gpr;
    const int small_total = total < ((int64_t)1 << 32);
    const int64_t nth = (int64_t)gridDim.x * blockDim.x;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += nth) {
        int64_t j, cg;
        divmod(g, gpr, small_total, j, cg);
        const int64_t c0 = cg << 2;
        const int nv = P.cols - c0 < 4 ? (int)(P.cols - c0) : 4;
        const int64_t r = idx[j];
        float w[4];
        if (r < 0 || r >= P.rows) {
            w[0] = w[1] = w[2] = w[3] = __int_as_float(0x7FC00000);
        } else {
            const int64_t e = r * P.cols + c0;
            int64_t bkt, rem;
            divmod(e, P.bucket, P.small, bkt, rem);
            decode4(P, qtab, e, bkt, rem, nv, w);
        }
        float* o = out + j * P.cols + c0;
        if (nv == 4 && (((uintptr_t)o) & 15) == 0) {
            const f4 v = {w[0], w[1], w[2], w[3]};
            *(f4*)o = v;
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) if (c < nv) o[c] = w[c];
        }
    }
}

// the fixed tree of include/qd_infer.h: every lane ends with the same bits (fp32 addition commutes)
__device__ __forceinline__ float wave_tree_sum(float v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_xor(v, s);
    return v;
}

template <int MT>
__global__ __launch_bounds__(256) void k_linear(Packed P, const float* x, int64_t m, const float* bias, float* y,
                                                int64_t step_q, int64_t step_r /* 256 = step_q bucket + step_r */) {
    __shared__ float qtab[256];
    build_quotients(qtab, P.levels);
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t r = uniform_wave_index(); r < P.rows; r += nwaves) {
        int64_t bkt0, rem0;
        divmod(r * P.cols + 4 * lane, P.bucket, P.small, bkt0, rem0);
        for (int64_t i0 = 0; i0 < m; i0 += MT) {
            const float* xr[MT];
#pragma unroll
            for (int t = 0; t < MT; ++t) xr[t] = x + (i0 + t < m ? i0 + t : m - 1) * P.cols + 4 * lane;   // per lane; a row past m: read row m - 1, store nothing
            float acc[MT];
#pragma unroll
            for (int t = 0; t < MT; ++t) acc[t] = 0.0f;
            int64_t bkt = bkt0, rem = rem0;
            for (int64_t c0 = 4 * lane, trip = 0; c0 < P.cols; c0 += 256, trip += 256) {
                const int nv = P.cols - c0 < 4 ? (int)(P.cols - c0) : 4;
                float w[4];
                decode4(P, qtab, r * P.cols + c0, bkt, rem, nv, w);
                if (nv == 4) {
#pragma unroll
                    for (int t = 0; t < MT; ++t) {
                        const f4u xv = *(const f4u*)(xr[t] + trip);
                        acc[t] = fmaf(xv.x, w[0], acc[t]);
                        acc[t] = fmaf(xv.y, w[1], acc[t]);
                        acc[t] = fmaf(xv.z, w[2], acc[t]);
                        acc[t] = fmaf(xv.w, w[3], acc[t]);
                    }
                } else {
#pragma unroll
                    for (int t = 0; t < MT; ++t) {
#pragma unroll
                        for (int c = 0; c < 4; ++c) if (c < nv) acc[t] = fmaf(xr[t][trip + c], w[c], acc[t]);
                    }
                }
                bkt += step_q; rem += step_r;
                if (rem >= P.bucket) { rem -= P.bucket; ++bkt; }
            }
            const float b = bias ? bias[r] : 0.0f;
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                const float v = wave_tree_sum(acc[t]);
                if (lane == t && i0 + t < m) y[(i0 + t) * P.rows + r] = bias ? v + b : v;
            }
        }
    }
}

bool describe(Packed& P, const uint8_t* packed, const float* alpha, const float* beta, int64_t rows, int64_t cols, int64_t bucket,
              int levels, int bits) {
    if (rows < 0 || cols < 0 || bucket < 0 || levels < 2 || levels > 256 || bits < 1 || bits > 8 || levels > (1 << bits)) return false;
    int64_t n = 0, nbits = 0;
    if (__builtin_mul_overflow(rows, cols, &n) || __builtin_mul_overflow(n, (int64_t)bits, &nbits) || nbits > INT64_MAX - 64) return false;
    if ((((uintptr_t)packed) & 3) || (((uintptr_t)alpha) & 3) || (((uintptr_t)beta) & 3)) return false;
    P.packed = packed; P.alpha = alpha; P.beta = beta;
    P.rows = rows; P.cols = cols;
    P.nbytes = (nbits + 7) >> 3;
    P.bucket = (bucket == 0 || n < bucket) ? (n > 0 ? n : 1) : bucket;
    P.levels = levels; P.bits = bits;
    P.small = n < ((int64_t)1 << 32);
    return true;
}

}  // namespace

extern "C" {

int qdi_abi_version(void) { return QDI_ABI_VERSION; }
const char* qdi_target_arch(void) { return "gfx950"; }

const char* qdi_error_string(int code) {
    if (code == 0) return "success";
    if (code == QDI_ERR_INVALID_ARGUMENT) return "invalid argument";
    if (code > 0) return hipGetErrorString((hipError_t)code);
    return "unknown error";
}

int qdi_set_grid_cap(int blocks) {
    const int prev = g_grid_cap;
    g_grid_cap = blocks >= 1 ? blocks : 0;
    return prev;
}

int qdi_embedding_packed_f32(const uint8_t* packed, const float* alpha, const float* beta, int64_t rows, int64_t cols, int64_t bucket,
                             int levels, int bits, const int64_t* idx, int64_t count, float* out, void* stream) {
    Packed P;
    if (!describe(P, packed, alpha, beta, rows, cols, bucket, levels, bits) || count < 0) return QDI_ERR_INVALID_ARGUMENT;
    if ((((uintptr_t)idx) & 7) || (((uintptr_t)out) & 3)) return QDI_ERR_INVALID_ARGUMENT;
    int64_t nout = 0;
    if (__builtin_mul_overflow(count, (cols + 3) >> 2, &nout) || nout > INT64_MAX / 4) return QDI_ERR_INVALID_ARGUMENT;
    if (count == 0 || cols == 0) return 0;
    if (!idx || !out || (rows > 0 && (!packed || !alpha || !beta))) return QDI_ERR_INVALID_ARGUMENT;
    const int blocks = capped((nout + 255) / 256, (int64_t)device_cus() * 16);
    hipLaunchKernelGGL(k_embedding, dim3(blocks), dim3(256), 0, (hipStream_t)stream, P, idx, count, out);
    return (int)hipGetLastError();
}

int qdi_linear_packed_f32(const uint8_t* packed, const float* alpha, const float* beta, int64_t rows, int64_t cols, int64_t bucket,
                          int levels, int bits, const float* x, int64_t m, const float* bias, float* y, void* stream) {
    Packed P;
    if (!describe(P, packed, alpha, beta, rows, cols, bucket, levels, bits) || m < 0) return QDI_ERR_INVALID_ARGUMENT;
    if ((((uintptr_t)x) & 3) || (((uintptr_t)bias) & 3) || (((uintptr_t)y) & 3)) return QDI_ERR_INVALID_ARGUMENT;
    int64_t t = 0;
    if (__builtin_mul_overflow(m, rows, &t) || __builtin_mul_overflow(m, cols, &t)) return QDI_ERR_INVALID_ARGUMENT;
    if (m == 0 || rows == 0) return 0;
    if (!y || (cols > 0 && (!packed || !alpha || !beta || !x))) return QDI_ERR_INVALID_ARGUMENT;
    const int blocks = capped((rows + 3) / 4, (int64_t)device_cus() * 8);
    const int64_t step_q = 256 / P.bucket, step_r = 256 % P.bucket;
    hipStream_t st = (hipStream_t)stream;
    if (m > 4) hipLaunchKernelGGL((k_linear<8>), dim3(blocks), dim3(256), 0, st, P, x, m, bias, y, step_q, step_r);
    else if (m > 2) hipLaunchKernelGGL((k_linear<4>), dim3(blocks), dim3(256), 0, st, P, x, m, bias, y, step_q, step_r);
    else if (m == 2) hipLaunchKernelGGL((k_linear<2>), dim3(blocks), dim3(256), 0, st, P, x, m, bias, y, step_q, step_r);
    else hipLaunchKernelGGL((k_linear<1>), dim3(blocks), dim3(256), 0, st, P, x, m, bias, y, step_q, step_r);
    return (int)hipGetLastError();
}

}  // extern "C"
