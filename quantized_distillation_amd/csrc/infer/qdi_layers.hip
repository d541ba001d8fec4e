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
#include "qdi_packed.h"       // Packed, describe, stream_bits, divmod, build_quotients, decode4, the host helpers: shared with the MFMA libraries

#include "../../../include/qd_infer.h"

using namespace qd;

namespace {

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

}  // namespace

extern "C" {

int qdi_abi_version(void) { return QDI_ABI_VERSION; }
const char* qdi_target_arch(void) { return "gfx950"; }

const char* qdi_error_string(int code) { return error_string(code, QDI_ERR_INVALID_ARGUMENT); }
int qdi_set_grid_cap(int blocks) { return set_grid_cap(blocks); }

int qdi_embedding_packed_f32(const uint8_t* packed, const float* alpha, const float* beta, int64_t rows, int64_t cols, int64_t bucket,
                             int levels, int bits, const int64_t* idx, int64_t count, float* out, void* stream) {
    Packed P;
    if (!describe(P, packed, alpha, beta, rows, cols, bucket, levels, bits) || count < 0) return QDI_ERR_INVALID_ARGUMENT;
    if ((((uintptr_t)idx) & 7) || misaligned(out)) return QDI_ERR_INVALID_ARGUMENT;
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
    if (misaligned(x) || misaligned(bias) || misaligned(y)) return QDI_ERR_INVALID_ARGUMENT;
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
