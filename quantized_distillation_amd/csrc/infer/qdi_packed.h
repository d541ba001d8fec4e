// qdi_packed.h -- the packed weight of include/qd_infer.h as the inference kernels see it: its by-value description, the
// argument checks every entry point starts with, the decode of a group of four consecutive weights, and the few host lines
// every entry file needs (grid cap, error string, alignment test).  Shared by all four inference libraries -- qdi_layers.hip
// (libqd_infer.so) directly; qdm_linear.hip (libqd_infer_mm.so), qdc_conv2d.hip (libqd_infer_conv.so) and qdr_lstm.hip
// (libqd_infer_rnn.so) through qdi_mm.h: one header for the weight value (decode4, and its loop again in finish4 -- see there),
// so every library gives, bit for bit, what qd_unpack_uniform_f32 writes.
//
// Everything sits in an unnamed namespace on purpose: each library is one translation unit, nothing here is exported, and
// the kernels' mangled names (which carry Packed) stay what they were when these lines lived in qdi_layers.hip.
#pragma once

#include "../qd_common.h"

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));     // a 16-byte access at the 4-byte alignment of fp32 data

namespace {

// By-value description of the packed weight, shared by all kernels.
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

// decode4 in two halves, for the kernels that issue a group's loads a slab ahead of its arithmetic (qdi_mm.h).
// fetch4 is LOADS ONLY: the two aligned stream words of stream_bits' common case, unshifted, and the (alpha, beta) of the
// first element's bucket.  Nothing is computed from a loaded value, so the compiler has no reason to wait for one before the
// caller's next instruction (with the shift in here every group's loads were followed by s_waitcnt vmcnt(0): one full memory
// latency per group).  finish4 shifts -- or, for the few groups at the very end of the stream, reads them byte by byte as
// stream_bits does -- and then runs decode4's loop.  The loop is decode4's, line for line: the weight value is written down
// twice in this header and the two must stay the same.  (decode4 is not written as finish4(fetch4()): the compiler then
// orders the loads of k_embedding and k_linear differently, and libqd_infer.so's device code is to stay byte for byte what
// it was.)
__device__ __forceinline__ bool stream_words_inside(const Packed& P, int64_t p) { return ((p >> 5) + 2) * 4 <= P.nbytes; }

// lo, hi: the stream words p >> 5 and (p >> 5) + 1, p = e bits -- left as they are where the two are not both inside the stream
// (finish4 does not look at them then); a0, b0: alpha and beta of bucket bkt.  Plain outputs, no struct and no default value:
// a loaded register that is copied or merged with a constant is a register the compiler waits for.
__device__ __forceinline__ void fetch4(const Packed& P, int64_t e, int64_t bkt, uint32_t& lo, uint32_t& hi, float& a0, float& b0) {
    const int64_t p = e * P.bits;
    if (stream_words_inside(P, p)) {
        lo = ((const uint32_t*)P.packed)[p >> 5];
        hi = ((const uint32_t*)P.packed)[(p >> 5) + 1];
    }
    a0 = P.alpha[bkt];
    b0 = P.beta[bkt];
}

// The nv <= 4 weights of the fetched group whose first element is e (bucket bkt, rem elements into it): w[c] for c < nv, 0 for the rest.
__device__ __forceinline__ void finish4(const Packed& P, const float* qtab, uint32_t lo, uint32_t hi, float a0, float b0, int64_t e, int64_t bkt,
                                        int64_t rem, int nv, float (&w)[4]) {
    const int64_t p = e * P.bits;
    const uint32_t code = stream_words_inside(P, p) ? (uint32_t)((((uint64_t)hi << 32) | lo) >> (p & 31)) : stream_bits(P.packed, p, P.nbytes);
    const uint32_t mask = (1u << P.bits) - 1u;
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

// A pointer to fp32 data (or the packed stream, read as 32-bit words) that is not 4-byte aligned; NULL is aligned.
inline bool misaligned(const void* p) { return (((uintptr_t)p) & 3) != 0; }

// The checks of include/qd_infer.h that concern the weight alone, and its description.  false: refuse the call.
inline bool describe(Packed& P, const uint8_t* packed, const float* alpha, const float* beta, int64_t rows, int64_t cols, int64_t bucket,
                     int levels, int bits) {
    if (rows < 0 || cols < 0 || bucket < 0 || levels < 2 || levels > 256 || bits < 1 || bits > 8 || levels > (1 << bits)) return false;
    int64_t n = 0, nbits = 0;
    if (__builtin_mul_overflow(rows, cols, &n) || __builtin_mul_overflow(n, (int64_t)bits, &nbits) || nbits > INT64_MAX - 64) return false;
    if (misaligned(packed) || misaligned(alpha) || misaligned(beta)) return false;
    P.packed = packed; P.alpha = alpha; P.beta = beta;
    P.rows = rows; P.cols = cols;
    P.nbytes = (nbits + 7) >> 3;
    P.bucket = (bucket == 0 || n < bucket) ? (n > 0 ? n : 1) : bucket;
    P.levels = levels; P.bits = bits;
    P.small = n < ((int64_t)1 << 32);
    return true;
}

// The test hook q??_set_grid_cap of every library: blocks per launch, 0 = none.  One variable per library, since each library
// is one translation unit.
int g_grid_cap = 0;

inline int set_grid_cap(int blocks) {
    const int prev = g_grid_cap;
    g_grid_cap = blocks >= 1 ? blocks : 0;
    return prev;
}

// The blocks of a launch: what the problem asks for, at most the kernel's own cap and the test hook's, at least one.
inline int capped(int64_t blocks, int64_t own_cap) {
    if (blocks > own_cap) blocks = own_cap;
    if (g_grid_cap >= 1 && blocks > g_grid_cap) blocks = g_grid_cap;
    return blocks < 1 ? 1 : (int)blocks;
}

// q??_error_string of every library; invalid_argument: its Q??_ERR_INVALID_ARGUMENT.
inline const char* error_string(int code, int invalid_argument) {
    if (code == 0) return "success";
    if (code == invalid_argument) return "invalid argument";
    if (code > 0) return hipGetErrorString((hipError_t)code);
    return "unknown error";
}

}  // namespace
