// qd_huffman.hip -- Huffman-coded model checkpoints: the chunked canonical-code bitstream of the quantized symbols of a
// whole model, written and read on the device (gfx950).
//
// The reference only accounts for this form (helpers/functions.py:226-262: the Huffman mean code length of
// quantization/help_functions.py:157-232 per quantized weight + 8 B of (alpha, beta) per bucket); compressed.py writes it
// to a file and reads it back with these kernels.  Layout (include/qd_hip.h): every tensor is cut into
// chunks of QD_HUF_CHUNK symbols, chunk c starts on the 32-bit word chunk_words[c], codewords are packed most significant
// bit first.
//
// encode : 3 launches per model -- per-chunk word counts, one exclusive scan over the chunks, the write (each chunk is
//          assembled in LDS with LDS atomics and stored as whole words: chunks never share a word in HBM)
// decode : 1 launch per model -- one lane per chunk (a prefix code is sequential inside a chunk), a 2^10-entry canonical
//          lookup table in LDS plus a slow path for longer codes, dequantization in registers, 64 symbols per lane staged
//          in LDS and stored row by row: each store instruction writes 64 consecutive floats of one chunk.
#include "qd_common.h"

#include "../../include/qd_hip.h"

using namespace qd;

namespace {

constexpr int CHUNK = QD_HUF_CHUNK;
constexpr int LUT_BITS = 10;
constexpr int ROUND = 64;                 // symbols per lane between two staged stores

// the tensor that owns chunk c: the last entry with first_chunk <= c (empty tensors share first_chunk with the next one)
__device__ __forceinline__ int find_tensor(const QdHufTensor* table, int nt, int64_t c) {
    int lo = 0, hi = nt - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_chunk <= c) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(v, off);
        if (lane >= off) v += t;
    }
    return v;
}

// (element offset, symbols) of chunk c inside its tensor
__device__ __forceinline__ void chunk_span(const QdHufTensor& T, int64_t c, int64_t& e0, int& cnt) {
    e0 = (c - T.first_chunk) * CHUNK;
    const int64_t left = T.n - e0;
    cnt = left < CHUNK ? (left > 0 ? (int)left : 0) : CHUNK;
}

// pass 1: words of every chunk (256 lanes, 4 symbols each)
__global__ __launch_bounds__(256) void k_huf_chunk_words(const QdHufTensor* table, int nt, const QdHufCode* code,
                                                         uint32_t* chunk_words) {
    __shared__ uint32_t len[256];
    __shared__ uint32_t part[4];
    const int tid = threadIdx.x;
    len[tid] = code->len[tid];
    const int64_t c = blockIdx.x;
    const QdHufTensor& T = table[find_tensor(table, nt, c)];
    int64_t e0;
    int cnt;
    chunk_span(T, c, e0, cnt);
    const uint8_t* s = T.sym + e0;
    __syncthreads();
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = tid * 4 + j;
        if (i < cnt) bits += len[s[i]];
    }
    bits = wave_sum(bits);
    if ((tid & 63) == 0) part[tid >> 6] = bits;
    __syncthreads();
    if (tid == 0) chunk_words[c] = (part[0] + part[1] + part[2] + part[3] + 31u) >> 5;
}

// pass 2: exclusive scan of the word counts in place, chunk_words[nchunks] = total (one block; tiles of 4096 chunks)
__global__ __launch_bounds__(1024) void k_huf_scan(uint32_t* chunk_words, int64_t nchunks) {
    __shared__ uint32_t wtot[16];
    __shared__ uint32_t carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < nchunks; base += 4096) {
        uint32_t v[4];
        uint32_t mine = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t i = base + tid * 4 + j;
            v[j] = i < nchunks ? chunk_words[i] : 0u;
            mine += v[j];
        }
        const uint32_t incl = wave_incl_scan(mine);
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        uint32_t off = carry;
        for (int w = 0; w < wave; ++w) off += wtot[w];
        uint32_t run = off + incl - mine;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t i = base + tid * 4 + j;
            if (i < nchunks) chunk_words[i] = run;
            run += v[j];
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t t = 0;
            for (int w = 0; w < 16; ++w) t += wtot[w];
            carry += t;
        }
        __syncthreads();
    }
    if (tid == 0) chunk_words[nchunks] = carry;
}

// pass 3: assemble every chunk in LDS (LDS atomics only), then store its whole words
__global__ __launch_bounds__(256) void k_huf_write(const QdHufTensor* table, int nt, const QdHufCode* code,
                                                   const uint32_t* chunk_words, uint32_t* words, int64_t max_words) {
    __shared__ uint32_t cw[256];
    __shared__ uint32_t len[256];
    __shared__ uint32_t lw[CHUNK + 1];
    __shared__ uint32_t part[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    cw[tid] = code->code[tid];
    len[tid] = code->len[tid];
    for (int i = tid; i <= CHUNK; i += 256) lw[i] = 0u;
    const int64_t c = blockIdx.x;
    const QdHufTensor& T = table[find_tensor(table, nt, c)];
    int64_t e0;
    int cnt;
    chunk_span(T, c, e0, cnt);
    const uint8_t* s = T.sym + e0;
    __syncthreads();
    uint32_t sy[4], ln[4], mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = tid * 4 + j;
        sy[j] = i < cnt ? (uint32_t)s[i] : 0u;
        ln[j] = i < cnt ? len[sy[j]] : 0u;
        mine += ln[j];
    }
    const uint32_t incl = wave_incl_scan(mine);
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    uint32_t p = incl - mine;
    for (int w = 0; w < wave; ++w) p += part[w];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t L = ln[j];
        if (L) {
            const uint32_t cd = cw[sy[j]];
            const uint32_t w = p >> 5, off = p & 31u;
            if (off + L <= 32u) {
                atomicOr(&lw[w], cd << (32u - off - L));
            } else {
                atomicOr(&lw[w], cd >> (off + L - 32u));
                atomicOr(&lw[w + 1], cd << (64u - off - L));
            }
            p += L;
        }
    }
    __syncthreads();
    const uint32_t w0 = chunk_words[c];
    uint32_t nw = chunk_words[c + 1] - w0;
    if (nw > (uint32_t)CHUNK) nw = 0;                       // never: a chunk holds at most CHUNK * 32 bits
    if ((int64_t)w0 + (int64_t)nw > max_words) return;      // never for a correctly sized buffer
    for (uint32_t i = tid; i < nw; i += 256) stg_nt(lw[i], words + w0 + i);
}

// one launch for the whole model: lane = chunk, 64 chunks per block
__global__ __launch_bounds__(64) void k_huf_decode(const uint32_t* words, int64_t nwords, const uint32_t* chunk_words,
                                                   const QdHufTensor* table, int nt, int64_t nchunks, const QdHufCode* code,
                                                   const float* alpha, const float* beta, const float* points) {
    __shared__ uint16_t lut[1 << LUT_BITS];                 // symbol | length << 8; length 0: a longer code (slow path)
    __shared__ uint32_t base[33], count[33], first[33];
    __shared__ uint8_t sorted[256];
    __shared__ float stage[64][ROUND + 1];
    __shared__ float* rowp[64];
    __shared__ int rowc[64];
    const int lane = threadIdx.x;
    for (int i = lane; i < 256; i += 64) sorted[i] = code->sorted[i];
    if (lane < 33) { base[lane] = code->base[lane]; count[lane] = code->count[lane]; first[lane] = code->first[lane]; }
    const int single = code->single;
    const int max_len = code->max_len;
    __syncthreads();
    const int lut_len = max_len < LUT_BITS ? max_len : LUT_BITS;
    for (int j = lane; j < (1 << LUT_BITS); j += 64) {
        uint32_t e = 0;
        for (int l = 1; l <= lut_len; ++l) {
            const uint32_t cc = (uint32_t)j >> (LUT_BITS - l);
            if (cc - base[l] < count[l]) { e = (uint32_t)sorted[first[l] + cc - base[l]] | ((uint32_t)l << 8); break; }
        }
        lut[j] = (uint16_t)e;
    }

    const int64_t c = (int64_t)blockIdx.x * 64 + lane;
    const bool active = c < nchunks;
    int cnt = 0;
    int64_t e0 = 0, bucket = 0, bidx = 0, rem = 0, fb = 0;
    int levels = 1, nonuni = 0;
    float* y = nullptr;
    const float* pts = points;
    uint32_t wp = 0, wend = 0;
    if (active) {
        const QdHufTensor& T = table[find_tensor(table, nt, c)];
        chunk_span(T, c, e0, cnt);
        y = T.y + e0;
        bucket = T.bucket;
        levels = T.levels;
        nonuni = T.nonuniform;
        fb = T.first_bucket;
        if (nonuni) pts = points + T.first_point;
        if (bucket > 0) { bidx = e0 / bucket; rem = e0 - bidx * bucket; }
        wp = chunk_words[c];
        const int64_t we = chunk_words[c + 1];
        wend = (uint32_t)(we < nwords ? we : nwords);
    }
    rowp[lane] = y;
    rowc[lane] = cnt;
    float a = 0.0f, b = 0.0f;
    if (cnt > 0) { a = alpha[fb + bidx]; b = beta[fb + bidx]; }
    const float sm1 = (float)(levels - 1);
    uint64_t buf = 0;
    int nb = 0;
    __syncthreads();

    for (int r = 0; r < CHUNK / ROUND; ++r) {
        for (int i = 0; i < ROUND; ++i) {
            const int e = r * ROUND + i;
            if (e >= cnt) break;
            if (nb < 32) {
                const uint32_t w = wp < wend ? words[wp] : 0u;
                ++wp;
                buf |= (uint64_t)w << (32 - nb);
                nb += 32;
            }
            uint32_t sym, L;
            if (single >= 0) {
                sym = (uint32_t)single;
                L = 0;
            } else {
                const uint32_t ent = lut[buf >> (64 - LUT_BITS)];
                sym = ent & 255u;
                L = ent >> 8;
                if (L == 0) {
                    sym = 0xffffu;
                    L = 32;                                 // no codeword (a corrupted stream): skip 32 bits
                    for (int l = LUT_BITS + 1; l <= max_len; ++l) {
                        const uint32_t cc = (uint32_t)(buf >> (64 - l));
                        if (cc - base[l] < count[l]) { sym = sorted[first[l] + cc - base[l]]; L = (uint32_t)l; break; }
                    }
                }
            }
            buf <<= L;
            nb -= (int)L;
            float v;
            if (sym >= (uint32_t)levels) {
                v = __builtin_nanf("");
            } else if (nonuni) {
                const float pt = pts[sym];
                v = pt * a;                                 // K4's rescale: two roundings, then + mean (0)
                v = v + b;
                v = v + 0.0f;
            } else {
                const float w = (float)sym / sm1;           // qd_unpack_uniform_f32's three ops
                v = w * a;
                v = v + b;
                v = v + 0.0f;
            }
            stage[lane][i] = v;
            if (bucket > 0 && ++rem == bucket) {
                rem = 0;
                ++bidx;
                if (e + 1 < cnt) { a = alpha[fb + bidx]; b = beta[fb + bidx]; }
            }
        }
        __syncthreads();
        for (int row = 0; row < 64; ++row) {
            const int e = r * ROUND + lane;
            if (e < rowc[row]) stg_nt(stage[row][lane], rowp[row] + e);
        }
        __syncthreads();
    }
}

int check_table_args(const QdHufTensor* table, int ntensors, int64_t nchunks, const QdHufCode* code) {
    if (!table || !code || ntensors < 1 || nchunks < 1 || nchunks > 0x7fffffffLL) return QD_ERR_INVALID_ARGUMENT;
    return 0;
}

}  // namespace

extern "C" {

int qd_huffman_encode(const QdHufTensor* table, int ntensors, int64_t nchunks, const QdHufCode* code, uint32_t* chunk_words,
                      uint32_t* words, int64_t max_words, void* stream) {
    if (check_table_args(table, ntensors, nchunks, code) || !chunk_words || !words || max_words < 1) return QD_ERR_INVALID_ARGUMENT;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_huf_chunk_words, dim3((unsigned)nchunks), dim3(256), 0, st, table, ntensors, code, chunk_words);
    hipLaunchKernelGGL(k_huf_scan, dim3(1), dim3(1024), 0, st, chunk_words, nchunks);
    hipLaunchKernelGGL(k_huf_write, dim3((unsigned)nchunks), dim3(256), 0, st, table, ntensors, code, chunk_words, words, max_words);
    return (int)hipGetLastError();
}

int qd_huffman_decode_f32(const uint32_t* words, int64_t nwords, const uint32_t* chunk_words, const QdHufTensor* table,
                          int ntensors, int64_t nchunks, const QdHufCode* code, const float* alpha, const float* beta,
                          const float* points, void* stream) {
    if (check_table_args(table, ntensors, nchunks, code) || !chunk_words || !alpha || !beta || nwords < 0 ||
        (nwords > 0 && !words))
        return QD_ERR_INVALID_ARGUMENT;
    const unsigned blocks = (unsigned)((nchunks + 63) / 64);
    hipLaunchKernelGGL(k_huf_decode, dim3(blocks), dim3(64), 0, (hipStream_t)stream, words, nwords, chunk_words, table, ntensors,
                       nchunks, code, alpha, beta, points);
    return (int)hipGetLastError();
}

}  // extern "C"
