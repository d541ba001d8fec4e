// qd_multi_symbols.hip -- the symbols of a whole model in one launch (K9s): what save_compressed stores of a uniformly quantized
// tensor -- the uint8 level index of every weight and the (alpha, beta) of every bucket -- for every tensor of a device table of
// QdSymbolDesc, each under its own level count and its own bucket size (per-channel scales).
//   qd_multi_symbols_plan, qd_multi_uniform_symbols_u8   k_multi_symbols: per tensor the level_idx / alpha / beta bits of
//   qd_uniform_f32(x_i, <scratch>, n_i, buckets[i], levels[i], alpha + first_bucket_i, beta + first_bucket_i, sym_i, ...).
// The per-tensor loop it replaces writes the fp32 result into a scratch tensor nobody reads: 4 B read + 4 B + 1 B written per
// element and a launch per tensor; here 4 B read + 1 B written and one launch.  Deterministic rounding, no clamp, no mean: the
// only configuration a compressed checkpoint stores.
//
// The loop is the one of k_multi_uniform_bk (qd_multi_uniform.hip): a wave strides over the tiles the plan counted with
// bucket_tiles (qd_multi.h), owner_of finds the tensor, levels[ti] and buckets[ti] are read with the descriptor and the tensor's
// geometry is re-derived whenever the wave moves on to another tensor.  The bodies are its five, written here from the
// primitives of qd_common.h without the fp32 store -- of the seven operations of qdq a symbol needs four:
//     level = rint(((v - beta) / alpha) * (s - 1))
//   row <= 256, a DPP row per bucket: a full row of 64 / 128 / 256 of a 16-byte aligned x is held in registers (sym_reg_row);
//     any other full row that is a multiple of 4 is read as float4 in two passes (sym_lanes4<16>); a ragged last row, a row
//     that is no multiple of 4 and an unaligned x go element by element (sym_lanes<16>);
//   row > 256, the wave per bucket in two passes: sym_lanes4<64> / sym_lanes<64> by the same rule.
// The float4 bodies hold four consecutive symbols per lane: one 4-byte store where sym + lo is 4-byte aligned, four 1-byte
// stores where it is not.  Which body runs and which store it takes never changes a bit: min / max do not depend on the order,
// the rest is element-wise, and the bucket-invariant division stands in for the IEEE one only where fastdiv_ok proves them equal
// (qd_common.h; only the LEVEL of the quotient is consumed here).
#include <type_traits>

#include "qd_common.h"
#include "qd_multi.h"
#include "../../include/qd_hip.h"

using namespace qd;

namespace {

// The symbol stores carry the non-temporal hint although the histogram and the encoder of save_compressed read the symbols back
// at once.  Measured both ways in one process on the 60 WRN-16-22 tensors (profiles/multi_symbols_store_ab.json): with
// per-channel bucket sizes the hint wins alone (122.2 against 129.7 us) and with the histogram behind it (144.0 against
// 147.1 us), disjoint ranges both; at [256] * 60 the two are within 2 % of each other (70.2 / 71.0 us alone, 93.0 / 91.3 us
// with the histogram).  false: plain stores.
constexpr bool kSymNT = true;

template <typename T>
__device__ __forceinline__ void store_sym(const T& v, T* p) {
    if (kSymNT) stg_nt(v, p); else stg(v, p);
}

// The level of one element: four separately rounded fp32 operations, the first four of qdq (qd_common.h).
template <bool FAST>
__device__ __forceinline__ float sym_level(float v, float a, float b, float sm1, float y) {
    float u = v - b;
    u = div_alpha<FAST>(u, a, y);
    const float t = u * sm1;
    return rintf(t);
}
// ... as the byte store_side1<MODE_QDQ> stores (qd_element.h): (uint8_t)(int)level -- v_cvt_i32_f32, a NaN level is 0
__device__ __forceinline__ uint32_t sym_byte(float level) { return (uint32_t)(uint8_t)(int)level; }

// four levels of one float4 at sym + e: one 4-byte store (s4: sym + e is 4-byte aligned) or four 1-byte stores, the same bytes
template <bool FAST>
__device__ __forceinline__ void store_sym4(const f4& v, float a, float b, float sm1, float y, uint8_t* dst, bool s4) {
    const uint32_t s0 = sym_byte(sym_level<FAST>(v.x, a, b, sm1, y)), s1 = sym_byte(sym_level<FAST>(v.y, a, b, sm1, y));
    const uint32_t s2 = sym_byte(sym_level<FAST>(v.z, a, b, sm1, y)), s3 = sym_byte(sym_level<FAST>(v.w, a, b, sm1, y));
    if (s4) {
        store_sym(s0 | (s1 << 8) | (s2 << 16) | (s3 << 24), (uint32_t*)dst);
    } else {
        store_sym((uint8_t)s0, dst); store_sym((uint8_t)s1, dst + 1); store_sym((uint8_t)s2, dst + 2); store_sym((uint8_t)s3, dst + 3);
    }
}

// The lanes of the wave that are in a body together take the bucket-invariant division when every one of their buckets is in
// the proven range (a scalar branch), else the IEEE one: call(std::true_type / std::false_type, y).
template <typename Body>
__device__ __forceinline__ void with_division(float a, Body body) {
    if (!__any(!fastdiv_ok(a))) body(std::true_type{}, 1.0f / a); else body(std::false_type{}, 0.0f);
}

// (alpha, beta) of a bucket: written by the first lane of the group that owns it
__device__ __forceinline__ void store_ab(float a, float b, float* alpha, float* beta, int64_t bkt, int l) {
    if (l == 0) { stg(a, alpha + bkt); stg(b, beta + bkt); }
}

// ---- one full bucket row of 64 V elements in the registers of the 16 lanes of a DPP row (l: the lane's place in it) ----
// x + lo 16-byte aligned.  The reduction of reg_row (qd_multi_uniform.h): NaN-propagating min / max, no flag.
template <int V>
__device__ __forceinline__ void sym_reg_row(const float* x, uint8_t* sym, int64_t lo, int64_t bkt, int l, float sm1, bool s4,
                                            float* alpha, float* beta) {
    const f4* src = (const f4*)(x + lo) + l;
    f4 v[V];
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = ldg_nt(src + j * 16);   // masters: read once
    float mn = pmin4(v[0]), mx = pmax4(v[0]);
#pragma unroll
    for (int j = 1; j < V; ++j) { mn = pmin(mn, pmin4(v[j])); mx = pmax(mx, pmax4(v[j])); }
    mn = row16_min(mn); mx = row16_max(mx);
    float a, b;
    alpha_beta(mn, mx, a, b);
    store_ab(a, b, alpha, beta, bkt, l);
    uint8_t* dst = sym + lo + l * 4;
    with_division(a, [&](auto fast, float y) {
#pragma unroll
        for (int j = 0; j < V; ++j) store_sym4<decltype(fast)::value>(v[j], a, b, sm1, y, dst + j * 64, s4);
    });
}

// ---- LANES lanes (16: a DPP row, 64: the wave) and one arbitrary bucket [lo, hi): element by element, two passes (the second
// is served by L1 / L2).  The reduction of bucket_lanes (qd_element.h): fminf / fmaxf and a NaN flag.
template <int LANES>
__device__ __forceinline__ void sym_lanes(const float* x, uint8_t* sym, int64_t lo, int64_t hi, int64_t bkt, int l, float sm1,
                                          float* alpha, float* beta) {
    float mn = INFINITY, mx = -INFINITY;
    bool nan = false;
    for (int64_t i = lo + l; i < hi; i += LANES) {
        const float v = ldg(x + i);
        mn = fminf(mn, v); mx = fmaxf(mx, v);
        nan |= (v != v);
    }
    if (LANES == 16) { mn = row16_min(mn); mx = row16_max(mx); }
    else { mn = wave_min(mn); mx = wave_max(mx); }
    if (group_any<LANES>(nan)) { mn = NAN; mx = NAN; }
    float a, b;
    alpha_beta(mn, mx, a, b);
    store_ab(a, b, alpha, beta, bkt, l);
    with_division(a, [&](auto fast, float y) {
        for (int64_t i = lo + l; i < hi; i += LANES)
            store_sym((uint8_t)sym_byte(sym_level<decltype(fast)::value>(ldg(x + i), a, b, sm1, y)), sym + i);
    });
}

// ---- the same for a FULL bucket of `row` elements, row a multiple of 4 and x + lo 16-byte aligned: float4 reads ----
template <int LANES>
__device__ __forceinline__ void sym_lanes4(const float* x, uint8_t* sym, int64_t lo, int64_t row, int64_t bkt, int l, float sm1,
                                           bool s4, float* alpha, float* beta) {
    const int64_t nv = row >> 2;
    const f4* src = (const f4*)(x + lo);
    float mn = INFINITY, mx = -INFINITY;
    bool nan = false;
    for (int64_t i = l; i < nv; i += LANES) {
        const f4 v = ldg(src + i);
        mn = fminf(mn, fminf(fminf(v.x, v.y), fminf(v.z, v.w)));
        mx = fmaxf(mx, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
        nan |= has_nan4(v);
    }
    if (LANES == 16) { mn = row16_min(mn); mx = row16_max(mx); }
    else { mn = wave_min(mn); mx = wave_max(mx); }
    if (group_any<LANES>(nan)) { mn = NAN; mx = NAN; }
    float a, b;
    alpha_beta(mn, mx, a, b);
    store_ab(a, b, alpha, beta, bkt, l);
    with_division(a, [&](auto fast, float y) {
        for (int64_t i = l; i < nv; i += LANES)
            store_sym4<decltype(fast)::value>(ldg(src + i), a, b, sm1, y, sym + lo + (i << 2), s4);
    });
}

// A wave takes the tiles wave, wave + nwaves, ...; uniform_wave_index() is scalar, so the tile -> tensor search, the descriptor
// and the two per-tensor arrays are read with scalar loads.  nb is the number of buckets of the tensor that are reached: what
// buckets[ti] gives, never more than the plan gave the tensor where the table says how many that is (the next descriptor's
// first_bucket), so that an array that disagrees with the plan stays inside the tensor's own alpha / beta rows; an entry < 1
// reaches none.  Symbol addresses are bounded by n whatever the arrays hold.
__global__ __launch_bounds__(256) void k_multi_symbols(const QdSymbolDesc* __restrict__ table, const int32_t* __restrict__ levels,
                                                       const int64_t* __restrict__ buckets, int ntensors, int64_t total_tiles,
                                                       float* __restrict__ alpha, float* __restrict__ beta) {
    const int lane = threadIdx.x & 63;
    const int sub = lane >> 4, l = lane & 15;
    const int64_t wave = uniform_wave_index();
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    int cur = -1;                                   // the tensor sm1 and geo belong to
    float sm1 = 1.0f;
    BucketTiles geo;
    geo.row = 1; geo.nb = 0; geo.tiles = 0; geo.wave = false;
    for (int64_t t = wave; t < total_tiles; t += nwaves) {
        const int ti = owner_of(table, ntensors, t);
        const QdSymbolDesc d = table[ti];
        if (d.n <= 0) continue;                     // (an empty tensor owns no tile)
        if (ti != cur) {
            cur = ti;
            sm1 = (float)(levels[ti] - 1);
            const int64_t bucket = buckets[ti];
            geo = bucket_tiles(d.n, bucket > 0 ? bucket : 1);
            if (bucket <= 0) geo.nb = 0;            // no bucket of this tensor is reached
            if (ti + 1 < ntensors) {
                const int64_t own = table[ti + 1].first_bucket - d.first_bucket;
                if (geo.nb > own) geo.nb = own > 0 ? own : 0;
            }
        }
        const int64_t local = t - d.first_tile;
        const bool row4 = ((((uintptr_t)d.x) & 15) == 0) && (geo.row & 3) == 0;   // rows that are a multiple of 4 then start aligned
        const bool s4 = (((uintptr_t)d.sym) & 3) == 0;                           // ... and so do their symbols
        float* const al = alpha + d.first_bucket;
        float* const be = beta + d.first_bucket;
        if (geo.wave) {
            const int64_t bkt = local;
            if (bkt >= geo.nb) continue;            // (a tile count that does not belong to this table reaches no bucket)
            const int64_t lo = bkt * geo.row;
            const int64_t hi = lo + geo.row < d.n ? lo + geo.row : d.n;
            if (row4 && hi - lo == geo.row) sym_lanes4<64>(d.x, d.sym, lo, geo.row, bkt, lane, sm1, s4, al, be);
            else sym_lanes<64>(d.x, d.sym, lo, hi, bkt, lane, sm1, al, be);
        } else {
            const int64_t bkt = local * 4 + sub;
            if (bkt >= geo.nb) continue;
            const int64_t lo = bkt * geo.row;
            const int64_t hi = lo + geo.row < d.n ? lo + geo.row : d.n;
            if (row4 && hi - lo == geo.row) {
                if (geo.row == 256) sym_reg_row<4>(d.x, d.sym, lo, bkt, l, sm1, s4, al, be);
                else if (geo.row == 128) sym_reg_row<2>(d.x, d.sym, lo, bkt, l, sm1, s4, al, be);
                else if (geo.row == 64) sym_reg_row<1>(d.x, d.sym, lo, bkt, l, sm1, s4, al, be);
                else sym_lanes4<16>(d.x, d.sym, lo, geo.row, bkt, l, sm1, s4, al, be);
            } else {
                sym_lanes<16>(d.x, d.sym, lo, hi, bkt, l, sm1, al, be);
            }
        }
    }
}

}  // namespace

extern "C" {

int qd_multi_symbols_plan(QdSymbolDesc* host_table, const int64_t* buckets, int ntensors, int64_t* total_tiles_out,
                          int64_t* total_buckets_out) {
    if (!host_table || !buckets || ntensors <= 0 || !total_tiles_out || !total_buckets_out) return QD_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < ntensors; ++i) {
        const QdSymbolDesc& d = host_table[i];
        if (buckets[i] <= 0 || d.n < 0 || (d.n > 0 && (!d.x || !d.sym))) return QD_ERR_INVALID_ARGUMENT;
    }
    int64_t nb = 0;
    *total_tiles_out = fill_prefix(host_table, ntensors, [host_table, buckets, &nb](QdSymbolDesc& d) -> int64_t {
        d.first_bucket = nb;
        if (d.n <= 0) return 0;
        const BucketTiles g = bucket_tiles(d.n, buckets[&d - host_table]);       // (the descriptor's position)
        nb += g.nb;
        return g.tiles;
    });
    *total_buckets_out = nb;
    return 0;
}

int qd_multi_uniform_symbols_u8(const QdSymbolDesc* table, const int32_t* levels, const int64_t* buckets, int ntensors,
                                int64_t total_tiles, float* alpha, float* beta, void* stream) {
    if (!table || ntensors <= 0 || total_tiles < 0 || !levels || !buckets || !alpha || !beta) return QD_ERR_INVALID_ARGUMENT;
    if ((((uintptr_t)levels) & 3) || (((uintptr_t)buckets) & 7) || (((uintptr_t)alpha) & 3) || (((uintptr_t)beta) & 3))
        return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    hipLaunchKernelGGL(k_multi_symbols, dim3(grid_blocks(total_tiles, 4, kNoOwnCap)), dim3(256), 0, (hipStream_t)stream, table,
                       levels, buckets, ntensors, total_tiles, alpha, beta);
    return (int)hipGetLastError();
}

}  // extern "C"
