// qd_ste.hip -- the straight-through-estimator (STE) backward kernels; like those of qd_reductions.hip, no instantiations of
// the bucket-transform template (qd_transform.h):
//   K7  qd_ste_bucket_backward_f32  uniformQuantization_variable.backward     quantization/quant_functions.py:319-406
//   K8  qd_clamp_f32, qd_truncated_ste_f32   the callers' 'truncated' STE     cnn_models/conv_forward_model.py:240-241,263-264
//   K7m qd_multi_ste_plan, qd_multi_ste_backward_f32  K7 of every parameter in one launch   conv_forward_model.py:253-266
//       qd_multi_ste_backward_levels_f32              the same with a level count per tensor (k_multi_ste_lv)
//       qd_multi_ste_in16_plan, qd_multi_ste_backward_in16_f32   the same reading fp16 / bf16 gradients (k_multi_ste_in16)
//       qd_multi_ste_buckets_plan, qd_multi_ste_backward_buckets_f32   a level count and a bucket size per tensor (k_multi_ste_bk)
// Its own translation unit: K7, K7m and K8 are the only users of ste_cut and of the two K7 bodies.
#include "qd_launch.h"         // shared helpers: workspace carving, launch geometry
#include "../../include/qd_hip.h"
#include "qd_multi.h"          // owner_of, fill_prefix for K7m

namespace {

// ---- K7: 'complicated' STE backward (quant_functions.py:319-406) --------------------------------
// Per bucket S = sum_i g_i (qs_i - u_i), out = g, out[jmax] += S, out[jmin] -= S.  Every TERM follows the reference's own
// fp32 operations -- qs = (q - beta_q) / alpha_q (:350, scale_down of the quantized tensor), u = (x - beta_q) / alpha_q,
// d = qs - u, t = g d (:400), each rounded -- so that only the order of the fp32 summation differs from the reference
// (torch.mm over a sparse +-1 matrix): the bucket sum agrees with a float64 sum of the same terms to ~1e-7 of sum|t|.
// (Round 2 hoisted the division out of the sum, S = (sum g (q - x)) / alpha_q: closer to exact arithmetic than the
// reference, but 3e-7 / 6e-6 of sum|t| away from THE REFERENCE at 16 / 256 levels, because the reference's two quotients
// are rounded before they are subtracted.)  The two quotients per element use the bucket-invariant division (three VALU
// operations each, qd_common.h); here the quotient itself is consumed, so the form is only taken when it is exact for
// every numerator of the bucket: alpha_q in [2^-60, 2^100] and no numerator x - beta_q in (0, max(2^-100, alpha_q 2^-120))
// -- scale_down's own condition (scale_fast_ok, qd_common.h): below 2^-100 the remainder underflows, and below
// alpha_q 2^-120 the quotient is DENORMAL and can differ from the IEEE one in its last bit, which an incoming gradient of
// 2^100 turns into half of the bucket sum -- a wave-uniform choice, otherwise the IEEE division.  Only the numerators
// x - beta_q are looked at: the others, q - beta_q, are 0 or at least one level step, about alpha_q / (s - 1), whose quotient
// is normal and which is far above 2^-100 for alpha_q >= 2^-60.  The level of each element (the only thing q depends on)
// comes from the same shortcuts as K1: bucket-invariant division of (x - beta) / alpha, and level / (s-1) from the per-row
// table for <= 16 levels.
template <bool FAST>
__device__ __forceinline__ float ste_term(float g, float q, float x, float aq, float bq, float yq) {
    float qs = q - bq;  qs = div_alpha<FAST>(qs, aq, yq);
    float u = x - bq;   u = div_alpha<FAST>(u, aq, yq);
    const float d = qs - u;
    return g * d;
}
// The key of scale_numerator_key (qd_common.h) for the numerator x - beta_q; a lane keeps the unsigned minimum over its
// elements and scale_fast_ok(alpha_q, min) decides.  beta_q is the bucket's minimum (level 0 dequantizes to beta exactly), so
// the numerator is >= 0; fabsf keeps the key meaningful should that ever change.
__device__ __forceinline__ unsigned ste_numerator_key(float x, float bq) { return __float_as_uint(fabsf(x - bq)) - 1u; }

// The gradient's element type G: float (every fp32 entry point; the code below is then what it always was), or _Float16 /
// __bf16 for qd_multi_ste_backward_in16_f32, which reads 16-bit gradients and widens them on load (Grad16<KIND>::type, widen,
// load16x4_nt: qd_multi.h).  The widening is exact and everything after the load is the fp32 arithmetic, so a launch on 16-bit
// gradients has the bits of the fp32 launch on a widened copy.
// this lane's four consecutive gradients of the register tile.  16-bit: one 8-byte load where g is 8-byte aligned (p is a
// multiple of four elements past g: wave-uniform), element by element otherwise; the same lane -> element map either way.
template <typename G>
__device__ __forceinline__ f4 ste_load_g4(const G* p, bool g8) {
    if constexpr (std::is_same<G, float>::value) {
        return __builtin_nontemporal_load((const f4*)p);
    } else {
        return load16x4_nt(p, g8);
    }
}

// vector path: LPB lanes per bucket, V float4 per lane, the whole bucket (x, g, q) in registers, one pass.  Index ties:
// the FIRST element (in memory order) at the top / bottom level of the quantized bucket (or the true arg of x).
// One tile (= one wave iteration, 64 / LPB buckets) of the vector path: the body of k_ste_backward_vec and of the register
// tiles of k_multi_ste, so that both sum a bucket in the same order.
template <int LPB, int V, typename G = float>
__device__ __forceinline__ void ste_vec_tile(const float* x, const G* g, float* out, int64_t nvec, int64_t t, int sub, int l,
                                             float sm1, int tie_mode, bool use_tab, float tab) {
    constexpr int BPW = 64 / LPB;                            // sub = lane / LPB: the bucket of the tile, l = lane % LPB
    constexpr int ROW = LPB * V * 4;
    {
        const int64_t bkt = t * BPW + sub;
        if (bkt >= nvec) return;
        const int64_t e0 = bkt * ROW + (int64_t)l * 4;
        f4 xv[V], gv[V], qv[V];
        const bool g8 = (((uintptr_t)g) & 7) == 0;          // (16-bit gradients only)
#pragma unroll
        for (int j = 0; j < V; ++j) {
            xv[j] = __builtin_nontemporal_load((const f4*)(x + e0) + j * LPB);
            gv[j] = ste_load_g4(g + e0 + j * LPB * 4, g8);
        }
        // NaN-propagating, as torch's min / max and as the forward kernel: a bucket that holds a NaN (or an infinity: alpha =
        // inf) quantizes to NaN as a whole, its sum S is NaN, and the reference adds and subtracts S at the FIRST NaN -- the
        // position torch's min and max both report (quant_functions.py:350,383-400)
        float mn = pmin4(xv[0]), mx = pmax4(xv[0]);
#pragma unroll
        for (int j = 1; j < V; ++j) { mn = pmin(mn, pmin4(xv[j])); mx = pmax(mx, pmax4(xv[j])); }
        mn = group_min<LPB>(mn); mx = group_max<LPB>(mx);
        float a, b;
        alpha_beta(mn, mx, a, b);
        auto quantize = [&](auto fast_c, auto tab_c) {
            constexpr bool FAST = decltype(fast_c)::value;
            constexpr bool TAB = decltype(tab_c)::value;
            const float y = FAST ? 1.0f / a : 0.0f;
            float lev;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                if (TAB) {
                    qv[j].x = qdq_tab<FAST>(xv[j].x, a, b, sm1, 0.0f, lev, tab, y); qv[j].y = qdq_tab<FAST>(xv[j].y, a, b, sm1, 0.0f, lev, tab, y);
                    qv[j].z = qdq_tab<FAST>(xv[j].z, a, b, sm1, 0.0f, lev, tab, y); qv[j].w = qdq_tab<FAST>(xv[j].w, a, b, sm1, 0.0f, lev, tab, y);
                } else {
                    qv[j].x = qdq<FAST>(xv[j].x, a, b, sm1, 0.0f, lev, y); qv[j].y = qdq<FAST>(xv[j].y, a, b, sm1, 0.0f, lev, y);
                    qv[j].z = qdq<FAST>(xv[j].z, a, b, sm1, 0.0f, lev, y); qv[j].w = qdq<FAST>(xv[j].w, a, b, sm1, 0.0f, lev, y);
                }
            }
        };
        const bool fa = !__any(!fastdiv_ok(a));              // wave-uniform
        if (fa) { if (use_tab) quantize(std::true_type{}, std::true_type{}); else quantize(std::true_type{}, std::false_type{}); }
        else { if (use_tab) quantize(std::false_type{}, std::true_type{}); else quantize(std::false_type{}, std::false_type{}); }
        float qmn = pmin4(qv[0]), qmx = pmax4(qv[0]);
#pragma unroll
        for (int j = 1; j < V; ++j) { qmn = pmin(qmn, pmin4(qv[j])); qmx = pmax(qmx, pmax4(qv[j])); }
        qmn = group_min<LPB>(qmn); qmx = group_max<LPB>(qmx);
        float aq, bq;
        alpha_beta(qmn, qmx, aq, bq);                       // scale_down of the QUANTIZED bucket, :350
        int jmax = 0x7fffffff, jmin = 0x7fffffff;           // index inside the bucket
        const bool ref_tie = tie_mode == QD_STE_TIE_REFERENCE;
        const bool bad = ref_tie ? (qmn != qmn) : (mn != mn);   // the searched tensor's min / max are NaN: both sit at its first NaN
        unsigned nkey = 0xFFFFFFFFu;                        // min over the lane's numerators x - beta_q
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int base = (j * LPB + l) * 4;
#define QD_STE_ELEM(c, off)                                                          \
            {                                                                        \
                nkey = min(nkey, ste_numerator_key(xv[j].c, bq));                    \
                const float sv = ref_tie ? qv[j].c : xv[j].c;                        \
                const bool top = bad ? (sv != sv) : (sv == (ref_tie ? qmx : mx));    \
                const bool bot = bad ? (sv != sv) : (sv == (ref_tie ? qmn : mn));    \
                jmax = (top && base + off < jmax) ? base + off : jmax;               \
                jmin = (bot && base + off < jmin) ? base + off : jmin;               \
            }
            QD_STE_ELEM(x, 0) QD_STE_ELEM(y, 1) QD_STE_ELEM(z, 2) QD_STE_ELEM(w, 3)
#undef QD_STE_ELEM
        }
        float sum = 0.0f;
        auto bucket_sum = [&](auto fast_c) {
            constexpr bool FAST = decltype(fast_c)::value;
            const float yq = FAST ? 1.0f / aq : 0.0f;
#pragma unroll
            for (int j = 0; j < V; ++j) {                    // per lane in memory order, then the DPP tree
                sum += ste_term<FAST>(gv[j].x, qv[j].x, xv[j].x, aq, bq, yq);
                sum += ste_term<FAST>(gv[j].y, qv[j].y, xv[j].y, aq, bq, yq);
                sum += ste_term<FAST>(gv[j].z, qv[j].z, xv[j].z, aq, bq, yq);
                sum += ste_term<FAST>(gv[j].w, qv[j].w, xv[j].w, aq, bq, yq);
            }
        };
        if (!__any(!scale_fast_ok(aq, nkey))) bucket_sum(std::true_type{}); else bucket_sum(std::false_type{});
        sum = group_sum<LPB>(sum); jmax = group_imin<LPB>(jmax); jmin = group_imin<LPB>(jmin);
        const bool touch = jmax != jmin || bad;             // constant bucket: +S and -S cancel; a NaN bucket: (g + S) - S = NaN there
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int base = (j * LPB + l) * 4;
            f4 o = gv[j];
            if (touch) {
                if (base + 0 == jmax) o.x = o.x + sum;  if (base + 0 == jmin) o.x = o.x - sum;
                if (base + 1 == jmax) o.y = o.y + sum;  if (base + 1 == jmin) o.y = o.y - sum;
                if (base + 2 == jmax) o.z = o.z + sum;  if (base + 2 == jmin) o.z = o.z - sum;
                if (base + 3 == jmax) o.w = o.w + sum;  if (base + 3 == jmin) o.w = o.w - sum;
            }
            if (V == 1) store_nt_pinned((QD_AS_GLOBAL f4*)(out + e0) + j * LPB, o);      // (the V = 1 instance loses the hint otherwise)
            else __builtin_nontemporal_store(o, (f4*)(out + e0) + j * LPB);
        }
    }
}

template <int LPB, int V>
__global__ __launch_bounds__(256) void k_ste_backward_vec(const float* x, const float* g, float* out, int64_t nvec,
                                                          float sm1, int tie_mode) {
    constexpr int BPW = 64 / LPB;
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t ntiles = (nvec + BPW - 1) / BPW;
    const bool use_tab = sm1 <= 15.0f;                       // DPP rows are active or inactive as a whole here (qdq_tab)
    const float tab = (float)(lane & 15) / sm1;
    const int sub = lane / LPB, l = lane % LPB;
    for (int64_t t = wave; t < ntiles; t += nwaves) ste_vec_tile<LPB, V>(x, g, out, nvec, t, sub, l, sm1, tie_mode, use_tab, tab);
}

// any bucket size / alignment: one wave per bucket, four passes over the (L1/L2-resident) bucket.  The body of k_ste_backward
// and of the generic tiles of k_multi_ste.
template <typename G = float>
__device__ __forceinline__ void ste_wave_bucket(const float* x, const G* g, float* out, int64_t n, int64_t row, int64_t bkt,
                                                int lane, float sm1, int tie_mode) {
    {
        const int64_t lo = bkt * row;
        const int64_t hi = lo + row < n ? lo + row : n;
        // pass 1: alpha/beta of x
        float mn = INFINITY, mx = -INFINITY;
        bool nan = false;
        for (int64_t i = lo + lane; i < hi; i += 64) { const float v = x[i]; mn = fminf(mn, v); mx = fmaxf(mx, v); nan |= (v != v); }
        mn = wave_min(mn); mx = wave_max(mx);
        if (group_any<64>(nan)) { mn = NAN; mx = NAN; }      // torch's min / max propagate a NaN (as the register-resident path does)
        float a, b;
        alpha_beta(mn, mx, a, b);
        // pass 2: min/max of the QUANTIZED bucket (the reference re-runs scale_down on q, :350)
        float qmn = INFINITY, qmx = -INFINITY;
        bool qnan = false;
        unsigned nkey = 0xFFFFFFFFu;
        for (int64_t i = lo + lane; i < hi; i += 64) {
            float lev;
            const float q = qdq(x[i], a, b, sm1, 0.0f, lev);
            qmn = fminf(qmn, q); qmx = fmaxf(qmx, q); qnan |= (q != q);
        }
        qmn = wave_min(qmn); qmx = wave_max(qmx);
        if (group_any<64>(qnan)) { qmn = NAN; qmx = NAN; }
        float aq, bq;
        alpha_beta(qmn, qmx, aq, bq);
        const bool bad = tie_mode == QD_STE_TIE_REFERENCE ? (qmn != qmn) : (mn != mn);   // min / max of the searched tensor are NaN: both at its first NaN
        for (int64_t i = lo + lane; i < hi; i += 64) nkey = min(nkey, ste_numerator_key(x[i], bq));
        // pass 3: S_b (the reference's own per-element operations, :400) and the first index at the top / bottom level
        // (or the true arg of x)
        float s = 0.0f;
        long long jmax = INT64_MAX, jmin = INT64_MAX;
        auto pass3 = [&](auto fast_c) {
            constexpr bool FAST = decltype(fast_c)::value;
            const float yq = FAST ? 1.0f / aq : 0.0f;
            for (int64_t i = lo + lane; i < hi; i += 64) {
                float lev;
                const float xv = x[i];
                const float q = qdq(xv, a, b, sm1, 0.0f, lev);
                s += ste_term<FAST>(widen(g[i]), q, xv, aq, bq, yq);
                const float sv = tie_mode == QD_STE_TIE_REFERENCE ? q : xv;
                const bool top = bad ? (sv != sv) : (sv == (tie_mode == QD_STE_TIE_REFERENCE ? qmx : mx));
                const bool bot = bad ? (sv != sv) : (sv == (tie_mode == QD_STE_TIE_REFERENCE ? qmn : mn));
                if (top && (long long)i < jmax) jmax = i;
                if (bot && (long long)i < jmin) jmin = i;
            }
        };
        if (!__any(!scale_fast_ok(aq, nkey))) pass3(std::true_type{}); else pass3(std::false_type{});
        s = wave_sum(s);
        jmax = wave_min_ll(jmax);
        jmin = wave_min_ll(jmin);
        // pass 4: out = g, +S at jmax, -S at jmin (they cancel when the bucket is constant)
        for (int64_t i = lo + lane; i < hi; i += 64) {
            float o = widen(g[i]);
            if (jmax != jmin || bad) {                     // (a NaN bucket: (g + S) - S = NaN at the first NaN, as the reference)
                if (i == jmax) o = o + s;
                if (i == jmin) o = o - s;
            }
            out[i] = o;
        }
    }
}

__global__ __launch_bounds__(256) void k_ste_backward(const float* x, const float* g, float* out, int64_t n,
                                                      int64_t row, int64_t first, int64_t nb, float sm1, int tie_mode) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t bkt = first + wave; bkt < nb; bkt += nwaves) ste_wave_bucket(x, g, out, n, row, bkt, lane, sm1, tie_mode);
}

// ---- K7: how a tensor is cut into the two bodies above -- the ONE statement of it ------------------
// qd_ste_bucket_backward_f32 (its two launches), qd_multi_ste_plan (the tile count) and k_multi_ste (the tile -> bucket map)
// all take it from ste_cut(), so a bucket is summed by the same body in the same order whichever entry point reaches it: that
// is what makes the one-launch form bit-identical to the per-tensor call.
//   * register path: when the bucket row is a row of QD_STE_SHAPES, the tensor has more than one bucket and x, g, out meet
//     the data alignment (kDataAlign), the n / row full buckets go through ste_vec_tile<LPB, V>, 64 / LPB buckets per tile;
//   * everything else -- the ragged last bucket after them, or every bucket of the tensor -- through ste_wave_bucket, one
//     bucket per wave iteration.
// X(row, lanes per bucket, float4 per lane): row = LPB x V x 4
#define QD_STE_SHAPES(X)                                                                                              \
    X(64, 16, 1)                                                                                                      \
    X(128, 16, 2)                                                                                                     \
    X(256, 16, 4) /* (32,2) and (64,1) lane groupings measured slower: 169-195 / 182-188 vs 166 us */                 \
    X(512, 64, 2)                                                                                                     \
    X(1024, 64, 4)

constexpr int ste_lanes_per_bucket(int64_t row) {        // 0: no register path at this row
#define QD_STE_LANES(ROW, LPB, V) if (row == ROW) return LPB;
    QD_STE_SHAPES(QD_STE_LANES)
#undef QD_STE_LANES
    return 0;
}

struct SteCut {
    int64_t row, nb;         // bucket row (the whole tensor when it is shorter than a bucket) and number of buckets
    int64_t nfull;           // buckets [0, nfull) take the register path, [nfull, nb) ste_wave_bucket
    int lpb;                 // lanes per bucket of the register path; 0: none
    int64_t vtiles;          // its tiles: ceil(nfull / (64 / lpb))
};
// n > 0.  ROW says which rows may take the register path: -1 (the host callers) any row of the table; k_multi_ste<LPB, V>
// passes its own LPB x V x 4 -- a launch has one bucket size -- so that the row stays a constant there (0: none).
template <int ROW = -1>
__host__ __device__ __forceinline__ SteCut ste_cut(const float* x, const float* g, const float* out, int64_t n, int64_t bucket) {
    SteCut c;
    c.row = n < bucket ? n : bucket;
    c.nb = (n + c.row - 1) / c.row;
    c.nfull = 0; c.lpb = 0; c.vtiles = 0;
    const int lpb = ROW < 0 ? ste_lanes_per_bucket(c.row) : c.row == ROW ? ste_lanes_per_bucket(ROW) : 0;
    const int64_t row = ROW > 0 ? ROW : c.row;              // (lpb > 0 under a ROW: it is the row)
    // n > row: more than one bucket (nb > 1)
    if (lpb > 0 && n > row && (((((uintptr_t)x) | ((uintptr_t)g) | ((uintptr_t)out)) & kDataAlign) == 0)) {
        const int64_t bpw = 64 / lpb;
        c.lpb = lpb;
        c.nfull = n / row;
        c.vtiles = (int64_t)((uint64_t)(c.nfull + bpw - 1) / (uint64_t)bpw);    // (unsigned: a shift, bpw being 4 or 1, whatever is known of n's sign)
    }
    return c;
}

// ---- K8: 'truncated' STE ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_clamp(float* w, int64_t n, float limit) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nth = (int64_t)gridDim.x * blockDim.x;
    int64_t done = 0;
    if ((((uintptr_t)w) & kDataAlign) == 0) {
        const int64_t n4 = n >> 2;
        for (int64_t i = tid; i < n4; i += nth) {
            f4 v = ((f4*)w)[i];
            f4 r;
            r.x = v.x > limit ? limit : (v.x < -limit ? -limit : v.x);
            r.y = v.y > limit ? limit : (v.y < -limit ? -limit : v.y);
            r.z = v.z > limit ? limit : (v.z < -limit ? -limit : v.z);
            r.w = v.w > limit ? limit : (v.w < -limit ? -limit : v.w);
            if (r.x != v.x || r.y != v.y || r.z != v.z || r.w != v.w) ((f4*)w)[i] = r;   // write only what changes
        }
        done = n4 << 2;
    }
    for (int64_t i = done + tid; i < n; i += nth) {
        float v = w[i];
        v = v > limit ? limit : v;
        v = v < -limit ? -limit : v;
        w[i] = v;
    }
}
// grad[|w| > limit] = 0: reads w (4 B) and touches grad only where the mask hits
__global__ __launch_bounds__(256) void k_truncated_ste(const float* w, float* grad, int64_t n, float limit) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nth = (int64_t)gridDim.x * blockDim.x;
    int64_t done = 0;
    if ((((uintptr_t)w | (uintptr_t)grad) & kDataAlign) == 0) {
        const int64_t n4 = n >> 2;
        for (int64_t i = tid; i < n4; i += nth) {
            const f4 v = __builtin_nontemporal_load((const f4*)w + i);
            const bool m0 = fabsf(v.x) > limit, m1 = fabsf(v.y) > limit, m2 = fabsf(v.z) > limit, m3 = fabsf(v.w) > limit;
            if (m0 | m1 | m2 | m3) {                      // one 16-byte read-modify-write instead of 4-byte pokes
                f4 gv = ((const f4*)grad)[i];
                gv.x = m0 ? 0.0f : gv.x; gv.y = m1 ? 0.0f : gv.y; gv.z = m2 ? 0.0f : gv.z; gv.w = m3 ? 0.0f : gv.w;
                ((f4*)grad)[i] = gv;
            }
        }
        done = n4 << 2;
    }
    for (int64_t i = done + tid; i < n; i += nth)
        if (fabsf(w[i]) > limit) grad[i] = 0.0f;
}

// ---- multi-tensor K7: the 'complicated' STE backward of every parameter of a model in one launch ----
// A tile = one wave iteration on one tensor; ste_cut() says which: tiles 0 .. vtiles - 1 of a tensor are its register tiles
// (bucket t * (64 / LPB) + lane / LPB), the tiles after them one bucket each from nfull on.
//
// The four kernels below are one tile body, multi_ste_tile, under four argument lists.  A kernel keeps the loop over its wave's
// tiles, the tile -> tensor search and where its level count and bucket size come from (kernel arguments, or SteTensor); the
// rest of a tile is one call.  ROW: the one bucket row that takes the register path in this instantiation (LPB x V x 4 -- a
// launch with ONE bucket size has at most one), 0: none, -1: any row of QD_STE_SHAPES, picked by a scalar switch (a bucket size
// per tensor).  G: the gradient's element type.  Every instantiation sees its own text only: a plain launch runs code that has
// never heard of level arrays or 16-bit loads.
template <int ROW, typename G>
__device__ __forceinline__ void multi_ste_tile(const QdSteDesc d, int64_t bucket, int64_t local, int lane, float sm1, int tie_mode,
                                               bool use_tab, float tab) {
    // 16-bit gradients: the cut is made from n, bucket, x and out alone -- g's alignment must not decide which body sums a bucket
    // -- which is what the plan counted (plan_ste_tiles)
    const SteCut c = ste_cut<ROW>(d.x, std::is_same<G, float>::value ? d.g : nullptr, d.out, d.n, bucket);
    const G* const g = (const G*)d.g;
    if (local < c.vtiles) {
        if constexpr (ROW > 0) {
            constexpr int LPB = ste_lanes_per_bucket(ROW), V = ROW / (LPB * 4);
            ste_vec_tile<LPB, V, G>(d.x, g, d.out, c.nfull, local, lane / LPB, lane % LPB, sm1, tie_mode, use_tab, tab);
        } else if constexpr (ROW < 0) {
            switch (c.row) {
#define QD_STE_TILE_CASE(R, LPB, V)                                                                                      \
            case R:                                                                                                      \
                ste_vec_tile<LPB, V, G>(d.x, g, d.out, c.nfull, local, lane / LPB, lane % LPB, sm1, tie_mode, use_tab, tab); \
                break;
            QD_STE_SHAPES(QD_STE_TILE_CASE)
#undef QD_STE_TILE_CASE
            default: break;
            }
        }
    } else {
        const int64_t bkt = c.nfull + (local - c.vtiles);   // (a tile count that does not belong to this table reaches no bucket)
        if (local >= 0 && bkt * c.row < d.n) ste_wave_bucket<G>(d.x, g, d.out, d.n, c.row, bkt, lane, sm1, tie_mode);
    }
}

// What a wave holds of the tensor it is on, where that comes from arrays: levels[ti], and buckets[ti] where there is such an array,
// are read with the descriptor (wave-uniform: scalar loads), and sm1, use_tab and tab -- the correctly rounded division of
// k_ste_backward_vec -- are derived whenever the wave moves on to another tensor.  BK: the kernel has a buckets array (a compile-time
// fact: the others carry no test of it); move_to then says whether the tensor has work -- an entry < 1 (the plan refuses one)
// leaves its tensor unwritten.
struct SteTensor {
    int cur = -1;                                   // the tensor the members below belong to
    float sm1 = 1.0f, tab = 0.0f;
    bool use_tab = false;
    int64_t bucket;                                 // the launch's, or buckets[cur]
    __device__ __forceinline__ explicit SteTensor(int64_t launch_bucket) : bucket(launch_bucket) {}
    template <bool BK = false>
    __device__ __forceinline__ bool move_to(int ti, int lane, const int32_t* levels, const int64_t* buckets = nullptr) {
        if (ti != cur) {
            cur = ti;
            sm1 = (float)(levels[ti] - 1);
            use_tab = sm1 <= 15.0f;
            tab = (float)(lane & 15) / sm1;
            if (BK) bucket = buckets[ti];
        }
        return !BK || bucket > 0;
    }
};

// one bucket size and one level count for the launch: k_multi_ste<LPB, V> is launched for the bucket size LPB x V x 4 (<0, 0>: any other)
template <int LPB, int V>
__global__ __launch_bounds__(256) void k_multi_ste(const QdSteDesc* __restrict__ table, int ntensors, int64_t total_tiles,
                                                   int64_t bucket, float sm1, int tie_mode) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = uniform_wave_index();      // scalar: owner_of runs on s_load
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const bool use_tab = sm1 <= 15.0f;
    const float tab = (float)(lane & 15) / sm1;
    for (int64_t t = wave; t < total_tiles; t += nwaves) {
        const QdSteDesc d = table[owner_of(table, ntensors, t)];        // (an empty tensor owns no tile)
        if (d.n <= 0) continue;
        multi_ste_tile<LPB * V * 4, float>(d, bucket, t - d.first_tile, lane, sm1, tie_mode, use_tab, tab);
    }
}

// a level count per tensor
template <int LPB, int V>
__global__ __launch_bounds__(256) void k_multi_ste_lv(const QdSteDesc* __restrict__ table, const int32_t* __restrict__ levels,
                                                      int ntensors, int64_t total_tiles, int64_t bucket, int tie_mode) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = uniform_wave_index();      // scalar: owner_of runs on s_load
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    SteTensor s(bucket);
    for (int64_t t = wave; t < total_tiles; t += nwaves) {
        const int ti = owner_of(table, ntensors, t);
        const QdSteDesc d = table[ti];                                  // (an empty tensor owns no tile)
        if (d.n <= 0) continue;
        if (!s.move_to(ti, lane, levels)) continue;
        multi_ste_tile<LPB * V * 4, float>(d, s.bucket, t - d.first_tile, lane, s.sm1, tie_mode, s.use_tab, s.tab);
    }
}

// a level count and a bucket size per tensor (qd_multi_ste_backward_buckets_f32): ste_cut<-1> -- the host callers' form -- with the
// tensor's own bucket says which body sums each of its buckets, as it told the plan and as it tells qd_ste_bucket_backward_f32
__global__ __launch_bounds__(256) void k_multi_ste_bk(const QdSteDesc* __restrict__ table, const int32_t* __restrict__ levels,
                                                      const int64_t* __restrict__ buckets, int ntensors, int64_t total_tiles,
                                                      int tie_mode) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = uniform_wave_index();      // scalar: owner_of runs on s_load
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    SteTensor s(0);
    for (int64_t t = wave; t < total_tiles; t += nwaves) {
        const int ti = owner_of(table, ntensors, t);
        const QdSteDesc d = table[ti];                                  // (an empty tensor owns no tile)
        if (d.n <= 0) continue;
        if (!s.move_to<true>(ti, lane, levels, buckets)) continue;
        multi_ste_tile<-1, float>(d, s.bucket, t - d.first_tile, lane, s.sm1, tie_mode, s.use_tab, s.tab);
    }
}

// k_multi_ste_lv reading 16-bit gradients (qd_multi_ste_backward_in16_f32): d.g addresses n fp16 / bf16 elements, x and out stay
// fp32, out never aliases g
template <int LPB, int V, int KIND>
__global__ __launch_bounds__(256) void k_multi_ste_in16(const QdSteDesc* __restrict__ table, const int32_t* __restrict__ levels,
                                                        int ntensors, int64_t total_tiles, int64_t bucket, int tie_mode) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = uniform_wave_index();      // scalar: owner_of runs on s_load
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    SteTensor s(bucket);
    for (int64_t t = wave; t < total_tiles; t += nwaves) {
        const int ti = owner_of(table, ntensors, t);
        const QdSteDesc d = table[ti];                                  // (an empty tensor owns no tile)
        if (d.n <= 0) continue;
        if (!s.move_to(ti, lane, levels)) continue;
        multi_ste_tile<LPB * V * 4, typename Grad16<KIND>::type>(d, s.bucket, t - d.first_tile, lane, s.sm1, tie_mode, s.use_tab,
                                                                 s.tab);
    }
}

// ---- K7m on the host: one plan, one argument check, one choice of the instantiation ----
// The plan of every form: tensor i of the table under bucket_of(i).  g_counts: g is an fp32 pointer and takes part in ste_cut's
// alignment test; otherwise (16-bit gradients) it must be 2-byte aligned and has no say in the cut -- multi_ste_tile's rule.
template <typename BucketOf>
int plan_ste_tiles(QdSteDesc* host_table, int ntensors, BucketOf bucket_of, bool g_counts, int64_t* total_tiles_out) {
    if (!host_table || ntensors <= 0 || !total_tiles_out) return QD_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < ntensors; ++i) {
        const QdSteDesc& d = host_table[i];
        if (bucket_of(i) <= 0 || d.n < 0 || (d.n > 0 && (!d.x || !d.g || !d.out || (!g_counts && (((uintptr_t)d.g) & 1)))))
            return QD_ERR_INVALID_ARGUMENT;
    }
    int i = 0;                                                          // (fill_prefix visits the descriptors in order)
    *total_tiles_out = fill_prefix(host_table, ntensors, [&](const QdSteDesc& d) -> int64_t {
        const int64_t bucket = bucket_of(i++);
        if (d.n <= 0) return 0;
        const SteCut c = ste_cut(d.x, g_counts ? d.g : nullptr, d.out, d.n, bucket);
        return c.vtiles + (c.nb - c.nfull);
    });
    return 0;
}

// What every K7m launch refuses.  An entry point passes what its signature has, and nullptr for an array / 1 for a bucket / 2 for
// a level count it does not have; `levels` and `buckets` (device arrays) must be aligned to their elements.
inline bool multi_ste_args_ok(const QdSteDesc* table, bool has_levels, const int32_t* levels, bool has_buckets, const int64_t* buckets,
                              int ntensors, int64_t total_tiles, int64_t bucket, int level_count, int tie_mode) {
    if (!table || ntensors <= 0 || total_tiles < 0 || bucket <= 0 || level_count < 2) return false;
    if (has_levels && (!levels || (((uintptr_t)levels) & 3))) return false;
    if (has_buckets && (!buckets || (((uintptr_t)buckets) & 7))) return false;
    return tie_mode == QD_STE_TIE_REFERENCE || tie_mode == QD_STE_TIE_TRUE_ARG;
}

// launch(LPB, V) as std::integral_constant<int, ...>: the row of QD_STE_SHAPES with LPB x V x 4 = bucket, <0, 0> where there is none
template <typename Launch>
inline void ste_dispatch(int64_t bucket, Launch launch) {
#define QD_STE_DISPATCH(ROW, LPB, V) if (bucket == ROW) return launch(std::integral_constant<int, LPB>{}, std::integral_constant<int, V>{});
    QD_STE_SHAPES(QD_STE_DISPATCH)
#undef QD_STE_DISPATCH
    launch(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
}

}  // namespace

extern "C" {

int qd_ste_bucket_backward_f32(const float* x, const float* g, float* out, int64_t n, int64_t bucket, int levels,
                               int tie_mode, void* stream) {
    if (n < 0 || bucket <= 0 || levels < 2 || (n > 0 && (!x || !g || !out))) return QD_ERR_INVALID_ARGUMENT;
    if (tie_mode != QD_STE_TIE_REFERENCE && tie_mode != QD_STE_TIE_TRUE_ARG) return QD_ERR_INVALID_ARGUMENT;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const float sm1 = (float)(levels - 1);
    const SteCut c = ste_cut(x, g, out, n, bucket);
#define QD_STE_LAUNCH(ROW, LPB, V)                                                                                       \
    if (c.lpb > 0 && c.row == ROW)                                                                                       \
        hipLaunchKernelGGL((k_ste_backward_vec<LPB, V>), dim3(blocks_for(c.vtiles, 4)), dim3(256), 0, st, x, g, out, c.nfull, \
                           sm1, tie_mode);
    QD_STE_SHAPES(QD_STE_LAUNCH)
#undef QD_STE_LAUNCH
    if (c.nfull < c.nb)
        hipLaunchKernelGGL(k_ste_backward, dim3(blocks_for(c.nb - c.nfull, 4)), dim3(256), 0, st, x, g, out, n, c.row, c.nfull,
                           c.nb, sm1, tie_mode);
    return check_launch();
}

int qd_clamp_f32(float* w, int64_t n, float limit, void* stream) {
    if (n < 0 || (n > 0 && !w)) return QD_ERR_INVALID_ARGUMENT;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_clamp, dim3(blocks_for(n, 256 * 4 * 4)), dim3(256), 0, (hipStream_t)stream, w, n, limit);
    return check_launch();
}

int qd_truncated_ste_f32(const float* w, float* grad, int64_t n, float limit, void* stream) {
    if (n < 0 || (n > 0 && (!w || !grad))) return QD_ERR_INVALID_ARGUMENT;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_truncated_ste, dim3(blocks_for(n, 256 * 4 * 4)), dim3(256), 0, (hipStream_t)stream, w, grad, n,
                       limit);
    return check_launch();
}

int qd_multi_ste_plan(QdSteDesc* host_table, int ntensors, int64_t bucket, int64_t* total_tiles_out) {
    return plan_ste_tiles(host_table, ntensors, [bucket](int) { return bucket; }, true, total_tiles_out);
}

int qd_multi_ste_buckets_plan(QdSteDesc* host_table, const int64_t* buckets, int ntensors, int64_t* total_tiles_out) {
    if (!buckets) return QD_ERR_INVALID_ARGUMENT;
    return plan_ste_tiles(host_table, ntensors, [buckets](int i) { return buckets[i]; }, true, total_tiles_out);
}

int qd_multi_ste_in16_plan(QdSteDesc* host_table, int ntensors, int64_t bucket, int64_t* total_tiles_out) {
    return plan_ste_tiles(host_table, ntensors, [bucket](int) { return bucket; }, false, total_tiles_out);
}

int qd_multi_ste_backward_f32(const QdSteDesc* table, int ntensors, int64_t total_tiles, int64_t bucket, int levels,
                              int tie_mode, void* stream) {
    if (!multi_ste_args_ok(table, false, nullptr, false, nullptr, ntensors, total_tiles, bucket, levels, tie_mode))
        return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    ste_dispatch(bucket, [&](auto lpb, auto v) {
        hipLaunchKernelGGL((k_multi_ste<decltype(lpb)::value, decltype(v)::value>), dim3(blocks_for(total_tiles, 4)), dim3(256), 0,
                           (hipStream_t)stream, table, ntensors, total_tiles, bucket, (float)(levels - 1), tie_mode);
    });
    return check_launch();
}

int qd_multi_ste_backward_levels_f32(const QdSteDesc* table, const int32_t* levels, int ntensors, int64_t total_tiles,
                                     int64_t bucket, int tie_mode, void* stream) {
    if (!multi_ste_args_ok(table, true, levels, false, nullptr, ntensors, total_tiles, bucket, 2, tie_mode))
        return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    ste_dispatch(bucket, [&](auto lpb, auto v) {
        hipLaunchKernelGGL((k_multi_ste_lv<decltype(lpb)::value, decltype(v)::value>), dim3(blocks_for(total_tiles, 4)), dim3(256), 0,
                           (hipStream_t)stream, table, levels, ntensors, total_tiles, bucket, tie_mode);
    });
    return check_launch();
}

int qd_multi_ste_backward_buckets_f32(const QdSteDesc* table, const int32_t* levels, const int64_t* buckets, int ntensors,
                                      int64_t total_tiles, int tie_mode, void* stream) {
    if (!multi_ste_args_ok(table, true, levels, true, buckets, ntensors, total_tiles, 1, 2, tie_mode)) return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    hipLaunchKernelGGL(k_multi_ste_bk, dim3(blocks_for(total_tiles, 4)), dim3(256), 0, (hipStream_t)stream, table, levels,
                       buckets, ntensors, total_tiles, tie_mode);
    return check_launch();
}

int qd_multi_ste_backward_in16_f32(const QdSteDesc* table, const int32_t* levels, int ntensors, int64_t total_tiles,
                                   int64_t bucket, int grad_kind, int tie_mode, void* stream) {
    if (!multi_ste_args_ok(table, true, levels, false, nullptr, ntensors, total_tiles, bucket, 2, tie_mode))
        return QD_ERR_INVALID_ARGUMENT;
    if (grad_kind != QD_GRAD_F16 && grad_kind != QD_GRAD_BF16) return QD_ERR_INVALID_ARGUMENT;
    if (total_tiles == 0) return 0;
    ste_dispatch(bucket, [&](auto lpb, auto v) {
        constexpr int LPB = decltype(lpb)::value, V = decltype(v)::value;
        auto kern = grad_kind == QD_GRAD_F16 ? k_multi_ste_in16<LPB, V, QD_GRAD_F16> : k_multi_ste_in16<LPB, V, QD_GRAD_BF16>;
        hipLaunchKernelGGL(kern, dim3(blocks_for(total_tiles, 4)), dim3(256), 0, (hipStream_t)stream, table, levels, ntensors,
                           total_tiles, bucket, tie_mode);
    });
    return check_launch();
}

}  // extern "C"
