/* qd_hip.h -- C ABI of libqd_hip.so, the MI355X (gfx950) fake-quantization kernels.
 *
 * This is the drop-in boundary of the hot path.  The reference
 * (antspy/quantized_distillation) has no FFI layer: its hot path is the Python module
 * `quantization` (quantization/__init__.py:4-8), a chain of unfused torch ops.  Each entry point
 * below replaces the chain of reference ops cited next to it (paths relative to the reference
 * root); the Python package `quantization` shipped in this repository keeps the reference's
 * signatures and binds these symbols with ctypes and, for the per-call entry points, with a small
 * CPython/ATen module (csrc/qd_torch_glue.cpp).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless it says "host";
 *   - tensors are contiguous fp32; `n` is the number of real elements;
 *   - `bucket`: elements per bucket, or 0 for "bucket_size=None" (one bucket = whole tensor);
 *     the bucket view follows quantization/help_functions.py:67-94:
 *       n <  bucket            -> 1 bucket of n elements
 *       n %  bucket == 0       -> n/bucket buckets
 *       otherwise              -> ceil(n/bucket) buckets, the last one padded with copies of
 *                                 x[n-1] (padding never changes min/max, so kernels ignore it);
 *   - all calls are asynchronous on `stream` (a hipStream_t passed as void*), never allocate,
 *     never synchronise with the host;
 *   - capture rule: every call that launches can therefore be recorded into a hipGraph (after one eager call of the same
 *     entry point on that stream).  By-value arguments and HOST arrays are frozen at record time; device memory -- inputs,
 *     descriptor tables, code books, `mean`, the workspace -- is read at replay time, and the workspace still needs no
 *     initialisation.  A refused call (negative return) records nothing and leaves the capture valid.  The one-launch
 *     single-bucket kernel is not recorded: a capturing stream takes the three-launch path, with the same bits
 *     (tests/test_hip_capture_abi.py replays every entry point on other data);
 *   - return value: 0 on success, a positive hipError_t if a launch failed, or a negative
 *     QD_ERR_* code for argument errors.  qd_error_string() describes either.
 *   - optional outputs may be NULL.
 *   - alignment: fp32 data pointers need the 4 bytes of their type and nothing more (a tensor view that starts 4, 8 or
 *     12 bytes into a 16-byte granule runs the same kernels at the same speed); int64 index outputs and workspaces 16
 *     bytes, uint8 level / index outputs 4 bytes, unless an entry point says otherwise.
 *   - `mean`: optional device scalar subtracted from every element before anything else
 *     (subtract_mean=True, quant_functions.py:66-68) and added back at the end (:148).
 *   - `clamp`/`max_element`: if clamp != 0, values are clamped to [-max_element, max_element]
 *     after the mean subtraction (quant_functions.py:72-74).
 *
 * NaN and +-inf in the inputs (both libraries, bit for bit; tests/test_hip_nonfinite.py, tests/test_nonfinite_host.py).  The
 * rules are the reference's (torch's min / max propagate a NaN, numpy's searchsorted orders a NaN after every number):
 *   - bucket statistics (qd_uniform_f32, qd_scale_down_f32, qd_nearest_point_f32 with prescaled == 0, qd_pack_uniform_f32,
 *     qd_multi_uniform_f32, qd_multi_uniform_global_f32): a NaN anywhere in a bucket makes its alpha and beta NaN and with
 *     them every output of THAT bucket -- no other bucket and, in a multi-tensor launch, no other tensor.  An infinity
 *     needs no rule of its own: alpha = inf (or NaN, when the bucket holds nothing but one infinity) and beta = -inf go
 *     through the same arithmetic -- u = (x - beta) / alpha is 0 or NaN, q is NaN or +-inf.
 *   - level index (`level_idx` of qd_uniform_f32, the codes of qd_pack_uniform_f32, the symbols of a uniform checkpoint):
 *     rint(u (levels - 1)) is an integer in [0, levels - 1] or NaN, never +-inf; a NaN level is stored as 0.  Unpacking such
 *     a code gives NaN again through the bucket's alpha / beta.  The stochastic branch of qd_uniform_f32 can reach level
 *     `levels`, one past the top (see there): its level index SATURATES at levels - 1, so the stored index is in
 *     [0, levels - 1] on every path and fits its byte at levels == 256.
 *   - point index (qd_nearest_point_f32 in both assign modes and both idx widths, qd_multi_nearest_f32, the symbols of a
 *     non-uniform checkpoint): a count of comparisons, hence in [0, k - 1] for every u; a NaN u takes the LAST point, k - 1.
 *     +inf takes k - 1 and -inf takes 0 by the comparisons themselves.  `points` are expected finite and sorted.
 *   - qd_inv_scale_f32, qd_unpack_uniform_f32, qd_huffman_decode_f32: plain IEEE u alpha + beta -- NaN / inf in u, alpha or
 *     beta propagate (0 x inf = NaN, inf - inf = NaN).
 *   - qd_point_grad_f32, qd_multi_point_grad_f32: every term g_i alpha_b is added to the bin of ITS index and to no other,
 *     so a NaN / inf gradient element or bucket alpha poisons exactly the points whose index set holds such an element
 *     (+inf and -inf on one point: NaN).
 *   - qd_clamp_f32 leaves a NaN as it is and maps +-inf to +-limit (torch.clamp); qd_truncated_ste_f32 keeps the gradient
 *     where w is NaN (|NaN| > limit is false) and zeroes it where w is +-inf.
 *   - qd_ste_bucket_backward_f32, qd_multi_ste_backward_f32: a bucket of x that holds a NaN or an infinity quantizes to NaN
 *     as a whole; out is NaN at the first such element (tie mode REFERENCE: at the bucket's first element) and g elsewhere.
 *   - qd_uniform_abs_f32, qd_scale_down_abs_f32, qd_inv_scale_abs_f32 ('absmax' / 'absnorm'; device only).  The reference's
 *     lines raise, so the rules are torch's operations on their evident repair: with v = x after mean subtraction and
 *     clamping, sign = torch.sign(v), m = |v|, norm = m.max(dim) or sqrt(sum m^2) in fp32 (oracle/oracle_np.py and, in torch's
 *     CPU ops, oracle/torch_port.py; tests/abs_cases.py, tests/test_abs_cases_host.py, tests/test_hip_abs.py):
 *       . a NaN anywhere in a bucket makes that bucket's norm NaN and every u, q and inverse output of it NaN; every other
 *         bucket is bit-identical to the same call without the NaN;
 *       . sign is 0 for a NaN of either sign bit and any payload and for +-0, and +-1 otherwise (+-inf and denormals too);
 *       . a bucket with +-inf and no NaN has norm +inf: u is 0 for its finite elements and NaN for its infinite ones, q and
 *         the inverse outputs are NaN as a whole (0 x inf);
 *       . absnorm: the squares are fp32 and their sum is rounded to fp32 before the square root, so a finite bucket whose sum
 *         of squares exceeds FLT_MAX has norm +inf (and falls under the rule above) and squares that underflow to 0
 *         contribute nothing; an ordinary norm is within (5e-7 + 2^-22) of sqrt(sum x^2) taken in float64;
 *       . a norm below 1e-10 is replaced by 1 after the reduction; a NaN norm stays NaN;
 *       . the padding of a ragged last bucket (copies of the last element) obeys the same rules: a NaN last element pads u
 *         with NaN and sign with 0.
 */
#ifndef QD_HIP_H
#define QD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QD_ERR_INVALID_ARGUMENT (-1)
#define QD_ERR_WORKSPACE_TOO_SMALL (-2)
#define QD_ERR_UNSUPPORTED (-3)

/* nearest-point assignment rules (quant_functions.py:267-273 vs :531-573) */
#define QD_ASSIGN_DISTANCE 0
#define QD_ASSIGN_MIDPOINT 1

/* tie rule of the 'complicated' STE backward */
#define QD_STE_TIE_REFERENCE 0 /* first element at the top/bottom LEVEL of the quantized bucket */
#define QD_STE_TIE_TRUE_ARG 1  /* true argmax/argmin of the input                               */

/* Library identification: ABI version (bumped on every change of an entry point's meaning or signature) and target arch.
 * History: 1 = rounds 1-3; 2 = qd_nearest_point_f32 accepts q == NULL (indices only), qd_uniform_f32 accepts q == NULL with
 * level_idx (levels only), qd_selftest_div_invariant, qd_digitize_histogram_f32 / qd_histogram_i64 / qd_level_histogram_f32
 * added, 4-byte data alignment; 3 = qd_scale_digitize_histogram_f32 added, QdDiffQuantDesc.first_row (partial rows of
 * qd_multi_point_grad_f32 per tensor size instead of 4 B + 1 for every tensor); qd_huffman_encode / qd_huffman_decode_f32
 * and qd_multi_ste_plan / qd_multi_ste_backward_f32 were added later without a bump (new symbols only, nothing existing
 * changed meaning).  qd_multi_dq_plan / qd_multi_nearest_f32 / qd_multi_point_grad_f32 take bucket == 0, buckets that are
 * no power of two and k up to 256, also without a bump: arguments that were rejected are now accepted; nothing existing
 * changed meaning.  qd_multi_uniform_levels_f32 / qd_multi_uniform_global_levels_f32 / qd_multi_ste_backward_levels_f32 (a level
 * count per tensor) are new symbols, likewise without a bump; so are qd_transform_plan and qd_set_grid_cap (host only), and
 * qd_multi_uniform_out16_f32 / qd_multi_uniform_global_out16_f32 (fp16 / bf16 outputs), and qd_multi_ste_in16_plan /
 * qd_multi_ste_backward_in16_f32 (fp16 / bf16 gradients), and qd_multi_nearest_out16_f32 / qd_multi_point_grad_in16_f32 (the
 * differentiable-quantization sweeps with fp16 / bf16 outputs and gradients; qd_multi_dq_plan now refuses an odd q or grad),
 * and qd_multi_buckets_plan / qd_multi_uniform_buckets_f32 / qd_multi_ste_buckets_plan / qd_multi_ste_backward_buckets_f32 (a
 * bucket size per tensor), and qd_multi_symbols_plan / qd_multi_uniform_symbols_u8 (QdSymbolDesc: the symbols of a whole model in
 * one launch).
 * The Python binding and _qd_glue.so compare the version THEY were built for with the library's. */
#define QD_ABI_VERSION 3
int qd_abi_version(void);
const char* qd_target_arch(void);
const char* qd_error_string(int code);

/* Bytes of device scratch the reductions need (global min/max, mean, point gradient).
 * One buffer of this size per stream is enough; contents need no initialisation. */
size_t qd_workspace_bytes(void);

/* bucket_size=None tensors (one bucket = whole tensor) of 16 Ki .. 1 Mi elements are processed by ONE launch -- load
 * once, grid-wide barrier on the per-block min/max, transform from registers (8 B/element) -- instead of reduce + fold +
 * apply.  The barrier never blocks: under contention a block gives up after 2 ms, folds the min/max of the whole tensor
 * itself and carries on; it depends on no other block (no departure counters, no "last block").
 *   mode 1 (default) = on, 0 = always the three-launch path;
 *   test hooks that reach the give-up path on an idle GPU: 2 = every block gives up at once, 3 = the blocks with
 *   blockIdx % 7 == 3, 4 = exactly one block (the middle one).
 * Returns the previous mode; any other value restores the default.  The only switch of this path (no environment
 * variable).  Process-wide, not thread-safe against concurrent launches. */
int qd_set_single_fused_mode(int mode);

/* Test hook: the cap on the number of blocks of every launch whose grid is sized from the problem.  The kernels loop over
 * tiles, chunks or buckets with a grid stride, but the default cap of 1 << 20 blocks only bounds the grid dimension, so the
 * second and later trips of those loops run only above billions of elements (and, in the nearest-point mode with the fine
 * cell table, above 24 blocks per compute unit).  Under a cap of 1, 2 or 3 blocks a tensor of a few thousand elements makes
 * them (tests/test_hip_grid_trips.py).  Every launch site takes min(its own cap, this cap) blocks; qd_transform_plan plans
 * under the cap that is set.  Not capped: grids that are not a free function of the problem size -- the one-launch single
 * bucket kernel (co-resident by construction), single-block folds, one block per output row, the fixed 2048-wave grid of
 * qd_multi_point_grad_f32, one block per Huffman chunk (csrc/qd_common.h lists them).
 *   blocks in 1 .. 1 << 20 sets the cap; any other value restores the default, 1 << 20.  Returns the previous value.
 * Results never depend on the cap, only the launch geometry does.  Process-wide, not thread-safe against concurrent
 * launches; no environment variable. */
int qd_set_grid_cap(int blocks);

/* Number of buckets / padded length of the bucket view (help_functions.py:67-94). Host only. */
int64_t qd_num_buckets(int64_t n, int64_t bucket);
int64_t qd_padded_length(int64_t n, int64_t bucket);

/* Which kernel(s) a call of qd_uniform_f32 / qd_scale_down_f32 / qd_nearest_point_f32 reaches, and with what launch geometry.
 * Host only, no device and no runtime call: the launcher of those three entry points runs the same function
 * (csrc/qd_plan.h: plan_transform) on the same numbers and launches what it returns, so the answer is the launch -- checked for
 * every bucket size on a machine without a GPU (tests/test_transform_plan.py), and against a trace on one
 * (profiles/dispatch_map.txt).  Pointers enter as alignment facts, the device as its compute-unit count, so the result does not
 * depend on the machine.  A new symbol (no ABI bump).
 * qd_transform_plan(queries, count, plans) fills plans[i] for queries[i]; returns 0, or QD_ERR_INVALID_ARGUMENT (nothing
 * written) for a null table, a mode outside 0 .. 2, n < 1, bucket < 0 or cus < 1 in any query. */
typedef struct QdTransformQuery {
    int32_t mode;            /* 0 qd_uniform_f32, 1 qd_scale_down_f32, 2 qd_nearest_point_f32                               */
    int32_t data_misalign;   /* (address of x | address of q / u) & 15; the data pointers need 4-byte alignment              */
    int32_t side_bytes;      /* level_idx asked for: 1; idx asked for: idx_bytes (1 or 8); 0: neither                        */
    int32_t side_misalign;   /* its address & 15 (level_idx needs 4-byte alignment, an int64 idx 16)                         */
    int32_t k, assign_mode, prescaled, q_null;      /* mode 2, as in qd_nearest_point_f32 (q_null: q == NULL)                */
    int32_t fused_capacity;  /* blocks of the one-launch single-bucket kernel that are resident at once (256 on MI355X);     */
                             /* 0: it may not be tried (qd_set_single_fused_mode(0), q aliases x, the stream is capturing)   */
    int32_t cus;             /* compute units of the device (256 on MI355X)                                                  */
    int64_t n, bucket;
} QdTransformQuery;
typedef struct QdPlannedLaunch {
    char kernel[40];         /* as tools/launch_coverage.py spells it, e.g. "k_bucket_wave_any<0,5,1>"                       */
    int32_t blocks, threads; /* grid and block size                                                                         */
    int64_t lds_bytes;       /* dynamic LDS                                                                                 */
} QdPlannedLaunch;
typedef struct QdTransformPlan {
    int64_t nb, row;         /* buckets, elements per bucket                                                                */
    int64_t nvec;            /* k_bucket_vec: leading full buckets it takes (0 for every other kernel)                       */
    int64_t m, nchunks;      /* k_bucket_chunk / k_bucket_chunk_any: buckets per chunk, whole chunks (0 otherwise)           */
    int64_t nbk, amask;      /* k_bucket_wave_any: its buckets are [0, nbk); ~31 (0 otherwise)                               */
    int32_t fine;            /* the kernel builds the fine cell table (k > 32, midpoint rule, no LDS staging of its own)     */
    int32_t nlaunch;         /* launches, in order: 1 .. 3; 0: the call is refused (indices only, no pre-scaled stream)      */
    QdPlannedLaunch launch[3];
} QdTransformPlan;
int qd_transform_plan(const QdTransformQuery* queries, int64_t count, QdTransformPlan* plans);

/* mean_out[0] = mean(x) (float64 accumulation, one rounding).  Replaces tensor.mean(),
 * quant_functions.py:67. */
int qd_mean_f32(const float* x, int64_t n, float* mean_out, void* workspace, size_t workspace_bytes, void* stream);

/* K1/K1g: uniformQuantization, linear scaling (quant_functions.py:155-194 with
 * ScalingFunction.scale_down :56-107 and inv_scale_down :131-152 fused):
 *     alpha_b = max_b - min_b (alpha < 1e-10 -> 1), beta_b = min_b
 *     q = rint((x - beta)/alpha * (levels-1)) / (levels-1) * alpha + beta   [each op rounded]
 * x, q: [n] (q may alias x: modify_in_place).  alpha, beta: [num_buckets] optional outputs.
 * level_idx: optional [n] uint8 output of the integer level rint(u*(levels-1)) (levels <= 256).
 * Levels only: q == NULL with level_idx given writes the levels (and alpha / beta if asked for) and nothing else -- 4 B read +
 * 1 B written per element; deterministic rounding without mean / clamp, bucket in {64, 128, 256, 512, 1024, 2048}, x 16-byte
 * aligned (the geometry of qd_pack_uniform_f32, whose 8-bit form this is); QD_ERR_UNSUPPORTED otherwise.
 * stochastic != 0 selects the stochastic-rounding branch (:174-187) with a counter-based
 * in-kernel generator keyed by (seed, element index): Philox4x32 with 7 rounds, counter = (element >> 2 as two words,
 * 0x51ed270b, 0x2545f491), key = seed (low word, high word), element e takes word e & 3; the draw is the word's top 24 bits
 * times 2^-24, in [0, 1).  With t = u (levels - 1), l = floor(t), p = t - l the element goes to level l + 1 where
 * draw <= p and to level l otherwise -- "<=" as the reference (:187), so an element exactly on a level (p == 0: each
 * bucket's minimum and maximum) still moves up when its draw is exactly 0.0, once in 2^24 draws, and the bucket's maximum
 * then comes out at level `levels`, ONE PAST THE TOP: q = ((levels - 1) / (levels - 1) + 1 / (levels - 1)) alpha + beta,
 * as the reference computes it.  level_idx is saturated at levels - 1 there (it keeps its documented range; at
 * levels == 256 the value 256 has no byte to go to).  The seed is a by-value launch argument: a captured launch replays
 * the same draws (the Python layer refuses a stochastic call during stream capture for that reason).
 * workspace is only used when the tensor is a single bucket (bucket == 0 or n < bucket).
 * levels: 2 .. 2^31 - 1 (INT_MAX), here and in every entry point that takes a level count; below 2 is
 * QD_ERR_INVALID_ARGUMENT.  A deliberate narrowing of the reference, whose quantizers take any s (they never convert it):
 * `levels` is an int, so a larger count cannot cross this ABI, and every Python entry point raises ValueError for one
 * instead of passing a truncated value on (2^32 + 16 would arrive as 16).  levels - 1 is converted to fp32 once, rounded to
 * nearest even as the reference's tensor ops round the Python int: exact up to 2^24 + 1 levels, 2^31 at 2^31 - 1 levels.
 * Nothing converts a level back to an integer except level_idx (levels <= 256). */
int qd_uniform_f32(const float* x, float* q, int64_t n, int64_t bucket, int levels, float* alpha, float* beta,
                   uint8_t* level_idx, const float* mean, int clamp, float max_element, int stochastic,
                   uint64_t seed, void* workspace, size_t workspace_bytes, void* stream);

/* K2: ScalingFunction.scale_down, linear (quant_functions.py:56-107).  u has the PADDED bucket
 * layout: qd_padded_length(n, bucket) elements; padding entries hold the scaled last element,
 * exactly as the reference's cat-then-scale produces.  u may alias x only when no padding is
 * needed.  alpha, beta: [num_buckets] (required: they are what inverts the scaling). */
int qd_scale_down_f32(const float* x, float* u, int64_t n, int64_t bucket, float* alpha, float* beta,
                      const float* mean, int clamp, float max_element, void* workspace, size_t workspace_bytes,
                      void* stream);

/* K3: ScalingFunction.inv_scale_down, linear (quant_functions.py:131-152): y = u*alpha + beta
 * (+ mean), padding dropped.  u: padded layout; y: [n]; y may alias u. */
int qd_inv_scale_f32(const float* u, float* y, int64_t n, int64_t bucket, const float* alpha, const float* beta,
                     const float* mean, void* stream);

/* First-occurrence arg-min / arg-max of each bucket, relative to the bucket start (int64), the
 * idx_min_rows / idx_max_rows of ScalingFunction (quant_functions.py:85-90,103-104).  Computed
 * on demand only (nothing on the per-step path reads them except the 'complicated' STE).  A bucket that holds a NaN
 * reports the position of its FIRST NaN for both, as torch.min / max(dim) do. */
int qd_bucket_argminmax_f32(const float* x, int64_t n, int64_t bucket, const float* mean, int clamp,
                            float max_element, int64_t* argmin, int64_t* argmax, void* workspace,
                            size_t workspace_bytes, void* stream);

/* K4/K5: nearest-point (non-uniform) quantization (quant_functions.py:196-290).
 *   prescaled == 0: x is the raw tensor [n]; it is scaled per bucket first (alpha/beta are
 *                   OUTPUTS, [num_buckets]);
 *   prescaled != 0: x is u in the unpadded layout [n], already scaled; alpha/beta are INPUTS
 *                   (the per-step path of differentiable quantization: the tensor is frozen,
 *                   only `points` change, quant_functions.py:449-469).
 * points: [k] sorted ascending, device.  assign_mode: QD_ASSIGN_DISTANCE (searchsorted-left +
 * strictly-closer-lower rule, :267-273) or QD_ASSIGN_MIDPOINT (#{midpoints <= u}, the
 * SearchSorted.query formulation, :531-573).  Each rule is defined by where a tie goes; tests/nearest_cases.py with
 * tests/test_nearest_cases_host.py (libqd_host.so, and each kernel by the plan) and tests/test_hip_nearest_ties.py (every
 * kernel of libqd_hip.so) pin both on points, midpoints, cell boundaries and their fp32 neighbours.
 * q: [n] = points[idx]*alpha + beta (+mean).  idx: optional, idx_bytes 8 (int64, what the
 * reference API returns) or 1 (uint8, k <= 256).  A NaN u -- every element of a bucket whose alpha or beta is NaN --
 * has index k - 1 (np.searchsorted orders a NaN last, :267-268 and :572) and value NaN.
 * Indices only (what SearchSorted.query returns, :531-563): prescaled != 0 with q == NULL and idx given -- n >= 4,
 * buckets of at least 4 elements (or bucket == 0), idx 16-byte (int64) / 4-byte (uint8) aligned; QD_ERR_INVALID_ARGUMENT
 * otherwise. */
int qd_nearest_point_f32(const float* x, int prescaled, const float* points, int k, int assign_mode, float* q,
                         void* idx, int idx_bytes, int64_t n, int64_t bucket, float* alpha, float* beta,
                         const float* mean, int clamp, float max_element, void* workspace, size_t workspace_bytes,
                         void* stream);

/* K6: nonUniformQuantization_variable.backward (quant_functions.py:471-506):
 *     grad_points[j] = sum_{i : idx_i == j} g_i * alpha_bucket(i)
 * Deterministic two-stage reduction (fixed order, no atomics).  idx_bytes 8 or 1. */
int qd_point_grad_f32(const float* g, const void* idx, int idx_bytes, const float* alpha, int64_t n, int64_t bucket,
                      int k, float* grad_points, void* workspace, size_t workspace_bytes, void* stream);

/* K7: 'complicated' straight-through backward of uniformQuantization_variable
 * (quant_functions.py:319-406, intended math): per bucket
 *     S_b = sum_i g_i*(qs_i - u_i);  out = g;  out[jmax_b] += S_b;  out[jmin_b] -= S_b.
 * Every term is the reference's own sequence of fp32 operations with IEEE quotients (the bucket-invariant division only in
 * buckets where it equals them: alpha_q in [2^-60, 2^100], every non-zero x - beta_q >= max(2^-100, alpha_q 2^-120)); only
 * the order of the fp32 sum differs.  Requires bucket > 0 (as the reference does, :332-334).  out may alias g. */
int qd_ste_bucket_backward_f32(const float* x, const float* g, float* out, int64_t n, int64_t bucket, int levels,
                               int tie_mode, void* stream);

/* K8: 'truncated' STE (cnn_models/conv_forward_model.py:240-241,263-264):
 * qd_clamp_f32: w = clamp(w, -limit, limit) in place (NaN stays NaN); qd_truncated_ste_f32: grad[|w| > limit] = 0 (a NaN w
 * keeps its gradient, an infinite one loses it). */
int qd_clamp_f32(float* w, int64_t n, float limit, void* stream);
int qd_truncated_ste_f32(const float* w, float* grad, int64_t n, float limit, void* stream);

/* Multi-tensor K1: one launch quantizes every parameter tensor of a model (the per-step loop
 * `for p in model.parameters(): p.data = uniformQuantization(p.data, s, bucket_size=...)[0]`,
 * cnn_models/conv_forward_model.py:235-247).  `table` is a DEVICE array of descriptors built
 * once per model; each tensor is bucketed independently with the same `bucket`/`levels`.
 * bucket must be > 0. */
typedef struct QdTensorDesc {
    const float* x;      /* master weights            */
    float* q;            /* quantized shadow (may alias x) */
    int64_t n;           /* elements                   */
    int64_t first_tile;  /* prefix sum of work tiles (filled by qd_multi_plan) */
} QdTensorDesc;

/* Host helper: fills first_tile of `ntensors` host descriptors, returns the total tile count
 * (pass it to qd_multi_uniform_f32 as total_tiles). */
int64_t qd_multi_plan(QdTensorDesc* host_table, int ntensors, int64_t bucket);
int qd_multi_uniform_f32(const QdTensorDesc* table, int ntensors, int64_t total_tiles, int64_t bucket, int levels,
                         void* stream);

/* Multi-tensor K1g: the same per-step loop with bucket_size=None (every tensor one bucket with its
 * own global min/max; e.g. cifar10_test.py:113): three launches for the whole model (per-tile
 * min/max, per-tensor fold, apply) instead of three per tensor.  qd_multi_global_plan fills
 * first_tile (1024-element tiles); alpha_beta: [ntensors][2] output; workspace >= total_tiles*8 bytes. */
int64_t qd_multi_global_plan(QdTensorDesc* host_table, int ntensors);
int qd_multi_uniform_global_f32(const QdTensorDesc* table, int ntensors, int64_t total_tiles, int levels,
                                float* alpha_beta, void* workspace, size_t workspace_bytes, void* stream);

/* Multi-tensor K1 / K1g with the options the reference's loops hand to every per-parameter call
 * (translation_models/model.py:162,200-209: stochasticRounding, maxElementAllowedForQuantization).  Tables and tile counts
 * come from qd_multi_plan / qd_multi_global_plan as above; mean subtraction is not offered (qd_mean_f32 is an
 * order-dependent sum of its own launch).
 *   Contract: with stochastic == 0 && clamp == 0 the result equals qd_multi_uniform_f32 / qd_multi_uniform_global_f32; in
 *   every configuration tensor i of the table equals
 *       qd_uniform_f32(x_i, q_i, n_i, bucket, levels, NULL, NULL, NULL, NULL, clamp, max_element, stochastic, seed0 + i, ...)
 *   bit for bit (bucket = 0 for the global form, whose alpha_beta rows are that call's alpha and beta).
 *   Seed rule: tensor i draws with seed0 + i modulo 2^64 -- i is the POSITION in the table, tensors without elements
 *   included -- and its element e takes word e & 3 of Philox block e >> 2, as qd_uniform_f32 documents.  seed0 is `seed`
 *   when seed_cell == NULL, else *seed_cell: one 8-byte-aligned word of DEVICE memory that the kernel reads (once per wave)
 *   and never writes.
 *   Capture: a by-value seed is frozen into a captured launch, which then replays the same draws.  A launch that reads
 *   seed_cell draws whatever the cell holds when the replay runs: advance the cell by ntensors on the same stream after the
 *   launch (inside the captured region) and every replay rounds anew, replay r using seed0 + r * ntensors + i.
 *   Errors: clamp != 0 with max_element not a positive number, or seed_cell not 8-byte aligned: QD_ERR_INVALID_ARGUMENT;
 *   the global form's workspace as above (QD_ERR_WORKSPACE_TOO_SMALL, nothing written); total_tiles == 0 returns 0
 *   without a launch.  stochastic == 0 ignores seed and seed_cell. */
int qd_multi_uniform_opt_f32(const QdTensorDesc* table, int ntensors, int64_t total_tiles, int64_t bucket, int levels,
                             int clamp, float max_element, int stochastic, uint64_t seed, const uint64_t* seed_cell,
                             void* stream);
int qd_multi_uniform_global_opt_f32(const QdTensorDesc* table, int ntensors, int64_t total_tiles, int levels,
                                    int clamp, float max_element, int stochastic, uint64_t seed, const uint64_t* seed_cell,
                                    float* alpha_beta, void* workspace, size_t workspace_bytes, void* stream);

/* Multi-tensor K1 / K1g with a level count PER TENSOR (per-layer bit widths, e.g. 8 bits for the first and the last layer and
 * 4 or 2 in between: what the per-tensor loop does when it calls uniformQuantization(t_i, s_i, ...)).  Tables and tile counts
 * come from qd_multi_plan / qd_multi_global_plan as above: neither depends on the level count.
 *   levels: a DEVICE array of ntensors int32 values, 4-byte aligned; entry i belongs to position i of the table, tensors
 *   without elements included.  The kernels read it (one scalar load per tile) and never write it.
 *   Contract: tensor i of the table equals
 *       qd_uniform_f32(x_i, q_i, n_i, bucket, levels[i], NULL, NULL, NULL, NULL, clamp, max_element, stochastic, seed0 + i, ...)
 *   bit for bit (bucket = 0 for the global form, whose alpha_beta row i is that call's alpha and beta; the row of a tensor
 *   without elements is (1, +inf)).  The seed rule, the capture rule, the workspace, aliasing (q may alias x) and
 *   total_tiles == 0 (returns 0 without a launch) are those of qd_multi_uniform_opt_f32 / qd_multi_uniform_global_opt_f32.
 *   Errors: levels == NULL or not 4-byte aligned, and everything the _opt entry points refuse: QD_ERR_INVALID_ARGUMENT; the
 *   global form's workspace: QD_ERR_WORKSPACE_TOO_SMALL, nothing written.
 *   The library cannot look into device memory without a synchronisation, so the VALUES of levels are the caller's: an entry
 *   < 2 gives wrong values in that tensor's output (q_i, and nothing else: no other tensor, no other memory). */
int qd_multi_uniform_levels_f32(const QdTensorDesc* table, const int32_t* levels, int ntensors, int64_t total_tiles,
                                int64_t bucket, int clamp, float max_element, int stochastic, uint64_t seed,
                                const uint64_t* seed_cell, void* stream);
int qd_multi_uniform_global_levels_f32(const QdTensorDesc* table, const int32_t* levels, int ntensors, int64_t total_tiles,
                                       int clamp, float max_element, int stochastic, uint64_t seed, const uint64_t* seed_cell,
                                       float* alpha_beta, void* workspace, size_t workspace_bytes, void* stream);

/* Multi-tensor K1 / K1g writing fp16 or bf16 OUTPUTS (fp32 master weights, a 16-bit student): the level-count-per-tensor forms
 * above with another store.  Device library only.  Tables and tile counts come from qd_multi_plan / qd_multi_global_plan, the
 * descriptor is QdTensorDesc -- but for these two entry points `q` addresses n 16-BIT elements (out_kind says which format),
 * needs 2-byte alignment only, and must not overlap any `x` of the table (x stays fp32, 4-byte aligned).
 *   Contract: element e of tensor i is the IEEE round-to-nearest-even conversion to fp16 / bf16 of element e of what
 *   qd_multi_uniform_levels_f32 / qd_multi_uniform_global_levels_f32 writes for the same arguments, bit for bit on the 16-bit
 *   patterns: a NaN stays a NaN (payload unspecified), +-inf stays, a finite value beyond the format's range becomes +-inf,
 *   fp16 subnormals are produced (not flushed), the sign of zero is kept.  All arithmetic is the fp32 launch's; only the
 *   store differs, and the global form's alpha_beta rows have the bits they have there.  Whatever the alignment of q (full
 *   buckets with x 16-byte and q 8-byte aligned take a register path, everything else a scalar one) the bits are the same,
 *   and nothing is written before q or from q + n on.
 *   levels: the device int32 array of qd_multi_uniform_levels_f32, always (one level count for all: equal entries).
 *   The seed rule, the capture rule, the workspace and total_tiles == 0 (returns 0 without a launch) are those of
 *   qd_multi_uniform_opt_f32 / qd_multi_uniform_global_opt_f32.
 *   Errors: out_kind other than the two below, and everything the _levels entry points refuse: QD_ERR_INVALID_ARGUMENT; the
 *   global form's workspace: QD_ERR_WORKSPACE_TOO_SMALL, nothing written. */
#define QD_OUT_F16 1
#define QD_OUT_BF16 2
int qd_multi_uniform_out16_f32(const QdTensorDesc* table, const int32_t* levels, int ntensors, int64_t total_tiles,
                               int64_t bucket, int out_kind, int clamp, float max_element, int stochastic, uint64_t seed,
                               const uint64_t* seed_cell, void* stream);
int qd_multi_uniform_global_out16_f32(const QdTensorDesc* table, const int32_t* levels, int ntensors, int64_t total_tiles,
                                      int out_kind, int clamp, float max_element, int stochastic, uint64_t seed,
                                      const uint64_t* seed_cell, float* alpha_beta, void* workspace, size_t workspace_bytes,
                                      void* stream);

/* Multi-tensor K7: the 'complicated' straight-through backward of every quantized parameter of a model in ONE launch (the
 * per-step loop `quantizeFunctions[idx].backward(p.grad.data)`, cnn_models/conv_forward_model.py:253-266).  `table` is a
 * DEVICE array of descriptors; each tensor is bucketed independently with the same bucket / levels / tie_mode and its result
 * is bit-identical to qd_ste_bucket_backward_f32 on the same pointers: every bucket takes the path the per-tensor call
 * would give it and is summed in that order.  No workspace, no allocation, no synchronisation.  bucket must be > 0. */
typedef struct QdSteDesc {
    const float* x;      /* full-precision weights the forward quantized   */
    const float* g;      /* dLoss/dq                                        */
    float* out;          /* result; may alias g                             */
    int64_t n;
    int64_t first_tile;  /* filled by qd_multi_ste_plan                     */
} QdSteDesc;
/* Host helper: fills first_tile of `ntensors` HOST descriptors (x, g, out, n set: the tile rule depends on the pointers'
 * alignment) and writes the total tile count, to be passed to qd_multi_ste_backward_f32.  A tile is one wave iteration on
 * one tensor.  Tensors whose bucket row (min(n, bucket)) is 64 / 128 / 256 / 512 / 1024, that hold more than one bucket and
 * whose x, g, out are 4-byte aligned own ceil((n / row) / B) register tiles of B = 4 (row <= 256) or 1 (row >= 512) full
 * buckets, then one single-bucket tile for a ragged last bucket; every other tensor owns one tile per bucket; an empty
 * tensor owns none.  Returns 0 or QD_ERR_INVALID_ARGUMENT. */
int qd_multi_ste_plan(QdSteDesc* host_table, int ntensors, int64_t bucket, int64_t* total_tiles_out);
int qd_multi_ste_backward_f32(const QdSteDesc* table, int ntensors, int64_t total_tiles, int64_t bucket, int levels,
                              int tie_mode, void* stream);
/* The same with a level count per tensor: `levels` as qd_multi_uniform_levels_f32 documents it (a DEVICE array of ntensors
 * int32, 4-byte aligned, entry i for position i of the table, empty tensors included; NULL or misaligned:
 * QD_ERR_INVALID_ARGUMENT).  Table and tile count come from qd_multi_ste_plan, which does not depend on the level count.
 * Tensor i equals qd_ste_bucket_backward_f32(x_i, g_i, out_i, n_i, bucket, levels[i], tie_mode, ...) bit for bit, every bucket
 * summed in the order that call sums it; out may alias g; total_tiles == 0 returns 0 without a launch.  An entry < 2 gives
 * wrong values in out_i and touches nothing else. */
int qd_multi_ste_backward_levels_f32(const QdSteDesc* table, const int32_t* levels, int ntensors, int64_t total_tiles,
                                     int64_t bucket, int tie_mode, void* stream);

/* Multi-tensor K7 reading fp16 or bf16 GRADIENTS (a 16-bit student's p.grad, fp32 master weights and fp32 master gradients):
 * qd_multi_ste_backward_levels_f32 with another load.  Device library only.  The descriptor is QdSteDesc -- but for these two
 * entry points `g` addresses n 16-BIT elements (grad_kind says which format) and needs 2-byte alignment only; x and out stay
 * fp32, 4-byte aligned; out must not overlap any g or x of the table (no in-place form: the element sizes differ).
 *   Contract: tensor i equals qd_ste_bucket_backward_f32(x_i, W(g_i), out_i, n_i, bucket, levels[i], tie_mode) bit for bit,
 *   where W is the exact widening of every element to fp32: fp16 and bf16 subnormals are kept (not flushed), the sign of zero
 *   is kept, +-inf stays +-inf, a NaN stays a NaN (payload unspecified).  All arithmetic is the fp32 launch's; only the load
 *   of g differs.  The bits do not depend on the alignment of g: plan and kernel cut a tensor into register tiles and
 *   single-bucket tiles from n, bucket, x and out alone, so a 2-byte-aligned g takes the register tiles whenever the fp32 call
 *   on a widened copy would (g is then read with 8-byte loads where it is 8-byte aligned, element by element otherwise).
 *   That is why the table must be planned by qd_multi_ste_in16_plan, not by qd_multi_ste_plan.
 *   Nothing is read before g or from g + n on, nothing is written before out or from out + n on.
 *   levels: the device int32 array of qd_multi_ste_backward_levels_f32, always (one level count for all: equal entries).
 *   total_tiles == 0 returns 0 without a launch.  No workspace, no allocation, no synchronisation.
 *   Errors (QD_ERR_INVALID_ARGUMENT, nothing written): grad_kind other than the two below; everything
 *   qd_multi_ste_backward_levels_f32 refuses; in the plan, what qd_multi_ste_plan refuses and an odd g address. */
#define QD_GRAD_F16 1
#define QD_GRAD_BF16 2
int qd_multi_ste_in16_plan(QdSteDesc* host_table, int ntensors, int64_t bucket, int64_t* total_tiles_out);
int qd_multi_ste_backward_in16_f32(const QdSteDesc* table, const int32_t* levels, int ntensors, int64_t total_tiles,
                                   int64_t bucket, int grad_kind, int tie_mode, void* stream);

/* Multi-tensor K1 and K7 with a level count AND a bucket size PER TENSOR (per-channel scales: for a contiguous [out, ...] weight
 * bucket_i = elements per output channel; what the per-tensor loop does when it calls uniformQuantization(t_i, s_i,
 * bucket_size=b_i) and ste_bucket_backward(..., b_i, s_i)).  Device library only.  The descriptors are QdTensorDesc / QdSteDesc.
 *   buckets: for the two plan calls a HOST array of ntensors int64 values, each > 0; for the two launches a DEVICE array of
 *   ntensors int64 values, 8-byte aligned; entry i belongs to position i of the table, tensors without elements included.  The
 *   kernels read it (one scalar load per tile) and never write it.  The device array MUST HOLD THE VALUES THE PLAN WAS MADE
 *   WITH: the library cannot look into device memory without a synchronisation.  (An entry that disagrees gives wrong values
 *   in, or leaves unwritten, tensors of that table and touches no other memory; an entry < 1 leaves its tensor unwritten.)
 *   levels: the device int32 array of qd_multi_uniform_levels_f32, always (one level count for all: equal entries).
 *   Tile rule of qd_multi_buckets_plan, with row = min(n, bucket) and nb = ceil(n / row): ceil(nb / 4) tiles for row <= 256 (a
 *   DPP row per bucket; full 16-byte aligned rows of 64 / 128 / 256 are held in registers, other full aligned rows that are a
 *   multiple of 4 are read as float4, the rest element by element), nb tiles for row > 256 (a wave per bucket, two passes).  A
 *   row of more than 64 Ki elements runs on one wave: correct, not tuned -- whole-tensor scaling is qd_multi_uniform_global_*.
 *   qd_multi_ste_buckets_plan counts as qd_multi_ste_plan does, tensor i under buckets[i].
 *   Contract: tensor i of the table equals, bit for bit,
 *       qd_uniform_f32(x_i, q_i, n_i, buckets[i], levels[i], NULL, NULL, NULL, NULL, clamp, max_element, stochastic, seed0 + i, ...)
 *       qd_ste_bucket_backward_f32(x_i, g_i, out_i, n_i, buckets[i], levels[i], tie_mode, ...)
 *   every bucket of the backward summed by the body and in the order that call uses.  q may alias x, out may alias g; nothing
 *   is written outside [q_i, q_i + n_i) / [out_i, out_i + n_i).  A tensor without elements owns no tile and keeps its position
 *   in levels, in buckets and in the seed rule.  The seed rule and the capture rule are those of qd_multi_uniform_opt_f32;
 *   total_tiles == 0 returns 0 without a launch.  No workspace, no allocation, no synchronisation.
 *   Errors (QD_ERR_INVALID_ARGUMENT, nothing written): levels or buckets NULL, levels not 4-byte or device buckets not 8-byte
 *   aligned; in a plan call a buckets entry <= 0, ntensors <= 0, total_tiles_out NULL, n < 0 or a NULL pointer of a tensor that
 *   has elements; everything qd_multi_uniform_levels_f32 / qd_multi_ste_backward_levels_f32 refuse. */
int qd_multi_buckets_plan(QdTensorDesc* host_table, const int64_t* buckets, int ntensors, int64_t* total_tiles_out);
int qd_multi_uniform_buckets_f32(const QdTensorDesc* table, const int32_t* levels, const int64_t* buckets, int ntensors,
                                 int64_t total_tiles, int clamp, float max_element, int stochastic, uint64_t seed,
                                 const uint64_t* seed_cell, void* stream);
int qd_multi_ste_buckets_plan(QdSteDesc* host_table, const int64_t* buckets, int ntensors, int64_t* total_tiles_out);
int qd_multi_ste_backward_buckets_f32(const QdSteDesc* table, const int32_t* levels, const int64_t* buckets, int ntensors,
                                      int64_t total_tiles, int tie_mode, void* stream);

/* The SYMBOLS of a whole model in one launch: what a compressed checkpoint stores of a uniformly quantized tensor -- the uint8
 * level index of every weight and the (alpha, beta) of every bucket -- for every tensor of a table, each under its own level
 * count and its own bucket size, without the fp32 result (4 B read + 1 B written per element; the per-tensor loop over
 * qd_uniform_f32 with its level output moves 9 B and launches once per tensor).  Device library only.
 *   buckets, levels: as for qd_multi_uniform_buckets_f32 -- buckets a HOST array for the plan and an 8-byte aligned DEVICE array
 *   holding the same values for the launch, levels a DEVICE int32 array, entry i for position i of the table; neither is written.
 *   qd_multi_symbols_plan counts tiles by the tile rule of qd_multi_buckets_plan and fills first_tile and first_bucket, the
 *   running sum of nb = ceil(n / min(n, bucket)); *total_buckets_out is the length alpha and beta need.
 *   Contract: tensor i of the table equals, bit for bit, the level_idx, alpha and beta of
 *       qd_uniform_f32(x_i, <scratch>, n_i, buckets[i], levels[i], alpha + first_bucket_i, beta + first_bucket_i, sym_i,
 *                      NULL, 0, 0, 0, 0, ...)
 *   deterministic rounding, no clamp, no mean: level = rint(((v - beta) / alpha) * (levels - 1)), each operation rounded to
 *   fp32, stored as (uint8_t)(int)level -- a bucket that holds a NaN or an infinity gets symbol 0 and that call's alpha / beta.
 *   Neither the alignment of x_i (any multiple of 4) nor that of sym_i (any) changes a bit.  Nothing is written outside
 *   [sym_i, sym_i + n_i), alpha[first_bucket_i .. + nb_i) and beta[first_bucket_i .. + nb_i); x is never written.  A tensor
 *   without elements owns no tile and no bucket and keeps its position in levels and buckets.  A levels entry outside 2 .. 256
 *   or a buckets entry that disagrees with the plan may give wrong values in that tensor's own outputs: symbol addresses are
 *   bounded by n_i, alpha / beta indices by the next descriptor's first_bucket (for the table's last tensor by
 *   ceil(n / min(n, buckets[i])): alpha and beta hold the plan's total_buckets entries under the values the plan was made with);
 *   a buckets entry < 1 leaves its tensor unwritten.  total_tiles == 0 returns 0 without a launch.  No workspace, no
 *   allocation, no synchronisation: the launch can be captured into a graph.
 *   Errors (QD_ERR_INVALID_ARGUMENT, nothing written): table, levels, buckets, alpha or beta NULL; levels, alpha or beta not
 *   4-byte, device buckets not 8-byte aligned; ntensors <= 0, total_tiles < 0; in the plan a NULL output, a buckets entry <= 0,
 *   n < 0 or a NULL pointer of a tensor that has elements. */
typedef struct QdSymbolDesc {
    const float* x;        /* n fp32 weights, 4-byte aligned; never written            */
    uint8_t* sym;          /* n level indices, any alignment; must not overlap x       */
    int64_t n;
    int64_t first_tile;    /* filled by the plan                                       */
    int64_t first_bucket;  /* filled by the plan: index of the tensor's first bucket   */
} QdSymbolDesc;
int qd_multi_symbols_plan(QdSymbolDesc* host_table, const int64_t* buckets, int ntensors, int64_t* total_tiles_out,
                          int64_t* total_buckets_out);
int qd_multi_uniform_symbols_u8(const QdSymbolDesc* table, const int32_t* levels, const int64_t* buckets, int ntensors,
                                int64_t total_tiles, float* alpha, float* beta, void* stream);

/* ---- 'absmax' / 'absnorm' scaling (type_scaling of ScalingFunction, quant_functions.py:109-127,144-146).
 * PARITY UNPINNED: the reference code for these two types raises on every torch version, so these
 * entry points implement the math those lines evidently intend (see qd_abs.hip):
 *     sign = sign(x), m = |x|, norm_b = max_b m (norm_kind 0) or sqrt(sum_b m^2) (norm_kind 1), < 1e-10 -> 1
 *     qd_scale_down_abs_f32 : u = m/norm_b and sign, both in the PADDED bucket layout; norm_out [num_buckets]
 *     qd_inv_scale_abs_f32  : y = u*norm_b*sign (+mean), padding dropped
 *     qd_uniform_abs_f32    : q = rint(u*(levels-1))/(levels-1)*norm_b*sign (+mean) */
int qd_uniform_abs_f32(const float* x, float* q, int64_t n, int64_t bucket, int levels, int norm_kind, float* norm_out,
                       const float* mean, int clamp, float max_element, void* workspace, size_t workspace_bytes,
                       void* stream);
int qd_scale_down_abs_f32(const float* x, float* u, float* sign, int64_t n, int64_t bucket, int norm_kind,
                          float* norm_out, const float* mean, int clamp, float max_element, void* workspace,
                          size_t workspace_bytes, void* stream);
int qd_inv_scale_abs_f32(const float* u, const float* sign, float* y, int64_t n, int64_t bucket, const float* norm,
                         const float* mean, void* stream);

/* ---- multi-tensor differentiable-quantization step: the per-tensor calls
 *     p_quantized.data = quantizationFunctions[i].forward(None, points[i].data)   (conv_forward_model.py:532)
 *     points[i].grad.data = quantizationFunctions[i].backward(p.grad.data)[1]     (conv_forward_model.py:545)
 * for ALL tensors in one launch each.  Arithmetic = qd_nearest_point_f32(prescaled, MIDPOINT) with
 * uint8 indices and qd_point_grad_f32.  1 <= k <= 256 (the index is a byte; a NaN u takes k - 1); bucket == 0 means "no
 * buckets" as everywhere in this header (one alpha[0] / beta[0] per tensor), any bucket > 0 is taken, and a tensor of
 * n <= bucket elements is one bucket.  `points` is one device array [ntensors][k] (so the optimizer updates a single
 * tensor); grad_points likewise.  Tuned: buckets 64 / 128 / 256 with k <= 64 and, forward only, bucket == 0.  Functional,
 * not tuned: k > 64 (the backward sweep then runs one wave per block, its lane-private bins [k][64] floats of LDS = 64 KB at
 * k = 256) and buckets that are no power of two (forward: a 16-lane group per bucket, element-wise; backward: alpha looked up
 * per element, a float4 can straddle a bucket end). */
typedef struct QdDiffQuantDesc {
    const float* u;       /* scaled weights, resident [n]                                  */
    float* q;             /* quantized weights out [n] (qd_multi_nearest_out16_f32: n 16-bit elements)   */
    uint8_t* idx;         /* point index out (forward) / in (backward) [n]                 */
    const float* alpha;   /* [num_buckets]                                                 */
    const float* beta;    /* [num_buckets]                                                 */
    const float* grad;    /* dLoss/dq [n] (backward only; qd_multi_point_grad_in16_f32: n 16-bit elements) */
    int64_t n;
    int64_t first_tile;   /* filled by qd_multi_dq_plan: prefix of forward tiles (4 buckets; bucket == 0: 1024 elements) */
    int64_t first_block;  /* filled by qd_multi_dq_plan: prefix of FULL 1024-element gradient tiles (backward) */
    int64_t first_row;    /* filled by qd_multi_dq_plan: prefix of the backward sweep's partial rows (ABI 3)  */
} QdDiffQuantDesc;
/* Host helper: fills first_tile / first_block / first_row, returns the total of forward tiles (bucket > 0: ceil(buckets / 4)
 * per tensor; bucket == 0: ceil(n / 1024) per tensor; an empty tensor has none), writes `total_blocks` = the
 * number of partial rows of the backward sweep: min(full 1024-element gradient tiles, 2048) + 1 per tensor (the 2048 waves of
 * the main grid stride over the ONE sequence of all tensors' full tiles and write one row per tensor they visit; one more
 * wave per tensor takes the n mod 1024 elements left); first_block, first_row and total_blocks do not depend on the bucket.
 * Pass it to qd_multi_point_grad_f32 unchanged. */
int64_t qd_multi_dq_plan(QdDiffQuantDesc* host_table, int ntensors, int64_t bucket, int64_t* total_blocks_out);
int qd_multi_nearest_f32(const QdDiffQuantDesc* table, int ntensors, int64_t total_tiles, int64_t bucket,
                         const float* points, int k, void* stream);
/* workspace: at least total_blocks * k floats, contents need no initialisation -- at k = 256 that is 1 KiB per partial row,
 * at most (2048 + 1) KiB ~ 2 MiB per tensor (WRN-16-22, 60 tensors: 21001 rows = 21.5 MB) */
int qd_multi_point_grad_f32(const QdDiffQuantDesc* table, int ntensors, int64_t total_blocks, int64_t bucket, int k,
                            float* grad_points, void* workspace, size_t workspace_bytes, void* stream);

/* The two sweeps for a 16-BIT STUDENT over fp32 masters: fp16 / bf16 quantized weights out, fp16 / bf16 gradients in.  Device
 * library only.  Both take the QdDiffQuantDesc table and the tile / row counts of qd_multi_dq_plan (the plan depends on no
 * pointer); u, alpha, beta, idx, points and grad_points are what they are above, fp32.  The two are independent: a table may
 * hold 16-bit q with fp32 grad or the reverse, each field read by the entry point that matches it.
 *
 * qd_multi_nearest_out16_f32: `q` addresses n 16-BIT elements (out_kind: QD_OUT_F16 / QD_OUT_BF16), needs 2-byte alignment
 *   only and must not overlap any `u`.
 *   Contract: element e of tensor i is the IEEE round-to-nearest-even conversion to fp16 / bf16 of what qd_multi_nearest_f32
 *   writes for the same arguments, bit for bit on the 16-bit pattern: a NaN stays a NaN (payload unspecified), +-inf stays, a
 *   finite value beyond the format's range becomes +-inf, fp16 subnormals are produced (not flushed), the sign of zero is
 *   kept.  idx is byte-identical to the fp32 launch's.  k, bucket (0 or any positive size) and the NaN rule (a NaN u takes
 *   k - 1) are those of qd_multi_nearest_f32.  The bits do not depend on the alignment of q (full buckets -- bucket 0: full
 *   1024-element tiles -- with u 16-byte, q 8-byte and idx 4-byte aligned take a register path that stores four values with one
 *   8-byte store, everything else goes element by element), and nothing is written before q or from q + n on.
 *   Errors (QD_ERR_INVALID_ARGUMENT, nothing written): what qd_multi_nearest_f32 refuses, and an out_kind other than the two.
 *
 * qd_multi_point_grad_in16_f32: `grad` addresses n 16-BIT elements (grad_kind: QD_GRAD_F16 / QD_GRAD_BF16) and needs 2-byte
 *   alignment only.
 *   Contract: row i of grad_points equals, bit for bit, what qd_multi_point_grad_f32 gives with grad_i replaced by its exact
 *   fp32 widening held at a 16-byte-aligned address (subnormals, -0, +-inf and NaN are kept by the widening); everything else
 *   is the same, the second stage included.  The alignment of the 16-bit gradient has no say in the summation order: where
 *   the fp32 kernel picks between a lane that owns four consecutive elements and a lane-strided element-wise walk from grad's
 *   alignment (the two sum in different orders), this one takes the four-consecutive assignment whenever idx is 4-byte aligned
 *   -- reading grad with 8-byte loads where it is 8-byte aligned and with narrower loads otherwise -- and the strided walk
 *   only with a misaligned idx, as the fp32 launch does; in the main grid and in the extra waves alike.  Nothing is read
 *   before grad or from grad + n on.
 *   Workspace, the checks on total_blocks and the error codes are those of qd_multi_point_grad_f32; a grad_kind other than the
 *   two: QD_ERR_INVALID_ARGUMENT.
 *
 * Odd addresses: the launches take a DEVICE table and cannot look into it without a synchronisation, so the pointers are
 * checked where the host sees them: qd_multi_dq_plan returns -1 (QD_ERR_INVALID_ARGUMENT), with no field written, when q or
 * grad of a tensor that has elements is odd -- wrong for fp32 and for 16-bit elements alike. */
int qd_multi_nearest_out16_f32(const QdDiffQuantDesc* table, int ntensors, int64_t total_tiles, int64_t bucket,
                               const float* points, int k, int out_kind /* QD_OUT_F16 | QD_OUT_BF16 */, void* stream);
int qd_multi_point_grad_in16_f32(const QdDiffQuantDesc* table, int ntensors, int64_t total_blocks, int64_t bucket, int k,
                                 int grad_kind /* QD_GRAD_F16 | QD_GRAD_BF16 */, float* grad_points, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* ---- packed-index codec (the compressed form whose SIZE the reference accounts for in
 * helpers/functions.py:226-262: bits*N/8 bytes of level indices + 8 bytes (alpha, beta) per
 * bucket) and the level histogram behind the Huffman accounting of
 * quantization/help_functions.py:175-232.
 * qd_pack_uniform_f32: quantize x with `levels` levels per bucket and store ONLY the level
 *   indices, `bits` (any of 1 ... 8; levels <= 2^bits) per element, element e in bits
 *   [e*bits, (e+1)*bits) of `packed` (qd_packed_bytes(n, bits) bytes, little endian inside a byte),
 *   plus alpha/beta [num_buckets] (optional).  bucket in {64,128,256,512,1024,2048}; x 16-byte aligned.
 *   The stream, for all eight widths: bit i of the stream is bit i & 7 of byte i >> 3; element e holds its index least
 *   significant bit first in stream bits [e*bits, (e+1)*bits) -- at 3, 5, 6 and 7 bits across a byte or a 32-bit word
 *   boundary where it falls on one; the unused high bits of the last byte are zero.  Every call of the three entry points
 *   writes, or reads, exactly qd_packed_bytes(n, bits) bytes of `packed` and not one more (`packed` 4-byte aligned for
 *   qd_pack_uniform_f32 and qd_unpack_uniform_f32, any alignment for qd_pack_levels_u8; the last partial 32-bit word is
 *   accessed byte by byte).  qd_pack_levels_u8 masks every symbol to `bits` bits.
 * qd_pack_levels_u8: the same packing for level indices that are already there (the level_idx output of qd_uniform_f32):
 *   together they give the packed form at ANY bucket size, bucket 0 = none included.
 * qd_unpack_uniform_f32: y = (index/(levels-1))*alpha + beta -- bit-identical to the output of
 *   qd_uniform_f32 on the same input.  Any bucket size (0: one alpha / beta for the tensor).
 * qd_histogram_u8: hist[j] = #{i : idx[i] == j}, j < k <= 256 (hist is overwritten).
 * qd_histogram_u8_ws: the same with a scratch buffer (8-byte aligned, qd_workspace_bytes() is enough; contents need no
 *   initialisation): per-block totals go there and are summed per bin in a fixed order -- no global atomics. */
int64_t qd_packed_bytes(int64_t n, int bits);
int qd_pack_uniform_f32(const float* x, int64_t n, int64_t bucket, int levels, int bits, uint8_t* packed, float* alpha,
                        float* beta, void* stream);
int qd_pack_levels_u8(const uint8_t* levels_idx, int64_t n, int bits, uint8_t* packed, void* stream);
int qd_unpack_uniform_f32(const uint8_t* packed, int64_t n, int64_t bucket, int levels, int bits, const float* alpha,
                          const float* beta, float* y, void* stream);
int qd_histogram_u8(const uint8_t* idx, int64_t n, int k, uint64_t* hist, void* stream);
int qd_histogram_u8_ws(const uint8_t* idx, int64_t n, int k, uint64_t* hist, void* workspace, size_t workspace_bytes,
                       void* stream);
/* qd_level_histogram_f32: hist[j] = number of elements of x whose quantization level (levels per bucket, as qd_uniform_f32
 * computes it) is j, j < levels <= 256 -- in ONE pass, 4 B read per element: the level indices are counted in the kernel that
 * computes them and never written.  bucket in {64 ... 2048}, x 16-byte aligned (QD_ERR_UNSUPPORTED otherwise: callers then
 * write the levels with qd_uniform_f32 and count them with qd_histogram_u8_ws).  Elements of a bucket that holds a NaN count as
 * level 0 (what the uint8 level output stores for them).  workspace as for qd_histogram_u8_ws. */
int qd_level_histogram_f32(const float* x, int64_t n, int64_t bucket, int levels, uint64_t* hist, void* workspace,
                           size_t workspace_bytes, void* stream);
/* The two histograms get_huffman_encoding_mean_bit_length needs when it runs on the device (quantization/help_functions.py:
 * 175-232; only the counters cross PCIe instead of every quantized tensor):
 * qd_digitize_histogram_f32: hist[c] = #{ i : #{ j < m : edges[j] <= v[i] } == c }, c = 0 .. m (hist has m + 1 entries; a NaN
 *   counts as c = m) -- np.digitize(v, edges) of :216-218 followed by np.unique(..., return_counts=True) of :223, for
 *   `edges` a DEVICE array of m <= 256 increasing float64 values, compared in float64 as numpy does.  v: the re-scaled
 *   quantized tensor (`scal.scale_down(q_tensor)`, :215), n elements, 4-byte aligned.
 * qd_histogram_i64: hist[j] = #{ i : idx[i] == j } for j < k <= 256 and hist[k] = #{ i : idx[i] outside [0, k) } (k + 1
 *   entries) -- the counts of the int64 indices nonUniformQuantization returns (:220-221).
 * Both: workspace as for qd_histogram_u8_ws (required when n > 0), deterministic (per-block totals summed in a fixed order). */
int qd_digitize_histogram_f32(const float* v, int64_t n, const double* edges, int m, uint64_t* hist, void* workspace,
                              size_t workspace_bytes, void* stream);
int qd_histogram_i64(const int64_t* idx, int64_t n, int k, uint64_t* hist, void* workspace, size_t workspace_bytes,
                     void* stream);
/* qd_scale_digitize_histogram_f32: the re-scale and the digitize + count of :215-223 in ONE pass over the quantized tensor q
 * (4 B read per element; the two-call form -- qd_scale_down_f32, then qd_digitize_histogram_f32 over its output -- moves 12):
 * hist[c] = #{ i : #{ j < m : edges[j] <= (double)u[i] } == c } with u = ScalingFunction('linear', bucket_size=bucket)
 * .scale_down(q), i.e. per bucket (q - min) / (max - min or 1), bit-identical to qd_scale_down_f32's output.  For the plain
 * configuration only (no mean subtraction, no max_element), bucket in {64 ... 2048}, q 16-byte aligned: QD_ERR_UNSUPPORTED
 * otherwise, and the caller takes the two-call form.  edges, hist, workspace as for qd_digitize_histogram_f32. */
int qd_scale_digitize_histogram_f32(const float* q, int64_t n, int64_t bucket, const double* edges, int m, uint64_t* hist,
                                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- Huffman-coded model checkpoints (quantized_distillation_amd/compressed.py).  The reference only
 * ACCOUNTS for this form: helpers/functions.py:226-262 charges the Huffman mean code length of
 * quantization/help_functions.py:157-232 per quantized weight plus 8 B (alpha, beta) per bucket, and saves the student as a
 * full fp32 state_dict (cifar10_test.py:265-270).  These two entry points write and read that form.
 * Symbols (one uint8 per element: the level index of qd_uniform_f32 or the point index of qd_nearest_point_f32) are coded
 * with ONE canonical code for the whole model, codewords of at most 32 bits, most significant bit first inside 32-bit words.
 * Every tensor is cut into chunks of QD_HUF_CHUNK symbols (its last chunk may be shorter); chunk c starts on word
 * chunk_words[c] of the bitstream and never shares a word with another chunk.
 * QdHufTensor: one entry per quantized tensor, in file order (a DEVICE array for libqd_hip.so, host for libqd_host.so).
 * QdHufCode: the canonical code, built from the code lengths (compressed.py: canonical_code). */
#define QD_HUF_CHUNK 1024
typedef struct QdHufTensor {
    const uint8_t* sym;      /* encode: the tensor's n symbols                                     */
    float* y;                /* decode: the tensor's n fp32 outputs                                */
    int64_t n;               /* elements                                                          */
    int64_t first_chunk;     /* sum of ceil(n_j / QD_HUF_CHUNK) over the tensors before this one    */
    int64_t first_bucket;    /* decode: index of the tensor's first (alpha, beta) in alpha / beta  */
    int64_t first_point;     /* decode, non-uniform: index of the tensor's first point in points   */
    int64_t bucket;          /* decode: bucket size, 0 = one (alpha, beta) for the whole tensor     */
    int32_t levels;          /* decode: s (uniform) or k (non-uniform); a symbol >= levels decodes to NaN */
    int32_t nonuniform;      /* decode: 0 = (idx/(s-1))*alpha + beta, 1 = points[idx]*alpha + beta */
} QdHufTensor;
typedef struct QdHufCode {
    uint32_t code[256];      /* codeword of each symbol, right-aligned                            */
    uint32_t base[33];       /* first codeword of each length                                     */
    uint32_t count[33];      /* number of codewords of each length                                */
    uint32_t first[33];      /* position in sorted[] of the first symbol of each length           */
    uint8_t len[256];        /* code length of each symbol, 0 = not in the code                   */
    uint8_t sorted[256];     /* symbols in canonical order (length, then symbol)                  */
    int32_t single;          /* the only symbol of a one-symbol code (0 bits per symbol), else -1  */
    int32_t max_len;         /* longest codeword, <= 32                                           */
} QdHufCode;
/* qd_huffman_encode: the chunked bitstream of every tensor of `table` in three launches, however many tensors there are
 *   (per-chunk word counts, one exclusive scan over the chunks, the write; each chunk is assembled in LDS and stored as whole
 *   words).  chunk_words: [nchunks + 1] outputs, chunk_words[nchunks] = total words.  words: [max_words] output; a chunk that
 *   would end beyond max_words is not written (callers size it from the histogram: sum(count*len)/32 + nchunks words).
 *   Lengths: help_functions.py:157-172 (huffman_encode) over the histogram of :213-231, canonically numbered.
 * qd_huffman_decode_f32: ONE launch decodes every tensor of `table` and dequantizes in registers, writing fp32 straight to
 *   each tensor's y: uniform (idx/(s-1))*alpha + beta, as qd_unpack_uniform_f32 (= uniformQuantization, quant_functions.py:
 *   155-194); non-uniform points[idx]*alpha + beta, as K4's rescale (quant_functions.py:278-286).  nwords bounds every read of
 *   the bitstream.  Both: 4-byte aligned arrays; nchunks >= 1, ntensors >= 1. */
int qd_huffman_encode(const QdHufTensor* table, int ntensors, int64_t nchunks, const QdHufCode* code, uint32_t* chunk_words,
                      uint32_t* words, int64_t max_words, void* stream);
int qd_huffman_decode_f32(const uint32_t* words, int64_t nwords, const uint32_t* chunk_words, const QdHufTensor* table,
                          int ntensors, int64_t nchunks, const QdHufCode* code, const float* alpha, const float* beta,
                          const float* points, void* stream);

/* ---- order statistics for initialize_quantization_points (quantization/help_functions.py:140-154: the reference
 * copies the scaled tensor to the host and calls np.percentile(a, linspace(0, 100, k)), which needs the two
 * neighbouring order statistics of each of the k virtual indices).
 * qd_order_stats_f32: out[t] (device, m floats) = the ranks[t]-th smallest element of x[0..n) (0-based; every NaN, with
 *   either sign bit and any payload, orders last -- after +inf -- and a rank among the NaNs returns a NaN, not the bits of
 *   a particular one; -0 before +0), found by a 12|10|10-bit radix SELECT: x is read three times and never sorted or modified.
 *   ranks is a HOST array of m non-decreasing values in [0, n); 1 <= m <= QD_ORDER_STATS_MAX_RANKS; n < 2^32
 *   (QD_ERR_UNSUPPORTED beyond either).  workspace: qd_order_stats_workspace_bytes(m) bytes of device memory.
 *   ranks is read during the call and never again: it may be freed when the call returns, and a captured launch replays
 *   the ranks it was recorded with on the x of the moment. */
#define QD_ORDER_STATS_MAX_RANKS 32
size_t qd_order_stats_workspace_bytes(int m);
int qd_order_stats_f32(const float* x, int64_t n, const int64_t* ranks, int m, float* out, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---- self test of the bucket-invariant division (csrc/qd_selftest.hip).  The quantize kernels replace the IEEE division
 * u = (x - beta) / alpha of quantization/quant_functions.py:106-107 by y = RN(1/alpha) once per bucket and two FMAs per
 * element (qd_common.h: div_alpha<true>), which must give the correctly rounded quotient bit for bit wherever it is used:
 * alpha in [2^-60, 2^100], n = 0 or n >= 2^-100 -- and, where the quotient itself is consumed (qd_scale_down_f32,
 * qd_scale_digitize_histogram_f32, the terms of qd_ste_bucket_backward_f32 / qd_multi_ste_backward_f32), n >=
 * alpha 2^-120 as well (a normal quotient).  This entry point generates `npairs` adversarial (n, alpha) pairs of
 * `family` 0 .. 5 on the device (0: the quantizer's own domain, 1: wide exponents, 2: all-ones / near-power-of-two
 * significands, 3: near-exact quotients around level and half-level values, 4: the edges of the stated ranges, 5: small
 * normal quotients 2^-120 .. 2^-50), evaluates
 * the shortcut with the very function the kernels inline and compares it with n / alpha.
 * result (device, 4 x uint64): pairs tested, mismatches, (n bits << 32 | alpha bits) of one mismatch, pairs skipped
 * as outside the domain.  tools/div_invariant_check.py, tests/test_hip_parity.py. */
int qd_selftest_div_invariant(uint64_t seed, int64_t npairs, int family, unsigned long long* result, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QD_HIP_H */
