/* qd_infer_gen.h -- C ABI of libqd_infer_gen.so: the END of a decoder step -- the vocabulary projection ("generator"),
 * log-softmax and top-k -- of a model whose generator weight W[V][dim] is kept as packed low-bit weights, on the MI355X (gfx950).
 *
 * A decoder step ends with logits = W x + bias over the whole vocabulary, their log-softmax and, in beam search, the best few
 * (log-prob, word) pairs of every row.  Around qdm_linear_packed_f32 that is the [m][V] logits written, read once or twice and
 * written again by log_softmax, and read once more by topk.  This library makes it two launches in which the logits leave the
 * registers only where the caller asks for the log-probs: qdn_generator_packed_f32 walks the weight as qdm_linear_packed_f32 does
 * and reduces every row's logits to (max, sum of exp, top-k) per PANEL of QDN_PANEL vocabulary rows in the lanes that hold
 * them; a second, small launch combines the panels.  It is an artifact of its own, as the other six are: this header and
 * libqd_infer_gen.so, and nothing of the other libraries.
 *
 * The format and the weight value are those of qd_infer.h ("The format is ...", "The weight value."): the stream of
 * qd_pack_uniform_f32 for a contiguous W[V][dim], one (alpha, beta) per flat bucket, bucket == 0 or fewer elements than a bucket
 * one bucket, 2 <= levels <= 256, 1 <= bits <= 8, levels <= 2^bits; w = (((float)c / (float)(levels - 1)) alpha[k] + beta[k]) + 0.0f,
 * bit for bit what qd_unpack_uniform_f32 writes.
 *
 * The Conventions of qd_infer.h hold as qd_infer_mm.h words them: device pointers, asynchronous on `stream`; every float pointer,
 * `packed` and `work` 4-byte aligned (top_idx 8-byte) and no other alignment changes a bit of a result; the call writes exactly
 * the outputs it was given and `work`, and reads nothing outside its inputs; TWO kernel launches on `stream`, no allocation
 * (`work` is the caller's), no synchronisation, no atomics, no wait of one block for another, so it can be recorded into a
 * hipGraph (by-value arguments frozen at record time, device memory read at replay time).  m == 0 or V == 0 returns 0 without a
 * launch; 0 on success, a positive hipError_t if a launch failed, QDN_ERR_INVALID_ARGUMENT (-1) -- nothing written, nothing
 * launched -- for what the call lists.
 */
#ifndef QD_INFER_GEN_H
#define QD_INFER_GEN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QDN_ABI_VERSION 1
#define QDN_ERR_INVALID_ARGUMENT (-1)

/* Vocabulary rows of a panel: the unit of the first launch's reductions.  A constant of the ABI, not a launch parameter: the
 * orders below depend on it, and a result is to be a function of (V, dim) alone. */
#define QDN_PANEL 64
/* The largest k. */
#define QDN_MAX_TOPK 16

int qdn_abi_version(void);          /* QDN_ABI_VERSION */
const char* qdn_target_arch(void);  /* "gfx950" */
const char* qdn_error_string(int code);

/* Test hook, as qdm_set_grid_cap of qd_infer_mm.h: at most `blocks` blocks per launch of this library, so that the later trips
 * of the kernels' loops (over panels and m-chunks; over rows) run at small shapes.  Process-wide, a plain int: set it before
 * launching, not concurrently.  Returns the previous cap; 0 (or any value < 1) means no cap and is what a fresh library has. */
int qdn_set_grid_cap(int blocks);

/* Bytes of `work` for a call with these sizes: 4 (2 + 2 k) m ceil(V / QDN_PANEL).  -1 for what the call refuses of them: a
 * negative V or m, k outside 0 .. QDN_MAX_TOPK, V > 2^31 - 1 - QDN_PANEL (a word index is an int32 inside the library), a
 * product that does not fit an int64. */
int64_t qdn_generator_work_bytes(int64_t V, int64_t m, int k);

/* For every row i < m of x: the logits z[r] = sum_c x[i][c] w[r][c] (+ bias[r]), r < V, and of them
 *   lse[i]            = log sum_r exp z[r]                                             -- always written;
 *   logp[i][r]        = z[r] - lse[i], one fp32 subtraction                            -- where logp is given;
 *   top_val[i][j], top_idx[i][j], j < k: the first k words in the TOTAL ORDER below, as z[r] - lse[i] (the same subtraction)
 *                       and r; with V < k the places from V on hold -inf and -1         -- where k > 0.
 * The logit.  z[r] has the bits qdm_linear_packed_f32 (qd_infer_mm.h) gives for the same arguments: ONE accumulator that starts
 *   at +0.0f and is carried through v_mfma_f32_16x16x4_f32 instructions, the columns in slabs of 64 front to back, inside a slab
 *   in groups of 16 front to back, inside the group at column g the four instructions take g + jj + {0, 4, 8, 12}; a last slab of
 *   fewer than 64 columns runs only the groups that hold a column, the columns of such a group past dim enter as 0 x 0; the bias
 *   is one fp32 addition, and a NULL bias adds nothing: no addition is made.  The bound of that header holds for it.
 * The total order of the words of a row.  a comes before b if a is NaN and b is not; or z[a] > z[b]; or the two are equal, or
 *   both NaN, and a < b as indices.  So ties go to the lower word index (+0.0f and -0.0f are equal) and NaN sorts first: the rule
 *   torch.topk follows.  It is the order of every selection below.  A selected word carries its logit as z[r] + 0.0f: top_val of a
 *   -0.0f logit is computed from +0.0f (it differs from z[r] - lse only in the sign of a zero result), of a NaN logit it is NaN.
 * Panels.  Panel p holds the words [QDN_PANEL p, QDN_PANEL p + QDN_PANEL) below V.  Per row and panel, all fp32, every operation
 *   rounded on its own:
 *     max_p  = the FIRST word's logit in the total order (NaN where the panel holds one).
 *     sum_p  = sum of expf(z[r] - max_p).  The panel is four tiles of 16 words; word r sits in tile (r % 64) / 16 at place
 *              r % 16.  Place j adds its words of tiles 0, 1, 2, 3 in this order to +0.0f; the 16 places are added by an xor tree,
 *              distance 8, 4, 2, 1.  A panel whose max_p is -inf has sum_p = +0.0f exactly (not exp(-inf - -inf)).
 *     its first min(k, words) words in the total order.
 *   The words at or past V of the last panel are no candidates and enter no sum.
 * The row.  M = the first of the max_p in the total order.  S = sum_p sum_p expf(max_p - M), a panel with max_p = -inf adding +0.0f:
 *   thread t of 256 adds the panels t, t + 256, ... front to back to +0.0f, an xor tree (distance 32, 16, .. 1) over each of the four
 *   waves, then ((w0 + w1) + w2) + w3.  lse = M + logf(S); where M is +inf or -inf, lse = M.  So a NaN logit makes lse NaN, a row
 *   whose logits are all -inf gives -inf and a +inf logit (with no NaN) gives +inf: what float64 torch.logsumexp gives.  An
 *   all -inf panel next to others changes no bit of lse.  The top k of the row are the first k of the panels' candidates.
 * Every order is a function of V and dim ALONE -- not of m, of where row i sits in x, of k, of whether logp was asked for, of
 *   bucket, levels, bits or the grid cap: row i of a call has the bits of the call on that row alone, and the same call gives
 *   the same bits every time.  expf and logf are the device library's: lse is promised to the float64 logsumexp of the fp32
 *   logits within 4 x what fp32 torch.logsumexp reaches (tests/test_hip_packed_gen.py, profiles/packed_gen_error.txt), not bits
 *   across compiler releases.
 * A NaN or inf weight in row r reaches z[r] of every row of x and, through the sums, lse; a non-finite x[i] reaches row i alone.
 * work: qdn_generator_work_bytes(V, m, k) bytes, written by the first launch and read by the second; its contents after the
 *   call are unspecified.  With logp given the first launch writes the logits there and the second subtracts lse in place.
 * -1 for: what qd_infer_mm.h refuses of a weight [V][dim] and of x, m, bias; what qdn_generator_work_bytes refuses; a
 *   misaligned pointer; and, when neither m nor V is 0: a NULL lse or work; a NULL x, packed, alpha or beta with dim > 0; a NULL
 *   top_val or top_idx with k > 0; lse, logp, top_val, top_idx or work equal to packed, alpha, beta, x or bias, or to each other
 *   (any other overlap of an output with an input is the caller's error and gives unspecified values, never an access outside
 *   the arrays).  With k == 0 top_val and top_idx are not looked at. */
int qdn_generator_packed_f32(const uint8_t* packed, const float* alpha, const float* beta,
                             int64_t V /* rows */, int64_t dim /* cols */, int64_t bucket, int levels, int bits,
                             const float* x /* [m][dim] */, int64_t m, const float* bias /* [V] or NULL */,
                             float* lse /* [m] */, float* logp /* [m][V] or NULL */,
                             int k, float* top_val /* [m][k] */, int64_t* top_idx /* [m][k] */,
                             void* work, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QD_INFER_GEN_H */
