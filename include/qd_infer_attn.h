/* qd_infer_attn.h -- C ABI of libqd_infer_attn.so: one step of Luong "global attention" (dot / general score) of a decoder
 * whose output projection W_out[dim][2 dim] is kept as packed low-bit weights, on the MI355X (gfx950).
 *
 * A decoder step with attention is, after the recurrent cells, score = keys . q, a masked softmax over the source, the context
 * ctx = align . values and attn_h = tanh(W_out [ctx ; x] + bias).  Around qdm_linear_packed_f32 that is seven launches and a
 * materialised [batch][2 dim] concatenation.  This library makes it two: qda_attn_context_f32 (scores, softmax and context of
 * a batch row in one block, the scores never leaving LDS) and qda_attn_out_packed_f32 (the packed weight walked in two
 * parts, its columns [0, dim) against ctx and [dim, 2 dim) against x, into one accumulator, tanhf in the lane that holds the
 * sum).  The `general` form's q = W_in query is one qdm_linear_packed_f32 of libqd_infer_mm.so before them.  It is an artifact
 * of its own, as the other five are: this header and libqd_infer_attn.so, and nothing of the other libraries.
 *
 * The format and the weight value are those of qd_infer.h ("The format is ...", "The weight value.") for the one contiguous
 * weight W_out[dim][2 dim]: the stream of qd_pack_uniform_f32, one (alpha, beta) per FLAT bucket -- a bucket may straddle rows
 * and the boundary between the two halves of a row --, bucket == 0 or fewer elements than a bucket one bucket, 2 <= levels <=
 * 256, 1 <= bits <= 8, levels <= 2^bits; w = (((float)c / (float)(levels - 1)) alpha[k] + beta[k]) + 0.0f, bit for bit what
 * qd_unpack_uniform_f32 writes.
 *
 * The Conventions of qd_infer.h hold for both calls: device pointers, asynchronous on `stream`; every float pointer 4-byte
 * aligned (`lengths` 8-byte) and no other alignment changes a bit of a result; each call writes exactly its outputs and reads
 * nothing outside its inputs; ONE kernel launch, no workspace, no allocation, no synchronisation, no atomics, no wait of one
 * block for another, so it can be recorded into a hipGraph (by-value arguments frozen at record time, device memory read at
 * replay time).  An empty batch, dim or S returns 0 without a launch; 0 on success, a positive hipError_t if the launch
 * failed, QDA_ERR_INVALID_ARGUMENT (-1) -- nothing written, nothing launched -- for what each call lists.
 */
#ifndef QD_INFER_ATTN_H
#define QD_INFER_ATTN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QDA_ABI_VERSION 1
#define QDA_ERR_INVALID_ARGUMENT (-1)

/* LDS a block of qda_attn_context_f32 may take, in bytes: what a workgroup can have on gfx950.  The call needs
 * 4 (16 + ceil4(dim) + ceil4(S)) bytes of it (ceil4: rounded up to a multiple of four) for the query and the scores; a dim
 * or an S with which that exceeds the limit is refused. */
#define QDA_CONTEXT_LDS_LIMIT 163840

int qda_abi_version(void);          /* QDA_ABI_VERSION */
const char* qda_target_arch(void);  /* "gfx950" */
const char* qda_error_string(int code);

/* Test hook, as qdm_set_grid_cap of qd_infer_mm.h: at most `blocks` blocks per launch of this library, so that the later
 * trips of the kernels' loops (over batch rows; over tiles) run at small shapes.  Process-wide, a plain int: set it before
 * launching, not concurrently.  Returns the previous cap; 0 (or any value < 1) means no cap and is what a fresh library has. */
int qda_set_grid_cap(int blocks);

/* Masked single-query attention over the source.  Per batch row b, with len = min(lengths[b], S) (lengths == NULL: len = S),
 * all fp32, every operation below rounded on its own (fmaf is one operation):
 *   score_s = sum_k q[b][k] keys[b][s][k] for s < len.  Lane l of 64 owns the column groups [4 (l + 64 t), + 4), t = 0, 1, ...:
 *             its partial sum starts at +0.0f and takes its columns front to back, part = fmaf(q_k, key_k, part) (the columns of
 *             the last group past dim enter as 0 x 0); the 64 partial sums are added by an xor tree, distance 32, 16, .. 1.
 *   m       = the largest score (fmaxf: a NaN score does not become m, it makes its own p NaN and through l the whole row).
 *   p_s     = expf(score_s - m);  l = sum_s p_s: thread t of 256 adds its p_s, s = t, t + 256, ..., front to back to +0.0f, an xor
 *             tree over each of the four waves, then ((w0 + w1) + w2) + w3.
 *   align[b][s] = p_s / l (correctly rounded) for s < len and exactly +0.0f for len <= s < S.
 *   ctx[b][k]   = align_0 values[b][0][k], then for s = 1 .. len - 1 in order ctx = fmaf(align_s, values[b][s][k], ctx).
 * Per batch row this is a GEMV and a weighted sum of rows: no matrix instructions.
 * The orders are functions of dim and of the row's len ALONE -- not of batch, of where the row sits in it, of the grid cap or
 * of which path served the context (below): row b of a call has the bits of the call on that row alone, and the same call
 * gives the same bits every time.  expf is the device library's: align is promised to the float64 softmax within 4 x what the
 * fp32 torch composition reaches (tests/test_hip_packed_attn.py, profiles/packed_attn_error.txt), not bits across compiler
 * releases.
 * Padding: keys[b][s] and values[b][s] with s >= len are NEVER read and may hold anything.
 * lengths[b] <= 0: align[b][0 .. S) and ctx[b][0 .. dim) are NaN, as torch's softmax of a row masked everywhere.
 * values may be the same pointer as keys.  Then, where 4 S ceil4(dim) bytes fit into QDA_CONTEXT_LDS_LIMIT next to the query
 * and the scores, the rows are kept in LDS during the score pass and the context pass reads them from there (the source is
 * read from memory once); otherwise the context pass reads values from memory.  The choice is made on the host from the
 * arguments alone and changes no bit of a result.
 * -1 for: a negative size; batch S dim not fitting an int64; a misaligned pointer; 4 (16 + ceil4(dim) + ceil4(S)) >
 * QDA_CONTEXT_LDS_LIMIT; and, when no size is 0: a NULL q, keys, values, align or ctx; align or ctx equal to q, keys, values or
 * to each other (any other overlap of an output with an input is the caller's error and gives unspecified values, never an
 * access outside the arrays). */
int qda_attn_context_f32(
    const float* q /* [batch][dim] */, const float* keys /* [batch][S][dim] */, const float* values /* [batch][S][dim] */,
    const int64_t* lengths /* [batch] or NULL */, int64_t batch, int64_t S, int64_t dim,
    float* align /* [batch][S] */, float* ctx /* [batch][dim] */, void* stream);

/* attn_h = tanhf(W_out [ctx ; x] + bias) for `batch` rows, the concatenation never made:
 *   pre[b][r] = sum_{k < dim} ctx[b][k] W_out[r][k] + sum_{k < dim} x[b][k] W_out[r][dim + k], r < dim, then pre + bias[r] (a NULL bias
 *   adds nothing: no addition is made); attn_h[b][r] = tanhf(pre[b][r]).  `pre`, where given, receives the sum as it enters tanhf.
 * Arithmetic of the sum, all fp32: ONE accumulator that starts at +0.0f and is carried through v_mfma_f32_16x16x4_f32
 *   instructions, each of which adds four products to it: first the part against ctx, then the part against x, each part as
 *   qdm_linear_packed_f32 takes a weight of dim columns (slabs of 64 front to back, groups of 16 front to back, inside the group at
 *   column g the four instructions take g + jj + {0, 4, 8, 12}; a last slab of fewer than 64 columns runs only the groups that
 *   hold a column, the columns of such a group past the end enter as 0 x 0).  A slab never holds columns of both parts.  The order
 *   is a function of dim ALONE: not of batch, of where a row sits in the batch, of bucket, levels, bits or the grid cap.  Row b
 *   of a call has the bits of the call on that row alone.
 * Bound: |pre - exact| <= 1e-6 (sum |terms| + |bias|); where every partial sum is exactly representable it is exact.  tanhf is the
 *   device library's: attn_h is promised to the float64 tanh of the fp32 pre within 4 x what torch's fp32 tanh reaches
 *   (profiles/packed_attn_error.txt), not bits across compiler releases.
 * A NaN or inf weight in row r reaches pre[:, r] (0 x inf = NaN) and no other column; a non-finite activation propagates as
 *   IEEE arithmetic does through the weight rows.
 * -1 for: what qd_infer.h refuses of a weight [dim][2 dim] (levels, bits, bucket, alignment, element or bit count not fitting);
 *   a negative size; 2 dim or batch dim not fitting an int64; a misaligned pointer; and, when neither batch nor dim is 0: a NULL
 *   packed, alpha, beta, ctx, x or attn_h; attn_h or pre equal to ctx, x or bias, or to each other. */
int qda_attn_out_packed_f32(
    const uint8_t* packed, const float* alpha, const float* beta, int64_t bucket, int levels, int bits, /* W_out [dim][2 dim] */
    int64_t dim, const float* ctx /* [batch][dim] */, const float* x /* [batch][dim] */, int64_t batch,
    const float* bias /* [dim] or NULL */, float* attn_h /* [batch][dim] */, float* pre /* [batch][dim] or NULL */,
    void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QD_INFER_ATTN_H */
