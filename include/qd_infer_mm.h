/* qd_infer_mm.h -- C ABI of libqd_infer_mm.so: the Linear layer of qd_infer.h for MANY rows of x (a batch, batch x beam x
 * time, a prefill), computed from the packed low-bit weights with fp32 matrix instructions on the MI355X (gfx950).
 *
 * qdi_linear_packed_f32 (qd_infer.h, libqd_infer.so) is the decode-time call: one wave per output row, at most 8 rows of x
 * per decode of the weights.  This library decodes a weight once per 64 rows of x and multiplies with
 * v_mfma_f32_16x16x4_f32: fp32 operands, fp32 accumulation.  Nothing is rounded that qd_infer.h does not round: x and y are
 * fp32 and every weight used is the weight value below.  It is an artifact of its own, as libqd_infer.so is: this header and
 * libqd_infer_mm.so, and nothing of the other two libraries.
 *
 * The format and the weight value are those of qd_infer.h ("The format is ...", "The weight value."): the stream of
 * qd_pack_uniform_f32 for a contiguous W[rows][cols], one (alpha, beta) per flat bucket, bucket == 0 or rows cols < bucket one
 * bucket, 2 <= levels <= 256, 1 <= bits <= 8, levels <= 2^bits; w = (((float)c / (float)(levels - 1)) alpha[k] + beta[k]) + 0.0f,
 * bit for bit what qd_unpack_uniform_f32 writes.  The Conventions of qd_infer.h hold word for word for the one call here:
 * device pointers, asynchronous on `stream`; `packed`, x, bias, y, alpha, beta 4-byte aligned and no other alignment changes
 * a bit of a result; writes exactly y[0 .. m rows), reads nothing outside packed[0 .. qd_packed_bytes(rows cols, bits)),
 * alpha / beta[0 .. num_buckets), x[0 .. m cols), bias[0 .. rows); ONE kernel launch, no workspace, no allocation, no
 * synchronisation, so it can be recorded into a hipGraph (by-value arguments frozen at record time, device memory read at
 * replay time); m == 0 or rows == 0 returns 0 without a launch; 0 on success, a positive hipError_t if the launch failed,
 * QDM_ERR_INVALID_ARGUMENT (-1) -- nothing written, nothing launched -- for a NULL required pointer with a non-zero size, a
 * negative size, levels outside 2 .. 256, bits outside 1 .. 8, levels > 2^bits, bucket < 0, a misaligned pointer, or sizes
 * whose product does not fit an int64.
 */
#ifndef QD_INFER_MM_H
#define QD_INFER_MM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QDM_ABI_VERSION 1
#define QDM_ERR_INVALID_ARGUMENT (-1)

int qdm_abi_version(void);          /* QDM_ABI_VERSION */
const char* qdm_target_arch(void);  /* "gfx950" */
const char* qdm_error_string(int code);

/* Test hook, as qdi_set_grid_cap of qd_infer.h: at most `blocks` blocks per launch of this library, so that the later trips
 * of the kernel's loop over tiles run at small shapes.  Process-wide, a plain int: set it before launching, not concurrently.
 * Returns the previous cap; 0 (or any value < 1) means no cap and is what a fresh library has. */
int qdm_set_grid_cap(int blocks);

/* Linear layer: y[i][r] = sum_c x[i][c] w[r][c] (+ bias[r]) for i < m, r < rows (= N, out_features), cols = K.  The argument
 * list of qdi_linear_packed_f32; `bias` may be NULL.
 * Arithmetic, all fp32.  Every output element has ONE accumulator that starts at +0.0f and is carried through
 * v_mfma_f32_16x16x4_f32 instructions, each of which adds four products x[i][c] w[r][c] to it.  The columns are taken in
 * slabs of 64, front to back; inside a slab in groups of 16, front to back; inside the group that starts at column g the four
 * instructions take the columns g + jj + {0, 4, 8, 12}, jj = 0, 1, 2, 3.  A last slab of fewer than 64 columns runs only the
 * groups that hold a column; the columns of such a group past K enter as 0 x 0.  The bias is added last, one fp32 addition.
 * This order is a function of cols ALONE: it does not depend on m, on where row i sits among the rows of x, on rows, bucket,
 * levels, bits or the grid cap; there is no split over K and there are no atomics, so row i of a call with m rows has the
 * bits of the call with m = 1 on x[i], and the same call gives the same bits every time.
 * The result is NOT bit-identical to qdi_linear_packed_f32's, whose order is another (and whose steps are fmaf); both lie
 * within the same bound, |y - exact| <= 1e-6 (sum_c |x w| + |bias|).  How the matrix unit rounds inside an instruction, and
 * what it makes of subnormal operands, products and sums, is the hardware's: for those this header promises the bound, not
 * bits.  Where every partial sum is exactly representable the result is exact, whatever the order.
 * A NaN or inf in row r of the weights reaches y[:, r] and no other output, one in x[i] reaches y[i, :] and no other, as IEEE
 * arithmetic propagates them (0 x inf = NaN).
 * Rows of x are taken 64 at a time; m > 64 runs further chunks inside the same launch, which decode the weights again. */
int qdm_linear_packed_f32(const uint8_t* packed, const float* alpha, const float* beta,
                          int64_t rows /* N */, int64_t cols /* K */, int64_t bucket, int levels, int bits,
                          const float* x /* [m][K] */, int64_t m, const float* bias /* [N] or NULL */,
                          float* y /* [m][N] */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QD_INFER_MM_H */
