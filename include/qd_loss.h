/* qd_loss.h -- C ABI of libqd_loss.so: the distillation loss of a training step -- its value AND its gradient with respect to the
 * student's logits -- in one pass over the logits, on the MI355X (gfx950).
 *
 * The loss of a distillation step is a weighted sum of KL(softmax(teacher / T) || softmax(student / T)) and of the cross entropy
 * of the student with the labels.  As a chain of tensor operations with autograd behind it, the [rows, cols] logits are read or
 * written well over a dozen times.  qdl_kd_loss_f32 reads the student's and the teacher's logits once (twice where a row does
 * not fit a workgroup's LDS) and writes the gradient once: 8 bytes read and 4 written per element.  It is an artifact of its own,
 * as the inference libraries are: this header and libqd_loss.so, and nothing of the other libraries.
 *
 * Conventions: device pointers, asynchronous on `stream`; every float pointer 4-byte aligned, `target` 8-byte aligned, and no
 * other alignment changes a bit of a result; the call writes exactly its four outputs and reads nothing outside its inputs; TWO
 * kernel launches on `stream` (k_kd_rows, k_kd_finish), no allocation, no synchronisation, no atomics, no wait of one block for
 * another, so it can be recorded into a hipGraph (by-value arguments frozen at record time, device memory read at replay time).
 * 0 on success, a positive hipError_t if a launch failed, QDL_ERR_INVALID_ARGUMENT (-1) -- nothing written, nothing launched --
 * for what the call lists.
 */
#ifndef QD_LOSS_H
#define QD_LOSS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QDL_ABI_VERSION 1
#define QDL_ERR_INVALID_ARGUMENT (-1)

/* The three stagings of a row between the two passes over it, chosen by cols ALONE (constants of the ABI, not launch parameters:
 * the summation orders below depend on the staging, and a row's result is to be a function of the row and cols alone):
 *   cols <= QDL_WAVE_COLS   one wave per row, the row in registers;
 *   cols <= QDL_LDS_COLS    one workgroup of 1024 lanes per row, the row in LDS: 8 QDL_LDS_COLS bytes and the reduction scratch
 *                           are the 160 KiB of a gfx950 workgroup;
 *   longer                  one workgroup per row, the second pass reads the row from memory again. */
#define QDL_WAVE_COLS 256
#define QDL_LDS_COLS 20224

int qdl_abi_version(void);          /* QDL_ABI_VERSION */
const char* qdl_target_arch(void);  /* "gfx950" */
const char* qdl_error_string(int code);

/* Test hook: at most `blocks` blocks per launch of k_kd_rows, so that the later trips of its loop over rows run at small shapes.
 * Process-wide, a plain int: set it before launching, not concurrently.  Returns the previous cap; 0 (or any value < 1) means no
 * cap and is what a fresh library has.  No bit of any output depends on it. */
int qdl_set_grid_cap(int blocks);

int64_t qdl_wave_cols(void);        /* QDL_WAVE_COLS */
int64_t qdl_lds_cols(void);         /* QDL_LDS_COLS */

/* For every row n < rows, with z = student[n], t = teacher[n], y = target[n], T = temperature, all fp32 and every operation
 * rounded on its own (no contraction):
 *   Mz = max z, Mt = max t;  az_c = (z_c - Mz) / T,  at_c = (t_c - Mt) / T   (T == 1: no division is made);
 *   Sz = sum_c expf(az_c), St = sum_c expf(at_c), S1 = sum_c expf(z_c - Mz)  (T == 1: S1 IS Sz, computed once);
 *   ps_c = expf(az_c) / Sz,  pt_c = expf(at_c) / St,  p1_c = expf(z_c - Mz) / S1   -- correctly rounded quotients;
 *   row_kl[n]  = sum_c pt_c ((at_c - logf(St)) - (az_c - logf(Sz)));
 *   row_nll[n] = logf(S1) - (z_y - Mz);
 *   grad[n][c] = (kl_scale / T) (ps_c - pt_c) + nll_scale (p1_c - [c == y]);
 *   loss[0]    = sum_n (kl_scale row_kl[n] + nll_scale row_nll[n]).
 * pt and ps are computed by the same operations in the same order: with teacher the bits of student, row_kl is exactly 0 and so
 * is the KL part of grad.  A pt_c that underflows to 0 contributes 0.
 * Orders.  Wave staging: lane l of 64 adds its columns l, l + 64, ... front to back to +0.0f, against the row's max; the lanes
 *   are added by an xor tree (distance 8, 4, 2, 1, 16, 32).  The other two: lane l of 1024 takes the groups l, l + 1024, ... of
 *   four columns front to back, then the lanes 0 .. take one each of the cols % 4 last columns; it keeps its sums of exp in online
 *   form -- a running (max m, sum s), s = s expf((m - m') / T) + (((e_0 + e_1) + e_2) + e_3) when a group moves m to m' --
 *   and the lanes are combined as sum_l s_l expf((m_l - M) / T), the same tree over each wave, the 16 waves front to back.
 *   row_kl is summed over the same lanes in the same way.  loss: lane l of 1024 adds the rows l, l + 1024, ... front to back to
 *   +0.0f, the same tree, the 16 waves front to back: an order that is a function of `rows` alone.
 * So row n of a call has the bits of the call on that row alone, whatever rows, n, the grid or the cap are.  expf and logf are the
 * device library's: the results are promised to float64 within 4 x what the same formulas reach in fp32 torch
 * (tests/test_hip_kd_loss.py, profiles/kd_loss_error.txt), not bits across compiler releases.
 * y == ignore_index: the row is NOT READ (it may hold anything); its grad is +0.0f, row_kl = row_nll = +0.0f.
 * y outside [0, cols) and not ignore_index: every output of the row is NaN (row_nll and grad among them); no other row changes.
 * A NaN, +inf or -inf anywhere in z or t of a row that is not ignored: every output of the row is NaN, and loss with it; no other
 *   row changes.  (-inf included: a logit that says "probability 0" is refused rather than computed with.)
 * rows == 0: loss[0] = +0.0f is written (one launch), nothing else is looked at but `loss`.
 * -1 for: a NULL student, teacher, target, grad, row_kl, row_nll (rows > 0) or loss; a pointer that is not 4-byte aligned (target:
 *   8-byte); rows < 0; cols < 0; cols == 0; rows cols that does not fit an int64 when counted in bytes; a temperature that is NaN,
 *   infinite, 0 or negative; grad, row_kl, row_nll or loss equal to student, teacher or target, or to each other (any other
 *   overlap of an output with another array is the caller's error and gives unspecified values, never an access outside the
 *   arrays). */
int qdl_kd_loss_f32(const float* student /* [rows][cols] */, const float* teacher /* [rows][cols] */,
                    const int64_t* target /* [rows] */, int64_t rows, int64_t cols,
                    float temperature, float kl_scale, float nll_scale, int64_t ignore_index,
                    float* grad /* [rows][cols] */, float* row_kl /* [rows] */, float* row_nll /* [rows] */,
                    float* loss /* [1] */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QD_LOSS_H */
