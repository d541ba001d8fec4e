/* qd_infer.h -- C ABI of libqd_infer.so: Linear and Embedding layers computed straight from the packed low-bit weights
 * of a quantized student, on the MI355X (gfx950).
 *
 * The training path (qd_hip.h, libqd_hip.so) produces the packed form -- qd_pack_uniform_f32 -- and decodes it back to
 * fp32.  This library CONSUMES it: a layer reads bits / 8 bytes per weight from memory and never holds the fp32 tensor.
 * It replaces no line of the reference (the reference never runs a packed student), so it is an artifact of its own: a
 * deployed student needs this header and libqd_infer.so and nothing of the training library.
 *
 * The format is what qd_pack_uniform_f32 / codec.pack_uniform(W, s, bucket, bits) write for a contiguous 2-D weight
 * W[rows][cols] (nn.Linear: [out_features][in_features]; nn.Embedding: [num_embeddings][dim]):
 *   - the stream: bit i is bit i & 7 of byte i >> 3; element e = r cols + c holds its level index LSB first in stream bits
 *     [e bits, (e + 1) bits); qd_packed_bytes(rows cols, bits) = ceil(rows cols bits / 8) bytes;
 *   - one (alpha, beta) per FLAT bucket of `bucket` elements: bucket k holds elements [k bucket, (k + 1) bucket) -- a row
 *     may straddle buckets and a bucket may span rows.  bucket == 0 ("bucket_size=None") and rows cols < bucket are one
 *     bucket for the tensor; any positive bucket size is accepted;
 *   - 2 <= levels <= 256, 1 <= bits <= 8, levels <= 2^bits.
 *
 * The weight value.  Element e with level index c in bucket k is
 *       w = (((float)c / (float)(levels - 1)) * alpha[k] + beta[k]) + 0.0f
 * every operation rounded to fp32 on its own, the division correctly rounded, nothing contracted: the four operations of
 * qd_unpack_uniform_f32, so w is what that call writes, bit for bit, NaN and inf buckets included.  (The kernels take the
 * quotient from a table of the `levels` correctly rounded quotients, built per block with the same division.)
 *
 * Conventions
 *   - every pointer is a DEVICE pointer; all calls are asynchronous on `stream` (a hipStream_t passed as void*);
 *   - alignment: `packed` 4 bytes; every float array 4 bytes; `idx` 8 bytes.  No other alignment changes a bit of a
 *     result (16-byte stores are used where an output address allows them, with the same values);
 *   - writes: exactly out[0 .. count cols) or y[0 .. m rows).  Reads: nothing outside packed[0 .. qd_packed_bytes(rows cols,
 *     bits)), alpha / beta[0 .. num_buckets), x[0 .. m cols), bias[0 .. rows), idx[0 .. count);
 *   - launch: a call takes no workspace, allocates nothing, never synchronises and is ONE kernel launch, so it can be
 *     recorded into a hipGraph; by-value arguments are frozen at record time, device memory is read at replay time;
 *   - empty calls: count == 0 or m == 0 (or nothing to write: cols == 0 for the embedding, rows == 0 for the linear layer)
 *     return 0 without a launch;
 *   - return value: 0 on success, a positive hipError_t if the launch failed, QDI_ERR_INVALID_ARGUMENT (-1) -- with
 *     nothing written and nothing launched -- for a NULL required pointer with a non-zero size, a negative size, levels
 *     outside 2 .. 256, bits outside 1 .. 8, levels > 2^bits, bucket < 0, a misaligned pointer, or sizes whose product
 *     does not fit an int64.  qdi_error_string() describes either.
 */
#ifndef QD_INFER_H
#define QD_INFER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QDI_ABI_VERSION 1
#define QDI_ERR_INVALID_ARGUMENT (-1)

int qdi_abi_version(void);          /* QDI_ABI_VERSION */
const char* qdi_target_arch(void);  /* "gfx950" */
const char* qdi_error_string(int code);

/* Test hook, as qd_set_grid_cap of qd_hip.h: at most `blocks` blocks per launch of this library, so that the later trips
 * of the kernels' grid-stride loops run at small shapes.  Process-wide, a plain int: set it before launching, not
 * concurrently.  Returns the previous cap; 0 (or any value < 1) means no cap and is what a fresh library has. */
int qdi_set_grid_cap(int blocks);

/* Embedding lookup: out[j][:] = w[idx[j]][:] for j < count, bit for bit the weight value above.
 * An index outside [0, rows) writes a row of NaN and reads nothing of `packed`, alpha or beta. */
int qdi_embedding_packed_f32(const uint8_t* packed, const float* alpha, const float* beta,
                             int64_t rows, int64_t cols, int64_t bucket, int levels, int bits,
                             const int64_t* idx, int64_t count, float* out /* [count][cols] */, void* stream);

/* Linear layer: y[i][r] = sum_c x[i][c] w[r][c] (+ bias[r]) for i < m, r < rows (= N, out_features), cols = K.
 * `bias` may be NULL.  Arithmetic, all fp32: one wave per output row; lane l of 64 owns the column groups
 * [4 (l + 64 t), 4 (l + 64 t) + 4), t = 0, 1, ..., and folds them front to back, column by column, into one accumulator
 * per row of x that starts at +0.0f -- EVERY step is acc = fmaf(x[i][c], w[r][c], acc), one rounding.  The 64 accumulators
 * are then added in a fixed tree: lane l += lane l ^ 32, then ^ 16, ^ 8, ^ 4, ^ 2, ^ 1 (plain fp32 additions); the bias is
 * added last, one fp32 addition.  The order is therefore a pure function of cols alone -- the same for every rows, bucket,
 * bits, m and grid cap -- there are no atomics, and the same call gives the same bits every time.
 * Rows of x are taken in tiles of 8 (4, 2, 1 when m is smaller); m > 8 runs further tiles inside the same launch, which
 * decode the weights again (functional, not tuned).  A NaN or inf in row r's weights or in x[i] propagates as IEEE
 * arithmetic does (0 x inf = NaN) into y[i][r] and into no other output. */
int qdi_linear_packed_f32(const uint8_t* packed, const float* alpha, const float* beta,
                          int64_t rows /* N */, int64_t cols /* K */, int64_t bucket, int levels, int bits,
                          const float* x /* [m][K] */, int64_t m, const float* bias /* [N] or NULL */,
                          float* y /* [m][N] */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QD_INFER_H */
